// Stand-alone program over zerokit_amd/csrc/quota_store.h for tests/test_quota_store_host.py:
//   cases <dir>     -fsanitize=address,undefined: a store of some 40 records is written with the state after each record
//                   kept; it reopens at the last one, after a compaction too; its journal is then cut at every offset (the
//                   open succeeds at the records wholly below the cut) and flipped at every byte (refused in the header
//                   and in every record but the last, opened without it in the last; never below the state before the flip)
//   fuzz <dir>      the same build: 8 000 seeded mutations of journal and snapshot (truncate, flip a bit, splice, oversized
//                   length fields, a payload altered under a fresh CRC); every open either succeeds with a well-formed
//                   ledger, on which one more draw is made, or is refused with a text of this library
//   crash <dir>     (no sanitizer; the test kills it) draw i (1-based) takes one id of member (i - 1) mod 32 under one
//                   external nullifier, and its number is printed once the draw has returned
// Prints "ok ..." and exits 0, or says what went wrong and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <utility>

#include "quotastore.cpp"

namespace {

constexpr uint64_t DEPTH = 5, MAX_EPOCHS = 4, CAP = 1 << DEPTH;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
void ext_of(uint64_t v, uint8_t out[32]) {
  memset(out, 0, 32);
  put_u64(out, v);
}
std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> b;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return b;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
bool spit(const std::string& path, const std::vector<uint8_t>& b) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = b.empty() || fwrite(b.data(), b.size(), 1, f) == 1;
  return fclose(f) == 0 && ok;
}
int fail(const char* what, uint64_t at) {
  printf("FAILED: %s (at %llu)\n", what, (unsigned long long)at);
  return 1;
}

// the window in its order with its slots, and every counter: what two ledgers must share to be the same ledger
struct State {
  std::vector<std::pair<std::vector<uint8_t>, uint32_t>> window;
  std::vector<uint32_t> used;
  bool operator==(const State& o) const { return window == o.window && used == o.used; }
};
State state_of(const HostLedger& h) {
  State s;
  const quota::Window& W = h.L.window;
  for (uint32_t j = 0; j < W.k; j++) {
    const uint8_t* e = (const uint8_t*)W.e[W.order[j]].w;
    s.window.push_back({std::vector<uint8_t>(e, e + 32), W.order[j]});
  }
  s.used = h.L.used;
  return s;
}
// the never-backwards rule: same window, no counter below
bool not_below(const State& got, const State& floor) {
  if (!(got.window == floor.window)) return false;
  for (size_t i = 0; i < floor.used.size(); i++)
    if (got.used[i] < floor.used[i]) return false;
  return true;
}

// operation `op` of the base sequence: windows, draws and draws by count over 32 members and five external nullifiers,
// one of which is never in a window
bool step(HostLedger* h, uint64_t op) {
  uint8_t ext[32 * 5];
  if (op == 0 || op == 14 || op == 29) {
    const uint64_t w[3][4] = {{1001, 1002, 1003, 0}, {1003, 1001, 1004, 0}, {1004, 1002, 1001, 1003}};
    const uint64_t* e = w[op == 0 ? 0 : op == 14 ? 1 : 2];
    size_t k = 0;
    for (; k < 4 && e[k]; k++) ext_of(e[k], ext + 32 * k);
    return h->set_epochs(ext, k) == 0;
  }
  const size_t n = 1 + rnd() % 5;
  uint64_t leaf[5];
  uint32_t limits[5], ids[5];
  uint8_t counts[5], status[5];
  for (size_t i = 0; i < n; i++) {
    leaf[i] = rnd() % CAP;
    ext_of(1001 + rnd() % 5, ext + 32 * i);
    limits[i] = leaf[i] % 3 == 0 ? 4 : 0xFFFFFFFFu;
    counts[i] = (uint8_t)(1 + rnd() % 4);
  }
  return h->draw(n, leaf, ext, limits, op % 3 == 0 ? counts : nullptr, ids, status) == 0;
}

struct Base {
  std::vector<uint8_t> wal, snap;   // the journal left uncompacted beside the first snapshot; a compacted snapshot
  std::vector<uint64_t> ends;       // the journal's end after each record
  std::vector<State> states;        // ... and the ledger then
};
bool write_base(const std::string& dir, uint64_t ops, Base& b) {
  std::string err;
  HostLedger* h = host_open(dir.c_str(), DEPTH, MAX_EPOCHS, 0, err);
  if (!h) return false;
  uint64_t info[8];
  h->st.info(info);
  b.ends.push_back(info[INFO_JOURNAL_BYTES]);
  b.states.push_back(state_of(*h));
  bool ok = true;
  for (uint64_t op = 0; op < ops && ok; op++) {
    ok = step(h, op);
    h->st.info(info);
    if (info[INFO_JOURNAL_BYTES] == b.ends.back()) continue;   // a draw that granted nothing
    b.ends.push_back(info[INFO_JOURNAL_BYTES]);
    b.states.push_back(state_of(*h));
  }
  ok = qs_close(h, 0) == 0 && ok;
  b.wal = slurp(dir + "/" + WAL_NAME);
  b.snap = slurp(dir + "/" + SNAP_NAME);
  return ok && b.wal.size() == b.ends.back();
}
bool compacted_snapshot(const std::string& dir, Base& b) {
  std::string err;
  HostLedger* h = host_open(dir.c_str(), DEPTH, MAX_EPOCHS, 0, err);
  if (!h || !(state_of(*h) == b.states.back()) || qs_close(h, 2) != 0) return false;
  b.snap = slurp(dir + "/" + SNAP_NAME);
  return b.snap.size() > SNAP_HEADER + 4;
}
// a work directory holding the first (empty) snapshot and this journal
bool stage(const std::string& work, const std::vector<uint8_t>& snap, const std::vector<uint8_t>* wal) {
  mkdir(work.c_str(), 0700);
  unlink((work + "/" + SNAP_NAME).c_str());
  unlink((work + "/" + WAL_NAME).c_str());
  return spit(work + "/" + SNAP_NAME, snap) && (!wal || spit(work + "/" + WAL_NAME, *wal));
}

int run_cases(const std::string& root) {
  mkdir(root.c_str(), 0700);
  const std::string base = root + "/base", work = root + "/work";
  Base b;
  if (!write_base(base, 44, b)) return fail("the base store could not be written", 0);
  const std::vector<uint8_t> snap1 = b.snap;
  const size_t records = b.ends.size() - 1;
  if (records < 36 || b.wal.size() > 8192) return fail("the base store has not the size the cases are made for", records);
  std::string err;
  // round trip, and once more behind a compaction
  for (int pass = 0; pass < 2; pass++) {
    HostLedger* h = host_open(base.c_str(), DEPTH, MAX_EPOCHS, 0, err);
    if (!h) return fail(err.c_str(), pass);
    uint64_t info[8];
    h->st.info(info);
    if (!(state_of(*h) == b.states.back()) || info[INFO_GENERATION] != (uint64_t)(1 + pass) || info[INFO_REPLAYED] != (pass ? 0 : records))
      return fail("the reopened ledger is not the one that was written", pass);
    if (qs_close(h, pass ? 0 : 2) != 0) return fail("close failed", pass);
  }
  // cut at every offset
  for (uint64_t cut = WAL_HEADER; cut <= b.wal.size(); cut++) {
    std::vector<uint8_t> w(b.wal.begin(), b.wal.begin() + cut);
    if (!stage(work, snap1, &w)) return fail("cannot write the cut journal", cut);
    size_t kept = 0;
    while (kept + 1 < b.ends.size() && b.ends[kept + 1] <= cut) kept++;
    HostLedger* h = host_open(work.c_str(), DEPTH, MAX_EPOCHS, 0, err);
    if (!h) return fail(err.c_str(), cut);
    uint64_t info[8];
    h->st.info(info);
    if (!(state_of(*h) == b.states[kept]) || info[INFO_REPLAYED] != kept || info[INFO_TORN] != cut - b.ends[kept])
      return fail("a cut journal did not open at the records wholly below the cut", cut);
    qs_close(h, 0);
  }
  // flipped at every byte
  uint64_t refused = 0, opened = 0;
  for (uint64_t at = 0; at < b.wal.size(); at++) {
    std::vector<uint8_t> w = b.wal;
    w[at] ^= (uint8_t)(1u << (rnd() % 8));
    if (!stage(work, snap1, &w)) return fail("cannot write the flipped journal", at);
    size_t whole = 0;
    while (at >= WAL_HEADER && whole + 1 < b.ends.size() && b.ends[whole + 1] <= at) whole++;
    HostLedger* h = host_open(work.c_str(), DEPTH, MAX_EPOCHS, 0, err);
    if (at < b.ends[records - 1]) {
      if (h) return fail("a flip before the last record was opened", at);
      if (err.find("corrupt") == std::string::npos || err.find("offset") == std::string::npos) return fail(err.c_str(), at);
      refused++;
      continue;
    }
    if (!h) return fail(err.c_str(), at);
    if (!(state_of(*h) == b.states[records - 1]) || !not_below(state_of(*h), b.states[whole]))
      return fail("a flip in the last record did not open at the record before it", at);
    qs_close(h, 0);
    opened++;
  }
  printf("ok cases: %llu records, %llu cuts, %llu flips refused, %llu opened at the record before\n", (unsigned long long)records,
         (unsigned long long)(b.wal.size() + 1 - WAL_HEADER), (unsigned long long)refused, (unsigned long long)opened);
  return 0;
}

int fuzz(const std::string& root) {
  mkdir(root.c_str(), 0700);
  const std::string base = root + "/base", work = root + "/work";
  Base b;
  if (!write_base(base, 30, b)) return fail("the base store could not be written", 0);
  const std::vector<uint8_t> snap1 = b.snap, wal0 = b.wal;
  if (!compacted_snapshot(base, b)) return fail("the base store could not be compacted", 0);
  const std::vector<uint8_t> snap0 = b.snap;
  std::vector<uint64_t> rec_at(b.ends.begin(), b.ends.end() - 1);   // where each record of wal0 starts
  uint64_t opened = 0, refused = 0;
  for (uint64_t it = 0; it < 8000; it++) {
    // the journal goes with the first snapshot, the damaged snapshot with no journal
    const bool on_wal = rnd() % 3 != 0;
    std::vector<uint8_t> x = on_wal ? wal0 : snap0;
    const uint64_t kind = rnd() % 5;
    if (kind == 0) {
      x.resize(rnd() % (x.size() + 1));
    } else if (kind == 1) {
      x[rnd() % x.size()] ^= (uint8_t)(1u << (rnd() % 8));
    } else if (kind == 2) {   // splice: a stretch of the file copied over another
      const uint64_t n = 1 + rnd() % 64, from = rnd() % x.size(), to = rnd() % x.size();
      for (uint64_t i = 0; i < n && from + i < x.size() && to + i < x.size(); i++) x[to + i] = x[from + i];
    } else if (kind == 3) {   // a length or count field far beyond the file
      const uint64_t huge = rnd() % 2 ? ~(uint64_t)0 - rnd() % 64 : ((uint64_t)1 << (20 + rnd() % 40)) + rnd() % 4096;
      if (on_wal) {
        const uint64_t at = rec_at[rnd() % rec_at.size()];
        const bool count = rnd() % 2;
        put_u64(x.data() + at + (count ? 8 + 1 : 0), huge);   // the payload's first count, or the frame's length
        if (count && rnd() % 2) put_u32(x.data() + at + 8 + get_u64(x.data() + at), crc32c(x.data() + at, 8 + get_u64(x.data() + at)));
      } else {
        const uint64_t k = get_u64(x.data() + 32);
        put_u64(x.data() + (rnd() % 2 ? 32 : SNAP_HEADER + 40 * k), huge);   // the window's size, or the first slot's pairs
        if (rnd() % 2) put_u32(x.data() + x.size() - 4, crc32c(x.data(), x.size() - 4));
      }
    } else {                  // a byte altered under a fresh checksum: what the CRC lets through is refused or applied whole
      if (on_wal) {
        const uint64_t at = rec_at[rnd() % rec_at.size()], len = get_u64(x.data() + at);
        x[at + 8 + rnd() % len] = (uint8_t)rnd();
        put_u32(x.data() + at + 8 + len, crc32c(x.data() + at, 8 + len));
      } else {
        x[8 + rnd() % (x.size() - 12)] = (uint8_t)rnd();
        put_u32(x.data() + x.size() - 4, crc32c(x.data(), x.size() - 4));
      }
    }
    if (!stage(work, on_wal ? snap1 : x, on_wal ? &x : nullptr)) return fail("cannot write the mutated file", it);
    std::string err;
    HostLedger* h = host_open(work.c_str(), DEPTH, MAX_EPOCHS, 0, err);
    if (!h) {
      if (err.compare(0, 14, "quota ledger: ") != 0) return fail(err.c_str(), it);
      refused++;
      continue;
    }
    const quota::Window& W = h->L.window;
    uint64_t info[8];
    h->st.info(info);
    if (W.k > MAX_EPOCHS || (uint32_t)__builtin_popcountll(W.live) != W.k || (W.live >> MAX_EPOCHS)) return fail("ill-formed window", it);
    for (uint32_t s = 0; s < MAX_EPOCHS; s++)
      for (uint64_t leaf = 0; leaf < CAP && !((W.live >> s) & 1); leaf++)
        if (h->L.used[(s << DEPTH) + leaf]) return fail("a counter in a slot that is not live", it);
    if (on_wal && info[INFO_REPLAYED] > rec_at.size()) return fail("more records than were written", it);
    // one more operation on what was opened, so that appending behind a cut tail is exercised as well
    if (!step(h, 1 + it % 13)) return fail(h->err.c_str(), it);
    if (qs_close(h, it % 7 == 0 ? 2 : 0) != 0) return fail("close failed", it);
    opened++;
  }
  if (!opened || !refused) return fail("the mutations were all of one kind", opened);
  printf("ok fuzz: 8000 mutations, %llu opened, %llu refused\n", (unsigned long long)opened, (unsigned long long)refused);
  return 0;
}

int crash(const std::string& dir) {
  std::string err;
  HostLedger* h = host_open(dir.c_str(), DEPTH, MAX_EPOCHS, 2048, err);
  if (!h) return fail(err.c_str(), 0);
  uint8_t ext[32];
  ext_of(1001, ext);
  if (h->set_epochs(ext, 1) != 0) return fail(h->err.c_str(), 0);
  for (uint64_t i = 1; i <= 1000000; i++) {
    const uint64_t leaf = (i - 1) % CAP;
    const uint32_t limit = 0xFFFFFFFFu;
    uint32_t id = 0;
    uint8_t status = 0;
    if (h->draw(1, &leaf, ext, &limit, nullptr, &id, &status) != 0) return fail(h->err.c_str(), i);
    if (status != quota::OK || id != (i - 1) / CAP) return fail("a draw gave another id than its turn's", i);
    if (printf("%llu\n", (unsigned long long)i) < 0 || fflush(stdout) != 0) return 1;   // nobody reads any more
  }
  qs_close(h, 1);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : "";
  if (dir.empty() || (mode != "cases" && mode != "fuzz" && mode != "crash")) {
    fprintf(stderr, "usage: %s cases|fuzz|crash <dir>\n", argv[0]);
    return 2;
  }
  if (mode == "cases") return run_cases(dir);
  if (mode == "fuzz") return fuzz(dir);
  return crash(dir);
}
