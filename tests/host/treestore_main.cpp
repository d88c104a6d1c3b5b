// Stand-alone program over zerokit_amd/csrc/tree_store.h for tests/test_tree_store_host.py:
//   fuzz <dir>      -fsanitize=address,undefined: a store of 24 operations is written, then 20 000 seeded mutations of its
//                   journal and snapshot (truncate, flip a bit, splice, oversized length fields, a payload altered under a
//                   fresh CRC) are opened; every open either succeeds with a well-formed image or returns an error
//   threads <dir>   -fsanitize=thread: the flusher at 1 ms against a thread that appends (and compacts) and another that
//                   calls sync() and info(); the store then reopens at the appender's state
//   crash <dir>     (no sanitizer; the test kills it) one-leaf records with flush_every_ms = 0: operation i (1-based)
//                   writes the value i to leaf (i - 1) mod 32 and its number is printed once the call has returned
// Prints "ok ..." and exits 0, or says what went wrong and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>

#include "treestore.cpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
void leaf_of(uint64_t v, uint8_t out[32]) {
  memset(out, 0, 32);
  put_u64(out, v);
  put_u64(out + 8, v * 0x9E3779B97F4A7C15ull);
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

// a mix of every record kind on a depth-5 tree, left uncompacted
bool write_base(const std::string& dir) {
  std::string err;
  HostTree* t = host_open(dir.c_str(), 5, 500, 0, 0, err);
  if (!t) return false;
  uint8_t leaves[32 * 8];
  bool ok = true;
  for (uint64_t op = 0; op < 24 && ok; op++) {
    for (int i = 0; i < 8; i++) leaf_of(100 * op + i, leaves + 32 * i);
    if (op % 4 == 0) {
      ok = t->set_range(op % 20, 1 + op % 8, leaves) == 0;
    } else if (op % 4 == 1) {
      uint64_t idx[3] = {op % 32, (op * 7) % 32, (op * 13 + 1) % 32};
      ok = t->set_scatter(3, idx, leaves) == 0;
    } else if (op % 4 == 2) {
      ok = t->set_meta(leaves, op) == 0;
    } else {
      uint64_t idx = op % 32;
      ok = t->set_scatter(1, &idx, leaves) == 0;
    }
  }
  ok = ts_close(t, 0) == 0 && ok;
  return ok;
}

int fuzz(const std::string& root) {
  const std::string base = root + "/base", work = root + "/work";
  if (!write_base(base)) return fail("the base store could not be written", 0);
  const std::vector<uint8_t> wal0 = slurp(base + "/rlnamd_tree.wal");
  std::vector<uint8_t> snap0 = slurp(base + "/rlnamd_tree.bin");
  if (wal0.size() < WAL_HEADER + 24 * REC_FRAME || snap0.size() < SNAP_HEADER + 4) return fail("the base store is too small", wal0.size());
  // (the snapshot of a fresh store is empty: a second base, compacted, gives the fuzzer leaves and metadata to damage)
  {
    std::string err;
    HostTree* t = host_open(base.c_str(), 5, 500, 0, 0, err);
    if (!t || ts_close(t, 1) != 0) return fail("the base store could not be compacted", 0);
    snap0 = slurp(base + "/rlnamd_tree.bin");
  }
  std::vector<uint64_t> rec_at;   // where each record of wal0 starts
  for (uint64_t at = WAL_HEADER; at + REC_FRAME <= wal0.size(); at += REC_FRAME + get_u64(wal0.data() + at)) rec_at.push_back(at);
  mkdir(work.c_str(), 0777);
  uint64_t opened = 0, refused = 0;
  for (uint64_t it = 0; it < 20000; it++) {
    // the journal goes with the generation-1 snapshot of an empty tree, the damaged snapshot with no journal
    const bool on_wal = rnd() % 3 != 0;
    std::vector<uint8_t> b = on_wal ? wal0 : snap0;
    const uint64_t kind = rnd() % 5;
    if (kind == 0) {
      b.resize(rnd() % (b.size() + 1));
    } else if (kind == 1) {
      b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
    } else if (kind == 2) {   // splice: a stretch of the file copied over another
      const uint64_t n = 1 + rnd() % 64, from = rnd() % b.size(), to = rnd() % b.size();
      for (uint64_t i = 0; i < n && from + i < b.size() && to + i < b.size(); i++) b[to + i] = b[from + i];
    } else if (kind == 3) {   // a length field far beyond the file
      const uint64_t huge = rnd() % 2 ? ~(uint64_t)0 - rnd() % 64 : ((uint64_t)1 << (20 + rnd() % 40)) + rnd() % 4096;
      if (on_wal) {
        const uint64_t at = rec_at[rnd() % rec_at.size()];
        put_u64(b.data() + at + (rnd() % 2 ? 0 : 8 + 9), huge);   // the frame's length, or the payload's first count
      } else {
        put_u64(b.data() + (rnd() % 2 ? 16 : 24), huge);           // next index, or metadata length
        if (rnd() % 2) put_u32(b.data() + b.size() - 4, crc32c(b.data(), b.size() - 4));
      }
    } else {                  // a byte altered under a fresh checksum: what the CRC lets through must still be refused or applied whole
      if (on_wal) {
        const uint64_t at = rec_at[rnd() % rec_at.size()], len = get_u64(b.data() + at);
        b[at + 8 + rnd() % std::min<uint64_t>(len, 40)] = (uint8_t)rnd();
        put_u32(b.data() + at + 8 + len, crc32c(b.data() + at, 8 + len));
      } else {
        b[8 + rnd() % (SNAP_HEADER - 8)] = (uint8_t)rnd();
        put_u32(b.data() + b.size() - 4, crc32c(b.data(), b.size() - 4));
      }
    }
    unlink((work + "/rlnamd_tree.bin").c_str());
    unlink((work + "/rlnamd_tree.wal").c_str());
    if (!spit(work + (on_wal ? "/rlnamd_tree.wal" : "/rlnamd_tree.bin"), b)) return fail("cannot write the mutated file", it);
    std::string err;
    HostTree* t = host_open(work.c_str(), 5, 500, 0, 0, err);
    if (!t) {
      if (err.compare(0, 19, "Merkle tree error: ") != 0) return fail(err.c_str(), it);
      refused++;
      continue;
    }
    if (t->im.depth != 5 || t->im.next > 32 || t->im.leaves.size() != t->im.next * 32) return fail("ill-formed image", it);
    uint64_t info[8];
    t->st.info(info);
    if (on_wal && info[INFO_REPLAYED] > 24) return fail("more records than were written", it);
    // one more operation on what was opened, so that appending after a cut tail is exercised as well
    uint8_t leaf[32];
    leaf_of(it, leaf);
    const uint64_t idx = it % 32;
    if (t->set_scatter(1, &idx, leaf) != 0) return fail(t->err.c_str(), it);
    if (ts_close(t, it % 7 == 0) != 0) return fail("close failed", it);
    opened++;
  }
  if (!opened || !refused) return fail("the mutations were all of one kind", opened);
  printf("ok fuzz: 20000 mutations, %llu opened, %llu refused\n", (unsigned long long)opened, (unsigned long long)refused);
  return 0;
}

int threads(const std::string& dir) {
  std::string err;
  HostTree* t = host_open(dir.c_str(), 6, 1, 16384, 1, err);
  if (!t) return fail(err.c_str(), 0);
  std::atomic<int> bad{0};
  std::atomic<bool> done{false};
  std::thread appender([&]() {
    uint8_t leaf[32];
    for (uint64_t i = 0; i < 3000; i++) {
      leaf_of(i + 1, leaf);
      const uint64_t idx = i % 64;
      if (t->set_scatter(1, &idx, leaf) != 0) bad++;
      if (i % 64 == 0) std::this_thread::sleep_for(std::chrono::milliseconds(1));   // lets the flusher find unsynced bytes
    }
    done = true;
  });
  std::thread syncer([&]() {
    uint64_t info[8];
    while (!done) {
      try {
        t->st.sync();
      } catch (const std::exception&) {
        bad++;
      }
      t->st.info(info);
      if (info[INFO_JOURNAL_BYTES] < WAL_HEADER) bad++;
    }
  });
  appender.join();
  syncer.join();
  uint64_t info[8];
  t->st.info(info);
  const std::vector<uint8_t> want = t->im.leaves;
  if (bad || info[INFO_COMPACTIONS] == 0 || info[INFO_SYNCS] == 0) return fail("appends, syncs or compactions failed", info[INFO_COMPACTIONS]);
  if (ts_close(t, 0) != 0) return fail("close failed", 0);
  t = host_open(dir.c_str(), 6, 1, 16384, 1, err);
  if (!t) return fail(err.c_str(), 1);
  const bool same = t->im.leaves == want && t->im.next == 64;
  ts_close(t, 1);
  if (!same) return fail("the reopened store differs from the appender's tree", 0);
  printf("ok threads: 3000 appends, %llu compactions, %llu syncs\n", (unsigned long long)info[INFO_COMPACTIONS],
         (unsigned long long)info[INFO_SYNCS]);
  return 0;
}

int crash(const std::string& dir) {
  std::string err;
  HostTree* t = host_open(dir.c_str(), 5, 0, 4096, 0, err);
  if (!t) return fail(err.c_str(), 0);
  uint8_t leaf[32];
  for (uint64_t i = 1; i <= 1000000; i++) {
    memset(leaf, 0, 32);
    put_u64(leaf, i);
    const uint64_t idx = (i - 1) % 32;
    if (t->set_scatter(1, &idx, leaf) != 0) return fail(t->err.c_str(), i);
    if (printf("%llu\n", (unsigned long long)i) < 0 || fflush(stdout) != 0) return 1;   // nobody reads any more
  }
  ts_close(t, 1);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : "";
  if (dir.empty() || (mode != "fuzz" && mode != "threads" && mode != "crash")) {
    fprintf(stderr, "usage: %s fuzz|threads|crash <dir>\n", argv[0]);
    return 2;
  }
  if (mode == "fuzz") return fuzz(dir);
  if (mode == "threads") return threads(dir);
  return crash(dir);
}
