// Stand-alone program over the retire of zerokit_amd/csrc/nullifier_log.h for the sanitizer build of
// tests/test_nullifier_retire_host.py (-fsanitize=address,undefined): a stream of line shares under two external
// nullifiers, the first half observed, one external nullifier retired, the second half observed, in several chunk
// sizes; then a retire of an absent external nullifier, get of a kept, a retired and a never-issued sequence number,
// the room a retire hands back filled exactly, and a retire of everything.
// The judge is a model of its own: a std::map from nullifier to the first share, rebuilt from the survivors at the
// retire, with a0 of the line through the two shares worked out on its own.  The shares are real line shares, so
// between two shares on a member's line that must be the member's a0.
// Prints "ok <shares judged>" and exits 0, or says what is wrong.
#include <stdio.h>

#include <array>
#include <map>

#include "nullifierretire.cpp"

namespace {

using rlnamd::Fr;
typedef std::array<uint8_t, 32> Bytes32;

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
Fr rnd_fr() {   // below 2^250: canonical
  uint32_t c[8];
  for (int i = 0; i < 8; i++) c[i] = (uint32_t)rnd();
  c[7] &= 0x03FFFFFFu;
  return Fr::from_canonical(c);
}
Bytes32 bytes_of(const Fr& v) {
  uint32_t c[8];
  v.to_canonical(c);
  Bytes32 b;
  memcpy(b.data(), c, 32);
  return b;
}

struct Share {
  Bytes32 nul, x, y, ext, a0;
  uint64_t tag;
  bool on_line;   // y = a0 + x a1 of the member
};
struct Member {
  Fr a0, a1;
  Bytes32 nul;
  std::vector<Share> sent;
};

// replays, the first x with another y, the nullifier under the other external nullifier, further messages on the line
std::vector<Share> make_stream(size_t n, size_t n_members, const Bytes32 ext[2]) {
  std::vector<Member> members(n_members);
  for (auto& m : members) m.a0 = rnd_fr(), m.a1 = rnd_fr(), m.nul = bytes_of(rnd_fr());
  std::vector<Share> out;
  for (size_t i = 0; i < n; i++) {
    const uint32_t mi = (uint32_t)(rnd() % n_members);
    Member& m = members[mi];
    const int kind = m.sent.empty() ? 0 : 1 + (int)(rnd() % 4);
    Share s;
    s.nul = m.nul;
    s.a0 = bytes_of(m.a0);
    const Fr x = rnd_fr();
    s.x = bytes_of(x);
    s.y = bytes_of(m.a0 + x * m.a1);
    s.ext = ext[mi & 1];
    s.on_line = true;
    if (kind == 1) s = m.sent[rnd() % m.sent.size()];
    if (kind == 2) s.x = m.sent[0].x, s.y = bytes_of(rnd_fr()), s.on_line = false;
    if (kind == 3) s.ext = ext[(mi & 1) ^ 1];
    s.tag = 1000 + 7 * i;
    m.sent.push_back(s);
    out.push_back(s);
  }
  return out;
}

Fr fr_of(const Bytes32& b) {
  uint32_t c[8];
  memcpy(c, b.data(), 32);
  return Fr::from_canonical(c);
}
// a0 of the line through two shares.  On a member's own line that is the member's a0 (checked where it applies); a
// share with the first x and another y is off the line, and after a retire it may meet a first record with another x.
Bytes32 line_secret(const struct Share& f, const struct Share& s);

struct Model {
  std::map<Bytes32, Share> seen;
  std::vector<Share> held;
  // -> status, secret, first tag
  void observe(const Share& s, uint8_t* status, Bytes32* secret, uint64_t* first_tag) {
    *status = NEW, *secret = Bytes32{}, *first_tag = s.tag;
    held.push_back(s);
    auto it = seen.find(s.nul);
    if (it == seen.end()) {
      seen[s.nul] = s;
      return;
    }
    *first_tag = it->second.tag;
    if (it->second.ext != s.ext) *status = FOREIGN;
    else if (it->second.x == s.x) *status = DUPLICATE;
    else *status = SPAM, *secret = line_secret(it->second, s);
    if (*status == SPAM && it->second.on_line && s.on_line && *secret != s.a0) *status = 99;   // the model itself is wrong
  }
  size_t retire(const Bytes32& ext) {
    std::vector<Share> left;
    for (const Share& s : held)
      if (s.ext != ext) left.push_back(s);
    const size_t gone = held.size() - left.size();
    held.swap(left);
    seen.clear();
    for (const Share& s : held) seen.emplace(s.nul, s);   // (emplace keeps the first)
    return gone;
  }
};

Bytes32 line_secret(const Share& f, const Share& s) {
  const Fr a1 = (fr_of(f.y) - fr_of(s.y)) * (fr_of(f.x) - fr_of(s.x)).inv();
  return bytes_of(fr_of(f.y) - fr_of(f.x) * a1);
}

#define CHECK(cond, ...)     \
  if (!(cond)) {             \
    printf(__VA_ARGS__);     \
    printf("\n");            \
    return 1;                \
  }

int observe_range(void* log, Model& M, const std::vector<Share>& st, size_t lo, size_t hi, size_t chunk, size_t counts[4],
                  size_t* judged) {
  for (size_t o = lo; o < hi; o += chunk) {
    const size_t n = std::min(chunk, hi - o);
    std::vector<uint8_t> flat(128 * n), status(n), secrets(32 * n);
    std::vector<uint64_t> tags(n), first(n);
    for (size_t i = 0; i < n; i++) {
      const Share& s = st[o + i];
      memcpy(&flat[128 * i], s.nul.data(), 32);
      memcpy(&flat[128 * i + 32], s.x.data(), 32);
      memcpy(&flat[128 * i + 64], s.y.data(), 32);
      memcpy(&flat[128 * i + 96], s.ext.data(), 32);
      tags[i] = s.tag;
    }
    CHECK(nr_observe(log, n, flat.data(), tags.data(), status.data(), secrets.data(), first.data()) == 0,
          "observe refused the call at share %zu", o);
    for (size_t i = 0; i < n; i++, (*judged)++) {
      uint8_t want;
      Bytes32 secret;
      uint64_t tag;
      M.observe(st[o + i], &want, &secret, &tag);
      counts[want]++;
      CHECK(status[i] == want && memcmp(&secrets[32 * i], secret.data(), 32) == 0 && first[i] == tag,
            "wrong verdict: share %zu, chunk %zu: status %d, expected %d", o + i, chunk, status[i], want);
    }
  }
  return 0;
}

int run(const std::vector<Share>& st, const Bytes32 ext[2], uint64_t capacity, uint64_t seed, size_t chunk, size_t* judged) {
  const size_t half = st.size() / 2;
  void* log = nr_new(capacity, seed);
  Model M;
  size_t before[4] = {0, 0, 0, 0}, after[4] = {0, 0, 0, 0};
  uint64_t removed = 0, info[6], tag = 0;
  uint8_t share[128];
  if (observe_range(log, M, st, 0, half, chunk, before, judged)) return 1;
  // an external nullifier nobody used: nothing goes
  const Bytes32 absent = bytes_of(rnd_fr());
  CHECK(nr_retire(log, 1, absent.data(), &removed) == 0 && removed == 0, "a retire of an absent external nullifier removed %zu",
        (size_t)removed);
  // the first one goes (given twice: a duplicate in the set is not an error)
  uint8_t twice[64];
  memcpy(twice, ext[0].data(), 32);
  memcpy(twice + 32, ext[0].data(), 32);
  const size_t gone = M.retire(ext[0]);
  CHECK(nr_retire(log, 2, twice, &removed) == 0 && removed == gone && gone > half / 4 && gone < half,
        "the retire removed %zu records, the model %zu", (size_t)removed, gone);
  CHECK(nr_check_table(log) == (int64_t)M.seen.size(), "after the rebuild the table does not hold one slot per key");
  CHECK(nr_seqs_ascend(log), "the sequence numbers of the survivors do not ascend");
  nr_info(log, info);
  CHECK(info[1] == half - gone && info[3] == M.seen.size() && info[4] == half && info[5] >= 1, "info after the retire is wrong");
  // get: every sequence number of the first half is kept or retired, the next one was never issued
  for (size_t i = 0; i < half; i++) {
    const int rc = nr_get(log, i, share, &tag);
    CHECK(rc == (st[i].ext == ext[0] ? 2 : 0), "get(%zu) returned %d", i, rc);
    if (rc == 0)
      CHECK(memcmp(share, st[i].nul.data(), 32) == 0 && memcmp(share + 96, st[i].ext.data(), 32) == 0 && tag == st[i].tag,
            "get(%zu) returned another record", i);
  }
  CHECK(nr_get(log, half, share, &tag) == 1, "get of a sequence number never issued was not refused as such");
  if (observe_range(log, M, st, half, st.size(), chunk, after, judged)) return 1;
  for (int k = 0; k < 4; k++) CHECK(after[k] >= 20, "the second half meets status %d only %zu times", k, after[k]);
  CHECK(nr_check_table(log) == (int64_t)M.seen.size(), "the table does not hold one slot per key at the end");
  // the room is exactly capacity - held: that many fit, one more does not
  nr_info(log, info);
  const size_t room = capacity - info[1];
  std::vector<uint8_t> flat(128 * (room + 1)), status(room + 1);
  for (size_t i = 0; i <= room; i++) {
    const Bytes32 v = bytes_of(rnd_fr());
    for (int k = 0; k < 4; k++) memcpy(&flat[128 * i + 32 * k], v.data(), 32);
  }
  CHECK(nr_observe(log, room + 1, flat.data(), nullptr, status.data(), nullptr, nullptr) == 1, "one share too many was not refused");
  CHECK(nr_observe(log, room, flat.data(), nullptr, status.data(), nullptr, nullptr) == 0, "the room left was not usable");
  CHECK(nr_observe(log, 1, flat.data(), nullptr, status.data(), nullptr, nullptr) == 1, "a full log took one more share");
  // default tags go on from the counter, which the retire did not lower
  CHECK(room == 0 || (nr_get(log, st.size(), share, &tag) == 0 && tag == st.size()), "a default tag is not the sequence number");
  // both external nullifiers go: what is left is the filler shares, and the counter is as it was
  uint8_t both[64];
  memcpy(both, ext[0].data(), 32);
  memcpy(both + 32, ext[1].data(), 32);
  CHECK(nr_retire(log, 2, both, &removed) == 0 && removed == st.size() - gone, "the retire of both removed %zu", (size_t)removed);
  nr_info(log, info);
  CHECK(info[1] == room && info[3] == (uint64_t)nr_check_table(log) && info[4] == st.size() + room, "info after the second retire is wrong");
  nr_free(log);
  return 0;
}

}  // namespace

int main() {
  const Bytes32 ext[2] = {bytes_of(rnd_fr()), bytes_of(rnd_fr())};
  const std::vector<Share> stream = make_stream(2048, 500, ext);
  size_t judged = 0;
  const size_t chunks[] = {2048, 1, 63, 1000};
  for (size_t c : chunks)
    if (run(stream, ext, 2048, 5, c, &judged)) return 1;
  if (run(stream, ext, 3000, 6, 257, &judged)) return 1;   // room left over
  // the refusals
  void* log = nr_new(16, 1);
  uint64_t removed = 0;
  std::vector<uint8_t> many(32 * 65, 0);
  uint8_t big[64];
  memset(big, 0, 32);
  memset(big + 32, 0xFF, 32);
  if (nr_retire(log, 1, nullptr, &removed) != 1 || nr_retire(log, 65, many.data(), &removed) != 2 ||
      nr_retire(log, 2, big, &removed) != 3 || removed != 1 || nr_retire(log, 0, nullptr, &removed) != 0 ||
      nr_retire(log, 64, many.data(), &removed) != 0) {
    printf("a refusal of retire is wrong\n");
    return 1;
  }
  nr_free(log);
  printf("ok %zu\n", judged);
  return 0;
}
