// Stand-alone program over zerokit_amd/csrc/nullifier_log.h for the sanitizer builds of tests/test_nullifier_log_host.py:
//   (no argument)   -fsanitize=address,undefined: a stream of line shares through the sequential policy, in one call
//                   and in chunks, and through a log so small that every walk collides and wraps around
//   threads         -fsanitize=thread: the same stream, every call's passes on 8 std::threads over the std::atomic
//                   policy, 50 times
// The judge is a model of its own: a std::map from nullifier to the first share, shares taken in index order.  The
// shares are real line shares -- member (a0, a1), message x, y = a0 + x a1 -- so a SPAM secret must be that member's a0.
// Prints "ok <shares judged>" and exits 0, or names the first share that is wrong.
#include <stdio.h>

#include <array>
#include <map>

#include "nullifierlog.cpp"

namespace {

using rlnamd::Fr;
typedef std::array<uint8_t, 32> Bytes32;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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
  Bytes32 nul, x, y, ext;
  uint32_t member;
};
struct Member {
  Fr a0, a1;
  Bytes32 nul;
  std::vector<Share> sent;
};

std::vector<Share> make_stream(size_t n, size_t n_members, std::vector<Member>& members) {
  members.resize(n_members);
  for (auto& m : members) {
    m.a0 = rnd_fr();
    m.a1 = rnd_fr();
    m.nul = bytes_of(rnd_fr());
  }
  const Bytes32 ext[2] = {bytes_of(rnd_fr()), bytes_of(rnd_fr())};
  std::vector<Share> out;
  for (size_t i = 0; i < n; i++) {
    const uint32_t mi = i + 1 == n ? out[0].member : (uint32_t)(rnd() % n_members);
    Member& m = members[mi];
    const int kind = m.sent.empty() ? 0 : i + 1 == n ? 4 : 1 + (int)(rnd() % 4);
    Share s;
    s.member = mi;
    s.nul = m.nul;
    const Fr x = rnd_fr();
    s.x = bytes_of(x);
    s.y = bytes_of(m.a0 + x * m.a1);
    s.ext = ext[mi & 1];
    if (kind == 1) s = m.sent[rnd() % m.sent.size()];              // an exact replay
    if (kind == 2) s.x = m.sent[0].x, s.y = bytes_of(rnd_fr());    // the first x with another y
    if (kind == 3) s.ext = ext[(mi & 1) ^ 1];                      // the nullifier under the other external nullifier
    m.sent.push_back(s);                                           // kind 4 (and 0): a new message on the member's line
    out.push_back(s);
  }
  return out;
}

struct Expect {
  uint8_t status;
  Bytes32 secret;
  uint64_t first_tag;
};
struct First {
  Share s;
  uint64_t tag;
};

int run(const std::vector<Share>& stream, const std::vector<Member>& members, uint64_t capacity, uint64_t seed, size_t chunk,
        int threads, size_t min_each, size_t* judged) {
  std::vector<uint8_t> flat(stream.size() * 128);
  std::vector<uint64_t> tags(stream.size());
  for (size_t i = 0; i < stream.size(); i++) {
    memcpy(&flat[128 * i], stream[i].nul.data(), 32);
    memcpy(&flat[128 * i + 32], stream[i].x.data(), 32);
    memcpy(&flat[128 * i + 64], stream[i].y.data(), 32);
    memcpy(&flat[128 * i + 96], stream[i].ext.data(), 32);
    tags[i] = 1000 + 7 * i;
  }
  std::map<Bytes32, First> seen;
  std::vector<Expect> want;
  size_t counts[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < stream.size(); i++) {
    const Share& s = stream[i];
    Expect e{NEW, Bytes32{}, tags[i]};
    auto it = seen.find(s.nul);
    if (it == seen.end()) {
      seen[s.nul] = First{s, tags[i]};
    } else {
      e.first_tag = it->second.tag;
      if (it->second.s.ext != s.ext) e.status = FOREIGN;
      else if (it->second.s.x == s.x) e.status = DUPLICATE;
      else e.status = SPAM, e.secret = bytes_of(members[s.member].a0);
    }
    counts[e.status]++;
    want.push_back(e);
  }
  for (int k = 0; k < 4; k++)
    if (counts[k] < min_each) {
      printf("the stream meets status %d only %zu times\n", k, counts[k]);
      return 1;
    }
  void* log = nl_new(capacity, seed);
  std::vector<uint8_t> status(stream.size()), secrets(stream.size() * 32);
  std::vector<uint64_t> first(stream.size());
  for (size_t o = 0; o < stream.size(); o += chunk) {
    const size_t n = std::min(chunk, stream.size() - o);
    if (nl_observe(log, n, &flat[128 * o], &tags[o], &status[o], &secrets[32 * o], &first[o], threads) != 0) {
      printf("observe refused the call at share %zu\n", o);
      return 1;
    }
  }
  for (size_t i = 0; i < stream.size(); i++, (*judged)++)
    if (status[i] != want[i].status || memcmp(&secrets[32 * i], want[i].secret.data(), 32) != 0 || first[i] != want[i].first_tag) {
      printf("wrong verdict: share %zu, chunk %zu, threads %d: status %d, expected %d\n", i, chunk, threads, status[i],
             want[i].status);
      return 1;
    }
  if (nl_check_table(log) != (int64_t)seen.size()) {
    printf("the table does not hold one slot per key (chunk %zu, threads %d)\n", chunk, threads);
    return 1;
  }
  if (nl_observe(log, capacity, flat.data(), nullptr, status.data(), nullptr, nullptr, threads) != 1) {
    printf("a call larger than the room left was not refused\n");
    return 1;
  }
  nl_free(log);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const bool threaded = argc > 1 && strcmp(argv[1], "threads") == 0;
  std::vector<Member> members;
  const std::vector<Share> stream = make_stream(2048, 700, members);
  size_t judged = 0;
  if (threaded) {
    for (int rep = 0; rep < 50; rep++)
      if (run(stream, members, 2048, 1 + rep, rep % 2 ? 257 : 2048, 8, 50, &judged)) return 1;
  } else {
    const size_t chunks[] = {2048, 1, 63, 1000};
    for (size_t c : chunks)
      if (run(stream, members, 2048, 5, c, 0, 50, &judged)) return 1;
    if (run(stream, members, 4000, 6, 2048, 0, 50, &judged)) return 1;   // room left over, a table twice as large
    // nearly every share a key of its own: the table as full as it gets (half), the longest walks, on one thread and three
    std::vector<Member> crowd;
    const std::vector<Share> full = make_stream(2048, 1 << 20, crowd);
    if (run(full, crowd, 2048, 7, 2048, 0, 0, &judged)) return 1;
    if (run(full, crowd, 2048, 7, 300, 3, 0, &judged)) return 1;
  }
  printf("ok %zu\n", judged);
  return 0;
}
