// A stand-alone program over tests/host/memberdir.cpp for the sanitizer build of tests/test_member_directory_host.py:
// it reads a file of steps with the model's answers, runs them through the header's sequential directory (and the
// threaded register), and prints "ok <answers judged>".  File (little-endian): capacity, seed, steps (3 x u64), then per
// step: op, n (2 x u64) and
//   0 register, 7 register on 8 threads   n x u64 indices | n x 32 idcs | n x u32 limits | u64 refused | n status
//   1 find      n x 32 idcs | n status | n x u64 index | n x u32 limit
//   2 resolve, 3 slash   n x 32 secrets | n x 32 keys | n take | u64 refused | n status | n x u64 index | n x u32 limit
//                        | slash: u64 removed
//   4 remove    n x u64 indices | u64 refused | n status
//   5 get       n x u64 indices | n live | n x 32 idcs | n x u32 limits
//   6 info      u64 live members; and at most half of the slots are taken
#include <stdio.h>
#include <stdlib.h>

#include "memberdir.cpp"

static std::vector<uint8_t> g_file;
static size_t g_at = 0;
static const uint8_t* take_bytes(size_t n) {
  if (g_at + n > g_file.size()) {
    fprintf(stderr, "the steps file ends early\n");
    exit(2);
  }
  const uint8_t* p = g_file.data() + g_at;
  g_at += n;
  return p;
}
template <class T>
static std::vector<T> take_vec(size_t n) {   // (copied out: the file's bytes are not aligned)
  std::vector<T> v(n);
  if (n) memcpy(v.data(), take_bytes(n * sizeof(T)), n * sizeof(T));
  return v;
}
static uint64_t take_u64() { return take_vec<uint64_t>(1)[0]; }
static void fail(uint64_t step, const char* what) {
  fprintf(stderr, "step %llu: %s (%s)\n", (unsigned long long)step, what, md_last());
  exit(1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) g_file.insert(g_file.end(), buf, buf + k);
  fclose(f);
  const uint64_t capacity = take_u64(), seed = take_u64(), steps = take_u64();
  void* h = md_new(capacity, seed);
  if (!h) return 2;
  uint64_t judged = 0;
  for (uint64_t s = 0; s < steps; s++) {
    const uint64_t op = take_u64(), n = take_u64();
    const size_t n1 = n ? n : 1;
    std::vector<uint8_t> status(n1), live(n1), idcs_out(32 * n1);
    std::vector<uint64_t> index(n1);
    std::vector<uint32_t> limit(n1);
    if (op == 0 || op == 7) {
      const std::vector<uint64_t> idx = take_vec<uint64_t>(n);
      const std::vector<uint8_t> idcs = take_vec<uint8_t>(32 * n);
      const std::vector<uint32_t> limits = take_vec<uint32_t>(n);
      const uint64_t refused = take_u64();
      const std::vector<uint8_t> want = take_vec<uint8_t>(n);
      const int rc = op == 0 ? md_register(h, n, idx.data(), idcs.data(), limits.data(), status.data())
                             : md_register_threads(h, n, idx.data(), idcs.data(), limits.data(), status.data(), 8);
      if ((uint64_t)rc != refused) fail(s, "register: refused or not");
      if (!refused && memcmp(status.data(), want.data(), n)) fail(s, "register: status");
    } else if (op == 1) {
      const std::vector<uint8_t> idcs = take_vec<uint8_t>(32 * n);
      const std::vector<uint8_t> want = take_vec<uint8_t>(n);
      const std::vector<uint64_t> want_index = take_vec<uint64_t>(n);
      const std::vector<uint32_t> want_limit = take_vec<uint32_t>(n);
      if (md_find(h, n, idcs.data(), status.data(), index.data(), limit.data())) fail(s, "find: refused");
      if (memcmp(status.data(), want.data(), n) || memcmp(index.data(), want_index.data(), 8 * n) ||
          memcmp(limit.data(), want_limit.data(), 4 * n))
        fail(s, "find: outputs");
    } else if (op == 2 || op == 3) {
      const std::vector<uint8_t> secrets = take_vec<uint8_t>(32 * n), keys = take_vec<uint8_t>(32 * n), take = take_vec<uint8_t>(n);
      const uint64_t refused = take_u64();
      const std::vector<uint8_t> want = take_vec<uint8_t>(n);
      const std::vector<uint64_t> want_index = take_vec<uint64_t>(n);
      const std::vector<uint32_t> want_limit = take_vec<uint32_t>(n);
      uint64_t removed = 0;
      const uint64_t want_removed = op == 3 ? take_u64() : 0;
      const int rc = op == 2 ? md_resolve(h, n, secrets.data(), keys.data(), take.data(), status.data(), index.data(), limit.data())
                             : md_slash(h, n, secrets.data(), keys.data(), take.data(), status.data(), index.data(), limit.data(), &removed);
      if ((uint64_t)rc != refused) fail(s, "resolve: refused or not");
      if (!refused && (memcmp(status.data(), want.data(), n) || memcmp(index.data(), want_index.data(), 8 * n) ||
                       memcmp(limit.data(), want_limit.data(), 4 * n) || removed != want_removed))
        fail(s, "resolve: outputs");
    } else if (op == 4) {
      const std::vector<uint64_t> idx = take_vec<uint64_t>(n);
      const uint64_t refused = take_u64();
      const std::vector<uint8_t> want = take_vec<uint8_t>(n);
      if ((uint64_t)md_remove(h, n, idx.data(), status.data()) != refused) fail(s, "remove: refused or not");
      if (!refused && memcmp(status.data(), want.data(), n)) fail(s, "remove: status");
    } else if (op == 5) {
      const std::vector<uint64_t> idx = take_vec<uint64_t>(n);
      const std::vector<uint8_t> want_live = take_vec<uint8_t>(n), want_idcs = take_vec<uint8_t>(32 * n);
      const std::vector<uint32_t> want_limit = take_vec<uint32_t>(n);
      if (md_get(h, n, idx.data(), live.data(), idcs_out.data(), limit.data())) fail(s, "get: refused");
      if (memcmp(live.data(), want_live.data(), n) || memcmp(idcs_out.data(), want_idcs.data(), 32 * n) ||
          memcmp(limit.data(), want_limit.data(), 4 * n))
        fail(s, "get: outputs");
    } else if (op == 6) {
      uint64_t info[8];
      md_info(h, info);
      if (info[1] != take_u64()) fail(s, "info: live members");
      if (info[3] > info[2] / 2) fail(s, "info: more than half of the slots are taken");
      judged++;
    } else {
      fail(s, "unknown step");
    }
    judged += n;
  }
  md_free(h);
  if (g_at != g_file.size()) return 3;
  printf("ok %llu\n", (unsigned long long)judged);
  return 0;
}
