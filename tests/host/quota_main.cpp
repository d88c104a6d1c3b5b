// Stand-alone program over zerokit_amd/csrc/quota_ledger.h for the sanitizer build of tests/test_quota_host.py
// (-fsanitize=address,undefined).  It reads one case file, written by the test from tests/quota_cases.py:
//   3 x uint64   depth, max_epochs, steps
//   per step     2 x uint64: kind (0 set_epochs, 1 draw, 2 counters), count c
//     set_epochs   ext 32 c | uint64: 1 if the model refuses the call
//     draw         leaf 8 c | ext 32 c | limits 4 c | the model's ids 4 c | statuses c
//     counters     leaf 8 c | ext 32 c | the model's counters 4 c | in-window flags c
// and plays the steps on a fresh sequential ledger.  Then, without a file: calls that must be refused, and a depth-1
// ledger with every slot of the largest window in use.
// Prints "ok <requests judged>" and exits 0, or says what is wrong.
#include <stdio.h>

#include "quota.cpp"

static int edges() {
  uint8_t ext[32 * 65] = {0};
  for (int j = 0; j < 65; j++) ext[32 * j] = (uint8_t)(j + 1);
  void* q = ql_new(1, 64);
  if (!q || ql_new(0, 1) || ql_new(25, 1) || ql_new(3, 0) || ql_new(3, 65)) return 1;
  if (ql_set_epochs(q, ext, 65) != 1 || ql_set_epochs(q, nullptr, 1) != 1 || ql_set_epochs(q, ext, 64) != 0) return 1;
  std::vector<uint64_t> leaf(128);
  std::vector<uint8_t> e(32 * 128), status(128);
  std::vector<uint32_t> limits(128, 1), ids(128);
  for (int i = 0; i < 128; i++) {
    leaf[i] = i & 1;
    memcpy(&e[32 * i], ext + 32 * (i / 2), 32);
  }
  for (int round = 0; round < 2; round++) {
    if (ql_draw(q, 128, leaf.data(), e.data(), limits.data(), ids.data(), status.data()) != 0) return 1;
    for (int i = 0; i < 128; i++)
      if (status[i] != (round ? quota::OVER : quota::OK) || ids[i] != (uint32_t)round) return 1;
  }
  leaf[5] = 2;
  if (ql_draw(q, 128, leaf.data(), e.data(), limits.data(), ids.data(), status.data()) != 1) return 1;
  if (ql_draw(q, 128, nullptr, e.data(), limits.data(), ids.data(), status.data()) != 1) return 1;
  if (ql_draw(q, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return 1;
  if (ql_set_epochs(q, ext + 32 * 64, 1) != 0) return 1;   // 64 leave, one comes
  uint64_t info[6];
  ql_info(q, info);
  if (info[0] != 1 || info[5] != 0) return 1;
  ql_free(q);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: quota_main <case file>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  size_t at = 0;
  bool short_file = false;
  auto take = [&](void* to, size_t bytes) {
    if (raw.size() - at < bytes) {
      short_file = true;
      memset(to, 0, bytes);
      return;
    }
    if (bytes) memcpy(to, raw.data() + at, bytes);
    at += bytes;
  };
  uint64_t head[3];
  take(head, sizeof head);
  void* q = short_file ? nullptr : ql_new(head[0], head[1]);
  if (!q) {
    printf("bad case file header\n");
    return 2;
  }
  size_t judged = 0;
  for (uint64_t step = 0; step < head[2]; step++) {
    uint64_t kc[2];
    take(kc, sizeof kc);
    if (short_file || kc[1] > raw.size()) break;
    const size_t c = kc[1];
    std::vector<uint64_t> leaf(c);
    std::vector<uint8_t> ext(32 * c), flags(c), got_flags(c);
    std::vector<uint32_t> limits(c), want(c), got(c);
    if (kc[0] == 0) {
      uint64_t refused;
      take(ext.data(), 32 * c);
      take(&refused, 8);
      if (short_file) break;
      if ((uint64_t)ql_set_epochs(q, ext.data(), c) != refused) {
        printf("step %llu: set_epochs of %zu: refused %d, the model says %llu\n", (unsigned long long)step, c, (int)!refused,
               (unsigned long long)refused);
        return 1;
      }
    } else {
      take(leaf.data(), 8 * c);
      take(ext.data(), 32 * c);
      if (kc[0] == 1) take(limits.data(), 4 * c);
      take(want.data(), 4 * c);
      take(flags.data(), c);
      if (short_file) break;
      if (kc[0] == 1) {
        if (ql_draw(q, c, leaf.data(), ext.data(), limits.data(), got.data(), got_flags.data()) != 0) {
          printf("step %llu: the draw was refused: %s\n", (unsigned long long)step, ql_last());
          return 1;
        }
      } else {
        ql_used(q, c, leaf.data(), ext.data(), got.data(), got_flags.data());
      }
      for (size_t i = 0; i < c; i++, judged++)
        if (got[i] != want[i] || got_flags[i] != flags[i]) {
          printf("step %llu (kind %llu), item %zu: %u / %d, expected %u / %d\n", (unsigned long long)step, (unsigned long long)kc[0], i,
                 got[i], got_flags[i], want[i], flags[i]);
          return 1;
        }
    }
  }
  if (short_file || at != raw.size()) {
    printf("the case file has the wrong size\n");
    return 2;
  }
  uint64_t info[6];
  ql_info(q, info);
  if (info[5] != 0) {
    printf("%llu counters are not zero in slots that hold no external nullifier\n", (unsigned long long)info[5]);
    return 1;
  }
  ql_free(q);
  if (edges() != 0) {
    printf("the edge calls went wrong\n");
    return 1;
  }
  printf("ok %zu\n", judged);
  return 0;
}
