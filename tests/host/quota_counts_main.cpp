// Stand-alone program over zerokit_amd/csrc/quota_ledger.h's draw by count for the sanitizer build of
// tests/test_quota_counts_host.py (-fsanitize=address,undefined).  It reads one case file, written by the test from
// tests/quota_counts_cases.py:
//   3 x uint64   depth, max_epochs, steps
//   per step     2 x uint64: kind (0 set_epochs, 2 counters, 3 draw_counts), count c
//     set_epochs    ext 32 c | uint64: 1 if the model refuses the call
//     counters      leaf 8 c | ext 32 c | the model's counters 4 c | in-window flags c
//     draw_counts   leaf 8 c | ext 32 c | limits 4 c | counts c | the model's firsts 4 c | statuses c
// and plays the steps on a fresh sequential ledger.  Then, without a file: the refusals, a counter next to 2^32 and the
// largest window with the largest count.
// Prints "ok <requests judged>" and exits 0, or says what is wrong.
#include <stdio.h>

#include "quota_counts.cpp"

static int edges() {
  uint8_t ext[32 * 64] = {0};
  for (int j = 0; j < 64; j++) ext[32 * j] = (uint8_t)(j + 1);
  void* q = ql_new(1, 64);
  if (!q || ql_set_epochs(q, ext, 64) != 0) return 1;
  std::vector<uint64_t> leaf(128);
  std::vector<uint8_t> e(32 * 128), status(128), counts(128, 255);
  std::vector<uint32_t> limits(128, 255), firsts(128);
  for (int i = 0; i < 128; i++) {
    leaf[i] = i & 1;
    memcpy(&e[32 * i], ext + 32 * (i / 2), 32);
  }
  for (int round = 0; round < 2; round++) {   // every counter of the ledger: one block of 255, then over
    if (ql_draw_counts(q, 128, leaf.data(), e.data(), limits.data(), counts.data(), firsts.data(), status.data()) != 0) return 2;
    for (int i = 0; i < 128; i++)
      if (status[i] != (round ? quota::OVER : quota::OK) || firsts[i] != (round ? 255u : 0u)) return 3;
  }
  counts[77] = 0;
  if (ql_draw_counts(q, 128, leaf.data(), e.data(), limits.data(), counts.data(), firsts.data(), status.data()) != 1) return 4;
  counts[77] = 1;
  if (ql_draw_counts(q, 128, leaf.data(), e.data(), limits.data(), nullptr, firsts.data(), status.data()) != 1) return 5;
  if (ql_draw_counts(q, 128, nullptr, e.data(), limits.data(), counts.data(), firsts.data(), status.data()) != 1) return 6;
  // n = 2^24 with arrays of one element: refused before any of them is read (the sanitizer sees a read past the end)
  if (ql_draw_counts(q, (size_t)1 << 24, leaf.data() + 127, e.data() + 32 * 127, limits.data() + 127, counts.data() + 127,
                     firsts.data() + 127, status.data() + 127) != 1)
    return 7;
  if (ql_draw_counts(q, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return 8;
  // a counter three below 2^32 - 1 under the limit 2^32 - 1: a block of 3 does not fit, and nothing wraps around
  if (ql_set_used(q, 1, ext, 0xFFFFFFFDu) != 0) return 9;
  uint64_t one_leaf[2] = {1, 1};
  uint32_t lim[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, got[2];
  uint8_t c[2] = {3, 2}, st[2], two_ext[64];
  memcpy(two_ext, ext, 32);
  memcpy(two_ext + 32, ext, 32);
  if (ql_draw_counts(q, 2, one_leaf, two_ext, lim, c, got, st) != 0) return 10;
  if (st[0] != quota::OVER || st[1] != quota::OVER || got[0] != lim[0] || got[1] != lim[1]) return 11;   // rank 3 pushes the 2 over
  c[0] = 2;
  if (ql_draw_counts(q, 1, one_leaf, two_ext, lim, c, got, st) != 0 || st[0] != quota::OK || got[0] != 0xFFFFFFFDu) return 12;
  uint32_t used;
  uint8_t inside;
  ql_used(q, 1, one_leaf, ext, &used, &inside);
  if (!inside || used != 0xFFFFFFFFu) return 13;
  uint32_t r[2];
  ql_issue_counts(0xFFFFFFFDu, 0, 3, 0xFFFFFFFFu, r);
  if (r[1] != quota::OVER || r[0] != 0xFFFFFFFFu) return 14;
  ql_issue_counts(0xFFFFFFFFu, 0xFFFFFFFFu, 255, 0xFFFFFFFFu, r);
  if (r[1] != quota::OVER) return 15;
  ql_free(q);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: quota_counts_main <case file>\n");
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
      if (bytes) memset(to, 0, bytes);
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
    std::vector<uint8_t> ext(32 * c), flags(c), got_flags(c), counts(c);
    std::vector<uint32_t> limits(c), want(c), got(c);
    if (kc[0] == 0) {
      uint64_t refused;
      take(ext.data(), 32 * c);
      take(&refused, 8);
      if (short_file) break;
      if ((uint64_t)ql_set_epochs(q, ext.data(), c) != refused) {
        printf("step %llu: set_epochs of %zu: the model says refused = %llu\n", (unsigned long long)step, c, (unsigned long long)refused);
        return 1;
      }
      continue;
    }
    if (kc[0] != 2 && kc[0] != 3) {
      printf("step %llu: unknown kind %llu\n", (unsigned long long)step, (unsigned long long)kc[0]);
      return 2;
    }
    take(leaf.data(), 8 * c);
    take(ext.data(), 32 * c);
    if (kc[0] == 3) take(limits.data(), 4 * c), take(counts.data(), c);
    take(want.data(), 4 * c);
    take(flags.data(), c);
    if (short_file) break;
    if (kc[0] == 3) {
      if (ql_draw_counts(q, c, leaf.data(), ext.data(), limits.data(), counts.data(), got.data(), got_flags.data()) != 0) {
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
  const int edge = edges();
  if (edge != 0) {
    printf("the edge calls went wrong at check %d\n", edge);
    return 1;
  }
  printf("ok %zu\n", judged);
  return 0;
}
