// CPU build of the nullifier log (zerokit_amd/csrc/nullifier_log.h: the insert and judge passes the kernels inline),
// for tests/test_nullifier_log_host.py and, as the one-thread host baseline, tools/nullifier_log_throughput.py.  Built
// with g++: the header makes no HIP call.  threads = 0 runs both passes on the calling thread over the sequential
// policy; threads >= 1 runs each pass on that many std::threads over the std::atomic policy, share i on thread
// i mod threads, so that neighbouring shares -- the ones that collide -- are always in different hands.
// tests/host/nullifierlog_main.cpp includes this file for the sanitizer programs.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "nullifier_log.h"

namespace {

using namespace rlnamd::nlog;

struct HostLog {
  uint64_t capacity, slots, seed, count = 0, longest = 0;
  std::vector<Row32> nul;
  std::vector<Row96> rest;
  std::vector<uint64_t> tags;
  std::vector<uint32_t> table;
  HostLog(uint64_t capacity_, uint64_t seed_)
      : capacity(capacity_), slots(slots_for(capacity_)), seed(seed_), nul(capacity_), rest(capacity_), tags(capacity_),
        table(slots_for(capacity_), EMPTY) {}
  View view() { return View{nul.data(), rest.data(), tags.data(), table.data(), slots, seed}; }

  template <class A>
  void passes(uint32_t first_id, uint32_t n, uint32_t lo, uint32_t stride, bool judging, uint8_t* status, uint8_t* secrets,
              uint64_t* first_tag, uint32_t* walk) {
    const View L = view();
    for (uint32_t i = lo; i < n; i += stride) {
      if (!judging) {
        *walk = std::max(*walk, insert<A>(L, first_id + i));
        continue;
      }
      const Verdict v = judge<A>(L, first_id + i);
      status[i] = v.status;
      if (secrets) memcpy(secrets + 32 * i, v.secret.w, 32);
      if (first_tag) first_tag[i] = L.tags[v.first];
      *walk = std::max(*walk, v.walk);
    }
  }

  // 0: done; 1: n does not fit; 2: a field element >= r
  int observe(size_t n, const uint8_t* shares, const uint64_t* tg, uint8_t* status, uint8_t* secrets, uint64_t* first_tag,
              int threads) {
    if (n > capacity - count) return 1;
    for (size_t i = 0; i < n; i++)
      if (!share_is_canonical(shares + 128 * i)) return 2;
    for (size_t i = 0; i < n; i++) {
      memcpy(nul[count + i].w, shares + 128 * i, 32);
      memcpy(&rest[count + i], shares + 128 * i + 32, 96);
      tags[count + i] = tg ? tg[i] : count + i;
    }
    const uint32_t first_id = (uint32_t)count, n32 = (uint32_t)n;
    for (int judging = 0; judging < 2; judging++) {   // the two kernels: every insert is done before any verdict
      if (threads <= 0) {
        uint32_t walk = 0;
        passes<SeqAtomics>(first_id, n32, 0, 1, judging, status, secrets, first_tag, &walk);
        longest = std::max<uint64_t>(longest, walk);
        continue;
      }
      std::vector<uint32_t> walks(threads, 0);
      std::vector<std::thread> pool;
      for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t]() {
          passes<StdAtomics>(first_id, n32, (uint32_t)t, (uint32_t)threads, judging, status, secrets, first_tag, &walks[t]);
        });
      for (auto& th : pool) th.join();
      for (uint32_t w : walks) longest = std::max<uint64_t>(longest, w);
    }
    count += n;
    return 0;
  }
};

}  // namespace

extern "C" {

void* nl_new(uint64_t capacity, uint64_t seed) { return new HostLog(capacity, seed); }
void nl_free(void* l) { delete (HostLog*)l; }
int nl_observe(void* l, size_t n, const uint8_t* shares, const uint64_t* tags, uint8_t* status, uint8_t* secrets,
               uint64_t* first_tag, int threads) {
  return ((HostLog*)l)->observe(n, shares, tags, status, secrets, first_tag, threads);
}
uint64_t nl_home_slot(void* l, const uint8_t key[32]) {
  Row32 k;
  memcpy(k.w, key, 32);
  return home_slot(k, ((HostLog*)l)->seed, ((HostLog*)l)->slots);
}
void nl_clear(void* l) {
  HostLog* h = (HostLog*)l;
  std::fill(h->table.begin(), h->table.end(), EMPTY);
  h->count = 0;
}
void nl_info(void* l, uint64_t out[4]) {
  HostLog* h = (HostLog*)l;
  out[0] = h->capacity;
  out[1] = h->count;
  out[2] = h->slots;
  out[3] = h->longest;
}
// how many entries of the table are taken, and whether each names a record whose key hashes onto a walk that reaches it
// without an EMPTY slot on the way (the invariant of open addressing); returns the number of taken entries, or -1
int64_t nl_check_table(void* l) {
  HostLog* h = (HostLog*)l;
  int64_t taken = 0;
  for (uint64_t s = 0; s < h->slots; s++) {
    const uint32_t id = h->table[s];
    if (id == EMPTY) continue;
    taken++;
    if (id >= h->count) return -1;
    for (uint64_t w = home_slot(h->nul[id], h->seed, h->slots); w != s; w = (w + 1) & (h->slots - 1))
      if (h->table[w] == EMPTY || same(h->nul[h->table[w]], h->nul[id])) return -1;
  }
  return taken;
}

}  // extern "C"
