// Nullifier log: every rate-limiting share seen in an epoch, keyed by its nullifier, and the verdict on each new one --
// the first sight of a nullifier, the same message again, or a second message of one member, whose identity secret the
// two shares give away (compute_id_secret / recover_id_secret, protocol/slashing.rs:12-100).  Everything the kernels of
// nullifier_log.hip inline is here, and there is no HIP call in here: a plain C++ compiler builds the same source for
// the CPU tests (tests/host/nullifierlog.cpp).
//
// Layout.  A share is 128 bytes, nullifier | x | y | external_nullifier, four canonical little-endian Fr.  Record `id`
// (the sequence number of the share: every observed share gets one, repeats included) is row `id` of three arrays:
//   nul[id]   32 B   the key, in an array of its own: a probe's key compare reads one row
//   rest[id]  96 B   x | y | external_nullifier
//   tags[id]   8 B   the caller's name for the message
// The table is open addressing over `slots` 32-bit entries, slots = max(16, smallest power of two >= 2 * capacity);
// EMPTY or a record id; linear probing with wrap-around from the home slot, a keyed hash (SipHash-1-3 under the log's
// seed) of the nullifier: shares may reach the log unverified, and a sender who does not know the seed cannot aim keys
// at one slot.
//
// One slot per key.  insert() walks from the home slot and at each slot tries CAS(EMPTY -> id).  A slot that is taken
// holds a record id, whose key is compared: equal keys settle there with atomicMin, different keys move on.  Equal keys
// walk the same sequence of slots and a slot is never emptied, so the first slot of that sequence that is EMPTY or holds
// the key is the same for all of them from the moment one of them takes it: a key owns exactly one slot, and after the
// insert pass that slot holds the lowest id that ever carried the key.  judge() runs in a later pass, walks to that slot
// and compares the share with record f found there.
//
// The atomics are a policy type A, so that the kernels and the CPU build compile the same source:
//   A::cas(p, expect, v)  compare-and-swap, returns what was there      A::min(p, v)  atomic minimum
//   A::load(p)            the entry as some lane has written it
// nullifier_log.hip passes device atomics of agent scope (the table is shared by all XCDs); SeqAtomics is the one-thread
// form (the host baseline and the model of the tests), StdAtomics is std::atomic for the threaded CPU test.
#pragma once
#include <stdint.h>

#include "field.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <atomic>
#endif

namespace rlnamd {
namespace nlog {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint64_t MAX_CAPACITY = (uint64_t)1 << 31;   // ids stay below EMPTY
constexpr uint8_t NEW = 0, DUPLICATE = 1, SPAM = 2, FOREIGN = 3;
constexpr uint8_t LOST = 255;   // never produced: a share whose key is not in the table (the host turns it into an error)

struct alignas(16) Row32 {
  uint32_t w[8];
};
struct alignas(16) Row96 {
  Row32 x, y, ext;
};

struct View {
  const Row32* nul;
  const Row96* rest;
  const uint64_t* tags;
  uint32_t* table;
  uint64_t slots;   // a power of two
  uint64_t seed;
};

RLN_HD uint64_t slots_for(uint64_t capacity) {
  uint64_t s = 16;
  while (s < 2 * capacity) s <<= 1;
  return s;
}

RLN_HD bool same(const Row32& a, const Row32& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.w[i] ^ b.w[i];
  return o == 0;
}

// SipHash-1-3 of the 32 key bytes (four 64-bit little-endian words) under (seed, a second word spun off the seed)
RLN_HD uint64_t rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
RLN_HD void sipround(uint64_t& v0, uint64_t& v1, uint64_t& v2, uint64_t& v3) {
  v0 += v1; v1 = rotl64(v1, 13); v1 ^= v0; v0 = rotl64(v0, 32);
  v2 += v3; v3 = rotl64(v3, 16); v3 ^= v2;
  v0 += v3; v3 = rotl64(v3, 21); v3 ^= v0;
  v2 += v1; v1 = rotl64(v1, 17); v1 ^= v2; v2 = rotl64(v2, 32);
}
RLN_HD uint64_t key_hash(const Row32& key, uint64_t seed) {
  uint64_t k1 = seed + 0x9E3779B97F4A7C15ull;   // splitmix64 of the seed
  k1 = (k1 ^ (k1 >> 30)) * 0xBF58476D1CE4E5B9ull;
  k1 = (k1 ^ (k1 >> 27)) * 0x94D049BB133111EBull;
  k1 ^= k1 >> 31;
  uint64_t v0 = seed ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = seed ^ 0x6c7967656e657261ull,
           v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint64_t m = (uint64_t)key.w[2 * i] | ((uint64_t)key.w[2 * i + 1] << 32);
    v3 ^= m;
    sipround(v0, v1, v2, v3);
    v0 ^= m;
  }
  const uint64_t len = (uint64_t)32 << 56;
  v3 ^= len;
  sipround(v0, v1, v2, v3);
  v0 ^= len;
  v2 ^= 0xff;
  sipround(v0, v1, v2, v3);
  sipround(v0, v1, v2, v3);
  sipround(v0, v1, v2, v3);
  return v0 ^ v1 ^ v2 ^ v3;
}
RLN_HD uint64_t home_slot(const Row32& key, uint64_t seed, uint64_t slots) { return key_hash(key, seed) & (slots - 1); }

// one thread, plain memory: the sequential form
struct SeqAtomics {
  static RLN_HD uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static RLN_HD void min(uint32_t* p, uint32_t v) {
    if (v < *p) *p = v;
  }
  static RLN_HD uint32_t load(const uint32_t* p) { return *p; }
};
#if !defined(__HIP_DEVICE_COMPILE__)
// host threads: the table entries taken as std::atomic (same size and alignment as the plain word)
struct StdAtomics {
  static_assert(sizeof(std::atomic<uint32_t>) == sizeof(uint32_t), "the table is read as std::atomic<uint32_t>");
  static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    reinterpret_cast<std::atomic<uint32_t>*>(p)->compare_exchange_strong(expect, v, std::memory_order_relaxed);
    return expect;   // on failure compare_exchange_strong has put the entry found there
  }
  static void min(uint32_t* p, uint32_t v) {
    std::atomic<uint32_t>* a = reinterpret_cast<std::atomic<uint32_t>*>(p);
    uint32_t cur = a->load(std::memory_order_relaxed);
    // (each failed exchange means another thread has lowered the entry: it only falls, and never below 0)
    while (v < cur && !a->compare_exchange_weak(cur, v, std::memory_order_relaxed)) {
    }
  }
  static uint32_t load(const uint32_t* p) {
    return reinterpret_cast<const std::atomic<uint32_t>*>(p)->load(std::memory_order_relaxed);
  }
};
#endif

// The probe loops below have two properties by construction:
//   * Every loop's trip count is bounded by `slots`.  The table is at most half full (slots >= 2 * capacity, one slot
//     per KEY, at most `capacity` records), so a walk reaches an EMPTY slot -- or its own key -- long before that.
//   * No lane ever waits for a value another lane will write.  A lane reads an entry once, acts on what it found and
//     moves on or is done: there is no spinning, no lock and no flag.  The records a compare reads were written by the
//     copy that preceded the kernel, never by a lane of it.
// Record `id` must be in nul[] before the call.  Returns the number of slots the walk looked at.
template <class A>
RLN_HD uint32_t insert(const View& L, uint32_t id) {
  const Row32 key = L.nul[id];
  uint64_t s = home_slot(key, L.seed, L.slots);
  for (uint64_t step = 0; step < L.slots; step++, s = (s + 1) & (L.slots - 1)) {
    const uint32_t old = A::cas(&L.table[s], EMPTY, id);
    if (old == EMPTY) return (uint32_t)step + 1;
    if (same(L.nul[old], key)) {
      A::min(&L.table[s], id);
      return (uint32_t)step + 1;
    }
  }
  return (uint32_t)L.slots;   // (not reached: the table is at most half full)
}

struct Verdict {
  uint8_t status;
  uint32_t first;    // record f: the lowest id that carries the share's nullifier
  uint32_t walk;     // slots looked at
  Row32 secret;      // a0 for SPAM, else zero
};

// Every share of the call has been through insert() in an EARLIER pass.
template <class A>
RLN_HD Verdict judge(const View& L, uint32_t id) {
  Verdict v;
  v.status = LOST;
  v.first = id;
  v.walk = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) v.secret.w[i] = 0;
  const Row32 key = L.nul[id];
  uint64_t s = home_slot(key, L.seed, L.slots);
  uint32_t f = EMPTY;
  for (uint64_t step = 0; step < L.slots; step++, s = (s + 1) & (L.slots - 1)) {
    const uint32_t e = A::load(&L.table[s]);
    v.walk = (uint32_t)step + 1;
    if (e == EMPTY) return v;   // (not reached: insert() has put the key on this walk)
    if (e == id || same(L.nul[e], key)) {
      f = e;
      break;
    }
  }
  if (f == EMPTY) return v;     // (not reached)
  v.first = f;
  if (f == id) {
    v.status = NEW;
    return v;
  }
  const Row96 mine = L.rest[id], first = L.rest[f];
  if (!same(first.ext, mine.ext)) {
    v.status = FOREIGN;         // recover_id_secret's ExternalNullifierMismatch
    return v;
  }
  if (same(first.x, mine.x)) {
    v.status = DUPLICATE;       // the same message again, or compute_id_secret's DivisionByZero
    return v;
  }
  // the line through (x_f, y_f) and (x, y): a1 = (y_f - y) / (x_f - x), a0 = y_f - x_f a1   (slashing.rs:12-36)
  const Fr xf = Fr::from_canonical(first.x.w), yf = Fr::from_canonical(first.y.w);
  const Fr a1 = (yf - Fr::from_canonical(mine.y.w)) * (xf - Fr::from_canonical(mine.x.w)).inv();
  (yf - xf * a1).to_canonical(v.secret.w);
  v.status = SPAM;
  return v;
}

// one share's four field elements: all canonical?
inline bool share_is_canonical(const uint8_t share_le[128]) {
  for (int k = 0; k < 4; k++) {
    uint32_t w[8];
    for (int i = 0; i < 8; i++) {
      const uint8_t* b = share_le + 32 * k + 4 * i;
      w[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    if (limbs_geq(w, FrParams::MOD)) return false;
  }
  return true;
}

}  // namespace nlog

// The log as a device-resident object (nullifier_log.hip): records and table in HBM, a non-blocking stream of its own and
// pinned staging.  It lives on the device that is current when it is made.  Not thread-safe: the C ABI's handle
// (capi.cpp) holds a mutex and serialises the calls on one log; different logs do not wait for each other.
// Every method throws rlnamd::Error.
struct NullifierLogDev {
  struct Impl;
  Impl* d = nullptr;
  NullifierLogDev(uint64_t capacity, uint64_t seed);   // 1 <= capacity <= 2^31; seed 0: drawn from getrandom
  ~NullifierLogDev();
  NullifierLogDev(const NullifierLogDev&) = delete;
  NullifierLogDev& operator=(const NullifierLogDev&) = delete;
  // n shares of 128 bytes; tags: n, or null for the sequence numbers; status: n; secrets_le (n * 32) and first_tag (n)
  // may be null.  Refused before anything is enqueued, the log left as it was: a null pointer with n > 0, n larger than
  // the room left, a field element >= r.
  void observe(size_t n, const uint8_t* shares_le, const uint64_t* tags, uint8_t* status, uint8_t* secrets_le,
               uint64_t* first_tag);
  void clear();   // a new epoch: empty table, no records, the same seed
  void get(uint64_t seq, uint8_t share_le[128], uint64_t* tag);
  uint64_t home_slot(const uint8_t nullifier_le[32]) const;   // host only
  void info(uint64_t out[8]);
};

}  // namespace rlnamd
