// Nullifier log: every rate-limiting share seen in the epochs of a relay's window, keyed by its nullifier, and the
// verdict on each new one -- the first sight of a nullifier, the same message again, or a second message of one member,
// whose identity secret the two shares give away (compute_id_secret / recover_id_secret, protocol/slashing.rs:12-100).
// Everything the kernels of nullifier_log.hip inline is here, and there is no HIP call in here: a plain C++ compiler
// builds the same source for the CPU tests (tests/host/nullifierlog.cpp, tests/host/nullifierretire.cpp).
//
// Layout.  A share is 128 bytes, nullifier | x | y | external_nullifier, four canonical little-endian Fr.  Record `id`
// (every observed share gets one, repeats included; its sequence number until a retire, see below) is row `id` of:
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
// Retiring.  retire(E), E a set of 1 .. 64 external nullifiers, removes every record whose external nullifier is in E:
// the epochs that have left a relay's window go, the ones still open stay.  The survivors keep their arrival order,
// their tags and their sequence numbers, and from then on every observe returns the statuses, secrets and first tags a
// fresh log with the same seed would return had it been fed only the surviving shares, with their stored tags, in
// their original order (what differs from that fresh log: default tags, and the counters that run over the life of
// the handle).  "The first record with this nullifier" is the first SURVIVING one: a nullifier seen under two external
// nullifiers survives under the one that was not retired, and that record becomes the first.  `capacity` counts
// records held, so a retire hands back the room of what it removed.
//
// Retaining.  retain(W), W a set of 1 .. 64 external nullifiers, is the same removal with the sense of the set turned
// round: every record whose external nullifier is NOT in W goes, however many different ones those carry -- what a relay
// asks for when its window moves or its clock has jumped (relay.h: the epoch window).  Everything said of a retire holds
// for it word for word; the two share every pass and differ in nlog::keeps alone, which is told the sense.
//
// Rows and sequence numbers.  A record's sequence number is its arrival index since the last clear; it never changes
// and is not issued again before the next clear, and a share observed without a tag is tagged with it (a retire does
// not lower that counter).  The table holds ROWS.  Until the first retire that removes something, row == sequence
// number and nothing is stored for it; from then on a fourth record array, seqs[row], ascending, names them, and
// find_seq() is the way from a sequence number to its row.  The survivors are moved in order, so the lowest row with a
// key is still the earliest arrival with it, which is all insert() and judge() ask of an id.
//
// The device keeps a spare set of the record arrays from a log's first retire on (the move is not in place: a
// destination row can be another lane's source) and swaps it with the live set: record memory doubles then, from 136
// to 2 * 144 bytes per record of capacity, plus 5 bytes per record of keep marks and positions.  A log that never
// retires pays nothing.  retire() below is the one-thread form, which can move in place.
//
// The atomics are a policy type A, so that the kernels and the CPU build compile the same source:
//   A::cas(p, expect, v)  compare-and-swap, returns what was there      A::min(p, v)  atomic minimum
//   A::load(p)            the entry as some lane has written it
// nullifier_log.hip passes device atomics of agent scope (the table is shared by all XCDs); SeqAtomics is the one-thread
// form (the host baseline and the model of the tests), StdAtomics is std::atomic for the threaded CPU test.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

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

#if defined(__HIPCC__)
// the kernels' form (nullifier_log.hip, relay.hip): agent scope, the table is shared by all XCDs
struct DevAtomics {
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;   // on failure the exchange has put the entry found there
  }
  static __device__ __forceinline__ void min(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// ---- retiring
constexpr uint32_t RETIRE_MAX = 64;
struct RetireSet {   // the external nullifiers of one retire or retain call, canonical; duplicates do no harm
  Row32 e[RETIRE_MAX];
  uint32_t k;
  uint32_t retain = 0;   // the sense of the set: 0, a retire, the records under e[] go; 1, a retain, only they stay
};

// is ext one of set[0 .. k)?  (the roots check of relay::gate and its window check are the same compare)
RLN_HD bool among(const Row32& ext, const Row32* set, uint32_t k) {
  bool hit = false;
  for (uint32_t j = 0; j < k; j++) hit |= same(ext, set[j]);
  return hit;
}

// the keep predicate.  A retire (retain false): the record stays unless its external nullifier is one of set[0 .. k).
// A retain: it stays only if it is one of them.
RLN_HD bool keeps(const Row32& ext, const Row32* set, uint32_t k, bool retain = false) { return among(ext, set, k) == retain; }

// sequence number -> row: binary search over the ascending seqs[0 .. count); `count` if no record carries it
RLN_HD uint64_t find_seq(const uint64_t* seqs, uint64_t count, uint64_t seq) {
  uint64_t lo = 0, hi = count;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (seqs[mid] < seq) lo = mid + 1;
    else hi = mid;
  }
  return lo < count && seqs[lo] == seq ? lo : count;
}

// the record arrays as something a retire may write
struct Records {
  Row32* nul;
  Row96* rest;
  uint64_t* tags;
  uint64_t* seqs;
};

// The sequential retire: mark, move, rebuild on one thread.  Row i goes to row (kept rows below i) <= i, so in
// ascending order the move is in place here; the device, one lane per record, moves into a spare set.  Then the table
// is emptied and the survivors are inserted again, which leaves the lowest surviving row of each key in the key's
// slot.  Returns the number of survivors; *distinct: taken slots, *longest: the longest walk of the rebuild.
// With E.retain set this is the sequential retain: the same passes over the other side of the set.
template <class A>
inline uint64_t retire(const Records& R, uint32_t* table, uint64_t slots, uint64_t seed, uint64_t count, const RetireSet& E,
                       uint64_t* distinct, uint32_t* longest) {
  uint64_t kept = 0;
  for (uint64_t i = 0; i < count; i++) {
    if (!keeps(R.rest[i].ext, E.e, E.k, E.retain != 0)) continue;
    if (kept != i) {
      R.nul[kept] = R.nul[i];
      R.rest[kept] = R.rest[i];
      R.tags[kept] = R.tags[i];
      R.seqs[kept] = R.seqs[i];
    }
    kept++;
  }
  if (kept == count) return kept;   // nothing removed: the table stands, *distinct and *longest are not touched
  *distinct = 0;
  *longest = 0;
  for (uint64_t s = 0; s < slots; s++) table[s] = EMPTY;
  const View L{R.nul, R.rest, R.tags, table, slots, seed};
  for (uint64_t id = 0; id < kept; id++) {
    const uint32_t walk = insert<A>(L, (uint32_t)id);
    if (walk > *longest) *longest = walk;
  }
  for (uint64_t s = 0; s < slots; s++) *distinct += table[s] != EMPTY;
  return kept;
}

// one field element, and one share's four: canonical?
inline bool element_is_canonical(const uint8_t le[32]) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) {
    const uint8_t* b = le + 4 * i;
    w[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  }
  return !limbs_geq(w, FrParams::MOD);
}
inline bool share_is_canonical(const uint8_t share_le[128]) {
  for (int k = 0; k < 4; k++)
    if (!element_is_canonical(share_le + 32 * k)) return false;
  return true;
}

// The checks of a retain, which need no log and no device.  Returns the empty string, or the text of the refusal.
inline std::string retain_refusal(const uint8_t* external_nullifiers_le, size_t k) {
  if (k > 0 && !external_nullifiers_le) return "nullifier log: retain was given a null pointer for k > 0 external nullifiers";
  if (k == 0) return "nullifier log: a retain of no external nullifiers would remove every record: use clear";
  if (k > RETIRE_MAX)
    return "nullifier log: retain takes at most " + std::to_string(RETIRE_MAX) + " external nullifiers a call, not " + std::to_string(k);
  for (size_t j = 0; j < k; j++)
    if (!element_is_canonical(external_nullifiers_le + 32 * j))
      return "nullifier log: external nullifier " + std::to_string(j) + " of the retain is not canonical (>= r)";
  return std::string();
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
  void clear();   // everything goes: empty table, no records, sequence numbers from 0 again, the same seed
  // k external nullifiers of 32 bytes, 0 <= k <= RETIRE_MAX: every record under one of them goes (the semantics are at
  // the top of this file); returns how many.  Refused before anything is enqueued, the log left as it was: a null
  // pointer with k > 0, k > RETIRE_MAX, an element >= r.  k = 0 and a set no record matches return 0 and move nothing.
  // A failed allocation leaves the log as it was.
  uint64_t retire(size_t k, const uint8_t* external_nullifiers_le);
  // k external nullifiers of 32 bytes, 1 <= k <= RETIRE_MAX: every record under none of them goes; returns how many.
  // The passes, the spare arrays, the counters of retire_info() and the behaviour on a failed allocation are retire's.
  // Refused before anything is enqueued (nlog::retain_refusal), the log left as it was.
  uint64_t retain(size_t k, const uint8_t* external_nullifiers_le);
  // by sequence number; one that was retired and one that was never issued are two different errors
  void get(uint64_t seq, uint8_t share_le[128], uint64_t* tag);
  uint64_t home_slot(const uint8_t nullifier_le[32]) const;   // host only
  void info(uint64_t out[8]);
  void retire_info(uint64_t out[8]);   // include/rln_amd.h: rlnamd_nullifier_log_retire_info

  // ---- for the relay step (relay.hip), whose kernels write a call's shares straight into rows [count, count + m) and
  // then run the insert and judge passes over them on the log's stream.  The caller holds the handle's mutex from
  // relay_rows() to relay_commit(); nothing of the log's host state changes in between.
  struct RelayRows {
    nlog::Records rows;   // seqs: null while the log is dense (row == sequence number)
    nlog::View view;
    uint64_t count, capacity, next_seq;
    void* stream;         // a hipStream_t
    int device;
  };
  RelayRows relay_rows();
  int device() const;   // fixed when the log is made: needs no lock
  // what observe() does on the host behind its passes: m rows taken, the call's longest walk, its NEW shares
  void relay_commit(uint64_t m, uint32_t walk, uint64_t fresh);
};

// test support (rlnamd_probe_log_positions): the position pass of a retire on buffers of its own -- keep: n bytes,
// pos: n exclusive counts of the non-zero bytes before each, *kept: their number
void probe_log_positions(const uint8_t* keep, size_t n, uint32_t* pos, uint64_t* kept);

}  // namespace rlnamd
