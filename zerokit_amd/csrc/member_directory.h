// Member directory: who sits at which leaf of a dense device tree, kept beside that tree.  It registers members from
// (index, identity commitment, limit) events and writes their rate commitments Poseidon(idc, limit) into the tree, it
// resolves identity secrets (what a nullifier log gives away for a double signaller) to leaves, and it slashes them.
// Everything the kernels of member_directory.hip inline is here, and there is no HIP call in here: a plain C++ compiler
// builds the same source for the CPU tests (tests/host/memberdir.cpp).
//
// ---- The contract.  A directory D belongs to one dense tree T and covers the leaf indices [0, capacity), 1 <= capacity
// <= min(2^depth, 2^31).  Per index it holds a state, FREE or LIVE, and for a LIVE index the member's identity commitment
// idc (canonical Fr) and its limit (uint32 >= 1).  At most one LIVE index carries a given idc.  D starts empty.  D writes
// only the leaves of the indices it registers or removes; a leaf written behind its back through the tree's own setters
// is not noticed.  D is not persisted: a directory made over a tree that already holds leaves is empty, and registering
// the same events again rebuilds it -- they write the same leaves, so the root does not move.
//
// register(n, indices, idcs, limits) -> status[n].  Refused as a whole, before anything is written, D and T untouched: a
// null pointer with n > 0, an index >= capacity, an index that occurs twice in the call, an idc >= r, a limit of 0.
// Otherwise the call is a SET of requests and its outcome does not depend on their order:
//   OCCUPIED  the index was LIVE before the call (checked first);
//   KNOWN     not OCCUPIED, and the idc was LIVE somewhere before the call, or another request of the call that is not
//             OCCUPIED carries the same idc at a lower index;
//   OK        otherwise: the index becomes LIVE with (idc, limit) and its leaf becomes Poseidon(idc, Fr(limit)).
// An OCCUPIED request never blocks another request with the same idc at a free index.  A call with duplicate idcs is
// NOT what every split of it gives: inside a call the lowest index wins, across calls the first call wins.
//
// find(n, idcs) -> FOUND with the live index and its limit, else UNKNOWN with index NO_INDEX and limit 0.
// resolve(n, secrets, take) -> the same for Poseidon(secret); take may be null (all); take[i] == 0 gives SKIPPED, the
//   secret is not read; a taken secret >= r refuses the call.
// remove(n, indices) -> REMOVED, or VACANT (the index was not LIVE, nothing is written); the refusals follow register's
//   index rules.  A removed index is FREE, its leaf is the tree's default leaf, and its idc may be registered again, at
//   the same index or another.
// slash(n, secrets, take) -> resolve's outputs, then remove of the distinct FOUND indices: exactly that composition.
// get(n, indices) -> live, idc, limit per index; repeats allowed; FREE rows read as zero.
//
// ---- Layout.  Rows by leaf index: idc[capacity] 32 B, limit[capacity] 4 B, state[capacity] 1 B (37 MiB at 2^20).  The
// table is open addressing over nlog::slots_for(capacity) 32-bit entries with linear probing from the home slot, a keyed
// hash (SipHash-1-3 under the directory's seed) of the idc: registrations arrive from outside, and a sender who does not
// know the seed cannot aim keys at one slot.  An entry is EMPTY, a leaf index, or TOMB for a removed member.  Walks pass
// TOMB and inserts never take it, so "the first slot of a key's sequence that is EMPTY or holds the key" stays one slot
// per key, as in nullifier_log.h.  TOMB slots accumulate: before a call that could leave more than slots / 2 entries
// taken the table is rebuilt from the LIVE rows, after which taken = live <= capacity <= slots / 2.
//
// ---- The passes of a register call.  Every compare reads rows written by an EARLIER pass, never by a lane of the same:
//   rows     OCCUPIED if state[index] is LIVE; else the row's idc is written and its state becomes CANDIDATE.  The
//            indices of a call are distinct, so nothing races.
//   insert   every candidate walks from its key's home slot: CAS(EMPTY -> index) takes a slot; a slot whose row has the
//            same key and was LIVE before the call ends the walk; a slot held by a candidate of this call with the same
//            key is lowered with an atomic minimum.
//   commit   every candidate walks to its key's slot.  Entry == own index: OK, the state becomes LIVE and the limit is
//            written (the kernel then writes the leaf).  Anything else: KNOWN, and the lane takes its row back.  A row
//            that is taken back is never in the table, so no other lane reads it.
// The probe loops keep the two properties nullifier_log.h states for its own:
//   * Every loop's trip count is bounded by `slots`.  At most slots / 2 entries are taken (the rebuild rule above), so a
//     walk reaches an EMPTY slot -- or its own key -- long before that.
//   * No lane ever waits for a value another lane will write.  A lane reads an entry once, acts on what it found and
//     moves on or is done: there is no spinning, no lock and no flag.
//
// The atomics are nlog's policy types: nlog::SeqAtomics (one thread: the host baseline and the model of the host tests),
// nlog::StdAtomics (the threaded CPU test), nlog::DevAtomics (the kernels, agent scope).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "nullifier_log.h"

namespace rlnamd {
namespace mdir {

using nlog::EMPTY;
using nlog::Row32;

constexpr uint32_t TOMB = 0xFFFFFFFEu;                 // a removed member's slot: passed by every walk, never taken
constexpr uint64_t MAX_CAPACITY = (uint64_t)1 << 31;   // leaf indices stay below TOMB
constexpr uint8_t FREE = 0, LIVE = 1, CANDIDATE = 2;   // CANDIDATE: only between the passes of one register call
constexpr uint8_t OK = 0, OCCUPIED = 1, KNOWN = 2;     // register
constexpr uint8_t PENDING = 254;                       // rows pass -> commit pass; never returned
constexpr uint8_t FOUND = 0, UNKNOWN = 1, SKIPPED = 2; // find, resolve, slash
constexpr uint8_t REMOVED = 0, VACANT = 1;             // remove
constexpr uint8_t LOST = 255;   // never produced: a candidate whose key is not on its walk (the host turns it into an error)
constexpr uint64_t NO_INDEX = ~(uint64_t)0;

struct View {
  Row32* idc;
  uint32_t* limit;
  uint8_t* state;
  uint32_t* table;
  uint64_t capacity;
  uint64_t slots;   // a power of two
  uint64_t seed;
};

RLN_HD Row32 zero_row() {
  Row32 z;
#pragma unroll
  for (int i = 0; i < 8; i++) z.w[i] = 0;
  return z;
}

// rows pass.  The indices of a call are distinct: no other lane touches row `index`.
RLN_HD uint8_t claim_row(const View& D, uint32_t index, const Row32& key) {
  if (D.state[index] == LIVE) return OCCUPIED;
  D.idc[index] = key;
  D.state[index] = CANDIDATE;
  return PENDING;
}

// insert pass, candidates only.  Returns the number of slots the walk looked at.
template <class A>
RLN_HD uint32_t insert(const View& D, uint32_t index) {
  const Row32 key = D.idc[index];
  uint64_t s = nlog::home_slot(key, D.seed, D.slots);
  for (uint64_t step = 0; step < D.slots; step++, s = (s + 1) & (D.slots - 1)) {
    const uint32_t old = A::cas(&D.table[s], EMPTY, index);
    if (old == EMPTY) return (uint32_t)step + 1;
    if (old == TOMB) continue;
    if (nlog::same(D.idc[old], key)) {
      // (the state was written by the rows pass or before the call: no lane of this pass changes it)
      if (D.state[old] == CANDIDATE) A::min(&D.table[s], index);
      return (uint32_t)step + 1;
    }
  }
  return (uint32_t)D.slots;   // (not reached: at most half of the slots are taken)
}

// a walk to the key's slot: the index found there, or EMPTY.  *walk: slots looked at.
template <class A>
RLN_HD uint32_t lookup(const View& D, const Row32& key, uint32_t* walk) {
  uint64_t s = nlog::home_slot(key, D.seed, D.slots);
  for (uint64_t step = 0; step < D.slots; step++, s = (s + 1) & (D.slots - 1)) {
    const uint32_t e = A::load(&D.table[s]);
    *walk = (uint32_t)step + 1;
    if (e == EMPTY) return EMPTY;
    if (e == TOMB) continue;
    if (nlog::same(D.idc[e], key)) return e;
  }
  return EMPTY;   // (not reached)
}

// commit pass, candidates only, behind the whole insert pass.  OK: the caller writes the leaf.
template <class A>
RLN_HD uint8_t commit(const View& D, uint32_t index, uint32_t limit, uint32_t* walk) {
  const Row32 key = D.idc[index];
  const uint32_t e = lookup<A>(D, key, walk);
  if (e == EMPTY) return LOST;   // (not reached: insert() has put the key on this walk)
  if (e == index) {
    D.limit[index] = limit;
    D.state[index] = LIVE;
    return OK;
  }
  D.idc[index] = zero_row();     // KNOWN: the row goes back (it is not in the table: nobody reads it)
  D.state[index] = FREE;
  return KNOWN;
}

struct Found {
  uint8_t status;
  uint64_t index;
  uint32_t limit;
};
template <class A>
RLN_HD Found find(const View& D, const Row32& key, uint32_t* walk) {
  const uint32_t e = lookup<A>(D, key, walk);
  if (e == EMPTY) return Found{UNKNOWN, NO_INDEX, 0};
  return Found{FOUND, e, D.limit[e]};
}

// remove pass.  The indices of a call are distinct; the lane looks for its own index, so it reads no other row.
// REMOVED: the caller writes the default leaf.
template <class A>
RLN_HD uint8_t remove(const View& D, uint32_t index, uint32_t* walk) {
  *walk = 0;
  if (D.state[index] != LIVE) return VACANT;
  const Row32 key = D.idc[index];
  uint64_t s = nlog::home_slot(key, D.seed, D.slots);
  for (uint64_t step = 0; step < D.slots; step++, s = (s + 1) & (D.slots - 1)) {
    const uint32_t e = A::cas(&D.table[s], index, TOMB);
    *walk = (uint32_t)step + 1;
    if (e == index || e == EMPTY) break;   // (EMPTY is not reached: a LIVE row is in the table)
  }
  D.idc[index] = zero_row();
  D.limit[index] = 0;
  D.state[index] = FREE;
  return REMOVED;
}

// rebuild, behind a fill of the table with EMPTY: a LIVE row takes the first EMPTY slot of its walk (the keys of LIVE
// rows are distinct, so nothing is compared)
template <class A>
RLN_HD uint32_t reinsert(const View& D, uint32_t index) {
  if (D.state[index] != LIVE) return 0;
  uint64_t s = nlog::home_slot(D.idc[index], D.seed, D.slots);
  for (uint64_t step = 0; step < D.slots; step++, s = (s + 1) & (D.slots - 1))
    if (A::cas(&D.table[s], EMPTY, index) == EMPTY) return (uint32_t)step + 1;
  return (uint32_t)D.slots;   // (not reached)
}

// does a call that may take up to n more slots need the rebuild first?
RLN_HD bool needs_rebuild(uint64_t taken, uint64_t n, uint64_t slots) { return taken + n > slots / 2; }

// ------------------------------------------------------------------------------------------------ refusals
// The checks that need no directory and no device.  Each returns the empty string, or the text of the refusal.
inline std::string new_refusal(uint64_t capacity, uint64_t tree_depth) {
  if (capacity == 0) return "member directory: the capacity must be at least 1";
  if (capacity > MAX_CAPACITY) return "member directory: the capacity must be at most 2^31 leaves";
  if (tree_depth < 63 && capacity > ((uint64_t)1 << tree_depth))
    return "member directory: a capacity of " + std::to_string(capacity) + " is more than the 2^" + std::to_string(tree_depth) +
           " leaves of the tree";
  return std::string();
}

inline std::string indices_refusal(const char* call, size_t n, const uint64_t* indices, uint64_t capacity, bool distinct) {
  for (size_t i = 0; i < n; i++)
    if (indices[i] >= capacity)
      return std::string("member directory: index ") + std::to_string(indices[i]) + " of request " + std::to_string(i) + " of the " +
             call + " is outside a directory of " + std::to_string(capacity) + " leaves";
  if (distinct && n > 1) {
    std::vector<uint64_t> sorted(indices, indices + n);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < n; i++)
      if (sorted[i] == sorted[i - 1])
        return std::string("member directory: index ") + std::to_string(sorted[i]) + " occurs twice in the " + call;
  }
  return std::string();
}

inline std::string register_refusal(size_t n, const uint64_t* indices, const uint8_t* idcs_le, const uint32_t* limits,
                                    const uint8_t* status, uint64_t capacity) {
  if (n == 0) return std::string();
  if (!indices || !idcs_le || !limits || !status) return "member directory: register was given a null pointer for n > 0 requests";
  if (n >= ((uint64_t)1 << 32)) return "member directory: a register takes fewer than 2^32 requests, not " + std::to_string(n);
  const std::string bad = indices_refusal("register", n, indices, capacity, true);
  if (!bad.empty()) return bad;
  for (size_t i = 0; i < n; i++)
    if (!nlog::element_is_canonical(idcs_le + 32 * i))
      return "member directory: identity commitment " + std::to_string(i) + " of the register is not canonical (>= r)";
  for (size_t i = 0; i < n; i++)
    if (limits[i] == 0) return "member directory: request " + std::to_string(i) + " of the register has a limit of 0";
  return std::string();
}

inline std::string find_refusal(size_t n, const uint8_t* idcs_le, const uint8_t* status, const uint64_t* index, const uint32_t* limit) {
  if (n == 0) return std::string();
  if (!idcs_le || !status || !index || !limit) return "member directory: find was given a null pointer for n > 0 requests";
  if (n >= ((uint64_t)1 << 32)) return "member directory: a find takes fewer than 2^32 requests, not " + std::to_string(n);
  return std::string();
}

// `call`: "resolve" or "slash"
inline std::string resolve_refusal(const char* call, size_t n, const uint8_t* secrets_le, const uint8_t* take, const uint8_t* status,
                                   const uint64_t* index, const uint32_t* limit) {
  if (n == 0) return std::string();
  if (!secrets_le || !status || !index || !limit)
    return std::string("member directory: ") + call + " was given a null pointer for n > 0 secrets";
  if (n >= ((uint64_t)1 << 32))
    return std::string("member directory: a ") + call + " takes fewer than 2^32 secrets, not " + std::to_string(n);
  for (size_t i = 0; i < n; i++)
    if ((!take || take[i]) && !nlog::element_is_canonical(secrets_le + 32 * i))
      return "member directory: secret " + std::to_string(i) + " of the " + call + " is not canonical (>= r)";
  return std::string();
}

inline std::string remove_refusal(size_t n, const uint64_t* indices, const uint8_t* status, uint64_t capacity) {
  if (n == 0) return std::string();
  if (!indices || !status) return "member directory: remove was given a null pointer for n > 0 requests";
  if (n >= ((uint64_t)1 << 32)) return "member directory: a remove takes fewer than 2^32 requests, not " + std::to_string(n);
  return indices_refusal("remove", n, indices, capacity, true);
}

inline std::string get_refusal(size_t n, const uint64_t* indices, const uint8_t* live, const uint8_t* idcs_le, const uint32_t* limits,
                               uint64_t capacity) {
  if (n == 0) return std::string();
  if (!indices || !live || !idcs_le || !limits) return "member directory: get was given a null pointer for n > 0 requests";
  if (n >= ((uint64_t)1 << 32)) return "member directory: a get takes fewer than 2^32 requests, not " + std::to_string(n);
  return indices_refusal("get", n, indices, capacity, false);
}

inline Row32 row_of(const uint8_t le[32]) {
  Row32 r;
  for (int i = 0; i < 8; i++) {
    const uint8_t* b = le + 4 * i;
    r.w[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  }
  return r;
}
inline void row_to(const Row32& r, uint8_t le[32]) {
  for (int i = 0; i < 32; i++) le[i] = (uint8_t)(r.w[i / 4] >> (8 * (i % 4)));
}

// ------------------------------------------------------------------------------------------ the sequential directory
// One thread, plain memory, the passes above in the order the device runs them: the host baseline and the model of the
// host tests.  It holds no tree and has no Poseidon: the leaves are the caller's business, and resolve() is given the
// commitments of its secrets (keys_le[i] = Poseidon(secret i), read only where the secret is taken).
// Every call returns the empty string, or the text of its refusal with the directory as it was.
struct SeqDirectory {
  uint64_t capacity, slots, seed;
  std::vector<Row32> idc;
  std::vector<uint32_t> limit, table;
  std::vector<uint8_t> state;
  uint64_t live = 0, taken = 0, rebuilds = 0, longest = 0, calls = 0;

  SeqDirectory(uint64_t capacity_, uint64_t seed_)
      : capacity(capacity_), slots(nlog::slots_for(capacity_)), seed(seed_), idc(capacity_, zero_row()), limit(capacity_, 0),
        table(slots, EMPTY), state(capacity_, FREE) {}
  View view() { return View{idc.data(), limit.data(), state.data(), table.data(), capacity, slots, seed}; }
  void walked(uint32_t w) {
    if (w > longest) longest = w;
  }
  void make_room(uint64_t n) {
    if (!needs_rebuild(taken, n, slots)) return;
    std::fill(table.begin(), table.end(), EMPTY);
    const View D = view();
    for (uint64_t i = 0; i < capacity; i++) walked(reinsert<nlog::SeqAtomics>(D, (uint32_t)i));
    taken = live;
    rebuilds++;
  }

  std::string do_register(size_t n, const uint64_t* indices, const uint8_t* idcs_le, const uint32_t* limits, uint8_t* status) {
    const std::string refused = register_refusal(n, indices, idcs_le, limits, status, capacity);
    if (!refused.empty()) return refused;
    calls++;
    make_room(n);
    const View D = view();
    for (size_t i = 0; i < n; i++) status[i] = claim_row(D, (uint32_t)indices[i], row_of(idcs_le + 32 * i));
    for (size_t i = 0; i < n; i++)
      if (status[i] == PENDING) walked(insert<nlog::SeqAtomics>(D, (uint32_t)indices[i]));
    for (size_t i = 0; i < n; i++) {
      if (status[i] != PENDING) continue;
      uint32_t w = 0;
      status[i] = commit<nlog::SeqAtomics>(D, (uint32_t)indices[i], limits[i], &w);
      walked(w);
      if (status[i] == OK) live++, taken++;
    }
    return std::string();
  }
  std::string do_find(size_t n, const uint8_t* idcs_le, uint8_t* status, uint64_t* index, uint32_t* lim) {
    const std::string refused = find_refusal(n, idcs_le, status, index, lim);
    if (!refused.empty()) return refused;
    calls++;
    lookup_keys(n, idcs_le, nullptr, status, index, lim);
    return std::string();
  }
  std::string do_resolve(size_t n, const uint8_t* secrets_le, const uint8_t* keys_le, const uint8_t* take, uint8_t* status,
                         uint64_t* index, uint32_t* lim, const char* call = "resolve") {
    const std::string refused = resolve_refusal(call, n, secrets_le, take, status, index, lim);
    if (!refused.empty()) return refused;
    calls++;
    lookup_keys(n, keys_le, take, status, index, lim);
    return std::string();
  }
  std::string do_remove(size_t n, const uint64_t* indices, uint8_t* status) {
    const std::string refused = remove_refusal(n, indices, status, capacity);
    if (!refused.empty()) return refused;
    calls++;
    drop(n, indices, status);
    return std::string();
  }
  std::string do_slash(size_t n, const uint8_t* secrets_le, const uint8_t* keys_le, const uint8_t* take, uint8_t* status,
                       uint64_t* index, uint32_t* lim, uint64_t* removed) {
    const std::string refused = do_resolve(n, secrets_le, keys_le, take, status, index, lim, "slash");
    if (!refused.empty()) return refused;
    std::vector<uint64_t> found;
    for (size_t i = 0; i < n; i++)
      if (status[i] == FOUND) found.push_back(index[i]);
    std::sort(found.begin(), found.end());
    found.erase(std::unique(found.begin(), found.end()), found.end());
    std::vector<uint8_t> st(found.size());
    drop(found.size(), found.data(), st.data());
    if (removed) *removed = found.size();
    return std::string();
  }
  std::string do_get(size_t n, const uint64_t* indices, uint8_t* live_out, uint8_t* idcs_le, uint32_t* limits) {
    const std::string refused = get_refusal(n, indices, live_out, idcs_le, limits, capacity);
    if (!refused.empty()) return refused;
    for (size_t i = 0; i < n; i++) {
      live_out[i] = state[indices[i]] == LIVE;
      row_to(idc[indices[i]], idcs_le + 32 * i);
      limits[i] = limit[indices[i]];
    }
    return std::string();
  }
  void info(uint64_t out[8]) const {
    out[0] = capacity, out[1] = live, out[2] = slots, out[3] = taken;
    out[4] = rebuilds, out[5] = longest, out[6] = calls, out[7] = 0;
  }

 private:
  void lookup_keys(size_t n, const uint8_t* keys_le, const uint8_t* take, uint8_t* status, uint64_t* index, uint32_t* lim) {
    const View D = view();
    for (size_t i = 0; i < n; i++) {
      Found f{SKIPPED, NO_INDEX, 0};
      if (!take || take[i]) {
        uint32_t w = 0;
        f = find<nlog::SeqAtomics>(D, row_of(keys_le + 32 * i), &w);
        walked(w);
      }
      status[i] = f.status, index[i] = f.index, lim[i] = f.limit;
    }
  }
  void drop(size_t n, const uint64_t* indices, uint8_t* status) {
    const View D = view();
    for (size_t i = 0; i < n; i++) {
      uint32_t w = 0;
      status[i] = remove<nlog::SeqAtomics>(D, (uint32_t)indices[i], &w);
      walked(w);
      if (status[i] == REMOVED) live--;
    }
  }
};

}  // namespace mdir

struct MerkleTreeDev;

// The directory as a device-resident object (member_directory.hip): rows and table in HBM beside the tree's nodes, pinned
// staging.  It BORROWS the tree, which must outlive it, and runs every pass on the tree's stream: that orders it against
// the tree's own calls and against the path gathers of proving by member with no extra event and no extra hardware queue.
// Not thread-safe: the C ABI's handle (capi.cpp) holds a mutex of its own and takes the tree handle's behind it for every
// call.  Every method throws rlnamd::Error; the refusals above come before anything is enqueued.
struct MemberDirectoryDev {
  struct Impl;
  Impl* d = nullptr;
  MemberDirectoryDev(MerkleTreeDev& tree, uint64_t capacity, uint64_t seed);   // seed 0: drawn from getrandom
  ~MemberDirectoryDev();
  MemberDirectoryDev(const MemberDirectoryDev&) = delete;
  MemberDirectoryDev& operator=(const MemberDirectoryDev&) = delete;
  void do_register(size_t n, const uint64_t* indices, const uint8_t* idcs_le, const uint32_t* limits, uint8_t* status);
  void find(size_t n, const uint8_t* idcs_le, uint8_t* status, uint64_t* index, uint32_t* limit);
  void resolve(size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status, uint64_t* index, uint32_t* limit);
  void slash(size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status, uint64_t* index, uint32_t* limit,
             uint64_t* removed);
  void remove(size_t n, const uint64_t* indices, uint8_t* status);
  void get(size_t n, const uint64_t* indices, uint8_t* live, uint8_t* idcs_le, uint32_t* limits);
  // [0] capacity [1] live members [2] table slots [3] slots taken, those of removed members included [4] table rebuilds
  // [5] longest walk of any call [6] calls [7] non-zero 16-byte words left in the staging that held secrets, device and
  // pinned (0 expected)
  void info(uint64_t out[8]);
  uint64_t capacity() const;
};

}  // namespace rlnamd
