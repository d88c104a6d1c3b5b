// Quota ledger: the message ids a signer has handed out, per member and external nullifier, and the draw that hands out
// the next ones -- the sending side's counterpart of the relay's epoch window (relay.h).  A second proof under one
// (external nullifier, member, message id) is two shares on one line, and every relay's k_relay_judge then recovers the
// member's identity secret; a service that signs for many members by leaf index (Prover::submit_members) keeps that
// from happening by drawing each proof's message id here.  The reference keeps no such state (zerokit leaves message ids
// to the caller); this is judged by the sequential text below, not by a reference binary.
// Everything the kernels of quota_ledger.hip inline is here, and there is no HIP call in here: a plain C++ compiler
// builds the same source for the CPU tests (tests/host/quota.cpp).
//
// State.  used[slot][leaf], max_epochs x 2^depth 32-bit counters: the next message id of member `leaf` under the external
// nullifier that holds `slot` of the window.  The window is up to max_epochs external nullifiers, each in a slot of its
// own; a slot that holds none has all its counters at zero.
//
// set_epochs(E).  An external nullifier of E that is in the window keeps its slot and its counters; one of the window
// that is not in E leaves, its slot is zeroed and free again; one of E that is new takes a free slot (the lowest), which
// may be one that has just been zeroed.  Duplicates in E count once.  An external nullifier that has left must not come
// back -- its counters are gone, and the ids drawn after its return would repeat the ids drawn before it left.
//
// draw.  Request i is (leaf_i, ext_i, limit_i), i = 0 .. n - 1, and its answer is closed-form:
//   ext_i not in the window                     NO_EPOCH; touches nothing
//   otherwise, with key (slot, leaf)            rank_i = the number of requests j < i of this call with the same key,
//                                               whatever their outcome; id_i = used + rank_i, `used` as it was before
//                                               the call; OK iff id_i < limit_i, else OVER
//   afterwards                                  used = 1 + the highest id issued for the key in this call; unchanged
//                                               if none was
// ids_out[i] = id_i for OK and limit_i otherwise (never a valid message id: the circuit's range check fails for it).  With one limit
// per member, as the protocol means it, the OK requests of a key are a prefix of its requests and this is drawing one by
// one in index order: OVER consumes nothing, and a call gives what any split of it into consecutive calls gives.  With
// differing limits for one member an id can be skipped (a request refused under a low limit still counts in the ranks
// behind it) but none is issued twice: ids issued in one call are used + distinct ranks, and the next call starts above
// the highest.
//
// The plan.  The ranks need the requests grouped by key with their order kept: a stable sort of (key, i) by key, then
// rank = position - position of the group's first.  Both the device and draw() below do exactly that; the device's sort is
// a radix sort of 8-bit digits over the leaf's bits and the slot's (DrawPlan), every pass three kernels and a scan, so
// that a call of n requests of ONE member and a call of n distinct members run the same passes over the same amount of
// data.
//
// draw_counts: blocks of ids, for the multi-message-id circuit, one proof of which uses up to max_out message slots.
// Request i is (leaf_i, ext_i, limit_i, count_i), count_i = 1 .. COUNT_MAX the number of ids it asks for:
//   ext_i not in the window                     NO_EPOCH; touches nothing
//   otherwise, with key (slot, leaf)            rank_i = the sum of count_j over the requests j < i of this call with the
//                                               same key, whatever their outcome; first_i = used + rank_i, `used` as it
//                                               was before the call; OK iff first_i + count_i <= limit_i (in 64 bits),
//                                               and the request then owns the ids first_i .. first_i + count_i - 1; else
//                                               OVER: a request is granted whole or not at all
//   afterwards                                  used = first + count of the key's last OK request of this call; unchanged
//                                               if there was none
// firsts_out[i] = first_i for OK and limit_i otherwise.  With every count 1 this is draw, word for word.  With one limit
// per member the OK requests of a key are a prefix of its requests: a later first is at least an earlier first + count,
// so once one request is over, all behind it are.  The blocks granted for a key, over any sequence of calls, are
// pairwise disjoint and each lies below its limit: within a call they are used + [rank_i, rank_i + count_i) with the
// ranks running sums of the counts, and the next call starts at or above the end of the last one granted.
// What does NOT carry over from draw: a refused request still counts in the ranks behind it, and here it counts with
// its whole block.  A request of 4 that is over pushes a request of 1 of the same member, later IN THE SAME CALL, over
// too, although one id was left -- the next call grants it.  So a call is not what every split of it into consecutive
// calls gives, one limit per member or not; only the all-ones case has that property.  Nothing is issued twice either
// way, and nothing above a limit.
// The plan is the one above with two more passes: the counts gathered into sorted order, and an exclusive sum over them
// (log_scan.h, as the bins are summed), so that rank = S[position] - S[position of the group's first].  n < 2^24
// requests of at most 255 ids keep every such sum below 2^32.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "nullifier_log.h"
#include "relay.h"

namespace rlnamd {
namespace quota {

using nlog::Row32;

constexpr uint8_t OK = 0, OVER = 1, NO_EPOCH = 2;
constexpr uint32_t EPOCHS_MAX = nlog::RETIRE_MAX;   // RLNAMD_RELAY_EPOCHS_MAX: a signer's window is a relay's
constexpr uint32_t DEPTH_MAX = 24;
constexpr uint32_t LEAF_BITS = 24;                  // a key is slot << 24 | leaf
constexpr uint32_t NO_SLOT = EPOCHS_MAX;            // the slot of a request outside the window: above every real one
constexpr uint32_t BLOCK = 256;                     // requests a workgroup (log_scan.h: LOG_LANES)
constexpr uint32_t DIGIT_BITS = 8, DIGITS = 1u << DIGIT_BITS;
constexpr uint32_t COUNT_MAX = relay::SLOTS_MAX;    // ids a request of draw_counts asks for: a count is a byte, as a share count is
constexpr uint64_t COUNTS_N_MAX = (uint64_t)1 << 24;   // requests a draw_counts call stays below: n x COUNT_MAX < 2^32
static_assert(COUNTS_N_MAX * COUNT_MAX < ((uint64_t)1 << 32), "the sums of a call's counts fit 32 bits");

// ---- the window
struct Window {
  Row32 e[EPOCHS_MAX];         // e[s]: the external nullifier in slot s, if bit s of `live` is set
  uint64_t live = 0;
  uint32_t order[EPOCHS_MAX];  // the slots in the order set_epochs was given them, duplicates once
  uint32_t k = 0;
};

// the slot of `ext` among the first `slots` of the window, or NO_SLOT
RLN_HD uint32_t slot_of(const Row32* e, uint64_t live, uint32_t slots, const Row32& ext) {
  uint32_t hit = NO_SLOT;
  for (uint32_t s = 0; s < slots; s++)
    if (((live >> s) & 1) && nlog::same(e[s], ext)) hit = s;   // (at most one slot holds an external nullifier)
  return hit;
}
RLN_HD uint32_t pack_key(uint32_t slot, uint32_t leaf) { return (slot << LEAF_BITS) | leaf; }
RLN_HD uint32_t key_slot(uint32_t key) { return key >> LEAF_BITS; }
RLN_HD uint32_t key_leaf(uint32_t key) { return key & ((1u << LEAF_BITS) - 1); }
// where a key's counter is, in max_epochs x 2^depth words
RLN_HD size_t counter_of(uint32_t key, uint32_t depth) { return ((size_t)key_slot(key) << depth) + key_leaf(key); }

// ---- the rule: rank -> id -> status
struct Issue {
  uint32_t id;      // what goes into ids_out
  uint8_t status;
};
RLN_HD Issue issue(uint32_t used, uint32_t rank, uint32_t limit) {
  const uint64_t id = (uint64_t)used + rank;
  Issue r;
  r.status = id < limit ? OK : OVER;
  r.id = id < limit ? (uint32_t)id : limit;
  return r;
}
// Behind the issue pass, at the last request of a group (sorted position `tail`): the group starts at `start`, and
// `last_ok` is 1 + the highest sorted position at or below `tail` whose request was OK (0: none so far).  Ids rise with
// the rank, so the group's highest id issued is the one of its last OK request.  Returns the counter's new value, or
// `used` when the group issued nothing.
RLN_HD uint32_t advance(uint32_t used, uint32_t start, uint32_t last_ok) {
  return last_ok > start ? used + (last_ok - 1 - start) + 1 : used;
}

// ---- the rule of draw_counts: rank (a sum of counts) -> first id -> status
RLN_HD Issue issue_counts(uint32_t used, uint32_t rank, uint32_t count, uint32_t limit) {
  const uint64_t first = (uint64_t)used + rank;
  const bool ok = first + count <= limit;   // 64 bits: used and limit may both be at 2^32 - 1
  Issue r;
  r.status = ok ? OK : OVER;
  r.id = ok ? (uint32_t)first : limit;
  return r;
}
// At the last request of a group, as advance(): `last_ok` is 1 + the highest sorted position of the group whose request
// was OK (at or below `start`: none), `rank_last` and `count_last` are that request's.  Firsts rise with the rank, so
// the group's last OK request owns its highest ids.  (No overflow: it was granted, so the sum is at most its limit.)
RLN_HD uint32_t advance_counts(uint32_t used, uint32_t start, uint32_t last_ok, uint32_t rank_last, uint32_t count_last) {
  return last_ok > start ? used + rank_last + count_last : used;
}

// ---- the plan of a draw
RLN_HD uint32_t scan_levels(size_t n) {   // log_scan.h: the levels of block sums above n items
  uint32_t levels = 0;
  do {
    n = (n + BLOCK - 1) / BLOCK;
    levels++;
  } while (n > 1);
  return levels;
}
struct DrawPlan {
  uint32_t passes;        // sort passes
  uint32_t shift[4];      // the bit each pass's digit starts at
  size_t blocks;          // workgroups of a pass: ceil(n / BLOCK)
  size_t bins;            // DIGITS * blocks: a pass's counts, digit-major
  uint32_t bin_levels;    // scan levels over the bins
  uint32_t rank_levels;   // scan levels over the n requests (group starts, last OK)
};
inline DrawPlan plan_for(size_t n, uint32_t depth) {
  DrawPlan P{};
  for (uint32_t b = 0; b < depth; b += DIGIT_BITS) P.shift[P.passes++] = b;   // the leaf's digits: 1 .. 3
  P.shift[P.passes++] = LEAF_BITS;                                            // the slot's: 0 .. NO_SLOT, seven bits
  P.blocks = (n + BLOCK - 1) / BLOCK;
  P.bins = (size_t)DIGITS * P.blocks;
  P.bin_levels = scan_levels(P.bins);
  P.rank_levels = scan_levels(n);
  return P;
}

// ---- refusals: the checks that need no object and no device.  Each returns the empty string or the text.
inline std::string new_refusal(size_t depth, size_t max_epochs) {
  if (depth < 1 || depth > DEPTH_MAX)
    return "quota ledger: the depth must be 1 .. " + std::to_string(DEPTH_MAX) + ", not " + std::to_string(depth);
  if (max_epochs < 1 || max_epochs > EPOCHS_MAX)
    return "quota ledger: max_epochs must be 1 .. " + std::to_string(EPOCHS_MAX) + " (RLNAMD_RELAY_EPOCHS_MAX), not " +
           std::to_string(max_epochs);
  return std::string();
}
inline std::string epochs_refusal(const uint8_t* external_nullifiers_le, size_t k, size_t max_epochs) {
  if (k == 0) return std::string();
  if (!external_nullifiers_le) return "quota ledger: set_epochs was given a null pointer for k > 0 external nullifiers";
  if (k > max_epochs)
    return "quota ledger: a window holds at most " + std::to_string(max_epochs) + " external nullifiers (max_epochs), not " +
           std::to_string(k);
  for (size_t j = 0; j < k; j++)
    if (!nlog::element_is_canonical(external_nullifiers_le + 32 * j))
      return "quota ledger: external nullifier " + std::to_string(j) + " of set_epochs is not canonical (>= r)";
  return std::string();
}
inline std::string draw_refusal(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                                const uint32_t* ids_out, const uint8_t* status, uint32_t depth, bool ids_wanted = true) {
  if (n == 0) return std::string();
  // (ids_wanted false: a held draw, whose ids stay on the device -- QuotaLedgerDev::draw_hold)
  if (!leaf_indices || !ext_le || !limits || (ids_wanted && !ids_out) || !status) return "quota ledger: draw was given a null pointer for n > 0 requests";
  if ((uint64_t)n >> 32) return "quota ledger: a draw takes fewer than 2^32 requests, not " + std::to_string(n);
  for (size_t i = 0; i < n; i++)
    if (leaf_indices[i] >> depth)
      return "quota ledger: leaf index " + std::to_string(leaf_indices[i]) + " of request " + std::to_string(i) +
             " is outside a ledger of depth " + std::to_string(depth);
  return std::string();
}
// one count, of request i: the text, or the empty string for 1 .. COUNT_MAX
inline std::string count_refusal(size_t i, uint64_t count) {
  if (count == 0) return "quota ledger: request " + std::to_string(i) + " of draw_counts asks for no id (a count is 1 .. " +
                         std::to_string(COUNT_MAX) + ")";
  if (count > COUNT_MAX)
    return "quota ledger: request " + std::to_string(i) + " of draw_counts asks for " + std::to_string(count) + " ids, more than " +
           std::to_string(COUNT_MAX);
  return std::string();
}
// draw_counts: the pointers first, then n -- before any array is read -- then what the arrays hold
inline std::string draw_counts_refusal(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                                       const uint8_t* counts, const uint32_t* firsts_out, const uint8_t* status, uint32_t depth,
                                       bool firsts_wanted = true) {
  if (n == 0) return std::string();
  if (!leaf_indices || !ext_le || !limits || (firsts_wanted && !firsts_out) || !status)
    return draw_refusal(n, leaf_indices, ext_le, limits, firsts_out, status, depth, firsts_wanted);
  if (!counts) return "quota ledger: draw_counts was given a null pointer for the counts of n > 0 requests";
  if ((uint64_t)n >= COUNTS_N_MAX) return "quota ledger: a draw by count takes fewer than 2^24 requests, not " + std::to_string(n);
  const std::string refused = draw_refusal(n, leaf_indices, ext_le, limits, firsts_out, status, depth, firsts_wanted);
  if (!refused.empty()) return refused;
  for (size_t i = 0; i < n; i++) {
    const std::string bad = count_refusal(i, counts[i]);
    if (!bad.empty()) return bad;
  }
  return std::string();
}

// The window after set_epochs(E), E checked (epochs_refusal).  *leaving: the slots whose counters are to be zeroed.
// SLOT ASSIGNMENT MUST STAY A PURE FUNCTION OF THE WINDOW HISTORY -- of `now`, E and max_epochs, and of nothing else (no
// clock, no address, no counter of calls).  The durable store (quota_store.h) journals E as set_epochs was given it and
// replays it through this function; the keys of the advance records behind it name slots, and they mean the same
// counters after a reopen only if replay hands every external nullifier the slot the live ledger gave it.
inline Window next_window(const Window& now, const uint8_t* external_nullifiers_le, size_t k, uint32_t max_epochs, uint64_t* leaving) {
  Window next;
  for (uint32_t s = 0; s < EPOCHS_MAX; s++) next.e[s] = now.e[s];
  std::vector<Row32> fresh;
  std::vector<int64_t> order;   // a slot, or -1 - (index into fresh)
  for (size_t j = 0; j < k; j++) {
    Row32 ext;
    memcpy(ext.w, external_nullifiers_le + 32 * j, 32);
    const uint32_t s = slot_of(now.e, now.live, max_epochs, ext);
    if (s != NO_SLOT) {
      if (!((next.live >> s) & 1)) order.push_back(s);
      next.live |= (uint64_t)1 << s;
      continue;
    }
    bool seen = false;
    for (const Row32& f : fresh) seen |= nlog::same(f, ext);
    if (seen) continue;
    order.push_back(-1 - (int64_t)fresh.size());
    fresh.push_back(ext);
  }
  *leaving = now.live & ~next.live;
  uint32_t free_slot = 0;
  std::vector<uint32_t> given(fresh.size());
  for (size_t f = 0; f < fresh.size(); f++) {   // (k <= max_epochs distinct elements: the slots suffice)
    while ((next.live >> free_slot) & 1) free_slot++;
    next.e[free_slot] = fresh[f];
    next.live |= (uint64_t)1 << free_slot;
    given[f] = free_slot;
  }
  for (int64_t o : order) next.order[next.k++] = o >= 0 ? (uint32_t)o : given[(size_t)(-1 - o)];
  return next;
}

// ---- the sequential ledger: the meaning of every call, on one thread
struct SeqLedger {
  uint32_t depth, max_epochs;
  Window window;
  std::vector<uint32_t> used;   // max_epochs << depth
  uint64_t draws = 0, issued = 0, over = 0, no_epoch = 0;
  SeqLedger(uint32_t depth_, uint32_t max_epochs_) : depth(depth_), max_epochs(max_epochs_), used((size_t)max_epochs_ << depth_, 0) {}

  std::string set_epochs(const uint8_t* external_nullifiers_le, size_t k) {
    const std::string refused = epochs_refusal(external_nullifiers_le, k, max_epochs);
    if (!refused.empty()) return refused;
    uint64_t leaving = 0;
    window = next_window(window, external_nullifiers_le, k, max_epochs, &leaving);
    for (uint32_t s = 0; s < max_epochs; s++)
      if ((leaving >> s) & 1) std::fill(used.begin() + ((size_t)s << depth), used.begin() + ((size_t)(s + 1) << depth), 0u);
    return std::string();
  }
  size_t epochs(uint8_t* out_le) const {
    for (uint32_t j = 0; j < window.k; j++) memcpy(out_le + 32 * j, window.e[window.order[j]].w, 32);
    return window.k;
  }
  std::string draw(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, uint32_t* ids_out,
                   uint8_t* status) {
    const std::string refused = draw_refusal(n, leaf_indices, ext_le, limits, ids_out, status, depth);
    if (!refused.empty()) return refused;
    if (n == 0) return std::string();
    std::vector<uint32_t> key(n), at(n);
    for (size_t i = 0; i < n; i++) {
      Row32 ext;
      memcpy(ext.w, ext_le + 32 * i, 32);
      key[i] = pack_key(slot_of(window.e, window.live, max_epochs, ext), (uint32_t)leaf_indices[i]);
      at[i] = (uint32_t)i;
    }
    std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint32_t start = 0, last_ok = 0;
    for (size_t j = 0; j < n; j++) {
      const uint32_t i = at[j], k = key[i];
      if (j == 0 || key[at[j - 1]] != k) start = (uint32_t)j;
      if (key_slot(k) == NO_SLOT) {
        status[i] = NO_EPOCH;
        ids_out[i] = limits[i];
        no_epoch++;
        continue;
      }
      uint32_t& counter = used[counter_of(k, depth)];
      const Issue r = issue(counter, (uint32_t)j - start, limits[i]);
      status[i] = r.status;
      ids_out[i] = r.id;
      if (r.status == OK) last_ok = (uint32_t)j + 1, issued++;
      else over++;
      if (j + 1 == n || key[at[j + 1]] != k) counter = advance(counter, start, last_ok);
    }
    draws++;
    return std::string();
  }
  // draw with blocks of ids: the same sort, S the running sum of the sorted counts.  `issued` counts ids.
  std::string draw_counts(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, const uint8_t* counts,
                          uint32_t* firsts_out, uint8_t* status) {
    const std::string refused = draw_counts_refusal(n, leaf_indices, ext_le, limits, counts, firsts_out, status, depth);
    if (!refused.empty()) return refused;
    if (n == 0) return std::string();
    std::vector<uint32_t> key(n), at(n);
    for (size_t i = 0; i < n; i++) {
      Row32 ext;
      memcpy(ext.w, ext_le + 32 * i, 32);
      key[i] = pack_key(slot_of(window.e, window.live, max_epochs, ext), (uint32_t)leaf_indices[i]);
      at[i] = (uint32_t)i;
    }
    std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint32_t start = 0, last_ok = 0, S = 0, S_start = 0, rank_last = 0, count_last = 0;
    for (size_t j = 0; j < n; S += counts[at[j]], j++) {
      const uint32_t i = at[j], k = key[i];
      if (j == 0 || key[at[j - 1]] != k) start = (uint32_t)j, S_start = S;
      if (key_slot(k) == NO_SLOT) {
        status[i] = NO_EPOCH;
        firsts_out[i] = limits[i];
        no_epoch++;
        continue;
      }
      uint32_t& counter = used[counter_of(k, depth)];
      const Issue r = issue_counts(counter, S - S_start, counts[i], limits[i]);
      status[i] = r.status;
      firsts_out[i] = r.id;
      if (r.status == OK) last_ok = (uint32_t)j + 1, rank_last = S - S_start, count_last = counts[i], issued += counts[i];
      else over++;
      if (j + 1 == n || key[at[j + 1]] != k) counter = advance_counts(counter, start, last_ok, rank_last, count_last);
    }
    draws++;
    return std::string();
  }
};

}  // namespace quota

// The ledger as a device-resident object (quota_ledger.hip): the counters in HBM, a non-blocking stream of its own and
// pinned staging.  It lives on the device that is current when it is made.  Not thread-safe: the C ABI's handle
// (capi.cpp) holds a mutex and serialises the calls on one ledger.  Every method throws rlnamd::Error.
struct QuotaLedgerDev {
  struct Impl;
  Impl* d = nullptr;
  QuotaLedgerDev(size_t depth, size_t max_epochs);   // quota::new_refusal
  // The ledger on a directory (quota_store.h): created when the directory is empty or absent, otherwise reopened -- the
  // window and every counter at or above everything ever issued -- or refused with the store's text: damage that
  // would lower a counter, another depth or max_epochs, a directory another object holds.  From then on
  //   draw, draw_counts         the kernels, then the draw's delta (the counters it moved, absolute values) copied back,
  //                             appended and fdatasynced, and ONLY THEN ids and statuses into the caller's arrays.  A
  //                             draw that granted nothing appends and syncs nothing.  A failed append fails the call:
  //                             the caller's arrays untouched, the block wiped, the counters advanced (ids burnt)
  //   draw_hold(_counts)        the same, durable before it returns
  //   set_epochs                the window record appended and synced, then the window applied
  //   the destructor            compacts if the journal holds records, then closes
  // journal_max_bytes: the journal's size behind which the call that crossed it compacts; 0: max(1 MiB, snapshot bytes).
  QuotaLedgerDev(const char* dir, size_t depth, size_t max_epochs, uint64_t journal_max_bytes);
  void compact();                             // the next generation's snapshot and an empty journal; throws without a store
  void store_info(uint64_t out[8]) const;     // include/rln_amd.h: rlnamd_quota_store_info; all zero without a store
  ~QuotaLedgerDev();                                 // zeroes the counters before they are freed
  QuotaLedgerDev(const QuotaLedgerDev&) = delete;
  QuotaLedgerDev& operator=(const QuotaLedgerDev&) = delete;
  // Refused (quota::epochs_refusal) before anything is enqueued, the ledger left as it was.  A HIP error behind the
  // checks is not a refusal: the external nullifiers that leave are out of the window then, the new ones not in it.
  void set_epochs(size_t k, const uint8_t* external_nullifiers_le);
  size_t epochs(uint8_t out_le[32 * quota::EPOCHS_MAX]) const;   // the window in the order it was given, duplicates once
  // Refused (quota::draw_refusal) before anything is enqueued, the ledger left as it was.  Who signs how often is as
  // secret as who proves: the staged requests, the sort's keys and every other per-call word, device and pinned, are
  // overwritten before draw returns, on error paths too.
  void draw(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, uint32_t* ids_out, uint8_t* status);
  // draw with a block of counts[i] ids a request (the text at the top).  Refused (quota::draw_counts_refusal) before
  // anything is enqueued; the same passes plus a gather and a sum over the counts; wiped as draw wipes.  info()'s
  // `issued` counts ids: the counts of the granted requests.
  void draw_counts(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, const uint8_t* counts,
                   uint32_t* firsts_out, uint8_t* status);
  // the counters of n (member, external nullifier) pairs: used_out[i], and in_window[i] = 0 with used_out[i] = 0 for an
  // external nullifier outside the window (diagnostics and tests: one small copy per pair)
  void used(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, uint32_t* used_out, uint8_t* in_window);
  void info(uint64_t out[8]);   // include/rln_amd.h: rlnamd_quota_info
  int device() const;

  // ---- for proving with drawn ids (Prover::submit_members_drawn), whose batches read a draw's ids where the draw left
  // them.  draw_hold is draw with two differences: only the statuses come back, and the call's block stays on the
  // device -- ids[0 .. n) valid, the ledger's stream idle -- until release(), which overwrites it as draw does.  Nothing
  // else may be called on the ledger in between; the caller holds the handle's mutex from draw_hold to release.  A reader
  // on another stream orders itself against `stream` with events.  held_ids: a slice of the ids to the host, for a batch
  // that stages its inputs there (one small copy).
  struct Held {
    const uint32_t* ids;   // on the device
    const uint8_t* status; // on the device, beside them
    void* stream;          // a hipStream_t
    int device;
    const uint8_t* counts = nullptr;   // draw_hold_counts: the requests' counts on the device (ids: each block's first id)
  };
  Held draw_hold(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, uint8_t* status);
  // draw_counts held the same way (Prover::submit_members_drawn_counts): held_ids gives the firsts, release() wipes
  Held draw_hold_counts(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, const uint8_t* counts,
                        uint8_t* status);
  void held_ids(size_t first, size_t count, uint32_t* out);
  void release();
  // ids[0 .. count) into field element `slot` of `count` rows of `row_words` 32-bit words each, on stream `on` (a
  // hipStream_t): the message id of staged input row i becomes ids[i], canonical, the seven words above it zero -- where
  // status[i] is OK.  A request that was refused gets REFUSED_WORD in all eight words: no field element (>= r), so the
  // witness interpreter refuses the row (WERR_INPUT_RANGE) and the batch yields an error code for it, not a proof.
  // (Its limit would NOT do: the interpreter evaluates the circuit's range check without asserting it, and the row
  // would come back as an invalid proof with error 0.)
  static constexpr uint32_t REFUSED_WORD = 0xFFFFFFFFu;
  static void fill_rows(const uint32_t* ids, const uint8_t* status, size_t count, uint32_t* rows, size_t row_words, uint32_t slot,
                        void* on);
  // The multi-message-id form: row i has max_out message slots from field element `msg_slot` on and, where has_sel, as
  // many selectors from `sel_slot` on.  A granted request of counts[i] ids: messageId[k] = firsts[i] + k and selector 1
  // for k < counts[i], both 0 above.  A refused one: REFUSED_WORD in all eight words of EVERY message slot, selectors 0.
  // fill_row_counts is the rule for one row, shared by the kernel and the host route of the prover.
  RLN_HD static void fill_row_counts(uint32_t* row, bool granted, uint32_t first, uint32_t count, uint32_t msg_slot, uint32_t sel_slot,
                                     bool has_sel, uint32_t max_out) {
    for (uint32_t k = 0; k < max_out; k++) {
      uint32_t* id = row + (size_t)(msg_slot + k) * 8;
      const bool used = granted && k < count;
      id[0] = granted ? (used ? first + k : 0) : REFUSED_WORD;
      for (int w = 1; w < 8; w++) id[w] = granted ? 0 : REFUSED_WORD;
      if (!has_sel) continue;
      uint32_t* sel = row + (size_t)(sel_slot + k) * 8;
      sel[0] = used ? 1 : 0;
      for (int w = 1; w < 8; w++) sel[w] = 0;
    }
  }
  static void fill_rows_counts(const uint32_t* firsts, const uint8_t* status, const uint8_t* counts, size_t count, uint32_t* rows,
                               size_t row_words, uint32_t msg_slot, uint32_t sel_slot, bool has_sel, uint32_t max_out, void* on);
  int depth() const;
};

}  // namespace rlnamd
