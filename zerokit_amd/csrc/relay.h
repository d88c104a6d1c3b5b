// Relay step: what happens to one message between its proof's verdict and the nullifier log's answer, per item.
// Everything the kernels of relay.hip inline is here, and there is no HIP call in here: a plain C++ compiler builds the
// same source for the CPU tests (tests/host/relay.cpp), the split of nullifier_log.h / nullifier_log.hip.
//
// A message is its proof's public values, in the verifier's order (n_values rows of 8 canonical little-endian words):
//   single (n_values == 5)                        y | root | nullifier | x | external_nullifier
//   multi  (n_values == 3 k + 3, k = max_out)     ys[k] | root | nullifiers[k] | x | external_nullifier | selector_used[k]
//
// The epoch window.  A relay may hold a window W of 1 .. 64 external nullifiers, the epochs it relays for.  A message
// that passes the three checks and whose external nullifier is not in W gets BAD_EPOCH and no share: a member's quota
// is per external nullifier, so a sender who proves under one the relay does not follow would otherwise never be
// rate-limited, and its records would never be retired.  Setting the window retains it in the log
// (NullifierLogDev::retain), so: everything a relay records lies in its window, and after every set_epochs the log
// holds only the window.  No window (k = 0): any external nullifier, the step as it was.
//
// Three passes, each one lane per message and each a kernel of its own, so that none reads what a lane of the same
// kernel writes:
//   gate   the verdict -- the first failing check in the order proof, root, signal (rln/src/public.rs:725-771), then
//          the epoch window -- and the message's share count: 1 for an accepted single proof, the number of selectors
//          equal to 1 for an accepted multi proof, 0 otherwise
//   emit   behind an exclusive sum of the counts (log_scan.h): the shares into rows [first, first + count) of the log's
//          record arrays, nullifier | x | y | external_nullifier as nullifier_log.h lays a record out, in slot order
//   fold   behind the log's insert and judge passes over the new rows: of the message's shares the first status in the
//          order SPAM, FOREIGN, DUPLICATE, NEW, and the secret and first tag of the lowest slot that has it
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nullifier_log.h"

namespace rlnamd {
namespace relay {

using nlog::Records;
using nlog::Row32;
using nlog::Row96;

constexpr uint8_t OK = 0, BAD_PROOF = 1, BAD_ROOT = 2, BAD_SIGNAL = 3, BAD_EPOCH = 4;
constexpr uint8_t SKIPPED = 4;   // RLNAMD_SHARE_SKIPPED: no share of this message was recorded
constexpr uint32_t ROOTS_MAX = 64;
constexpr uint32_t EPOCHS_MAX = nlog::RETIRE_MAX;   // a window is what one retain call takes
constexpr uint32_t SLOTS_MAX = 255;   // a share count is a byte

// where the values of a message are
struct Layout {
  uint32_t n_values, k;   // k message slots
  uint32_t multi;
  RLN_HD uint32_t y(uint32_t s) const { return multi ? s : 0; }
  RLN_HD uint32_t root() const { return multi ? k : 1; }
  RLN_HD uint32_t nullifier(uint32_t s) const { return multi ? k + 1 + s : 2; }
  RLN_HD uint32_t x() const { return multi ? 2 * k + 1 : 3; }
  RLN_HD uint32_t ext() const { return multi ? 2 * k + 2 : 4; }
  RLN_HD uint32_t selector(uint32_t s) const { return 2 * k + 3 + s; }   // multi only
};
// the layout of a circuit with n_values public values and max_out message slots; false: not one of the two above
inline bool layout_for(uint64_t n_values, uint64_t max_out, Layout* out) {
  if (max_out == 0 || max_out > SLOTS_MAX) return false;
  if (n_values == 5 && max_out == 1) {
    *out = Layout{5, 1, 0};
    return true;
  }
  if (n_values == 3 * max_out + 3) {
    *out = Layout{(uint32_t)n_values, (uint32_t)max_out, 1};
    return true;
  }
  return false;
}

RLN_HD Row32 value(const uint32_t* vals, uint32_t index) {
  Row32 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.w[i] = vals[8 * index + i];
  return r;
}
// a selector element: 0, 1, or 2 for anything else
RLN_HD uint32_t selector_of(const uint32_t* vals, uint32_t index) {
  uint32_t high = 0;
#pragma unroll
  for (int i = 1; i < 8; i++) high |= vals[8 * index + i];
  const uint32_t low = vals[8 * index];
  return (high == 0 && low <= 1) ? low : 2;
}
RLN_HD bool slot_used(const Layout& L, const uint32_t* vals, uint32_t s) { return !L.multi || selector_of(vals, L.selector(s)) == 1; }

struct Gate {
  uint8_t verdict, count;
};
// vals: the message's values; ok: the verifier's verdict; x: hash_to_field of its signal; roots: n_roots accepted roots
// (0: any root, ffi_verify_with_roots' rule); window: n_window external nullifiers (0: no window, any of them)
RLN_HD Gate gate(const Layout& L, const uint32_t* vals, uint8_t ok, const Row32& x, const Row32* roots, uint32_t n_roots,
                 const Row32* window = nullptr, uint32_t n_window = 0) {
  Gate g{OK, 0};
  uint32_t used = 0;
  bool selectors = true;
  if (L.multi) {
    for (uint32_t s = 0; s < L.k; s++) {
      const uint32_t v = selector_of(vals, L.selector(s));
      selectors &= v <= 1;
      used += v == 1;
    }
  } else {
    used = 1;
  }
  if (!ok || !selectors) {
    g.verdict = BAD_PROOF;
    return g;
  }
  if (n_roots) {
    const Row32 root = value(vals, L.root());
    bool hit = false;
    for (uint32_t j = 0; j < n_roots; j++) hit |= nlog::same(root, roots[j]);
    if (!hit) {
      g.verdict = BAD_ROOT;
      return g;
    }
  }
  if (!nlog::same(value(vals, L.x()), x)) {
    g.verdict = BAD_SIGNAL;
    return g;
  }
  if (n_window && !nlog::among(value(vals, L.ext()), window, n_window)) {
    g.verdict = BAD_EPOCH;
    return g;
  }
  g.count = (uint8_t)used;
  return g;
}

// The shares of a message whose gate gave `count` > 0, into rows [first_row, first_row + count); share j of it has
// sequence number first_seq + j, which is its tag when the call brought none, and goes into seqs[] once the log
// stores them (R.seqs non-null).  Nothing is written at or beyond row `capacity`.
RLN_HD void emit(const Layout& L, const uint32_t* vals, uint32_t count, uint64_t first_row, uint64_t first_seq, bool tagged,
                 uint64_t tag, const Records& R, uint64_t capacity) {
  const Row32 x = value(vals, L.x()), ext = value(vals, L.ext());
  uint32_t j = 0;
  for (uint32_t s = 0; s < L.k && j < count; s++) {
    if (!slot_used(L, vals, s)) continue;
    const uint64_t row = first_row + j;
    if (row >= capacity) return;   // (not reached: the step asks for room for the worst case before it starts)
    R.nul[row] = value(vals, L.nullifier(s));
    Row96 rest;
    rest.x = x;
    rest.y = value(vals, L.y(s));
    rest.ext = ext;
    R.rest[row] = rest;
    R.tags[row] = tagged ? tag : first_seq + j;
    if (R.seqs) R.seqs[row] = first_seq + j;
    j++;
  }
}

struct Picked {
  uint8_t status;
  Row32 secret;
  uint64_t first_tag;
};
// the order in which a message's shares speak for it: SPAM, FOREIGN, DUPLICATE, NEW; anything else (nlog::LOST) first of
// all, so that the host sees it
RLN_HD uint32_t rank_of(uint8_t status) {
  return status == nlog::SPAM ? 1 : status == nlog::FOREIGN ? 2 : status == nlog::DUPLICATE ? 3 : status == nlog::NEW ? 4 : 0;
}
// status, secret, first: what the judge pass wrote for the message's `count` shares, in slot order
RLN_HD Picked fold(uint32_t count, const uint8_t* status, const Row32* secret, const uint64_t* first) {
  Picked p;
  p.status = SKIPPED;
  p.first_tag = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) p.secret.w[i] = 0;
  uint32_t best = 5;
  for (uint32_t j = 0; j < count; j++) {
    const uint32_t r = rank_of(status[j]);
    if (r < best) {   // strictly: the lowest slot with the winning status
      best = r;
      p.status = status[j];
      p.secret = secret[j];
      p.first_tag = first[j];
    }
  }
  return p;
}

// The checks of a step that need no object and no device.  Returns null, or the text of the refusal.
inline const char* check_arguments(size_t n, const void* proofs, const void* values_le, const void* signals,
                                   const uint64_t* offsets, const void* xs_le, const void* roots_le, size_t n_roots,
                                   const void* verdict, const void* status) {
  if (n == 0) return nullptr;
  if (!proofs || !values_le || !verdict || !status) return "relay step: null pointer for n > 0 messages";
  if (n_roots > ROOTS_MAX) return "relay step: at most 64 roots (RLNAMD_RELAY_ROOTS_MAX)";
  if (n_roots && !roots_le) return "relay step: null roots for n_roots > 0";
  const bool triple = signals || offsets;
  if (triple && xs_le) return "relay step: both signals and xs_le were given, a step takes one of them";
  if (!triple && !xs_le) return "relay step: neither signals nor xs_le were given";
  return nullptr;
}

// The checks of set_epochs, which need no object and no device: k = 0 switches the window off and looks at nothing,
// anything else is what a retain of the set would refuse.  Returns the empty string, or the text of the refusal.
inline std::string epochs_refusal(const uint8_t* external_nullifiers_le, size_t k) {
  if (k == 0) return std::string();
  if (external_nullifiers_le && k > EPOCHS_MAX)
    return "relay: a window holds at most " + std::to_string(EPOCHS_MAX) + " external nullifiers (RLNAMD_RELAY_EPOCHS_MAX), not " +
           std::to_string(k);
  return nlog::retain_refusal(external_nullifiers_le, k);
}

}  // namespace relay

class GpuVerifier;
struct HasherDev;

// The relay step as a device-resident object (relay.hip).  It borrows a verifier, a log and (optionally) a hasher, all
// on one device, and owns the buffers between them.  Not thread-safe, and it takes none of the borrowed objects' locks:
// the C ABI's handle (capi.cpp) holds its own mutex and theirs for the length of a step.  Every method throws
// rlnamd::Error.
struct RelayDev {
  struct Impl;
  Impl* d = nullptr;
  // lanes: 0 | 1 | 8 as GpuVerifier::verify.  Refuses objects on different devices and a circuit whose public values are
  // neither of the two layouts above.
  // flags: OPTIMISTIC -- a chunk that would run a lane per proof takes the verifier's combined check
  // (GpuVerifier::relay_enqueue_combined / relay_settle) unless a cool-down lasts; OPTIMISTIC_TEAMS with it -- the team
  // chunks too, the rule of GpuVerifier::verify_optimistic(team_checks).  Every other chunk is the exact pass.
  static constexpr int OPTIMISTIC = 1, OPTIMISTIC_TEAMS = 2;
  // null, or why `flags` is refused (include/rln_amd.h: rlnamd_relay_new_ex)
  static const char* check_flags(int flags) {
    if (flags & ~(OPTIMISTIC | OPTIMISTIC_TEAMS)) return "unknown flag bits";
    if ((flags & OPTIMISTIC_TEAMS) && !(flags & OPTIMISTIC)) return "RLNAMD_RELAY_OPTIMISTIC_TEAMS needs RLNAMD_RELAY_OPTIMISTIC";
    return nullptr;
  }
  RelayDev(GpuVerifier& verifier, uint64_t max_out, NullifierLogDev& log, HasherDev* hasher, int lanes, int flags = 0);
  ~RelayDev();
  RelayDev(const RelayDev&) = delete;
  RelayDev& operator=(const RelayDev&) = delete;
  // include/rln_amd.h: rlnamd_relay_step.  Everything it refuses it refuses before anything is enqueued, with the log,
  // the hasher and the verifier untouched.
  void step(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values, const uint8_t* signals,
            size_t signals_len, const uint64_t* offsets, const uint8_t* xs_le, const uint8_t* roots_le, size_t n_roots,
            const uint64_t* tags, uint8_t* verdict, uint8_t* status, uint8_t* secrets_le, uint64_t* first_tag);
  // include/rln_amd.h: rlnamd_relay_set_epochs.  k >= 1: the log retains the set, and only then is it the window;
  // returns what the retain removed.  k = 0: no window from now on, nothing removed.  A refused call (relay::
  // epochs_refusal) and a retain that throws leave the window and the log as they were.  The caller holds the log's lock.
  // retain = false installs the set alone: for a caller that has run the log's retain itself (ffi.cpp, whose window
  // may be older than its device relay).
  uint64_t set_epochs(size_t k, const uint8_t* external_nullifiers_le, bool retain = true);
  size_t epochs(uint8_t out_le[32 * relay::EPOCHS_MAX]) const;   // the window, in the order it was given; returns k
  void info(uint64_t out[8]);
};

}  // namespace rlnamd
