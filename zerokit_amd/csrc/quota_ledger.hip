// The quota ledger on the device: the kernels over quota_ledger.h and the QuotaLedgerDev object.
//
// One draw() call: a host check, the requests (leaf, limit, external nullifier) copied into the call's block, then on the
// ledger's stream
//   k_quota_key                 key[i] = slot << 24 | leaf, the slot looked up in the window (in LDS, as k_relay_gate
//                               holds its roots); a request outside the window gets the slot above all others
//   per sort pass (DrawPlan: one 8-bit digit of the leaf's bits or the slot's, least significant first)
//     k_quota_count             bins[digit][block] = the block's requests with that digit
//     k_scan_up / k_scan_down   where each (digit, block) starts in the output (log_scan.h)
//     k_quota_scatter           (key, i) to that start plus the request's place among the block's requests of the same
//                               digit, in lane order: the pass is stable
//   k_quota_heads               mark[j] = j where sorted position j starts a group of equal keys
//   k_max_up / k_max_down       start[j] = the running maximum of the marks: where j's group starts; rank = j - start[j]
//   k_quota_issue               id and status by quota::issue, written to the request's own index; ok[j] = j + 1 if granted
//   k_max_up / k_max_down       last[j] = the running maximum of ok: the last granted position at or below j
//   k_quota_advance             the last lane of each group stores the group's counter (quota::advance)
// then one copy back of ids and statuses, one memset over the whole block and one stream wait.
// draw_counts() is the same call with blocks of ids: behind the sort
//   k_quota_weights             w[j] = the count of the request at sorted position j
//   k_scan_up / k_scan_down     S[j] = the counts before j (log_scan.h, as the bins are summed: no look-back)
// and k_quota_issue_counts / k_quota_advance_counts in the place of the two kernels above, with rank = S[j] - S[start[j]]
// and quota::issue_counts / advance_counts as the rule.  Sort, heads and both running maxima are the same kernels.
// The rule of nullifier_log.hip holds: passes are ordered by kernel boundaries only, and no lane waits for, or reads,
// what another lane of the same kernel writes.  The issue pass reads the counters, the advance pass behind it writes
// them, one lane per key.  Nothing walks a chain per duplicate: n requests of one member and n requests of n members run
// the same kernels over the same n words (profiles/quota_ledger.md).
//
// A ledger opened on a directory (quota_store.h) journals every draw before an id of it leaves the call.  Which counters a
// draw moved is known only here, so behind the advance pass
//   k_quota_delta_mark          flag[j] = 1 iff sorted position j is the last of its group, its key is counted and the
//                               group was granted something
//   k_scan_up / k_scan_down     pos[j] = the flags before j
//   k_quota_delta_pack          rec[pos[j]] = (key[j], the counter as the advance pass left it); the total m to one word
// then one copy brings back m and one the m pairs, the record is appended and synced, and only then do ids and statuses
// reach the caller's arrays.  A ledger without a store launches none of this and its block has none of these arrays.
// A snapshot compacts the counters where they live, one live slot at a time: k_quota_snap_mark (a byte per counter,
// != 0), the same scan, k_quota_snap_pack ((leaf, used) in leaf order), one copy of the count and one of the pairs, in
// temporary memory that is zeroed before it is freed.  A reopen uploads the replayed image in pieces and k_quota_restore
// stores one pair per lane into the zeroed counters: the image has one entry per key, so plain stores do.
//
// Proving with drawn ids (Prover::submit_members_drawn): draw_hold() is the same call that copies back the statuses alone
// and leaves the block where it is until release(); in between, k_quota_fill -- launched by the prover on its own stream,
// ordered against the ledger's by events -- copies each batch's ids into the messageId slot of its staged input rows.
#include "quota_ledger.h"

#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "log_scan.h"
#include "quota_store.h"

namespace rlnamd {

using nlog::Row32;

static_assert(quota::BLOCK == LOG_LANES, "a draw's workgroup is the scan's");
static_assert(quota::DIGITS == LOG_LANES, "k_quota_count writes one bin a lane");

namespace {

__global__ void __launch_bounds__(LOG_LANES) k_quota_key(const Row32* __restrict__ window, uint64_t live, uint32_t slots,
                                                         const uint32_t* __restrict__ leaf, const Row32* __restrict__ ext, uint32_t n,
                                                         uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  __shared__ Row32 lds_window[quota::EPOCHS_MAX];
  for (uint32_t j = threadIdx.x; j < slots * 8; j += LOG_LANES) lds_window[j >> 3].w[j & 7] = window[j >> 3].w[j & 7];
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  key[i] = quota::pack_key(quota::slot_of(lds_window, live, slots, ext[i]), leaf[i]);
  val[i] = i;
}

__device__ __forceinline__ uint32_t digit_of(uint32_t key, uint32_t shift) { return (key >> shift) & (quota::DIGITS - 1); }

// bins[digit * blocks + block]: the LDS counts are the only words lanes share, and only their totals are read
__global__ void __launch_bounds__(LOG_LANES) k_quota_count(const uint32_t* __restrict__ key, uint32_t n, uint32_t shift,
                                                           uint32_t* __restrict__ bins) {
  __shared__ uint32_t count[quota::DIGITS];
  count[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) atomicAdd(&count[digit_of(key[i], shift)], 1u);
  __syncthreads();
  bins[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = count[threadIdx.x];
}

// A request's place among its block's requests with the same digit, in lane order: the lanes of its wave below it (a
// ballot per digit bit leaves the mask of the wave's lanes with the same digit), plus the counts of the waves below.
__global__ void __launch_bounds__(LOG_LANES) k_quota_scatter(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                             uint32_t n, uint32_t shift, const uint32_t* __restrict__ bin_start,
                                                             uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
  __shared__ uint32_t wave_count[LOG_LANES / 64][quota::DIGITS];
#pragma unroll
  for (uint32_t w = 0; w < LOG_LANES / 64; w++) wave_count[w][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = i < n;
  const uint32_t k = live ? key[i] : 0, v = live ? val[i] : 0, d = digit_of(k, shift);
  uint64_t peers = __ballot(live);
#pragma unroll
  for (uint32_t b = 0; b < quota::DIGIT_BITS; b++) {
    const bool bit = (d >> b) & 1;
    const uint64_t with = __ballot(bit);
    peers &= bit ? with : ~with;
  }
  const uint32_t below = __popcll(peers & (((uint64_t)1 << lane) - 1));
  if (live && below == 0) wave_count[wave][d] = __popcll(peers);   // the lowest lane with the digit speaks for it
  __syncthreads();
  if (!live) return;
  uint32_t place = below;
  for (uint32_t w = 0; w < wave; w++) place += wave_count[w][d];
  const uint32_t to = bin_start[(size_t)d * gridDim.x + blockIdx.x] + place;
  if (to >= n) return;   // (not reached; a write past the arrays is not an answer to a wrong position)
  key_out[to] = k;
  val_out[to] = v;
}

__global__ void __launch_bounds__(LOG_LANES) k_quota_heads(const uint32_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ mark) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j < n) mark[j] = (j > 0 && key[j] != key[j - 1]) ? j : 0;
}

__device__ __forceinline__ bool counted(uint32_t key, uint32_t slots, uint32_t depth) {
  return quota::key_slot(key) < slots && (quota::key_leaf(key) >> depth) == 0;   // NO_SLOT is above every real slot
}

__global__ void __launch_bounds__(LOG_LANES) k_quota_issue(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                           const uint32_t* __restrict__ start, const uint32_t* __restrict__ limits,
                                                           const uint32_t* __restrict__ counters, uint32_t depth, uint32_t slots,
                                                           uint32_t n, uint32_t* __restrict__ ids, uint8_t* __restrict__ status,
                                                           uint32_t* __restrict__ ok) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = key[j], i = val[j];
  ok[j] = 0;
  if (i >= n) return;   // (not reached)
  const uint32_t limit = limits[i];
  if (!counted(k, slots, depth)) {
    ids[i] = limit;
    status[i] = quota::NO_EPOCH;
    return;
  }
  const quota::Issue r = quota::issue(counters[quota::counter_of(k, depth)], j - start[j], limit);
  ids[i] = r.id;
  status[i] = r.status;
  if (r.status == quota::OK) ok[j] = j + 1;
}

__global__ void __launch_bounds__(LOG_LANES) k_quota_advance(const uint32_t* __restrict__ key, const uint32_t* __restrict__ start,
                                                             const uint32_t* __restrict__ last, uint32_t* __restrict__ counters,
                                                             uint32_t depth, uint32_t slots, uint32_t n) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = key[j];
  if (j + 1 < n && key[j + 1] == k) return;   // the group's last lane alone
  if (!counted(k, slots, depth)) return;
  uint32_t* counter = counters + quota::counter_of(k, depth);
  const uint32_t used = *counter, next = quota::advance(used, start[j], last[j]);
  if (next != used) __hip_atomic_store(counter, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- blocks of ids (draw_counts)
__global__ void __launch_bounds__(LOG_LANES) k_quota_weights(const uint32_t* __restrict__ val, const uint8_t* __restrict__ counts,
                                                             uint32_t n, uint32_t* __restrict__ w) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = val[j];
  w[j] = i < n ? counts[i] : 0;   // (i >= n: not reached)
}

// S: the exclusive sums of w.  start[j] <= j, so every index read is below n.
__global__ void __launch_bounds__(LOG_LANES) k_quota_issue_counts(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                                  const uint32_t* __restrict__ start, const uint32_t* __restrict__ limits,
                                                                  const uint32_t* __restrict__ w, const uint32_t* __restrict__ S,
                                                                  const uint32_t* __restrict__ counters, uint32_t depth, uint32_t slots,
                                                                  uint32_t n, uint32_t* __restrict__ firsts, uint8_t* __restrict__ status,
                                                                  uint32_t* __restrict__ ok) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = key[j], i = val[j], st = start[j];
  ok[j] = 0;
  if (i >= n || st > j) return;   // (not reached)
  const uint32_t limit = limits[i];
  if (!counted(k, slots, depth)) {
    firsts[i] = limit;
    status[i] = quota::NO_EPOCH;
    return;
  }
  const quota::Issue r = quota::issue_counts(counters[quota::counter_of(k, depth)], S[j] - S[st], w[j], limit);
  firsts[i] = r.id;
  status[i] = r.status;
  if (r.status == quota::OK) ok[j] = j + 1;
}

__global__ void __launch_bounds__(LOG_LANES) k_quota_advance_counts(const uint32_t* __restrict__ key, const uint32_t* __restrict__ start,
                                                                    const uint32_t* __restrict__ last, const uint32_t* __restrict__ w,
                                                                    const uint32_t* __restrict__ S, uint32_t* __restrict__ counters,
                                                                    uint32_t depth, uint32_t slots, uint32_t n) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = key[j];
  if (j + 1 < n && key[j + 1] == k) return;   // the group's last lane alone
  if (!counted(k, slots, depth)) return;
  const uint32_t st = start[j], l = last[j];
  if (l <= st || l > j + 1) return;           // nothing granted in this group (l > j + 1: not reached)
  uint32_t* counter = counters + quota::counter_of(k, depth);
  const uint32_t used = *counter, next = quota::advance_counts(used, st, l, S[l - 1] - S[st], w[l - 1]);
  if (next != used) __hip_atomic_store(counter, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the delta of a draw, for the journal of a ledger with a store.  `last` is the running maximum the advance pass
// read: a group was granted something iff it is above the group's start.
__global__ void __launch_bounds__(LOG_LANES) k_quota_delta_mark(const uint32_t* __restrict__ key, const uint32_t* __restrict__ start,
                                                                const uint32_t* __restrict__ last, uint32_t depth, uint32_t slots,
                                                                uint32_t n, uint8_t* __restrict__ flag) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = key[j];
  const bool tail = !(j + 1 < n && key[j + 1] == k);
  flag[j] = tail && counted(k, slots, depth) && last[j] > start[j] && last[j] <= j + 1;
}

// the counters are read behind the advance pass that wrote them: their absolute values
__global__ void __launch_bounds__(LOG_LANES) k_quota_delta_pack(const uint32_t* __restrict__ key, const uint8_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ pos, const uint32_t* __restrict__ counters,
                                                                uint32_t depth, uint32_t n, uint2* __restrict__ rec,
                                                                uint32_t* __restrict__ total) {
  const uint32_t j = blockIdx.x * LOG_LANES + threadIdx.x;
  if (j >= n) return;
  const bool moved = flag[j] != 0;
  const uint32_t to = pos[j];
  if (j == n - 1) *total = to + moved;
  if (!moved || to >= n) return;   // (to >= n: not reached)
  const uint32_t k = key[j];       // counted: the mark pass saw to it
  rec[to] = make_uint2(k, counters[quota::counter_of(k, depth)]);
}

// ---- a snapshot: the non-zero counters of one slot, compacted in leaf order (n = 2^depth <= 2^24 counters)
__global__ void __launch_bounds__(LOG_LANES) k_quota_snap_mark(const uint32_t* __restrict__ counters, uint32_t n,
                                                               uint8_t* __restrict__ mark) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) mark[i] = counters[i] != 0;
}
__global__ void __launch_bounds__(LOG_LANES) k_quota_snap_pack(const uint32_t* __restrict__ counters, const uint8_t* __restrict__ mark,
                                                               const uint32_t* __restrict__ pos, uint32_t n, uint2* __restrict__ pairs,
                                                               uint32_t* __restrict__ total) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  const bool kept = mark[i] != 0;
  const uint32_t to = pos[i];
  if (i == n - 1) *total = to + kept;
  if (!kept || to >= n) return;   // (to >= n: not reached)
  pairs[to] = make_uint2(i, counters[i]);
}

// ---- a reopen: one (key, used) pair a lane into the zeroed counters; the keys are distinct, a plain store does
__global__ void __launch_bounds__(LOG_LANES) k_quota_restore(const uint2* __restrict__ pairs, uint32_t m, uint32_t depth, uint32_t slots,
                                                             uint32_t* __restrict__ counters) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= m) return;
  const uint2 p = pairs[i];
  if (!counted(p.x, slots, depth)) return;   // (not reached: the store refuses such a pair)
  counters[quota::counter_of(p.x, depth)] = p.y;
}

// Proving with drawn ids (Prover::enqueue): a lane per staged input row, behind the row's staging on the same stream
__global__ void __launch_bounds__(LOG_LANES) k_quota_fill(const uint32_t* __restrict__ ids, const uint8_t* __restrict__ status,
                                                          uint32_t n, uint32_t* __restrict__ rows, size_t row_words, uint32_t slot) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  uint32_t* to = rows + (size_t)i * row_words + (size_t)slot * 8;
  const bool granted = status[i] == quota::OK;   // refused: no field element, the interpreter refuses the row
  to[0] = granted ? ids[i] : QuotaLedgerDev::REFUSED_WORD;
#pragma unroll
  for (int w = 1; w < 8; w++) to[w] = granted ? 0 : QuotaLedgerDev::REFUSED_WORD;
}

// the same with blocks of ids (Prover::submit_members_drawn_counts): max_out message slots and selectors a row
__global__ void __launch_bounds__(LOG_LANES) k_quota_fill_counts(const uint32_t* __restrict__ firsts, const uint8_t* __restrict__ status,
                                                                 const uint8_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ rows,
                                                                 size_t row_words, uint32_t msg_slot, uint32_t sel_slot, bool has_sel,
                                                                 uint32_t max_out) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  const uint32_t count = counts[i];
  // (a count above max_out is refused on the host before the draw; a row is never written past its slots)
  QuotaLedgerDev::fill_row_counts(rows + (size_t)i * row_words, status[i] == quota::OK && count <= max_out, firsts[i], count, msg_slot,
                                  sel_slot, has_sel, max_out);
}

void wipe_host(void* p, size_t n) {   // through a volatile pointer: not elided as dead (ffi_wire.h: secure_zero)
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

size_t nonzero_words16(const uint8_t* p, size_t bytes) {
  size_t c = 0;
  for (size_t o = 0; o + 16 <= bytes; o += 16) {
    uint8_t any = 0;
    for (int k = 0; k < 16; k++) any |= p[o + k];
    c += any != 0;
  }
  return c;
}

struct OnDevice {   // the ledger's device for the length of a call, the caller's afterwards
  int prev = 0, dev;
  explicit OnDevice(int dev_) : dev(dev_) {
    RLN_HIP(hipGetDevice(&prev));
    if (prev != dev) RLN_HIP(hipSetDevice(dev));
  }
  ~OnDevice() {
    if (prev != dev) (void)hipSetDevice(prev);
  }
};

// The block of one call of n requests, in bytes from its start; every array starts 16-byte aligned.
//   in  (pinned -> device, one copy):  leaf 4 n | limits 4 n | ext 32 n | counts n
//   out (device -> pinned, one copy):  ids 4 n | status n
//   the rest is the device's alone:    two (key, val) pairs, start, ok, the sorted counts w and their sums S, the bins and
//                                      their starts, the scans' block sums
// counts, w and S are there for a draw_counts call alone: the block of a plain draw is what it was without them.
// The delta's arrays -- flags n | positions 4 n | (key, used) pairs 8 n | their number, one word -- come last, and only
// in the block of a ledger with a store: without one the block is what it was.
struct Block {
  size_t np, leaf, limits, ext, counts, ids, status, key[2], val[2], start, ok, w, wsum, bins, bin_start, sums, dflag, dpos, drec,
      dtotal, bytes;
  size_t delta_host_bytes() const { return 8 * np + 16; }   // the pinned copy: the pairs, then their number
  size_t in_bytes() const { return ids; }
  size_t out_bytes() const { return key[0] - ids; }
  Block(size_t n, bool by_count, bool delta) {
    np = (n + 3) / 4 * 4;
    const quota::DrawPlan P = quota::plan_for(n, 1);
    size_t at = 0;
    auto take = [&](size_t b) {
      const size_t here = at;
      at += (b + 15) / 16 * 16;
      return here;
    };
    leaf = take(4 * np);
    limits = take(4 * np);
    ext = take(32 * np);
    counts = take(by_count ? np : 0);
    ids = take(4 * np);
    status = take(np);
    for (int s = 0; s < 2; s++) key[s] = take(4 * np), val[s] = take(4 * np);
    start = take(4 * np);
    ok = take(4 * np);
    w = take(by_count ? 4 * np : 0);
    wsum = take(by_count ? 4 * np : 0);
    bins = take(4 * P.bins);
    bin_start = take(4 * P.bins);
    sums = take(4 * std::max(ScanPlan(P.bins).words, ScanPlan(n).words));
    dflag = take(delta ? np : 0);
    dpos = take(delta ? 4 * np : 0);
    drec = take(delta ? 8 * np : 0);
    dtotal = take(delta ? 16 : 0);
    bytes = at;
  }
};

}  // namespace

struct QuotaLedgerDev::Impl {
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t depth = 0, max_epochs = 0;
  quota::Window window;           // (a member: the copy to the device reads it)
  DevBuf<uint32_t> counters;      // max_epochs << depth
  DevBuf<Row32> window_dev;       // EPOCHS_MAX rows
  uint64_t draws = 0, issued = 0, over = 0, no_epoch = 0;
  // the block of one call of up to stage_n requests, all zero between calls, on the device and in the pinned copies
  size_t stage_n = 0, stage_bytes = 0, in_cap = 0, out_cap = 0;
  DevBuf<uint8_t> block;
  uint8_t* in_host = nullptr;
  uint8_t* out_host = nullptr;
  size_t held_n = 0;   // draw_hold's requests while their block is kept (quota_ledger.h); 0: none
  bool held_by_count = false;   // ... and whether that draw was one by count: the block's layout
  // a ledger opened on a directory: the store, and the pinned copy of a draw's delta (null without a store)
  std::unique_ptr<qstore::QuotaStore> store;
  // Set as the last step of the durable constructor, once window and counters are on the device as the store has them.
  // Until then nothing may be written from the device's state: the counters are zero, or restored in part, and a
  // snapshot of them would put the ledger below ids it has issued.
  bool restored = false;
  uint8_t* delta_host = nullptr;
  size_t delta_cap = 0;
  Block block_of(size_t n, bool by_count) const { return Block(n, by_count, store != nullptr); }
  void init(size_t depth, size_t max_epochs);
  void restore(const qstore::Image& im, bool fail_midway);
  void compact_now();
  // behind the call that let the journal outgrow its threshold.  The call itself is done and durable; a compaction that
  // fails leaves the journal as it is (or the store refusing writes, which the next call reports).
  void compact_if_due() {
    if (!store || !store->wants_compaction()) return;
    try {
      compact_now();
    } catch (const std::exception&) {
    }
  }

  // counts null: a plain draw
  void run(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, const uint8_t* counts,
           uint32_t* ids_out, uint8_t* status, bool hold);
  void reserve(size_t n) {
    if (n <= stage_n) return;
    release_staging();
    const size_t m = n < 1024 ? 1024 : n;
    const Block B = block_of(m, true);   // the larger of the two layouts
    RLN_HIP(hipHostMalloc((void**)&in_host, B.in_bytes(), hipHostMallocDefault));
    in_cap = B.in_bytes();
    memset(in_host, 0, in_cap);
    RLN_HIP(hipHostMalloc((void**)&out_host, B.out_bytes(), hipHostMallocDefault));
    out_cap = B.out_bytes();
    memset(out_host, 0, out_cap);
    if (store) {
      RLN_HIP(hipHostMalloc((void**)&delta_host, B.delta_host_bytes(), hipHostMallocDefault));
      delta_cap = B.delta_host_bytes();
      memset(delta_host, 0, delta_cap);
    }
    block.alloc(B.bytes);
    RLN_HIP(hipMemsetAsync(block.p, 0, B.bytes, stream));
    stage_n = m;
    stage_bytes = B.bytes;
  }
  // (what a call left is zero already -- draw() wipes before it returns -- and is wiped once more before it is freed)
  void release_staging() {
    if (block.p) {
      (void)hipMemsetAsync(block.p, 0, stage_bytes, stream);
      (void)hipStreamSynchronize(stream);
    }
    if (in_host) {
      wipe_host(in_host, in_cap);
      (void)hipHostFree(in_host);
    }
    if (out_host) {
      wipe_host(out_host, out_cap);
      (void)hipHostFree(out_host);
    }
    if (delta_host) {
      wipe_host(delta_host, delta_cap);
      (void)hipHostFree(delta_host);
    }
    block.release();
    in_host = out_host = delta_host = nullptr;
    stage_n = stage_bytes = in_cap = out_cap = delta_cap = 0;
  }
  ~Impl() {
    held_n = 0;
    // rlnamd_quota_free compacts, then closes.  A FAILED OPEN NEVER WRITES A SNAPSHOT: a ledger whose construction
    // threw (no memory for the counters, an error while the image was uploaded) is destroyed here too, and its store is
    // closed as it was found -- the journal still holds the truth for the next open.
    if (stream && store && restored && store->has_records()) {
      try {
        compact_now();
      } catch (const std::exception&) {
      }
    }
    if (stream) {
      if (counters.p) (void)hipMemsetAsync(counters.p, 0, counters.bytes(), stream);   // who signed how often
      (void)hipStreamSynchronize(stream);
    }
    release_staging();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

void QuotaLedgerDev::Impl::init(size_t depth_, size_t max_epochs_) {
  RLN_HIP(hipGetDevice(&device));
  RLN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  depth = (uint32_t)depth_;
  max_epochs = (uint32_t)max_epochs_;
  counters.alloc(max_epochs_ << depth_);
  window_dev.alloc(quota::EPOCHS_MAX);
  RLN_HIP(hipMemsetAsync(counters.p, 0, counters.bytes(), stream));
  RLN_HIP(hipMemsetAsync(window_dev.p, 0, window_dev.bytes(), stream));
  RLN_HIP(hipStreamSynchronize(stream));
}

QuotaLedgerDev::QuotaLedgerDev(size_t depth, size_t max_epochs) {
  const std::string refused = quota::new_refusal(depth, max_epochs);
  if (!refused.empty()) throw Error(refused);
  require_gpu();
  Impl* m = new Impl;
  try {
    m->init(depth, max_epochs);
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

// The store is opened, and refused, on the host before a device is asked for; then the image goes to the device.
QuotaLedgerDev::QuotaLedgerDev(const char* dir, size_t depth, size_t max_epochs, uint64_t journal_max_bytes) {
  const std::string refused = quota::new_refusal(depth, max_epochs);
  if (!refused.empty()) throw Error(refused);
  if (!dir || !dir[0]) throw Error("quota ledger: open was given no directory");
  Impl* m = new Impl;
  try {
    qstore::Image im;
    m->store.reset(new qstore::QuotaStore);
    try {
      m->store->open(dir, depth, max_epochs, journal_max_bytes, im);
    } catch (const qstore::StoreError& e) {
      throw Error(e.what());
    }
    require_gpu();
    m->init(depth, max_epochs);
    // (test hook: the open fails here, "init", or behind the first piece of the image, "restore" -- as it would for want
    // of device memory -- so that a test can hold the directory against what it was)
    const char* fail = getenv("RLNAMD_QUOTA_OPEN_FAULT");
    if (fail && !strcmp(fail, "init")) throw Error("quota ledger: RLNAMD_QUOTA_OPEN_FAULT=init");
    m->restore(im, fail && !strcmp(fail, "restore"));
    m->restored = true;
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

// the replayed image into the zeroed counters, PIECE pairs a copy; the window as set_epochs puts it there
void QuotaLedgerDev::Impl::restore(const qstore::Image& im, bool fail_midway) {
  constexpr size_t PIECE = (size_t)1 << 18;
  window = im.window;
  RLN_HIP(hipMemcpyAsync(window_dev.p, window.e, sizeof window.e, hipMemcpyHostToDevice, stream));
  RLN_HIP(hipStreamSynchronize(stream));
  if (im.used.empty()) return;
  DevBuf<uint2> piece(std::min(PIECE, im.used.size()));
  std::vector<uint2> host;
  host.reserve(piece.n);
  struct Zeroed {   // success or error: the piece is zero before it is freed
    Impl& m;
    DevBuf<uint2>& piece;
    std::vector<uint2>& host;
    ~Zeroed() {
      (void)hipMemsetAsync(piece.p, 0, piece.bytes(), m.stream);
      (void)hipStreamSynchronize(m.stream);
      wipe_host(host.data(), host.size() * sizeof(uint2));
    }
  } zeroed{*this, piece, host};
  auto flush = [&]() {
    if (host.empty()) return;
    RLN_HIP(hipMemcpyAsync(piece.p, host.data(), host.size() * sizeof(uint2), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_quota_restore, dim3(div_up(host.size(), LOG_LANES)), dim3(LOG_LANES), 0, stream, (const uint2*)piece.p,
                       (uint32_t)host.size(), depth, max_epochs, counters.p);
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipStreamSynchronize(stream));   // the host vector is filled again behind this
    wipe_host(host.data(), host.size() * sizeof(uint2));
    host.clear();
  };
  for (const auto& kv : im.used) {
    host.push_back(make_uint2(kv.first, kv.second));
    if (host.size() == piece.n || (fail_midway && host.size() == 1)) {
      flush();
      if (fail_midway) throw Error("quota ledger: RLNAMD_QUOTA_OPEN_FAULT=restore");
    }
  }
  flush();
  store->set_restored(im.used.size());
}

// The counters as the snapshot of the next generation: each live slot compacted on the device, in the window's order.
void QuotaLedgerDev::Impl::compact_now() {
  if (!store) throw Error("quota ledger: this ledger has no store (it was made by rlnamd_quota_new)");
  if (!restored) throw Error("quota ledger: internal error, a compaction before the store's image is on the device");
  if (held_n) throw Error("quota ledger: internal error, a compaction while a draw's ids are held");
  OnDevice on(device);
  const size_t N = (size_t)1 << depth;
  const ScanPlan SP(N);
  // pairs 8 N | positions 4 N | the scan's block sums | the number of pairs (16 bytes) | marks N
  const size_t pairs_at = 0, pos_at = 8 * N, sums_at = pos_at + 4 * N, total_at = sums_at + 4 * ((SP.words + 3) / 4 * 4),
               mark_at = total_at + 16, bytes = mark_at + N;
  DevBuf<uint8_t> tmp(bytes);
  struct Zeroed {   // success or error: zeroed before it is freed
    Impl& m;
    DevBuf<uint8_t>& tmp;
    ~Zeroed() {
      (void)hipMemsetAsync(tmp.p, 0, tmp.bytes(), m.stream);
      (void)hipStreamSynchronize(m.stream);
    }
  } zeroed{*this, tmp};
  RLN_HIP(hipMemsetAsync(tmp.p, 0, bytes, stream));
  try {
    store->compact(window, [&](uint32_t slot, std::vector<uint32_t>& leaf_used) {
      const uint32_t* slot_counters = counters.p + ((size_t)slot << depth);
      uint8_t* mark = tmp.p + mark_at;
      uint32_t* pos = (uint32_t*)(tmp.p + pos_at);
      uint32_t* total = (uint32_t*)(tmp.p + total_at);
      const dim3 grid(div_up(N, LOG_LANES)), lanes(LOG_LANES);
      hipLaunchKernelGGL(k_quota_snap_mark, grid, lanes, 0, stream, slot_counters, (uint32_t)N, mark);
      scan_positions((const uint8_t*)mark, N, pos, (uint32_t*)(tmp.p + sums_at), stream);
      hipLaunchKernelGGL(k_quota_snap_pack, grid, lanes, 0, stream, slot_counters, (const uint8_t*)mark, (const uint32_t*)pos, (uint32_t)N,
                         (uint2*)(tmp.p + pairs_at), total);
      RLN_HIP(hipGetLastError());
      uint32_t pairs = 0;
      RLN_HIP(hipMemcpyAsync(&pairs, total, 4, hipMemcpyDeviceToHost, stream));
      RLN_HIP(hipStreamSynchronize(stream));
      if (pairs > N) throw Error("quota ledger: internal error, a slot came back with more pairs than counters");
      leaf_used.resize(2 * (size_t)pairs);
      if (!pairs) return;
      RLN_HIP(hipMemcpyAsync(leaf_used.data(), tmp.p + pairs_at, 8 * (size_t)pairs, hipMemcpyDeviceToHost, stream));
      RLN_HIP(hipStreamSynchronize(stream));
    });
  } catch (const qstore::StoreError& e) {
    throw Error(e.what());
  }
}

void QuotaLedgerDev::compact() { d->compact_now(); }

void QuotaLedgerDev::store_info(uint64_t out[8]) const {
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (d->store) d->store->info(out);
}

QuotaLedgerDev::~QuotaLedgerDev() {
  if (!d) return;
  int prev = 0;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
  delete d;
  if (move) (void)hipSetDevice(prev);
}

int QuotaLedgerDev::device() const { return d->device; }
int QuotaLedgerDev::depth() const { return (int)d->depth; }

void QuotaLedgerDev::fill_rows(const uint32_t* ids, const uint8_t* status, size_t count, uint32_t* rows, size_t row_words,
                               uint32_t slot, void* on) {
  if (count == 0) return;
  if (count > 0xFFFFFFFFull || (size_t)slot * 8 + 8 > row_words) throw Error("quota ledger: fill_rows: the slot is outside the row");
  hipLaunchKernelGGL(k_quota_fill, dim3(div_up(count, LOG_LANES)), dim3(LOG_LANES), 0, (hipStream_t)on, ids, status, (uint32_t)count,
                     rows, row_words, slot);
  RLN_HIP(hipGetLastError());
}

void QuotaLedgerDev::fill_rows_counts(const uint32_t* firsts, const uint8_t* status, const uint8_t* counts, size_t count, uint32_t* rows,
                                      size_t row_words, uint32_t msg_slot, uint32_t sel_slot, bool has_sel, uint32_t max_out, void* on) {
  if (count == 0) return;
  if (count > 0xFFFFFFFFull || max_out == 0 || ((size_t)msg_slot + max_out) * 8 > row_words ||
      (has_sel && ((size_t)sel_slot + max_out) * 8 > row_words))
    throw Error("quota ledger: fill_rows_counts: the slots are outside the row");
  hipLaunchKernelGGL(k_quota_fill_counts, dim3(div_up(count, LOG_LANES)), dim3(LOG_LANES), 0, (hipStream_t)on, firsts, status, counts,
                     (uint32_t)count, rows, row_words, msg_slot, sel_slot, has_sel, max_out);
  RLN_HIP(hipGetLastError());
}

void QuotaLedgerDev::set_epochs(size_t k, const uint8_t* external_nullifiers_le) {
  Impl& m = *d;
  // the host check: nothing is enqueued and nothing of the ledger changes before it has passed
  const std::string refused = quota::epochs_refusal(external_nullifiers_le, k, m.max_epochs);
  if (!refused.empty()) throw Error(refused);
  uint64_t leaving = 0;
  const quota::Window next = quota::next_window(m.window, external_nullifiers_le, k, m.max_epochs, &leaving);
  // A ledger with a store: the window record is appended and synced first, then the window is applied.  A failure to
  // append is a refusal like the ones above.  A crash between the two reopens into the new window, under which nothing
  // was signed yet.  A HIP error behind the record leaves the journal a window ahead of this object: the store takes no
  // more writes then -- and the ledger so draws nothing more -- until it is reopened.
  struct Ahead {
    Impl& m;
    bool applied = false;
    ~Ahead() {
      if (!applied && m.store) m.store->poison("a set_epochs that failed on the device behind its record");
    }
  };
  if (m.store) {
    try {
      m.store->append_window(k, external_nullifiers_le);
    } catch (const qstore::StoreError& e) {
      throw Error(e.what());
    }
  }
  Ahead ahead{m};
  // From here on only a HIP error can stop the call, and such an error is not a refusal: the ledger is not left as it
  // was.  It is left SAFE: the external nullifiers that leave are taken out of the host's window first (a draw looks
  // slots up with the host's `live` mask), so no id is drawn under an epoch whose counters may be zeroed in part; the new
  // ones are not in yet.  A slot whose zeroing did not finish may keep counters above zero for its next holder, which
  // skips ids and never repeats one.
  if (leaving) {
    quota::Window mid = m.window;
    mid.live &= ~leaving;
    mid.k = 0;
    for (uint32_t j = 0; j < m.window.k; j++)
      if ((mid.live >> m.window.order[j]) & 1) mid.order[mid.k++] = m.window.order[j];
    m.window = mid;
  }
  OnDevice on(m.device);
  for (uint32_t s = 0; s < m.max_epochs; s++)
    if ((leaving >> s) & 1) RLN_HIP(hipMemsetAsync(m.counters.p + ((size_t)s << m.depth), 0, (size_t)4 << m.depth, m.stream));
  RLN_HIP(hipMemcpyAsync(m.window_dev.p, next.e, sizeof next.e, hipMemcpyHostToDevice, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
  m.window = next;
  ahead.applied = true;
  m.compact_if_due();
}

size_t QuotaLedgerDev::epochs(uint8_t out_le[32 * quota::EPOCHS_MAX]) const {
  const quota::Window& W = d->window;
  for (uint32_t j = 0; j < W.k; j++) memcpy(out_le + 32 * j, W.e[W.order[j]].w, 32);
  return W.k;
}

void QuotaLedgerDev::draw(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits, uint32_t* ids_out,
                          uint8_t* status) {
  d->run(n, leaf_indices, ext_le, limits, nullptr, ids_out, status, false);
  d->compact_if_due();
}

void QuotaLedgerDev::draw_counts(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                                 const uint8_t* counts, uint32_t* firsts_out, uint8_t* status) {
  // the host check: nothing is enqueued and nothing of the ledger changes before it has passed
  const std::string refused = quota::draw_counts_refusal(n, leaf_indices, ext_le, limits, counts, firsts_out, status, d->depth);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  d->run(n, leaf_indices, ext_le, limits, counts, firsts_out, status, false);
  d->compact_if_due();
}

QuotaLedgerDev::Held QuotaLedgerDev::draw_hold(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                                               uint8_t* status) {
  d->run(n, leaf_indices, ext_le, limits, nullptr, nullptr, status, true);
  if (!d->held_n) return Held{nullptr, nullptr, (void*)d->stream, d->device};
  const Block B = d->block_of(d->held_n, d->held_by_count);
  return Held{(const uint32_t*)(d->block.p + B.ids), d->block.p + B.status, (void*)d->stream, d->device};
}

QuotaLedgerDev::Held QuotaLedgerDev::draw_hold_counts(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le,
                                                      const uint32_t* limits, const uint8_t* counts, uint8_t* status) {
  const std::string refused = quota::draw_counts_refusal(n, leaf_indices, ext_le, limits, counts, nullptr, status, d->depth, false);
  if (!refused.empty()) throw Error(refused);
  if (n) d->run(n, leaf_indices, ext_le, limits, counts, nullptr, status, true);
  if (!d->held_n) return Held{nullptr, nullptr, (void*)d->stream, d->device, nullptr};
  const Block B = d->block_of(d->held_n, true);
  return Held{(const uint32_t*)(d->block.p + B.ids), d->block.p + B.status, (void*)d->stream, d->device, d->block.p + B.counts};
}

void QuotaLedgerDev::held_ids(size_t first, size_t count, uint32_t* out) {
  Impl& m = *d;
  if (count == 0) return;
  if (first > m.held_n || count > m.held_n - first) throw Error("quota ledger: internal error, ids asked for beyond the draw that is held");
  OnDevice on(m.device);
  RLN_HIP(hipMemcpyAsync(out, m.block.p + m.block_of(m.held_n, m.held_by_count).ids + 4 * first, 4 * count, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
}

void QuotaLedgerDev::release() {
  Impl& m = *d;
  if (!m.held_n) return;
  const Block B = m.block_of(m.held_n, m.held_by_count);
  m.held_n = 0;
  wipe_host(m.out_host, B.out_bytes());
  if (m.delta_host) wipe_host(m.delta_host, B.delta_host_bytes());
  int prev = 0;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != m.device && hipSetDevice(m.device) == hipSuccess;
  const hipError_t e1 = hipMemsetAsync(m.block.p, 0, B.bytes, m.stream), e2 = hipStreamSynchronize(m.stream);
  if (move) (void)hipSetDevice(prev);
  RLN_HIP(e1);
  RLN_HIP(e2);
  m.compact_if_due();
}

void QuotaLedgerDev::Impl::run(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                               const uint8_t* counts, uint32_t* ids_out, uint8_t* status, bool hold) {
  Impl& m = *this;
  if (m.held_n) throw Error("quota ledger: internal error, a draw while another draw's ids are held");
  // the host check: nothing is enqueued and nothing of the ledger changes before it has passed
  const std::string refused = quota::draw_refusal(n, leaf_indices, ext_le, limits, ids_out, status, m.depth, !hold);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  if (m.store) {   // a store that takes no more writes draws nothing: its ids could not be made durable
    try {
      m.store->check_writable();
    } catch (const qstore::StoreError& e) {
      throw Error(e.what());
    }
  }
  OnDevice on(m.device);
  m.reserve(n);
  const Block B = m.block_of(n, counts != nullptr);
  const quota::DrawPlan P = quota::plan_for(n, m.depth);
  struct Wipe {   // success or error: the call's block is zero again when draw() returns (a held draw: at release())
    Impl& m;
    const Block& B;
    bool device_done = false, held = false;
    ~Wipe() {
      wipe_host(m.in_host, B.in_bytes());
      if (m.delta_host) wipe_host(m.delta_host, B.delta_host_bytes());   // journalled, or the call failed
      if (held) return;
      if (!device_done) {
        (void)hipMemsetAsync(m.block.p, 0, B.bytes, m.stream);
        (void)hipStreamSynchronize(m.stream);
      }
      wipe_host(m.out_host, B.out_bytes());
    }
  } wipe{m, B};

  uint32_t* h_leaf = (uint32_t*)(m.in_host + B.leaf);
  for (size_t i = 0; i < n; i++) h_leaf[i] = (uint32_t)leaf_indices[i];
  memcpy(m.in_host + B.limits, limits, 4 * n);
  memcpy(m.in_host + B.ext, ext_le, 32 * n);
  if (counts) memcpy(m.in_host + B.counts, counts, n);
  uint8_t* base = m.block.p;
  auto words = [&](size_t off) { return (uint32_t*)(base + off); };
  const uint32_t n32 = (uint32_t)n, blocks = (uint32_t)P.blocks, slots = m.max_epochs;
  const dim3 grid(blocks), lanes(LOG_LANES);
  RLN_HIP(hipMemcpyAsync(base, m.in_host, B.in_bytes(), hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_quota_key, grid, lanes, 0, m.stream, (const Row32*)m.window_dev.p, m.window.live, slots,
                     (const uint32_t*)words(B.leaf), (const Row32*)(base + B.ext), n32, words(B.key[0]), words(B.val[0]));
  int cur = 0;
  for (uint32_t p = 0; p < P.passes; p++, cur ^= 1) {
    hipLaunchKernelGGL(k_quota_count, grid, lanes, 0, m.stream, (const uint32_t*)words(B.key[cur]), n32, P.shift[p], words(B.bins));
    scan_positions((const uint32_t*)words(B.bins), P.bins, words(B.bin_start), words(B.sums), m.stream);
    hipLaunchKernelGGL(k_quota_scatter, grid, lanes, 0, m.stream, (const uint32_t*)words(B.key[cur]),
                       (const uint32_t*)words(B.val[cur]), n32, P.shift[p], (const uint32_t*)words(B.bin_start),
                       words(B.key[cur ^ 1]), words(B.val[cur ^ 1]));
  }
  const uint32_t* key = words(B.key[cur]);
  const uint32_t* val = words(B.val[cur]);
  hipLaunchKernelGGL(k_quota_heads, grid, lanes, 0, m.stream, key, n32, words(B.start));
  scan_running_max(words(B.start), n, words(B.start), words(B.sums), m.stream);
  if (counts) {
    hipLaunchKernelGGL(k_quota_weights, grid, lanes, 0, m.stream, val, (const uint8_t*)(base + B.counts), n32, words(B.w));
    scan_positions((const uint32_t*)words(B.w), n, words(B.wsum), words(B.sums), m.stream);
    hipLaunchKernelGGL(k_quota_issue_counts, grid, lanes, 0, m.stream, key, val, (const uint32_t*)words(B.start),
                       (const uint32_t*)words(B.limits), (const uint32_t*)words(B.w), (const uint32_t*)words(B.wsum),
                       (const uint32_t*)m.counters.p, m.depth, slots, n32, words(B.ids), base + B.status, words(B.ok));
    scan_running_max(words(B.ok), n, words(B.ok), words(B.sums), m.stream);
    hipLaunchKernelGGL(k_quota_advance_counts, grid, lanes, 0, m.stream, key, (const uint32_t*)words(B.start),
                       (const uint32_t*)words(B.ok), (const uint32_t*)words(B.w), (const uint32_t*)words(B.wsum), m.counters.p, m.depth,
                       slots, n32);
  } else {
    hipLaunchKernelGGL(k_quota_issue, grid, lanes, 0, m.stream, key, val, (const uint32_t*)words(B.start),
                       (const uint32_t*)words(B.limits), (const uint32_t*)m.counters.p, m.depth, slots, n32, words(B.ids),
                       base + B.status, words(B.ok));
    scan_running_max(words(B.ok), n, words(B.ok), words(B.sums), m.stream);
    hipLaunchKernelGGL(k_quota_advance, grid, lanes, 0, m.stream, key, (const uint32_t*)words(B.start), (const uint32_t*)words(B.ok),
                       m.counters.p, m.depth, slots, n32);
  }
  RLN_HIP(hipGetLastError());
  uint32_t* h_moved = nullptr;   // a ledger with a store: where the number of counters this draw moved arrives
  if (m.store) {
    hipLaunchKernelGGL(k_quota_delta_mark, grid, lanes, 0, m.stream, key, (const uint32_t*)words(B.start), (const uint32_t*)words(B.ok),
                       m.depth, slots, n32, base + B.dflag);
    scan_positions((const uint8_t*)(base + B.dflag), n, words(B.dpos), words(B.sums), m.stream);
    hipLaunchKernelGGL(k_quota_delta_pack, grid, lanes, 0, m.stream, key, (const uint8_t*)(base + B.dflag),
                       (const uint32_t*)words(B.dpos), (const uint32_t*)m.counters.p, m.depth, n32, (uint2*)(base + B.drec),
                       words(B.dtotal));
    RLN_HIP(hipGetLastError());
    h_moved = (uint32_t*)(m.delta_host + 8 * B.np);
    RLN_HIP(hipMemcpyAsync(h_moved, base + B.dtotal, 4, hipMemcpyDeviceToHost, m.stream));
  }
  if (hold) {   // the statuses alone; the ids stay where they are
    RLN_HIP(hipMemcpyAsync(m.out_host + (B.status - B.ids), base + B.status, B.out_bytes() - (B.status - B.ids), hipMemcpyDeviceToHost,
                           m.stream));
  } else {
    RLN_HIP(hipMemcpyAsync(m.out_host, base + B.ids, B.out_bytes(), hipMemcpyDeviceToHost, m.stream));
    if (!m.store) RLN_HIP(hipMemsetAsync(base, 0, B.bytes, m.stream));   // behind the copy, in stream order
  }
  RLN_HIP(hipStreamSynchronize(m.stream));
  size_t moved = 0;
  if (m.store) {   // the second copy: the pairs, now that their number is known; then the block's wipe
    moved = *h_moved;
    if (moved > n) throw Error("quota ledger: internal error, a draw moved more counters than it has requests");
    if (moved) RLN_HIP(hipMemcpyAsync(m.delta_host, base + B.drec, 8 * moved, hipMemcpyDeviceToHost, m.stream));
    if (!hold) RLN_HIP(hipMemsetAsync(base, 0, B.bytes, m.stream));
    if (moved || !hold) RLN_HIP(hipStreamSynchronize(m.stream));
  }
  wipe.device_done = !hold;

  const uint8_t* h_status = m.out_host + (B.status - B.ids);
  for (size_t i = 0; i < n; i++)
    if (h_status[i] > quota::NO_EPOCH) throw Error("quota ledger: internal error, a request came back without a status");
  // Durable before any id leaves the call: the record is appended and synced, and only then are ids and statuses copied
  // into the caller's arrays (a held draw: before draw_hold returns, so before anything is staged for proving).  A draw
  // that granted nothing appends nothing.  If this fails the call fails: the caller's arrays are untouched, the block is
  // wiped (a held draw's too: it is not held), the counters stay advanced -- those ids are burnt, the safe side -- and
  // the ledger stays usable, since the next record carries absolute values.
  if (moved) {
    try {
      m.store->append_advance(moved, (const uint32_t*)m.delta_host);
    } catch (const qstore::StoreError& e) {
      throw Error(e.what());
    }
  }
  if (!hold) memcpy(ids_out, m.out_host, 4 * n);
  memcpy(status, h_status, n);
  for (size_t i = 0; i < n; i++) {
    m.issued += h_status[i] == quota::OK ? (counts ? counts[i] : 1) : 0;   // ids
    m.over += h_status[i] == quota::OVER;
    m.no_epoch += h_status[i] == quota::NO_EPOCH;
  }
  m.draws++;
  if (hold) {
    wipe.held = true;
    m.held_n = n;
    m.held_by_count = counts != nullptr;
  }
}

void QuotaLedgerDev::used(size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, uint32_t* used_out, uint8_t* in_window) {
  Impl& m = *d;
  if (n == 0) return;
  if (!leaf_indices || !ext_le || !used_out || !in_window) throw Error("quota ledger: used was given a null pointer for n > 0 pairs");
  for (size_t i = 0; i < n; i++)
    if (leaf_indices[i] >> m.depth)
      throw Error("quota ledger: leaf index " + std::to_string(leaf_indices[i]) + " of pair " + std::to_string(i) +
                  " is outside a ledger of depth " + std::to_string(m.depth));
  OnDevice on(m.device);
  for (size_t i = 0; i < n; i++) {
    Row32 ext;
    memcpy(ext.w, ext_le + 32 * i, 32);
    const uint32_t s = quota::slot_of(m.window.e, m.window.live, m.max_epochs, ext);
    used_out[i] = 0;
    in_window[i] = s != quota::NO_SLOT;
    if (s == quota::NO_SLOT) continue;
    RLN_HIP(hipMemcpyAsync(&used_out[i], m.counters.p + quota::counter_of(quota::pack_key(s, (uint32_t)leaf_indices[i]), m.depth), 4,
                           hipMemcpyDeviceToHost, m.stream));
  }
  RLN_HIP(hipStreamSynchronize(m.stream));
}

void QuotaLedgerDev::info(uint64_t out[8]) {
  Impl& m = *d;
  out[0] = m.window.k;
  out[1] = m.draws;
  out[2] = m.issued;
  out[3] = m.over;
  out[4] = m.no_epoch;
  out[5] = 0;
  out[6] = m.depth;
  out[7] = m.max_epochs;
  if (m.stage_n) {
    OnDevice on(m.device);
    std::vector<uint8_t> dev(m.stage_bytes);
    RLN_HIP(hipMemcpyAsync(dev.data(), m.block.p, m.stage_bytes, hipMemcpyDeviceToHost, m.stream));
    RLN_HIP(hipStreamSynchronize(m.stream));
    out[5] = nonzero_words16(dev.data(), m.stage_bytes) + nonzero_words16(m.in_host, m.in_cap) + nonzero_words16(m.out_host, m.out_cap) +
             (m.delta_host ? nonzero_words16(m.delta_host, m.delta_cap) : 0);
  }
}

}  // namespace rlnamd
