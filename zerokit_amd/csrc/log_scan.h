// Exclusive sums over n items on the device, by block sums of block sums: one kernel per level up and one per level
// down, as many levels as n asks for (256 items a block: 4 for 2^24 + 1).  Shared by nullifier_log.hip (the positions of
// the records a retire keeps) and relay.hip (the log rows of each proof's shares); device code, included by .hip units
// only.  The rule of nullifier_log.hip holds: a level reads what the kernel before it wrote, no lane waits for, or
// reads, what another lane of the same kernel writes.  A single-pass scan, in which a block looks back at its
// predecessors' sums, would be fewer launches and is exactly what that rule forbids: it spins on other workgroups'
// stores across XCDs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace rlnamd {

constexpr uint32_t LOG_LANES = 256;

// exclusive sum over the workgroup's LOG_LANES values, *total: their sum.  Every lane of the workgroup calls it.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_sum[LOG_LANES / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += below;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < LOG_LANES / 64; w++) {
    if (w < wave) base += wave_sum[w];
    all += wave_sum[w];
  }
  *total = all;
  return base + inc - v;
}
// an item of the scan's input: a keep mark counts as 0 or 1, a block sum as itself, a share count (a proof's used
// message slots, 0 .. max_out) as its value
struct ShareCount {
  uint8_t v;
};
__device__ __forceinline__ uint32_t scan_item(uint8_t v) { return v != 0; }
__device__ __forceinline__ uint32_t scan_item(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t scan_item(ShareCount c) { return c.v; }

// one level up: sums[b] = the sum of block b's items
template <class T>
__global__ void __launch_bounds__(LOG_LANES) k_scan_up(const T* __restrict__ in, size_t n, uint32_t* __restrict__ sums) {
  const size_t i = (size_t)blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t total;
  block_scan(i < n ? scan_item(in[i]) : 0, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one level down: out[i] = the items before i, base[b] (the level above, already exclusive; null at the top: one block)
// plus the items of block b before i.  in == out for the levels of block sums: a lane reads and writes its own word.
template <class T>
__global__ void __launch_bounds__(LOG_LANES) k_scan_down(const T* in, size_t n, const uint32_t* __restrict__ base,
                                                         uint32_t* out) {
  const size_t i = (size_t)blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t total;
  const uint32_t before = block_scan(i < n ? scan_item(in[i]) : 0, &total);
  if (i < n) out[i] = (base ? base[blockIdx.x] : 0) + before;
}

// the levels of block sums above n items: level j + 1 has one entry per LOG_LANES entries of level j, the last has one
struct ScanPlan {
  std::vector<size_t> len, off;
  size_t words = 0;
  explicit ScanPlan(size_t n) {
    do {
      n = (n + LOG_LANES - 1) / LOG_LANES;
      len.push_back(n);
      off.push_back(words);
      words += n;
    } while (n > 1);
  }
};
// items[0 .. n) -> pos[0 .. n), n >= 1; sums: ScanPlan(n).words words.  Returns where the sum of all items is (on the
// device).
template <class T>
const uint32_t* scan_positions(const T* items, size_t n, uint32_t* pos, uint32_t* sums, hipStream_t stream) {
  const ScanPlan P(n);
  const size_t top = P.len.size();   // levels 1 .. top of block sums; level `top` is the one word with the total
  auto level = [&](size_t j) { return sums + P.off[j - 1]; };
  hipLaunchKernelGGL(k_scan_up<T>, dim3(P.len[0]), dim3(LOG_LANES), 0, stream, items, n, level(1));
  for (size_t j = 1; j < top; j++)
    hipLaunchKernelGGL(k_scan_up<uint32_t>, dim3(P.len[j]), dim3(LOG_LANES), 0, stream, (const uint32_t*)level(j), P.len[j - 1],
                       level(j + 1));
  for (size_t j = top - 1; j >= 1; j--)
    hipLaunchKernelGGL(k_scan_down<uint32_t>, dim3(P.len[j]), dim3(LOG_LANES), 0, stream, (const uint32_t*)level(j), P.len[j - 1],
                       (const uint32_t*)(j + 1 < top ? level(j + 1) : nullptr), level(j));
  hipLaunchKernelGGL(k_scan_down<T>, dim3(P.len[0]), dim3(LOG_LANES), 0, stream, items, n,
                     (const uint32_t*)(1 < top ? level(1) : nullptr), pos);
  RLN_HIP(hipGetLastError());
  return level(top);
}

// ---- running maxima, the same levels with max in the place of + (quota_ledger.hip: the start of each request's group
// and the last request so far that was granted are both "the highest marked position at or below mine").  0 is the
// identity: an item that marks nothing is 0.
// The maximum of the workgroup's values at or below the lane (Inclusive) or strictly below it, *total: of all of them.
template <bool Inclusive>
__device__ __forceinline__ uint32_t block_scan_max(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_max[LOG_LANES / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = __shfl_up(inc, d, 64);
    if ((int)lane >= d && below > inc) inc = below;
  }
  const uint32_t before = __shfl_up(inc, 1, 64);
  if (lane == 63) wave_max[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < LOG_LANES / 64; w++) {
    if (w < wave && wave_max[w] > base) base = wave_max[w];
    if (wave_max[w] > all) all = wave_max[w];
  }
  *total = all;
  const uint32_t mine = Inclusive ? inc : (lane ? before : 0);
  return mine > base ? mine : base;
}
template <class T>
__global__ void __launch_bounds__(LOG_LANES) k_max_up(const T* __restrict__ in, size_t n, uint32_t* __restrict__ sums) {
  const size_t i = (size_t)blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t total;
  block_scan_max<true>(i < n ? scan_item(in[i]) : 0, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// base[b]: the maximum of everything before block b (null at the top).  in == out is allowed, as in k_scan_down.
template <bool Inclusive>
__global__ void __launch_bounds__(LOG_LANES) k_max_down(const uint32_t* in, size_t n, const uint32_t* __restrict__ base,
                                                        uint32_t* out) {
  const size_t i = (size_t)blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t total;
  const uint32_t m = block_scan_max<Inclusive>(i < n ? in[i] : 0, &total);
  const uint32_t b = base ? base[blockIdx.x] : 0;
  if (i < n) out[i] = m > b ? m : b;
}
// out[i] = max(items[0 .. i]), n >= 1; sums: ScanPlan(n).words words; items == out is allowed
inline void scan_running_max(const uint32_t* items, size_t n, uint32_t* out, uint32_t* sums, hipStream_t stream) {
  const ScanPlan P(n);
  const size_t top = P.len.size();
  auto level = [&](size_t j) { return sums + P.off[j - 1]; };
  hipLaunchKernelGGL(k_max_up<uint32_t>, dim3(P.len[0]), dim3(LOG_LANES), 0, stream, items, n, level(1));
  for (size_t j = 1; j < top; j++)
    hipLaunchKernelGGL(k_max_up<uint32_t>, dim3(P.len[j]), dim3(LOG_LANES), 0, stream, (const uint32_t*)level(j), P.len[j - 1], level(j + 1));
  for (size_t j = top - 1; j >= 1; j--)   // the block maxima become "everything before my block": exclusive
    hipLaunchKernelGGL(k_max_down<false>, dim3(P.len[j]), dim3(LOG_LANES), 0, stream, (const uint32_t*)level(j), P.len[j - 1],
                       (const uint32_t*)(j + 1 < top ? level(j + 1) : nullptr), level(j));
  hipLaunchKernelGGL(k_max_down<true>, dim3(P.len[0]), dim3(LOG_LANES), 0, stream, items, n,
                     (const uint32_t*)(1 < top ? level(1) : nullptr), out);
  RLN_HIP(hipGetLastError());
}

}  // namespace rlnamd
