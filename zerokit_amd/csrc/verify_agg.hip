// The optimistic form of the device verifier (verify_agg_math.h): a lane per proof computes its part of one combined
// pairing check -- the shared reject rules, r A, r C and the r x_j, then the Miller loop of the one pair (r A, B) --
// and the parts are folded 64 to 1 per launch until one is left.  GpuVerifier (verify.hip) draws the scalars, copies
// the last partial and the reject flags back and decides with vm::finish_host.  For the relay step it draws one seed
// per chunk instead, and k_verify_agg_scalars derives the scalars here (verify_agg_scalars.h).
//
// The levels of the fold are separate launches of k_verify_reduce, ordered by the stream.  A workgroup reads what
// workgroups of the launch before wrote; it never waits for a workgroup of its own launch and no flag is passed
// between workgroups.  The reason is the one the nullifier log's scan gives: workgroups of one launch may run on
// different XCDs, whose L2s are not coherent with each other, while a kernel boundary makes every store of the
// earlier launch visible.
#include <algorithm>

#include "common.h"
#include "verify.h"
#include "verify_agg_math.h"
#include "verify_agg_scalars.h"

namespace rlnamd {

using vm::Partial;
using vm::PrepAgg;
using vm::PreparedKey;

// proofs: n x 32 words, vals: n x nv x 8 words, scalars: n x 4 words
__global__ __launch_bounds__(64) void k_verify_prepare_agg(const PreparedKey* __restrict__ vk, const uint32_t* __restrict__ proofs,
                                                           const uint32_t* __restrict__ vals, const uint32_t* __restrict__ scalars,
                                                           PrepAgg* __restrict__ prep, Partial* __restrict__ part,
                                                           Fr* __restrict__ sums, uint8_t* __restrict__ rejected, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t nv = vk->n_values;
  vm::prepare_agg(vk, proofs + (size_t)32 * i, vals + (size_t)8 * nv * i, scalars + (size_t)4 * i, &prep[i], &part[i].c,
                  sums + (size_t)(nv + 1) * i);
  rejected[i] = (prep[i].flags & vm::P_REJECT) ? 1 : 0;
}
__global__ __launch_bounds__(64) void k_verify_miller_agg(const PreparedKey* __restrict__ vk, const PrepAgg* __restrict__ prep,
                                                          Partial* __restrict__ part, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  vm::F12 acc;
  vm::miller_loop_pair(vk, &prep[i], &acc);
  part[i].f = acc;
}
// One level: workgroup g folds partials 64 g .. 64 g + 63 of `in` (identities past n_in) through LDS, 64 x 512 bytes,
// and writes out[g]; lane j sums column j of the group's Fr rows.  n1 = n_values + 1.
__global__ __launch_bounds__(64) void k_verify_reduce(const Partial* __restrict__ in, const Fr* __restrict__ in_sums,
                                                      uint32_t n_in, Partial* __restrict__ out, Fr* __restrict__ out_sums,
                                                      uint32_t n1) {
  __shared__ Partial slots[vm::FOLD];
  const uint32_t lane = threadIdx.x, first = blockIdx.x * vm::FOLD;
  if (first + lane < n_in) slots[lane] = in[first + lane];
  else vm::partial_identity(&slots[lane]);
  __syncthreads();
  for (uint32_t stride = vm::FOLD / 2; stride; stride >>= 1) {
    vm::fold_step(slots, lane, stride);
    __syncthreads();
  }
  if (lane == 0) out[blockIdx.x] = slots[0];
  const uint32_t count = n_in - first < (uint32_t)vm::FOLD ? n_in - first : (uint32_t)vm::FOLD;
  for (uint32_t j = lane; j < n1; j += vm::FOLD)
    out_sums[(size_t)blockIdx.x * n1 + j] = vm::sum_column(in_sums + (size_t)first * n1, count, n1, j);
}

// The scalars of a chunk from its seed (verify_agg_scalars.h): a lane derives the scalars of 8 consecutive proofs with
// one permutation and stores those below n, 16 bytes each.  seed: 8 words; scalars: n x 4 words, 16-byte aligned, and
// not the seed's own words -- every lane reads the seed, so it lies where no lane writes.
__global__ __launch_bounds__(64) void k_verify_agg_scalars(const uint32_t* __restrict__ seed, uint64_t chunk,
                                                           uint32_t* __restrict__ scalars, uint32_t n) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if ((uint64_t)g * aggsc::GROUP >= n) return;
  uint64_t s[4], out[16];
#pragma unroll
  for (int k = 0; k < 4; k++) s[k] = (uint64_t)seed[2 * k] | ((uint64_t)seed[2 * k + 1] << 32);
  aggsc::derive_group(s, chunk, g, out);
  uint4* dst = (uint4*)scalars + (size_t)g * aggsc::GROUP;
  const uint32_t left = n - g * aggsc::GROUP;
#pragma unroll
  for (uint32_t j = 0; j < aggsc::GROUP; j++)
    if (j < left)
      dst[j] = make_uint4((uint32_t)out[2 * j], (uint32_t)(out[2 * j] >> 32), (uint32_t)out[2 * j + 1],
                          (uint32_t)(out[2 * j + 1] >> 32));
}

void verify_agg_scalars_enqueue(void* stream, const uint32_t* seed, uint64_t chunk, uint32_t* scalars, uint32_t n) {
  const uint32_t groups = div_up(n, aggsc::GROUP);
  hipLaunchKernelGGL(k_verify_agg_scalars, dim3(div_up(groups, 64u)), dim3(64), 0, (hipStream_t)stream, seed, chunk,
                     scalars, n);
}

int verify_agg_reduce_enqueue(void* stream, const AggBuffers& b, uint32_t n, uint32_t n_values) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(64);
  int cur = 0;
  uint32_t left = n;
  do {   // n = 1 still takes one level: the last partial is always a folded one
    const uint32_t groups = div_up(left, (uint32_t)vm::FOLD);
    hipLaunchKernelGGL(k_verify_reduce, dim3(groups), block, 0, st, b.part[cur], b.sums[cur], left, b.part[cur ^ 1],
                       b.sums[cur ^ 1], n_values + 1);
    cur ^= 1;
    left = groups;
  } while (left > 1);
  return cur;
}

int verify_agg_enqueue(void* stream, const PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals,
                       const uint32_t* scalars, const AggBuffers& b, uint32_t n, uint32_t n_values) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(div_up(n, 64)), block(64);
  hipLaunchKernelGGL(k_verify_prepare_agg, grid, block, 0, st, vk, proofs, vals, scalars, b.prep, b.part[0], b.sums[0],
                     b.rejected, n);
  hipLaunchKernelGGL(k_verify_miller_agg, grid, block, 0, st, vk, b.prep, b.part[0], n);
  return verify_agg_reduce_enqueue(stream, b, n, n_values);
}

}  // namespace rlnamd
