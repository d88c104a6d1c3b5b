// The optimistic form of the device verifier with a team of 8 lanes per proof (verify_agg_team_math.h): the shape for
// the combined check of a call that does not fill the chip with a lane per proof.  A workgroup is one wave = 8 proofs,
// the grid is ceil(n / 8), as in verify_team.hip, whose LDS exchange this unit shares (verify_team_lds.h).  Two kernels
// produce the per-proof partials that verify_agg.hip's lane kernels produce -- the same PrepAgg, Partial and Fr rows
// in HBM -- and the unchanged levels of k_verify_reduce fold them.
//
//   kernel                        LDS per workgroup (8 teams)
//   k_verify_prepare_agg_team      8 192 B   flag words, candidates, the three points
//   k_verify_miller_agg_team      14 848 B   f, the running point, the one line of a step
//
// A team past the end of the batch redoes the last proof and skips only the stores to HBM: no lane leaves before the
// last exchange.  No flag passes between workgroups; the levels of the fold stay separate launches (verify_agg.hip
// says why).  A unit of its own, so that verify_agg.hip and verify_team.hip compile to what they did.
#include "verify.h"

#include "common.h"
#include "verify_agg_team_math.h"
#include "verify_team_lds.h"

namespace rlnamd {

using vm::Partial;
using vm::PrepAgg;
using vm::PreparedKey;

// proofs: n x 32 words, vals: n x nv x 8 words, scalars: n x 4 words
__global__ __launch_bounds__(64) void k_verify_prepare_agg_team(const PreparedKey* __restrict__ vk, const uint32_t* __restrict__ proofs,
                                                                const uint32_t* __restrict__ vals, const uint32_t* __restrict__ scalars,
                                                                PrepAgg* __restrict__ prep, Partial* __restrict__ part,
                                                                Fr* __restrict__ sums, uint8_t* __restrict__ rejected, uint32_t n) {
  const vt::TeamIndex ti = vt::team_index(blockIdx.x, threadIdx.x / vt::TEAM, n);
  const LdsX x = team_exchange(vt::PREP_SLOTS, vt::PREP_AGG_SCRATCH);
  const uint32_t nv = vk->n_values;
  vt::t_prepare_agg(x, vk, proofs + (size_t)32 * ti.i, vals + (size_t)8 * nv * ti.i, scalars + (size_t)4 * ti.i, &prep[ti.i],
                    &part[ti.i].c, sums + (size_t)(nv + 1) * ti.i, &rejected[ti.i], ti.live);
}
// lanes 0..5 of a live team write coefficient k of part[i].f
__global__ __launch_bounds__(64) void k_verify_miller_agg_team(const PreparedKey* __restrict__ vk, const PrepAgg* __restrict__ prep,
                                                               Partial* __restrict__ part, uint32_t n) {
  const vt::TeamIndex ti = vt::team_index(blockIdx.x, threadIdx.x / vt::TEAM, n);
  const LdsX x = team_exchange(vt::PAIR_SLOTS, vt::PAIR_SCRATCH);
  vt::t_miller_loop_pair(x, vk, &prep[ti.i]);
  if (ti.live && x.lane < 6) part[ti.i].f.c[x.lane] = x.f(0, x.lane);
}

int verify_agg_team_enqueue(void* stream, const PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals,
                            const uint32_t* scalars, const AggBuffers& b, uint32_t n, uint32_t n_values) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(div_up(n, vt::TEAMS_PER_WAVE)), block(64);
  hipLaunchKernelGGL(k_verify_prepare_agg_team, grid, block, lds_bytes(vt::PREP_SLOTS, vt::PREP_AGG_SCRATCH), st, vk, proofs,
                     vals, scalars, b.prep, b.part[0], b.sums[0], b.rejected, n);
  hipLaunchKernelGGL(k_verify_miller_agg_team, grid, block, lds_bytes(vt::PAIR_SLOTS, vt::PAIR_SCRATCH), st, vk, b.prep,
                     b.part[0], n);
  return verify_agg_reduce_enqueue(stream, b, n, n_values);
}

}  // namespace rlnamd
