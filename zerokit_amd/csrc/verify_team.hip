// Groth16 verification on the device with a team of 8 lanes per proof: the shape for calls that do not fill the chip
// with a lane per proof (verify.hip).  A workgroup is one wave = 8 proofs, the grid is ceil(n / 8), so 8 192 proofs are
// one wave for each SIMD of an MI355X.  Three kernels per chunk with the same Prep / F12 records in HBM between them
// and the same prepared key as the lane-per-proof kernels; the mathematics is verify_team_math.h, whose exchange
// memory is LDS here: every Fq12 value and every point of the Miller loop lives there (lane k writes its 64-byte
// coefficient, reads what its row needs; the lanes of a team read the same operand at the same address).
//
//   kernel                      LDS per workgroup (8 teams)
//   k_verify_prepare_team       17 408 B   flag words, candidates, points, one x_i IC_i per lane
//   k_verify_miller_team        22 528 B   f, alpha_beta, the running point, the lines of a step
//   k_verify_final_exp_team     31 744 B   the ten Fq12 temporaries of the final exponentiation
//
// A team past the end of the batch redoes the last proof and skips only the stores to HBM: no lane leaves before the
// last exchange.  A unit of its own, so that verify.hip compiles to what it did before and the two build in parallel.
#include "verify.h"

#include "common.h"
#include "verify_team_lds.h"   // the device's exchange: LdsX, team_exchange, lds_bytes

namespace rlnamd {

using vm::F12;
using vm::Prep;
using vm::PreparedKey;

// proofs: n x 32 words, vals: n x nv x 8 words
__global__ __launch_bounds__(64) void k_verify_prepare_team(const PreparedKey* __restrict__ vk, const uint32_t* __restrict__ proofs,
                                                            const uint32_t* __restrict__ vals, Prep* __restrict__ prep, uint32_t n) {
  const vt::TeamIndex ti = vt::team_index(blockIdx.x, threadIdx.x / vt::TEAM, n);
  const LdsX x = team_exchange(vt::PREP_SLOTS, vt::PREP_SCRATCH);
  vt::t_prepare(x, vk, proofs + (size_t)32 * ti.i, vals + (size_t)8 * vk->n_values * ti.i, &prep[ti.i], ti.live);
}
__global__ __launch_bounds__(64) void k_verify_miller_team(const PreparedKey* __restrict__ vk, const Prep* __restrict__ prep,
                                                           F12* __restrict__ f, uint32_t n) {
  const vt::TeamIndex ti = vt::team_index(blockIdx.x, threadIdx.x / vt::TEAM, n);
  const LdsX x = team_exchange(vt::MILLER_SLOTS, vt::MILLER_SCRATCH);
  vt::t_miller_loop(x, vk, &prep[ti.i]);
  if (ti.live && x.lane < 6) f[ti.i].c[x.lane] = x.f(0, x.lane);
}
// ok and gt may each be null
__global__ __launch_bounds__(64) void k_verify_final_exp_team(const PreparedKey* __restrict__ vk, const Prep* __restrict__ prep,
                                                              const F12* __restrict__ f, uint8_t* __restrict__ ok,
                                                              uint32_t* __restrict__ gt, uint32_t n) {
  const vt::TeamIndex ti = vt::team_index(blockIdx.x, threadIdx.x / vt::TEAM, n);
  const LdsX x = team_exchange(vt::FINAL_SLOTS, vt::FINAL_SCRATCH);
  vt::t_load(x, 0, &f[ti.i]);
  vt::t_final_exponentiation(x, vk);
  vt::t_finish(x, &prep[ti.i], ti.live, ok ? ok + ti.i : nullptr, gt ? gt + (size_t)96 * ti.i : nullptr);
}

void verify_team_enqueue(void* stream, const PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals, Prep* prep,
                         F12* f, uint8_t* ok, uint32_t* gt, uint32_t n) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(div_up(n, vt::TEAMS_PER_WAVE)), block(64);
  hipLaunchKernelGGL(k_verify_prepare_team, grid, block, lds_bytes(vt::PREP_SLOTS, vt::PREP_SCRATCH), st, vk, proofs, vals,
                     prep, n);
  hipLaunchKernelGGL(k_verify_miller_team, grid, block, lds_bytes(vt::MILLER_SLOTS, vt::MILLER_SCRATCH), st, vk, prep, f, n);
  hipLaunchKernelGGL(k_verify_final_exp_team, grid, block, lds_bytes(vt::FINAL_SLOTS, vt::FINAL_SCRATCH), st, vk, prep, f,
                     ok, gt, n);
}

}  // namespace rlnamd
