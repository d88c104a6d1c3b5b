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
#include "verify_team_math.h"

namespace rlnamd {

using vm::F12;
using vm::Prep;
using vm::PreparedKey;

extern __shared__ uint4 vt_lds_raw[];

namespace {

// The device's exchange (verify_team_math.h): this thread is one lane of one team, the team's memory is a slice of LDS
struct LdsX {
  static constexpr int NL = 1;
  uint32_t base;  // the team's first Fq2 unit
  int lane, n_slots;
  __device__ __forceinline__ int lane_lo() const { return lane; }
  __device__ __forceinline__ int lane_hi() const { return lane + 1; }
  __device__ __forceinline__ int li(int) const { return 0; }
  __device__ __forceinline__ Fq2* mem() const { return reinterpret_cast<Fq2*>(vt_lds_raw) + base; }
  __device__ __forceinline__ Fq2& f(int slot, int i) const { return mem()[2 + 6 * slot + i]; }
  __device__ __forceinline__ Fq2& s(int i) const { return mem()[2 + 6 * n_slots + i]; }
  __device__ __forceinline__ uint32_t& w(int i) const { return reinterpret_cast<uint32_t*>(mem())[i]; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};
__device__ __forceinline__ LdsX team_exchange(int n_slots, int n_scratch) {
  const uint32_t team = threadIdx.x / vt::TEAM;
  return {team * (uint32_t)vt::team_units(n_slots, n_scratch), (int)(threadIdx.x % vt::TEAM), n_slots};
}
constexpr size_t lds_bytes(int n_slots, int n_scratch) {
  return (size_t)vt::TEAMS_PER_WAVE * vt::team_units(n_slots, n_scratch) * sizeof(Fq2);
}

}  // namespace

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
