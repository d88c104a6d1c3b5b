// The device's exchange memory for the team forms of the verifier (verify_team_math.h's policy X): this thread is one
// lane of one team, the team's memory is a slice of the workgroup's dynamic LDS.  Shared by verify_team.hip and
// verify_agg_team.hip; device units only.
#pragma once
#include "verify_team_math.h"

namespace rlnamd {

extern __shared__ uint4 vt_lds_raw[];

namespace {

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

}  // namespace rlnamd
