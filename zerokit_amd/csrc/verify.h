// Device Groth16 verifier (verify.hip): n compressed proofs and their public inputs in, one verdict per proof out,
// with the accept / reject decisions of the host path (capi.cpp: verify_common).  One per Prover, made on first use
// (Prover::gpu_verifier); it owns its stream, its device buffers and its pinned staging and never takes the prover's
// locks or slots, so verification and proving may be in flight on one device at the same time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <mutex>

#include "zkey.h"

namespace rlnamd {

namespace vm {
struct PreparedKey;
struct Prep;
struct F12;
struct PrepAgg;
struct Partial;
}  // namespace vm

class GpuVerifier {
 public:
  // Proofs per pass over the three kernels.  A lane verifies one proof, a workgroup is one wave, so a full chunk is
  // 1 024 waves: one for each SIMD of an MI355X (256 CUs x 4).  Staging for a chunk is 65 536 x (128 + 32 n_values)
  // bytes of pinned memory in and 65 536 bytes out; any n runs as ceil(n / CHUNK) passes.
  static constexpr size_t CHUNK = 65536;
  // The same pass with a team of 8 lanes per proof (verify_team.hip): 8 proofs per wave, so a full chunk is again one
  // wave per SIMD.  A verification's serial chain is about a third as long, which is what a call that cannot fill the
  // chip with a lane per proof waits for.
  static constexpr size_t TEAM_CHUNK = 8192;
  // verify_team_max: a call of at most this many proofs takes teams when the shape is left to the verifier: the
  // largest measured n at which the teams' median is below the lane-per-proof minimum (profiles/verify_gpu_lanes.md)
  static constexpr size_t TEAM_MAX = 1024;
  // forced_lanes: 0 the verifier chooses by n, 1 / 8 every call that leaves the choice open takes that shape
  // (ProverTuning::verify_lanes)
  explicit GpuVerifier(const Zkey& zk, int forced_lanes = 0);   // uploads the prepared key to the current device
  ~GpuVerifier();
  GpuVerifier(const GpuVerifier&) = delete;
  GpuVerifier& operator=(const GpuVerifier&) = delete;
  // ok (n bytes) and gt384 (n x 384 bytes, the final-exponentiated pairing products) may each be null.  Throws
  // MalformedVerifyingKey when nv + 1 is not the key's gamma_abc_g1.size().  Calls from several threads serialise.
  // lanes: 1 a lane per proof, 8 a team per proof, 0 the verifier's choice; anything else throws.
  void verify(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, uint8_t* ok, uint8_t* gt384,
              int lanes = 0);
  // chunks run so far with a lane per proof ([0]) and in team form ([1]); for tests
  void passes(size_t out[2]);

  // ---- the optimistic form (verify_agg.hip, verify_agg_math.h): the verdicts of verify(), up to the bound below.
  // Per chunk of CHUNK proofs: the proofs that the reject rules of vm::prepare refuse get ok = 0 at once; the rest pass
  // ONE combined pairing check under scalars r_i in [1, 2^128) drawn inside the call (getrandom), after the proofs are
  // fixed.  If it accepts, they all get ok = 1: a chunk that holds an invalid proof is accepted with probability at
  // most about 2^-128 over the scalars.  If it rejects, the chunk runs through the exact pass of verify(), which names
  // the bad proofs, and the next `cooldown` chunks skip the combined check.
  // team_checks false: taken only where verify() would run a lane per proof (n > TEAM_MAX, or lanes = 1); a call that
  // takes teams is verify() unchanged.  team_checks true: a call that takes teams (lanes = 8, or lanes = 0 with
  // n <= TEAM_MAX or teams forced) runs the combined check in team form (verify_agg_team.hip) per chunk of TEAM_CHUNK
  // proofs, and a chunk it rejects runs through the exact team pass.  TEAM_MAX was measured for the exact forms only; it
  // is the threshold of lanes = 0 here too, so that one call size means one shape.  One cool-down serves both shapes.
  // scalars16: null (drawn), or n x 16 bytes little-endian, none zero (a test hook: supplied scalars void the bound).
  void verify_optimistic(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, const uint8_t* scalars16,
                         uint8_t* ok, int lanes = 0, bool team_checks = false);
  // test / diagnosis: the final-exponentiated combined value of all n proofs (the product over the chunks) as
  // gt_words orders it, 1 = accept, and rejected[i] = 1 where the reject rules refuse proof i.  No fallback.
  // lanes: 1 a lane per proof (chunks of CHUNK), 8 a team per proof (chunks of TEAM_CHUNK); anything else throws.
  void aggregate(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, const uint8_t* scalars16,
                 uint8_t gt384[384], uint8_t* rejected, int lanes = 1);
  // the same with the scalars of chunk c of the call derived on the device from (seed32, c): verify_agg_scalars.h
  void aggregate_seeded(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, const uint8_t seed32[32],
                        uint8_t gt384[384], uint8_t* rejected, int lanes = 1);
  // Chunks after a fallback that go straight to the exact pass.  A sender of one bad proof per chunk then costs at
  // most one wasted combined check per cooldown + 1 chunks.  16 is a policy bound on that overhead, not a measured
  // optimum; 0 means no cool-down.
  static constexpr size_t COOLDOWN_DEFAULT = 16;
  void set_cooldown(size_t chunks);
  // [0] chunks checked combined, [1] accepted, [2] fell back, [3] chunks that skipped the check during a cool-down,
  // [4] proofs the reject rules refused in combined checks, [5] cool-down chunks left, [6] the setting, [7] the
  // chunks of [0] that were checked in team form
  void optimistic_stats(uint64_t out[8]);
  // diagnosis: [0] nanoseconds the combined checks have spent in vm::finish_host (the host's three fixed pairs and the
  // one final exponentiation per chunk), [1] the number of those calls
  void finish_time(uint64_t out[2]);

  // ---- for the relay step (relay.hip): one chunk of the exact pass enqueued and NOT waited for, its proofs, values and
  // verdicts left on the device for the kernels the relay runs behind an event on relay_stream().  The caller holds
  // relay_mutex() for the whole step, runs on device(), and waits (through that event) before the next chunk: the
  // staging buffer and d_in are the ones verify() uses.
  struct RelayChunk {
    const uint32_t* proofs;   // n x 32 words
    const uint32_t* vals;     // n x n_values x 8 words
    const uint8_t* ok;        // n
    bool ok_is_rejected = false;   // ok[i] = 1 where the reject rules refuse proof i, and every other proof is valid
  };
  std::mutex& relay_mutex();
  int device() const;
  size_t n_values() const;
  void* relay_stream();                         // a hipStream_t
  bool relay_team(size_t n, int lanes) const;   // verify()'s choice of shape for a call of n proofs
  RelayChunk relay_enqueue(size_t n, const uint8_t* proofs, const uint8_t* values_le, bool team);   // n <= the shape's chunk
  // The same chunk under the combined check of verify_optimistic, in two calls so that the caller can enqueue other
  // streams' work between them.  relay_enqueue_combined stages the chunk, draws ONE 32-byte seed (getrandom, after the
  // proofs and values are in the staging buffer), copies both in, and enqueues the scalar kernel
  // (verify_agg_scalars.h), the combined kernels of the shape and the copy back of the last partial, its sums and the n
  // reject flags; it does not wait.  relay_settle waits for the stream, finishes on the host (vm::finish_host) and
  // counts as verify_optimistic counts (optimistic_stats [0] [1] [2] [4] [7], finish_time).  Accepted: the chunk, with
  // ok_is_rejected set.  Rejected: the cool-down is set and the exact kernels of the same shape are enqueued over the
  // proofs and values already resident, with no second copy in; passes() goes up and ok is the exact verdict.
  // relay_cooldown_skip: true while a cool-down lasts (one chunk of it is used up, [3] goes up): the caller then takes
  // relay_enqueue.  The cool-down and the counters are the ones verify_optimistic uses.
  bool relay_cooldown_skip();
  void relay_enqueue_combined(size_t n, const uint8_t* proofs, const uint8_t* values_le, bool team);
  RelayChunk relay_settle();

 private:
  struct Impl;
  std::unique_ptr<Impl> d_;
};

// verify_team.hip: the three team kernels over n <= TEAM_CHUNK proofs, enqueued on `stream` (a hipStream_t)
void verify_team_enqueue(void* stream, const vm::PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals,
                         vm::Prep* prep, vm::F12* f, uint8_t* ok, uint32_t* gt, uint32_t n);


// verify_agg.hip: the kernels of one combined check over n <= CHUNK proofs, enqueued on `stream`.  part[0] and sums[0]
// hold n entries (sums: rows of n_values + 1), part[1] and sums[1] ceil(n / 64); the levels of the fold alternate
// between them.  Returns the index of the pair that holds the last partial in entry 0.
struct AggBuffers {
  vm::PrepAgg* prep;
  vm::Partial* part[2];
  Fr* sums[2];
  uint8_t* rejected;
};
int verify_agg_enqueue(void* stream, const vm::PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals,
                       const uint32_t* scalars, const AggBuffers& b, uint32_t n, uint32_t n_values);
// verify_agg.hip: n scalars of 16 bytes from the 8 seed words at `seed` and the chunk counter (verify_agg_scalars.h),
// enqueued on `stream`.  scalars is 16-byte aligned and does not overlap the seed.
void verify_agg_scalars_enqueue(void* stream, const uint32_t* seed, uint64_t chunk, uint32_t* scalars, uint32_t n);
// verify_agg.hip: the levels of the fold alone, over the n partials in part[0] / sums[0]; the same return value
int verify_agg_reduce_enqueue(void* stream, const AggBuffers& b, uint32_t n, uint32_t n_values);
// verify_agg_team.hip: the same combined check with a team of 8 lanes per proof, n <= TEAM_CHUNK: its two kernels, then
// verify_agg_reduce_enqueue.  Returns what verify_agg_enqueue returns.
int verify_agg_team_enqueue(void* stream, const vm::PreparedKey* vk, const uint32_t* proofs, const uint32_t* vals,
                            const uint32_t* scalars, const AggBuffers& b, uint32_t n, uint32_t n_values);

}  // namespace rlnamd
