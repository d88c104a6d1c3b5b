// Device Groth16 verifier (verify.hip): n compressed proofs and their public inputs in, one verdict per proof out,
// with the accept / reject decisions of the host path (capi.cpp: verify_common).  One per Prover, made on first use
// (Prover::gpu_verifier); it owns its stream, its device buffers and its pinned staging and never takes the prover's
// locks or slots, so verification and proving may be in flight on one device at the same time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>

#include "zkey.h"

namespace rlnamd {

class GpuVerifier {
 public:
  // Proofs per pass over the three kernels.  A lane verifies one proof, a workgroup is one wave, so a full chunk is
  // 1 024 waves: one for each SIMD of an MI355X (256 CUs x 4).  Staging for a chunk is 65 536 x (128 + 32 n_values)
  // bytes of pinned memory in and 65 536 bytes out; any n runs as ceil(n / CHUNK) passes.
  static constexpr size_t CHUNK = 65536;
  explicit GpuVerifier(const Zkey& zk);   // uploads the prepared key to the current device
  ~GpuVerifier();
  GpuVerifier(const GpuVerifier&) = delete;
  GpuVerifier& operator=(const GpuVerifier&) = delete;
  // ok (n bytes) and gt384 (n x 384 bytes, the final-exponentiated pairing products) may each be null.  Throws
  // MalformedVerifyingKey when nv + 1 is not the key's gamma_abc_g1.size().  Calls from several threads serialise.
  void verify(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, uint8_t* ok, uint8_t* gt384);

 private:
  struct Impl;
  std::unique_ptr<Impl> d_;
};

}  // namespace rlnamd
