// Groth16 verification on the device: a lane per proof (the kernels below) or a team of 8 lanes per proof
// (verify_team.hip; GpuVerifier::verify chooses by the size of the call), three kernels per chunk (decompress + subgroup test + public
// input combination -> Miller loop -> final exponentiation) with a small per-proof record in HBM between them.  The
// mathematics is verify_math.h; the prepared verifying key (line coefficients of gamma and delta, the Miller value of
// (-alpha, beta), the d * IC_i rows, Frobenius constants: a few tens of KiB) is uploaded once and read at
// wave-uniform addresses.
//
// The Fq12-level routines of verify_math.h are out of line; the base-field products inside them are inlined (the
// two-product forms with one Montgomery reduction, field.h).  The build with one shared out-of-line product
// (RLN_NOINLINE_MUL) compiles three times faster and was 16 % slower on the device (35.5 against 30.0 ms per pass up to
// 8 192 proofs, alternated on one box; profiles/verify_gpu.md).
#include "verify.h"

#include <string.h>

#include <mutex>
#include <vector>

#include "common.h"
#include "prover.h"
#include "verify_key.h"

namespace rlnamd {

using vm::F12;
using vm::Prep;
using vm::PreparedKey;

// proofs: n x 32 words, vals: n x nv x 8 words
__global__ __launch_bounds__(64) void k_verify_prepare(const PreparedKey* __restrict__ vk, const uint32_t* __restrict__ proofs,
                                                       const uint32_t* __restrict__ vals, Prep* __restrict__ prep, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  vm::prepare(vk, proofs + (size_t)32 * i, vals + (size_t)8 * vk->n_values * i, &prep[i]);
}
__global__ __launch_bounds__(64) void k_verify_miller(const PreparedKey* __restrict__ vk, const Prep* __restrict__ prep,
                                                      F12* __restrict__ f, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  F12 acc;
  vm::miller_loop(vk, &prep[i], &acc);
  vm::f12_mul(&acc, &acc, &vk->alpha_beta);
  f[i] = acc;
}
// ok and gt may each be null
__global__ __launch_bounds__(64) void k_verify_final_exp(const PreparedKey* __restrict__ vk, const Prep* __restrict__ prep,
                                                         const F12* __restrict__ f, uint8_t* __restrict__ ok,
                                                         uint32_t* __restrict__ gt, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  F12 acc = f[i];
  vm::final_exponentiation(vk, &acc, &acc);
  const bool rejected = (prep[i].flags & vm::P_REJECT) != 0;
  if (ok) ok[i] = (!rejected && vm::f12_is_one(acc)) ? 1 : 0;
  if (gt) vm::gt_words(acc, rejected, gt + (size_t)96 * i);
}

struct GpuVerifier::Impl {
  std::mutex mu;
  int dev = 0;
  size_t nv = 0;
  hipStream_t st = nullptr;
  DevBuf<PreparedKey> key;
  DevBuf<G1Affine> ic;
  // Proofs and public inputs are public: nothing here is secret, so none of these buffers is wiped after use and
  // rlnamd_prover_residue does not look at them.
  DevBuf<uint32_t> d_in;    // CHUNK x (32 + 8 nv) words: the proofs, then the values
  DevBuf<Prep> d_prep;
  DevBuf<F12> d_f;
  DevBuf<uint8_t> d_ok;
  DevBuf<uint32_t> d_gt;    // allocated by the first call that asks for GT values
  uint8_t* h_in = nullptr;  // pinned
  uint8_t* h_ok = nullptr;
  uint8_t* h_gt = nullptr;
  size_t cap = 0;           // proofs the buffers hold: grows to the largest chunk seen, at most CHUNK
  int forced_lanes = 0;     // 0: the shape follows the size of the call
  size_t n_passes[2] = {0, 0};   // chunks run with a lane per proof, in team form (under mu)

  void reserve(size_t n, bool want_gt) {
    if (n > cap) {
      release_host();
      d_in.alloc(n * (32 + 8 * nv));
      d_prep.alloc(n);
      d_f.alloc(n);
      d_ok.alloc(n);
      d_gt.release();
      RLN_HIP(hipHostMalloc((void**)&h_in, n * (128 + 32 * nv), hipHostMallocDefault));
      RLN_HIP(hipHostMalloc((void**)&h_ok, n, hipHostMallocDefault));
      cap = n;
    }
    if (want_gt && !d_gt.p) {
      d_gt.alloc(cap * 96);
      RLN_HIP(hipHostMalloc((void**)&h_gt, cap * 384, hipHostMallocDefault));
    }
  }
  void release_host() {
    if (h_in) (void)hipHostFree(h_in);
    if (h_ok) (void)hipHostFree(h_ok);
    if (h_gt) (void)hipHostFree(h_gt);
    h_in = h_ok = h_gt = nullptr;
    cap = 0;
  }
  void chunk(size_t n, const uint8_t* proofs, const uint8_t* values, uint8_t* ok, uint8_t* gt384, bool team) {
    reserve(n, gt384 != nullptr);
    memcpy(h_in, proofs, 128 * n);
    memcpy(h_in + 128 * n, values, 32 * nv * n);
    RLN_HIP(hipMemcpyAsync(d_in.p, h_in, n * (128 + 32 * nv), hipMemcpyHostToDevice, st));
    const uint32_t* d_proofs = d_in.p;
    const uint32_t* d_vals = d_in.p + 32 * n;
    if (team) {
      verify_team_enqueue(st, key.p, d_proofs, d_vals, d_prep.p, d_f.p, ok ? d_ok.p : nullptr, gt384 ? d_gt.p : nullptr,
                          (uint32_t)n);
    } else {
      const dim3 grid(div_up(n, 64)), block(64);
      hipLaunchKernelGGL(k_verify_prepare, grid, block, 0, st, key.p, d_proofs, d_vals, d_prep.p, (uint32_t)n);
      hipLaunchKernelGGL(k_verify_miller, grid, block, 0, st, key.p, d_prep.p, d_f.p, (uint32_t)n);
      hipLaunchKernelGGL(k_verify_final_exp, grid, block, 0, st, key.p, d_prep.p, d_f.p, ok ? d_ok.p : nullptr,
                         gt384 ? d_gt.p : nullptr, (uint32_t)n);
    }
    RLN_HIP(hipGetLastError());
    n_passes[team ? 1 : 0]++;
    if (ok) RLN_HIP(hipMemcpyAsync(h_ok, d_ok.p, n, hipMemcpyDeviceToHost, st));
    if (gt384) RLN_HIP(hipMemcpyAsync(h_gt, d_gt.p, n * 384, hipMemcpyDeviceToHost, st));
    RLN_HIP(hipStreamSynchronize(st));
    if (ok) memcpy(ok, h_ok, n);
    if (gt384) memcpy(gt384, h_gt, n * 384);
  }
};

GpuVerifier::GpuVerifier(const Zkey& zk, int forced_lanes) : d_(new Impl) {
  require_gpu();
  Impl& D = *d_;
  D.forced_lanes = (forced_lanes == 1 || forced_lanes == 8) ? forced_lanes : 0;
  RLN_HIP(hipGetDevice(&D.dev));
  PreparedKey K;
  std::vector<G1Affine> rows;
  vm::prepare_key(zk, &K, &rows);
  D.nv = K.n_values;
  D.ic.alloc(rows.size());
  D.key.alloc(1);
  K.ic_mult = D.ic.p;
  RLN_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
  RLN_HIP(hipMemcpyAsync(D.ic.p, rows.data(), rows.size() * sizeof(G1Affine), hipMemcpyHostToDevice, D.st));
  RLN_HIP(hipMemcpyAsync(D.key.p, &K, sizeof(K), hipMemcpyHostToDevice, D.st));
  RLN_HIP(hipStreamSynchronize(D.st));
}

GpuVerifier::~GpuVerifier() {
  if (!d_) return;
  if (d_->st) {
    (void)hipStreamSynchronize(d_->st);
    (void)hipStreamDestroy(d_->st);
  }
  d_->release_host();
}

void GpuVerifier::verify(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, uint8_t* ok,
                         uint8_t* gt384, int lanes) {
  Impl& D = *d_;
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("verify: lanes must be 0 (choose), 1 or 8");
  if (nv != D.nv) throw Error("MalformedVerifyingKey");
  if (n == 0) return;
  std::lock_guard<std::mutex> lk(D.mu);
  // One threshold: a call that a lane per proof cannot spread over the chip takes teams
  if (lanes == 0) lanes = D.forced_lanes ? D.forced_lanes : (n <= TEAM_MAX ? 8 : 1);
  const bool team = lanes == 8;
  const size_t step = team ? TEAM_CHUNK : CHUNK;
  int cur = 0;
  RLN_HIP(hipGetDevice(&cur));
  if (cur != D.dev) RLN_HIP(hipSetDevice(D.dev));
  try {
    for (size_t off = 0; off < n; off += step) {
      const size_t m = n - off < step ? n - off : step;
      D.chunk(m, proofs + 128 * off, values_le + 32 * nv * off, ok ? ok + off : nullptr,
              gt384 ? gt384 + 384 * off : nullptr, team);
    }
  } catch (...) {
    if (cur != D.dev) (void)hipSetDevice(cur);
    throw;
  }
  if (cur != D.dev) RLN_HIP(hipSetDevice(cur));
}

void GpuVerifier::passes(size_t out[2]) {
  std::lock_guard<std::mutex> lk(d_->mu);
  out[0] = d_->n_passes[0];
  out[1] = d_->n_passes[1];
}

GpuVerifier& Prover::gpu_verifier() {
  std::lock_guard<std::mutex> lk(verifier_mu_);
  if (!verifier_) verifier_ = std::make_shared<GpuVerifier>(zk_, tuning().verify_lanes);
  return *verifier_;
}

}  // namespace rlnamd
