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
#include <sys/random.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "common.h"
#include "prover.h"
#include "verify_agg_math.h"
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
  // the optimistic form: its buffers are made by the first call that takes it
  vm::AggKey agg_key;
  DevBuf<vm::PrepAgg> d_pa;
  DevBuf<vm::Partial> d_part[2];
  DevBuf<Fr> d_sums[2];
  uint8_t* h_last = nullptr;     // pinned: the last partial, then its n_values + 1 sums
  size_t agg_cap = 0;
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};   // [5]: the chunks of [0] checked in team form
  size_t cooldown = COOLDOWN_DEFAULT, cooldown_left = 0;
  uint64_t finish_ns = 0, finish_calls = 0;   // the host's share of the combined checks: time inside vm::finish_host
  // the relay's combined chunk between relay_enqueue_combined and relay_settle
  struct Pending {
    size_t n = 0;
    bool team = false;
  } pending;
  uint64_t seeds_drawn = 0;   // the chunk counter of the seeds drawn here: a seed is used once whatever it is

  void reserve(size_t n, bool want_gt) {
    if (n > cap) {
      release_host();
      // + 4 words: a proof's scalar in the optimistic form; + 8: the seed they are derived from, in front of them
      d_in.alloc(n * (32 + 8 * nv + 4) + 8);
      d_prep.alloc(n);
      d_f.alloc(n);
      d_ok.alloc(n);
      d_gt.release();
      RLN_HIP(hipHostMalloc((void**)&h_in, n * (128 + 32 * nv + 16) + 32, hipHostMallocDefault));
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
    if (h_last) (void)hipHostFree(h_last);
    h_in = h_ok = h_gt = h_last = nullptr;
    cap = agg_cap = 0;
  }
  void reserve_agg(size_t n) {
    reserve(n, false);
    if (agg_cap >= cap) return;
    const size_t groups = div_up(cap, (size_t)vm::FOLD);
    d_pa.alloc(cap);
    d_part[0].alloc(cap);
    d_part[1].alloc(groups);
    d_sums[0].alloc(cap * (nv + 1));
    d_sums[1].alloc(groups * (nv + 1));
    if (!h_last) RLN_HIP(hipHostMalloc((void**)&h_last, sizeof(vm::Partial) + (nv + 1) * sizeof(Fr), hipHostMallocDefault));
    agg_cap = cap;
  }
  // One combined check over n <= CHUNK proofs: the final-exponentiated value, and rejected[i] = 1 where the reject
  // rules refuse proof i.  scalars16: null (drawn here, after the proofs were copied into the staging buffer, which
  // is what the device reads) or n x 16 bytes.  team: a team of 8 lanes per proof, n <= TEAM_CHUNK.
  Fq12 agg_chunk(size_t n, const uint8_t* proofs, const uint8_t* values, const uint8_t* scalars16, uint8_t* rejected,
                 bool team) {
    reserve_agg(n);
    memcpy(h_in, proofs, 128 * n);
    memcpy(h_in + 128 * n, values, 32 * nv * n);
    uint8_t* sc = h_in + (128 + 32 * nv) * n;
    if (scalars16) {
      memcpy(sc, scalars16, 16 * n);
    } else {
      for (size_t off = 0; off < 16 * n;) {   // getrandom returns at most 32 MiB - 1 bytes per call
        const ssize_t got = getrandom(sc + off, 16 * n - off, 0);
        if (got < 0) throw Error("verify_optimistic: getrandom failed");
        off += (size_t)got;
      }
      static const uint8_t zero[16] = {0};
      for (size_t i = 0; i < n; i++)
        while (!memcmp(sc + 16 * i, zero, 16))
          if (getrandom(sc + 16 * i, 16, 0) != 16) throw Error("verify_optimistic: getrandom failed");
    }
    RLN_HIP(hipMemcpyAsync(d_in.p, h_in, n * (128 + 32 * nv + 16), hipMemcpyHostToDevice, st));
    const AggBuffers b{d_pa.p, {d_part[0].p, d_part[1].p}, {d_sums[0].p, d_sums[1].p}, d_ok.p};
    const int at = (team ? verify_agg_team_enqueue : verify_agg_enqueue)(st, key.p, d_in.p, d_in.p + 32 * n,
                                                                         d_in.p + (32 + 8 * nv) * n, b, (uint32_t)n,
                                                                         (uint32_t)nv);
    RLN_HIP(hipGetLastError());
    agg_copy_back(n, at);
    RLN_HIP(hipStreamSynchronize(st));
    memcpy(rejected, h_ok, n);
    return agg_finish();
  }
  // the copies back of a combined check, enqueued: the last partial, its sums and the n reject flags
  void agg_copy_back(size_t n, int at) {
    RLN_HIP(hipMemcpyAsync(h_last, d_part[at].p, sizeof(vm::Partial), hipMemcpyDeviceToHost, st));
    RLN_HIP(hipMemcpyAsync(h_last + sizeof(vm::Partial), d_sums[at].p, (nv + 1) * sizeof(Fr), hipMemcpyDeviceToHost, st));
    RLN_HIP(hipMemcpyAsync(h_ok, d_ok.p, n, hipMemcpyDeviceToHost, st));
  }
  // the host's finish over what agg_copy_back brought, once the stream has been waited for
  Fq12 agg_finish() {
    vm::Partial last;
    std::vector<Fr> sums(nv + 1);
    memcpy(&last, h_last, sizeof(last));
    memcpy(sums.data(), h_last + sizeof(last), (nv + 1) * sizeof(Fr));
    const auto t0 = std::chrono::steady_clock::now();
    const Fq12 value = vm::finish_host(agg_key, last, sums.data());
    finish_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    finish_calls++;
    return value;
  }
  // agg_chunk's front with the scalars derived on the device (verify_agg_scalars.h), enqueued and not waited for.  The
  // staging buffer holds proofs | values | seed and goes up in one copy; on the device the scalars lie 8 words behind
  // the values, behind the seed, because every lane of the scalar kernel reads the seed.  seed32: null (drawn here,
  // after the proofs were copied into the staging buffer) or given, then `chunk` is the caller's counter.
  void agg_enqueue_seeded(size_t n, const uint8_t* proofs, const uint8_t* values, const uint8_t* seed32, uint64_t chunk,
                          bool team) {
    reserve_agg(n);
    memcpy(h_in, proofs, 128 * n);
    memcpy(h_in + 128 * n, values, 32 * nv * n);
    uint8_t* sd = h_in + (128 + 32 * nv) * n;
    if (seed32) {
      memcpy(sd, seed32, 32);
    } else {
      for (size_t off = 0; off < 32;) {
        const ssize_t got = getrandom(sd + off, 32 - off, 0);
        if (got < 0) throw Error("verify_optimistic: getrandom failed");
        off += (size_t)got;
      }
      chunk = seeds_drawn++;
    }
    RLN_HIP(hipMemcpyAsync(d_in.p, h_in, n * (128 + 32 * nv) + 32, hipMemcpyHostToDevice, st));
    uint32_t* d_seed = d_in.p + (32 + 8 * nv) * n;
    uint32_t* d_scalars = d_seed + 8;
    verify_agg_scalars_enqueue(st, d_seed, chunk, d_scalars, (uint32_t)n);
    const AggBuffers b{d_pa.p, {d_part[0].p, d_part[1].p}, {d_sums[0].p, d_sums[1].p}, d_ok.p};
    const int at = (team ? verify_agg_team_enqueue : verify_agg_enqueue)(st, key.p, d_in.p, d_in.p + 32 * n, d_scalars, b,
                                                                         (uint32_t)n, (uint32_t)nv);
    RLN_HIP(hipGetLastError());
    agg_copy_back(n, at);
  }
  // runs f with the verifier's device current
  template <class F>
  void on_device(F f) {
    int cur = 0;
    RLN_HIP(hipGetDevice(&cur));
    if (cur != dev) RLN_HIP(hipSetDevice(dev));
    try {
      f();
    } catch (...) {
      if (cur != dev) (void)hipSetDevice(cur);
      throw;
    }
    if (cur != dev) RLN_HIP(hipSetDevice(cur));
  }
  // the copy in and the three kernels of one chunk, enqueued
  void enqueue_chunk(size_t n, const uint8_t* proofs, const uint8_t* values, bool ok, bool gt, bool team) {
    reserve(n, gt);
    memcpy(h_in, proofs, 128 * n);
    memcpy(h_in + 128 * n, values, 32 * nv * n);
    RLN_HIP(hipMemcpyAsync(d_in.p, h_in, n * (128 + 32 * nv), hipMemcpyHostToDevice, st));
    enqueue_exact(n, ok, gt, team);
  }
  // the three kernels of one chunk over the n proofs and values resident in d_in, enqueued
  void enqueue_exact(size_t n, bool ok, bool gt, bool team) {
    const uint32_t* d_proofs = d_in.p;
    const uint32_t* d_vals = d_in.p + 32 * n;
    if (team) {
      verify_team_enqueue(st, key.p, d_proofs, d_vals, d_prep.p, d_f.p, ok ? d_ok.p : nullptr, gt ? d_gt.p : nullptr,
                          (uint32_t)n);
    } else {
      const dim3 grid(div_up(n, 64)), block(64);
      hipLaunchKernelGGL(k_verify_prepare, grid, block, 0, st, key.p, d_proofs, d_vals, d_prep.p, (uint32_t)n);
      hipLaunchKernelGGL(k_verify_miller, grid, block, 0, st, key.p, d_prep.p, d_f.p, (uint32_t)n);
      hipLaunchKernelGGL(k_verify_final_exp, grid, block, 0, st, key.p, d_prep.p, d_f.p, ok ? d_ok.p : nullptr,
                         gt ? d_gt.p : nullptr, (uint32_t)n);
    }
    RLN_HIP(hipGetLastError());
    n_passes[team ? 1 : 0]++;
  }
  void chunk(size_t n, const uint8_t* proofs, const uint8_t* values, uint8_t* ok, uint8_t* gt384, bool team) {
    enqueue_chunk(n, proofs, values, ok != nullptr, gt384 != nullptr, team);
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
  D.agg_key = vm::agg_key(zk);
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
  D.on_device([&]() {
    for (size_t off = 0; off < n; off += step) {
      const size_t m = n - off < step ? n - off : step;
      D.chunk(m, proofs + 128 * off, values_le + 32 * nv * off, ok ? ok + off : nullptr,
              gt384 ? gt384 + 384 * off : nullptr, team);
    }
  });
}

static void check_scalars(size_t n, const uint8_t* scalars16) {
  static const uint8_t zero[16] = {0};
  for (size_t i = 0; scalars16 && i < n; i++)
    if (!memcmp(scalars16 + 16 * i, zero, 16)) throw Error("verify_optimistic: a supplied scalar is zero");
}

void GpuVerifier::verify_optimistic(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv,
                                    const uint8_t* scalars16, uint8_t* ok, int lanes, bool team_checks) {
  Impl& D = *d_;
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("verify: lanes must be 0 (choose), 1 or 8");
  if (nv != D.nv) throw Error("MalformedVerifyingKey");
  if (n == 0) return;
  if (!proofs || !values_le || !ok) throw Error("verify_optimistic: null argument");
  check_scalars(n, scalars16);
  // verify()'s choice.  TEAM_MAX was measured for the exact forms only; the combined check keeps it so that a call
  // size means one shape, whichever form runs
  if (lanes == 0) lanes = D.forced_lanes ? D.forced_lanes : (n <= TEAM_MAX ? 8 : 1);
  const bool team = lanes == 8;
  if (team && !team_checks) return verify(n, proofs, values_le, nv, ok, nullptr, 8);   // teams: not aggregated
  const size_t step = team ? TEAM_CHUNK : CHUNK;
  std::lock_guard<std::mutex> lk(D.mu);
  D.on_device([&]() {
    for (size_t off = 0; off < n; off += step) {
      const size_t m = n - off < step ? n - off : step;
      const uint8_t *pr = proofs + 128 * off, *va = values_le + 32 * nv * off;
      if (D.cooldown_left) {
        D.cooldown_left--;
        D.stats[3]++;
        D.chunk(m, pr, va, ok + off, nullptr, team);
        continue;
      }
      D.stats[0]++;
      if (team) D.stats[5]++;
      const bool accept = D.agg_chunk(m, pr, va, scalars16 ? scalars16 + 16 * off : nullptr, ok + off, team).is_one();
      size_t refused = 0;
      for (size_t i = 0; i < m; i++) {
        refused += ok[off + i];
        ok[off + i] = ok[off + i] ? 0 : 1;
      }
      D.stats[4] += refused;
      if (accept) {
        D.stats[1]++;
      } else {
        D.stats[2]++;
        D.cooldown_left = D.cooldown;
        D.chunk(m, pr, va, ok + off, nullptr, team);   // the exact pass of the same shape names the bad ones
      }
    }
  });
}

void GpuVerifier::aggregate(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv,
                            const uint8_t* scalars16, uint8_t gt384[384], uint8_t* rejected, int lanes) {
  Impl& D = *d_;
  if (lanes != 1 && lanes != 8) throw Error("verify_aggregate: lanes must be 1 or 8");
  if (nv != D.nv) throw Error("MalformedVerifyingKey");
  if (!gt384 || (n && (!proofs || !values_le || !rejected))) throw Error("verify_aggregate: null argument");
  check_scalars(n, scalars16);
  Fq12 all = Fq12::one();
  std::lock_guard<std::mutex> lk(D.mu);
  D.on_device([&]() {
    const size_t step = lanes == 8 ? TEAM_CHUNK : CHUNK;
    for (size_t off = 0; off < n; off += step) {
      const size_t m = n - off < step ? n - off : step;
      all = f12_mul(all, D.agg_chunk(m, proofs + 128 * off, values_le + 32 * nv * off,
                                     scalars16 ? scalars16 + 16 * off : nullptr, rejected + off, lanes == 8));
    }
  });
  vm::fq12_words(all, gt384);
}

void GpuVerifier::aggregate_seeded(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv,
                                   const uint8_t seed32[32], uint8_t gt384[384], uint8_t* rejected, int lanes) {
  Impl& D = *d_;
  if (lanes != 1 && lanes != 8) throw Error("verify_aggregate: lanes must be 1 or 8");
  if (nv != D.nv) throw Error("MalformedVerifyingKey");
  if (!gt384 || !seed32 || (n && (!proofs || !values_le || !rejected))) throw Error("verify_aggregate: null argument");
  Fq12 all = Fq12::one();
  std::lock_guard<std::mutex> lk(D.mu);
  D.on_device([&]() {
    const size_t step = lanes == 8 ? TEAM_CHUNK : CHUNK;
    for (size_t off = 0, c = 0; off < n; off += step, c++) {
      const size_t m = n - off < step ? n - off : step;
      D.agg_enqueue_seeded(m, proofs + 128 * off, values_le + 32 * nv * off, seed32, (uint64_t)c, lanes == 8);
      RLN_HIP(hipStreamSynchronize(D.st));
      memcpy(rejected + off, D.h_ok, m);
      all = f12_mul(all, D.agg_finish());
    }
  });
  vm::fq12_words(all, gt384);
}

void GpuVerifier::set_cooldown(size_t chunks) {
  std::lock_guard<std::mutex> lk(d_->mu);
  d_->cooldown = chunks;
  if (d_->cooldown_left > chunks) d_->cooldown_left = chunks;
}

void GpuVerifier::optimistic_stats(uint64_t out[8]) {
  std::lock_guard<std::mutex> lk(d_->mu);
  for (int i = 0; i < 5; i++) out[i] = d_->stats[i];
  out[5] = d_->cooldown_left;
  out[6] = d_->cooldown;
  out[7] = d_->stats[5];
}

void GpuVerifier::finish_time(uint64_t out[2]) {
  std::lock_guard<std::mutex> lk(d_->mu);
  out[0] = d_->finish_ns;
  out[1] = d_->finish_calls;
}

std::mutex& GpuVerifier::relay_mutex() { return d_->mu; }
int GpuVerifier::device() const { return d_->dev; }
size_t GpuVerifier::n_values() const { return d_->nv; }
void* GpuVerifier::relay_stream() { return (void*)d_->st; }
bool GpuVerifier::relay_team(size_t n, int lanes) const {
  if (lanes == 0) lanes = d_->forced_lanes ? d_->forced_lanes : (n <= TEAM_MAX ? 8 : 1);
  return lanes == 8;
}
GpuVerifier::RelayChunk GpuVerifier::relay_enqueue(size_t n, const uint8_t* proofs, const uint8_t* values_le, bool team) {
  Impl& D = *d_;
  if (n == 0 || n > (team ? TEAM_CHUNK : CHUNK)) throw Error("verify: internal error, a relay chunk of the wrong size");
  D.enqueue_chunk(n, proofs, values_le, true, false, team);
  return RelayChunk{D.d_in.p, D.d_in.p + 32 * n, D.d_ok.p};
}
bool GpuVerifier::relay_cooldown_skip() {
  Impl& D = *d_;
  if (!D.cooldown_left) return false;
  D.cooldown_left--;
  D.stats[3]++;
  return true;
}
void GpuVerifier::relay_enqueue_combined(size_t n, const uint8_t* proofs, const uint8_t* values_le, bool team) {
  Impl& D = *d_;
  if (n == 0 || n > (team ? TEAM_CHUNK : CHUNK)) throw Error("verify: internal error, a relay chunk of the wrong size");
  D.pending = Impl::Pending();
  D.agg_enqueue_seeded(n, proofs, values_le, nullptr, 0, team);
  D.stats[0]++;
  if (team) D.stats[5]++;
  D.pending.n = n;
  D.pending.team = team;
}
GpuVerifier::RelayChunk GpuVerifier::relay_settle() {
  Impl& D = *d_;
  const size_t n = D.pending.n;
  const bool team = D.pending.team;
  if (n == 0) throw Error("verify: internal error, no combined relay chunk is in flight");
  D.pending = Impl::Pending();
  RLN_HIP(hipStreamSynchronize(D.st));
  size_t refused = 0;
  for (size_t i = 0; i < n; i++) refused += D.h_ok[i];
  const bool accept = D.agg_finish().is_one();
  D.stats[4] += refused;
  RelayChunk out{D.d_in.p, D.d_in.p + 32 * n, D.d_ok.p, accept};
  if (accept) {
    D.stats[1]++;
  } else {
    D.stats[2]++;
    D.cooldown_left = D.cooldown;
    D.enqueue_exact(n, true, false, team);   // over the inputs the combined kernels read: nothing is copied in again
  }
  return out;
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
