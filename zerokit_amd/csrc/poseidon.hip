#include "poseidon.h"

#include <mutex>

namespace rlnamd {

__global__ void k_fr_to29(const Fr* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr29 v = Fr29::from_fq(src[t]);
  v.normalize();
#pragma unroll
  for (int k = 0; k < 9; k++) dst[t * 9 + k] = v.v[k];
}

void PoseidonDev::init() {
  if (ready) return;
  require_gpu();
  for (int t = 2; t <= POSEIDON_MAX_T; t++) {
    PoseidonParams P = poseidon_derive_params(t);
    rf[t] = P.rf;
    rp[t] = P.rp;
    ark[t].alloc(P.ark.size());
    mds[t].alloc(P.mds.size());
    RLN_HIP(hipMemcpy(ark[t].p, P.ark.data(), P.ark.size() * sizeof(Fr), hipMemcpyHostToDevice));
    RLN_HIP(hipMemcpy(mds[t].p, P.mds.data(), P.mds.size() * sizeof(Fr), hipMemcpyHostToDevice));
    ark29[t].alloc(P.ark.size() * 9);
    mds29[t].alloc(P.mds.size() * 9);
    hipLaunchKernelGGL(k_fr_to29, dim3(div_up(P.ark.size(), 64)), dim3(64), 0, 0, ark[t].p, ark29[t].p, (uint32_t)P.ark.size());
    hipLaunchKernelGGL(k_fr_to29, dim3(div_up(P.mds.size(), 64)), dim3(64), 0, 0, mds[t].p, mds29[t].p, (uint32_t)P.mds.size());
    // sparse partial rounds: k0 | row0 | u | a_fin | ark2
    std::vector<Fr> all;
    off_k0[t] = all.size(); all.insert(all.end(), P.k0.begin(), P.k0.end());
    off_row0[t] = all.size(); all.insert(all.end(), P.row0.begin(), P.row0.end());
    off_u[t] = all.size(); all.insert(all.end(), P.u.begin(), P.u.end());
    off_afin[t] = all.size(); all.insert(all.end(), P.a_fin.begin(), P.a_fin.end());
    off_ark2[t] = all.size(); all.insert(all.end(), P.ark2.begin(), P.ark2.end());
    DevBuf<Fr> tmp(all.size());
    RLN_HIP(hipMemcpy(tmp.p, all.data(), all.size() * sizeof(Fr), hipMemcpyHostToDevice));
    opt29[t].alloc(all.size() * 9);
    hipLaunchKernelGGL(k_fr_to29, dim3(div_up(all.size(), 64)), dim3(64), 0, 0, tmp.p, opt29[t].p, (uint32_t)all.size());
    RLN_HIP(hipDeviceSynchronize());
  }
  ready = true;
}

// one constant set per device: hipMalloc'ed memory belongs to the device that was current, and a process may drive
// several (rlnamd_pool: one replica per GPU)
PoseidonDev& poseidon_dev() {
  static std::mutex mu;
  static PoseidonDev per_device[64];
  int dev = 0;
  RLN_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) throw Error("device ordinal out of range");
  std::lock_guard<std::mutex> lk(mu);
  per_device[dev].init();
  return per_device[dev];
}

PoseidonView poseidon_view(int t) {
  if (t < 2 || t > POSEIDON_MAX_T) throw Error("unsupported Poseidon width t=" + std::to_string(t));
  PoseidonDev& d = poseidon_dev();
  const uint32_t* o = d.opt29[t].p;
  return {d.ark[t].p, d.mds[t].p, d.rf[t], d.rp[t], d.ark29[t].p, d.mds29[t].p, o + 9 * d.off_k0[t], o + 9 * d.off_row0[t],
          o + 9 * d.off_u[t], o + 9 * d.off_afin[t], o + 9 * d.off_ark2[t]};
}

template <int T>
__global__ void __launch_bounds__(256) k_poseidon_batch(const uint32_t* __restrict__ in, size_t n,
                                                        uint32_t* __restrict__ out, PoseidonView pv) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr x[T - 1];
#pragma unroll
  for (int j = 0; j < T - 1; j++) x[j] = Fr::from_canonical(in + (i * (T - 1) + j) * 8);
  Fr h = poseidon_hash_dev<T>(x, pv);
  h.to_canonical(out + i * 8);
}

void poseidon_hash_batch_device(const uint8_t* d_in, size_t n, int arity, uint8_t* d_out, hipStream_t s) {
  if (n == 0) return;
  PoseidonView pv = poseidon_view(arity + 1);
  dim3 grid(div_up(n, 256)), block(256);
  const uint32_t* in = (const uint32_t*)d_in;
  uint32_t* out = (uint32_t*)d_out;
  switch (arity) {
    case 1: hipLaunchKernelGGL(k_poseidon_batch<2>, grid, block, 0, s, in, n, out, pv); break;
    case 2: hipLaunchKernelGGL(k_poseidon_batch<3>, grid, block, 0, s, in, n, out, pv); break;
    case 3: hipLaunchKernelGGL(k_poseidon_batch<4>, grid, block, 0, s, in, n, out, pv); break;
    case 4: hipLaunchKernelGGL(k_poseidon_batch<5>, grid, block, 0, s, in, n, out, pv); break;
    case 5: hipLaunchKernelGGL(k_poseidon_batch<6>, grid, block, 0, s, in, n, out, pv); break;
    case 6: hipLaunchKernelGGL(k_poseidon_batch<7>, grid, block, 0, s, in, n, out, pv); break;
    case 7: hipLaunchKernelGGL(k_poseidon_batch<8>, grid, block, 0, s, in, n, out, pv); break;
    case 8: hipLaunchKernelGGL(k_poseidon_batch<9>, grid, block, 0, s, in, n, out, pv); break;
    default: throw Error("unsupported Poseidon arity " + std::to_string(arity));
  }
  RLN_HIP(hipGetLastError());
}

}  // namespace rlnamd
