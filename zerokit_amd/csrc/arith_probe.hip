// Arithmetic probes (test support, beside rlnamd_selftest_fq29): the device branches of field.h (inline-asm carry chains,
// the generated product-scanning multiply of mont_mac.inc), every primitive of fq29.h with its lane-form group laws,
// poseidon.h's five-term dot product and witness_ops.h's witness_slow_op, each run on operand tuples the caller supplies.
// The proving kernels reach these functions only with pseudo-random operands; here a test chooses them (limbs at their
// class maxima, values that land on p before the conditional subtraction, carries in every column) and compares the raw
// results with big-integer arithmetic (tests/test_gpu_field_ops.py).
//
// One lane handles one tuple (blockDim = 64, guarded tail); operands are loaded from global memory, so nothing
// constant-folds; results are stored as the function returned them.  The host side copies in and out and converts nothing.
// Same functions, same flags as the shipped kernels (no RLN_NOINLINE_MUL, no RLN_DEVICE_FERMAT); one kernel holds all
// operations of a field behind a switch, so register allocation around them may differ from a proving kernel's.
#include "arith_probe.h"

#include <type_traits>

#include "../../include/rln_amd.h"
#include "common.h"
#include "curve.h"
#include "fq29.h"
#include "poseidon.h"
#include "prover_kernels.h"
#include "prover_plan.h"
#include "witness_ops.h"

namespace rlnamd {
namespace {

struct Shape {
  uint32_t in_words, out_words;
};

// ---- 8 x 32 --------------------------------------------------------------------------------------------------
// operands and results are 8-word elements; {number of operands, number of results} per operation
constexpr Shape FIELD_SHAPE[RLNAMD_PROBE_FP_OPS] = {
    {2, 1}, {2, 1}, {1, 1}, {1, 1}, {2, 1}, {1, 1},   // add sub neg dbl mul sqr
    {4, 1}, {6, 1}, {8, 1}, {4, 1},                   // dot2 dot3 dot4 dot2_sub
    {1, 1}, {1, 1}, {1, 1},                           // from_canonical to_canonical inv
    {4, 2}, {2, 2}, {2, 2},                           // Fq2 mul sqr inv
};

template <class F>
__global__ void __launch_bounds__(64) k_probe_field(uint32_t op, uint32_t na, uint32_t no, size_t n,
                                                    const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t* src = in + t * na * 8;
  uint32_t* dst = out + t * no * 8;
  F a[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if ((uint32_t)k < na) {
#pragma unroll
      for (int j = 0; j < 8; j++) a[k].v[j] = src[k * 8 + j];
    } else {
      a[k] = F::zero();
    }
  }
  F r = F::zero(), r1 = F::zero();
  switch (op) {
    case RLNAMD_PROBE_FP_ADD: r = a[0] + a[1]; break;
    case RLNAMD_PROBE_FP_SUB: r = a[0] - a[1]; break;
    case RLNAMD_PROBE_FP_NEG: r = a[0].neg(); break;
    case RLNAMD_PROBE_FP_DBL: r = a[0].dbl(); break;
    case RLNAMD_PROBE_FP_MUL: r = a[0] * a[1]; break;
    case RLNAMD_PROBE_FP_SQR: r = a[0].sqr(); break;
    case RLNAMD_PROBE_FP_DOT2: r = F::dot2(a[0], a[1], a[2], a[3]); break;
    case RLNAMD_PROBE_FP_DOT3: r = F::dot3(a[0], a[1], a[2], a[3], a[4], a[5]); break;
    case RLNAMD_PROBE_FP_DOT4: r = F::dot4(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); break;
    case RLNAMD_PROBE_FP_DOT2_SUB: r = F::dot2_sub(a[0], a[1], a[2], a[3]); break;
    case RLNAMD_PROBE_FP_FROM_CANONICAL: r = F::from_canonical(a[0].v); break;
    case RLNAMD_PROBE_FP_TO_CANONICAL: a[0].to_canonical(r.v); break;
    case RLNAMD_PROBE_FP_INV: r = a[0].inv(); break;
    default:
      if constexpr (std::is_same<F, Fq>::value) {
        const Fq2 x{a[0], a[1]}, y{a[2], a[3]};
        Fq2 z = Fq2::zero();
        if (op == RLNAMD_PROBE_FQ2_MUL) z = x * y;
        else if (op == RLNAMD_PROBE_FQ2_SQR) z = x.sqr();
        else if (op == RLNAMD_PROBE_FQ2_INV) z = x.inv();
        r = z.c0;
        r1 = z.c1;
      }
      break;
  }
#pragma unroll
  for (int j = 0; j < 8; j++) dst[j] = r.v[j];
  if (no == 2) {
#pragma unroll
    for (int j = 0; j < 8; j++) dst[8 + j] = r1.v[j];
  }
}

// ---- 9 x 29 primitives ------------------------------------------------------------------------------------------
// words per tuple; a 9 x 29 element is 9 words, an 8 x 32 element 8
constexpr Shape F29_SHAPE[RLNAMD_PROBE_F29_OPS] = {
    {18, 9}, {27, 9}, {9, 9}, {18, 9},                // mul mul_add sqr sqr_add
    {36, 9}, {45, 9}, {54, 9}, {54, 9}, {72, 9}, {72, 9}, {90, 9},   // dot2 dot2_add dot3 dot3<wide> dot4 dot4<wide> dotn29<5>
    {18, 9}, {18, 9}, {18, 9}, {18, 9},               // sub K2 K4 K6 K8
    {9, 9}, {9, 9}, {9, 9}, {9, 9},                   // neg_lazy K2 K4 K6 K8
    {9, 9}, {9, 1}, {8, 9}, {9, 8},                   // normalize is_zero_mod_q slice pack_reduced
    {8, 9}, {9, 8}, {17, 8}, {8, 9},                  // from_fq to_fq mul_mont from_canonical
    {8, 9}, {9, 8},                                   // unpack29 pack29_reduced
    {0, 0}, {0, 0}, {72, 36}, {144, 72}, {16, 16}, {32, 32},   // G1 walk, G2 walk (by steps), G1 add, G2 add, to_table29 G1, G2
};

template <class F>
__device__ __forceinline__ F ld29(const uint32_t* p) {
  F x;
#pragma unroll
  for (int j = 0; j < 9; j++) x.v[j] = p[j];
  return x;
}
template <class F>
__device__ __forceinline__ void st29(uint32_t* p, const F& x) {
#pragma unroll
  for (int j = 0; j < 9; j++) p[j] = x.v[j];
}
template <class M>
__device__ __forceinline__ M ld32(const uint32_t* p) {
  M x;
#pragma unroll
  for (int j = 0; j < 8; j++) x.v[j] = p[j];
  return x;
}
template <class M>
__device__ __forceinline__ void st32(uint32_t* p, const M& x) {
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = x.v[j];
}

template <class F, class M, class C>
__global__ void __launch_bounds__(64) k_probe_f29(uint32_t op, uint32_t in_words, uint32_t out_words, size_t n,
                                                  const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t* s = in + t * in_words;
  uint32_t* d = out + t * out_words;
  auto A = [&](int k) { return ld29<F>(s + 9 * k); };
  switch (op) {
    case RLNAMD_PROBE_F29_MUL: st29(d, F::mul(A(0), A(1))); break;
    case RLNAMD_PROBE_F29_MUL_ADD: st29(d, F::mul_add(A(0), A(1), A(2))); break;
    case RLNAMD_PROBE_F29_SQR: st29(d, F::sqr(A(0))); break;
    case RLNAMD_PROBE_F29_SQR_ADD: {
      const F add = A(1);
      st29(d, F::sqr_add(A(0), &add));
      break;
    }
    case RLNAMD_PROBE_F29_DOT2: st29(d, F::dot2(A(0), A(1), A(2), A(3))); break;
    case RLNAMD_PROBE_F29_DOT2_ADD: st29(d, F::dot2_add(A(0), A(1), A(2), A(3), A(4))); break;
    case RLNAMD_PROBE_F29_DOT3: st29(d, F::template dot3<false>(A(0), A(1), A(2), A(3), A(4), A(5))); break;
    case RLNAMD_PROBE_F29_DOT3_WIDE: st29(d, F::template dot3<true>(A(0), A(1), A(2), A(3), A(4), A(5))); break;
    case RLNAMD_PROBE_F29_DOT4: st29(d, F::template dot4<false>(A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7))); break;
    case RLNAMD_PROBE_F29_DOT4_WIDE: st29(d, F::template dot4<true>(A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7))); break;
    case RLNAMD_PROBE_F29_DOTN5:
      if constexpr (std::is_same<F, Fr29>::value) {   // poseidon.h: operands a0 b0 a1 b1 ... as in the dot products above
        Fr29 a[5], b[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
          a[k] = A(2 * k);
          b[k] = A(2 * k + 1);
        }
        st29(d, poseidon_dotn29<5>(a, b));
      }
      break;
    case RLNAMD_PROBE_F29_SUB_K2: st29(d, F::sub(A(0), C::K2, A(1))); break;
    case RLNAMD_PROBE_F29_SUB_K4: st29(d, F::sub(A(0), C::K4, A(1))); break;
    case RLNAMD_PROBE_F29_SUB_K6: st29(d, F::sub(A(0), C::K6, A(1))); break;
    case RLNAMD_PROBE_F29_SUB_K8: st29(d, F::sub(A(0), C::K8, A(1))); break;
    case RLNAMD_PROBE_F29_NEG_K2: st29(d, F::neg_lazy(C::K2, A(0))); break;
    case RLNAMD_PROBE_F29_NEG_K4: st29(d, F::neg_lazy(C::K4, A(0))); break;
    case RLNAMD_PROBE_F29_NEG_K6: st29(d, F::neg_lazy(C::K6, A(0))); break;
    case RLNAMD_PROBE_F29_NEG_K8: st29(d, F::neg_lazy(C::K8, A(0))); break;
    case RLNAMD_PROBE_F29_NORMALIZE: {
      F x = A(0);
      x.normalize();
      st29(d, x);
      break;
    }
    case RLNAMD_PROBE_F29_IS_ZERO: d[0] = A(0).is_zero_mod_q() ? 1u : 0u; break;
    case RLNAMD_PROBE_F29_SLICE: st29(d, F::slice(ld32<M>(s))); break;
    case RLNAMD_PROBE_F29_PACK_REDUCED: st32(d, A(0).pack_reduced()); break;
    case RLNAMD_PROBE_F29_FROM_FQ: st29(d, F::from_fq(ld32<M>(s))); break;
    case RLNAMD_PROBE_F29_TO_FQ: st32(d, A(0).to_fq()); break;
    case RLNAMD_PROBE_F29_MUL_MONT: st32(d, F::mul_mont(ld32<M>(s), ld29<F>(s + 8))); break;
    case RLNAMD_PROBE_F29_FROM_CANONICAL:   // the witness interpreters' input conversion
      st29(d, F::mul(F::slice(ld32<M>(s)), F::from_const(C::FROM_CANON)));
      break;
    case RLNAMD_PROBE_F29_UNPACK29:
      if constexpr (std::is_same<F, Fq29>::value) {
        uint32_t w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = s[j];
        st29(d, unpack29(w));
      }
      break;
    case RLNAMD_PROBE_F29_PACK29_REDUCED:
      if constexpr (std::is_same<F, Fq29>::value) {
        uint32_t w[8];
        pack29_reduced(A(0), w);
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = w[j];
      }
      break;
    default: break;
  }
}

// ---- 9 x 29 group law, lane forms -------------------------------------------------------------------------------
__device__ __forceinline__ void ld_entry(const uint32_t* p, G1Affine29* e) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    e->x[j] = p[j];
    e->y[j] = p[8 + j];
  }
}
__device__ __forceinline__ void ld_entry(const uint32_t* p, G2Affine29* e) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    e->x0[j] = p[j];
    e->x1[j] = p[8 + j];
    e->y0[j] = p[16 + j];
    e->y1[j] = p[24 + j];
  }
}
__device__ __forceinline__ void st_entry(uint32_t* p, const G1Affine29& e) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    p[j] = e.x[j];
    p[8 + j] = e.y[j];
  }
}
__device__ __forceinline__ void st_entry(uint32_t* p, const G2Affine29& e) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    p[j] = e.x0[j];
    p[8 + j] = e.x1[j];
    p[16 + j] = e.y0[j];
    p[24 + j] = e.y1[j];
  }
}
__device__ __forceinline__ void ld_acc(const uint32_t* p, G1Acc29* a) {
  a->X = ld29<Fq29>(p);
  a->Y = ld29<Fq29>(p + 9);
  a->ZZ = ld29<Fq29>(p + 18);
  a->ZZZ = ld29<Fq29>(p + 27);
}
__device__ __forceinline__ void st_acc(uint32_t* p, const G1Acc29& a) {
  st29(p, a.X);
  st29(p + 9, a.Y);
  st29(p + 18, a.ZZ);
  st29(p + 27, a.ZZZ);
}
__device__ __forceinline__ void ld_acc(const uint32_t* p, G2Acc29* a) {
  Fq2_29* const c[4] = {&a->X, &a->Y, &a->ZZ, &a->ZZZ};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    c[k]->c0 = ld29<Fq29>(p + 18 * k);
    c[k]->c1 = ld29<Fq29>(p + 18 * k + 9);
  }
}
__device__ __forceinline__ void st_acc(uint32_t* p, const G2Acc29& a) {
  const Fq2_29* const c[4] = {&a.X, &a.Y, &a.ZZ, &a.ZZZ};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    st29(p + 18 * k, c[k]->c0);
    st29(p + 18 * k + 9, c[k]->c1);
  }
}

// a lane starts from infinity and applies madd for each of its `steps` entries (flag word, then the table entry; flag
// bit 0 = negate, bit 1 = no entry at this step), writing the raw accumulator after every step
template <class Acc, class Aff29, uint32_t EW, uint32_t AW>
__global__ void __launch_bounds__(64) k_probe_walk(uint32_t steps, size_t n, const uint32_t* __restrict__ in,
                                                   uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t* s = in + t * steps * (1 + EW);
  uint32_t* d = out + t * steps * AW;
  Acc acc = Acc::inf();
#pragma unroll 1
  for (uint32_t i = 0; i < steps; i++, s += 1 + EW, d += AW) {
    const uint32_t flag = s[0];
    Aff29 e;
    ld_entry(s + 1, &e);
    if (!(flag & 2u)) acc.madd(e, (flag & 1u) != 0);
    st_acc(d, acc);
  }
}
template <class Acc, uint32_t AW>
__global__ void __launch_bounds__(64) k_probe_acc_add(size_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  Acc a, b;
  ld_acc(in + t * 2 * AW, &a);
  ld_acc(in + t * 2 * AW + AW, &b);
  a.add(b);
  st_acc(out + t * AW, a);
}
__global__ void __launch_bounds__(64) k_probe_table_g1(size_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const G1Affine a{ld32<Fq>(in + t * 16), ld32<Fq>(in + t * 16 + 8)};
  st_entry(out + t * 16, to_table29(a));
}
__global__ void __launch_bounds__(64) k_probe_table_g2(size_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t* s = in + t * 32;
  const G2Affine a{{ld32<Fq>(s), ld32<Fq>(s + 8)}, {ld32<Fq>(s + 16), ld32<Fq>(s + 24)}};
  st_entry(out + t * 32, to_table29(a));
}

// ---- witness operations -----------------------------------------------------------------------------------------
// Mul / Add / Sub never reach witness_slow_op in the interpreters (they are their fast path); the probe answers them with
// the 8 x 32 operators, as the host interpreter of witness_sched.cpp does, so that one table covers all twenty operations
__global__ void __launch_bounds__(64) k_probe_witness_op(size_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t* s = in + t * 17;
  const uint32_t op = s[0];
  const Fr a = ld32<Fr>(s + 1), b = ld32<Fr>(s + 9);
  uint32_t err = WERR_NONE;
  Fr r;
  if (op == G_MUL) r = a * b;
  else if (op == G_ADD) r = a + b;
  else if (op == G_SUB) r = a - b;
  else r = witness_slow_op(op, a, b, &err);
  st32(out + t * 9, r);
  out[t * 9 + 8] = err;
}

// ---- the quotient's transforms ------------------------------------------------------------------------------------
// canonical values, dense [vector][index][lane] with nb lanes <-> Montgomery, [vector][index][B] (the prover's layout);
// one thread per value, lanes of a wave on consecutive lanes of the layout
__global__ void __launch_bounds__(64) k_probe_lanes_in(const uint32_t* __restrict__ in, Fr* __restrict__ data, size_t rows,
                                                        uint32_t B, uint32_t nb) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= rows * nb) return;
  const size_t row = t / nb;
  const uint32_t p = (uint32_t)(t % nb);
  data[row * B + p] = Fr::from_canonical(in + t * 8);
}
__global__ void __launch_bounds__(64) k_probe_lanes_out(const Fr* __restrict__ data, uint32_t* __restrict__ out, size_t rows,
                                                         uint32_t B, uint32_t nb) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= rows * nb) return;
  const size_t row = t / nb;
  const uint32_t p = (uint32_t)(t % nb);
  data[row * B + p].to_canonical(out + t * 8);
}

constexpr size_t PROBE_MAX_TUPLES = (size_t)1 << 22;

template <class L>
void probe_run(size_t n, size_t in_words, size_t out_words, const uint32_t* in, uint32_t* out, L launch) {
  if (n == 0) return;
  if (!in || !out) throw Error("probe: null buffer");
  if (n > PROBE_MAX_TUPLES) throw Error("probe: more than 2^22 tuples in one call");
  require_gpu();
  DevBuf<uint32_t> din(n * in_words), dout(n * out_words);
  RLN_HIP(hipMemcpy(din.p, in, n * in_words * 4, hipMemcpyHostToDevice));
  launch(dim3(div_up(n, 64)), dim3(64), (const uint32_t*)din.p, dout.p);
  RLN_HIP(hipGetLastError());
  RLN_HIP(hipMemcpy(out, dout.p, n * out_words * 4, hipMemcpyDeviceToHost));
}

}  // namespace

void probe_field(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out) {
  if (field != 0 && field != 1) throw Error("probe_field: field is 0 (Fr) or 1 (Fq)");
  if (op >= RLNAMD_PROBE_FP_OPS || (field == 0 && op >= RLNAMD_PROBE_FQ2_MUL)) throw Error("probe_field: unknown operation");
  const Shape sh = FIELD_SHAPE[op];
  if (in_words != sh.in_words * 8 || out_words != sh.out_words * 8) throw Error("probe_field: word counts do not match the operation");
  probe_run(n, in_words, out_words, in, out, [&](dim3 g, dim3 b, const uint32_t* di, uint32_t* dq) {
    if (field == 0) hipLaunchKernelGGL(k_probe_field<Fr>, g, b, 0, 0, op, sh.in_words, sh.out_words, n, di, dq);
    else hipLaunchKernelGGL(k_probe_field<Fq>, g, b, 0, 0, op, sh.in_words, sh.out_words, n, di, dq);
  });
}

void probe_f29(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out) {
  if (field != 0 && field != 1) throw Error("probe_f29: field is 0 (Fr29) or 1 (Fq29)");
  if (op >= RLNAMD_PROBE_F29_OPS) throw Error("probe_f29: unknown operation");
  const bool fq_only = op == RLNAMD_PROBE_F29_UNPACK29 || op == RLNAMD_PROBE_F29_PACK29_REDUCED || op >= RLNAMD_PROBE_G1_WALK;
  if ((fq_only && field != 1) || (op == RLNAMD_PROBE_F29_DOTN5 && field != 0)) throw Error("probe_f29: operation not defined for this field");
  if (op == RLNAMD_PROBE_G1_WALK || op == RLNAMD_PROBE_G2_WALK) {
    const uint32_t ew = op == RLNAMD_PROBE_G1_WALK ? 16 : 32, aw = op == RLNAMD_PROBE_G1_WALK ? 36 : 72;
    const uint32_t steps = in_words / (1 + ew);
    if (steps < 1 || steps > 32 || in_words != steps * (1 + ew) || out_words != steps * aw)
      throw Error("probe_f29: a walk takes 1 .. 32 steps of (flag, entry) and returns an accumulator per step");
    probe_run(n, in_words, out_words, in, out, [&](dim3 g, dim3 b, const uint32_t* di, uint32_t* dq) {
      if (op == RLNAMD_PROBE_G1_WALK)
        hipLaunchKernelGGL((k_probe_walk<G1Acc29, G1Affine29, 16, 36>), g, b, 0, 0, steps, n, di, dq);
      else
        hipLaunchKernelGGL((k_probe_walk<G2Acc29, G2Affine29, 32, 72>), g, b, 0, 0, steps, n, di, dq);
    });
    return;
  }
  const Shape sh = F29_SHAPE[op];
  if (in_words != sh.in_words || out_words != sh.out_words) throw Error("probe_f29: word counts do not match the operation");
  probe_run(n, in_words, out_words, in, out, [&](dim3 g, dim3 b, const uint32_t* di, uint32_t* dq) {
    if (op == RLNAMD_PROBE_G1_ADD) hipLaunchKernelGGL((k_probe_acc_add<G1Acc29, 36>), g, b, 0, 0, n, di, dq);
    else if (op == RLNAMD_PROBE_G2_ADD) hipLaunchKernelGGL((k_probe_acc_add<G2Acc29, 72>), g, b, 0, 0, n, di, dq);
    else if (op == RLNAMD_PROBE_G1_TABLE) hipLaunchKernelGGL(k_probe_table_g1, g, b, 0, 0, n, di, dq);
    else if (op == RLNAMD_PROBE_G2_TABLE) hipLaunchKernelGGL(k_probe_table_g2, g, b, 0, 0, n, di, dq);
    else if (field == 0) hipLaunchKernelGGL((k_probe_f29<Fr29, Fr, Fr29C>), g, b, 0, 0, op, in_words, out_words, n, di, dq);
    else hipLaunchKernelGGL((k_probe_f29<Fq29, Fq, Fq29C>), g, b, 0, 0, op, in_words, out_words, n, di, dq);
  });
}

void probe_quotient_transform(int logn, int lds, uint32_t B, uint32_t nb, uint32_t vectors, const uint32_t* in, uint32_t* out) {
  if (logn < 1 || logn > 18) throw Error("probe_quotient_transform: logn is 1 .. 18");
  if (lds && logn < 9) throw Error("probe_quotient_transform: the LDS kernels take logn 9 .. 18");
  if (nb < 1 || nb > B) throw Error("probe_quotient_transform: 1 <= nb <= B");
  if (vectors < 1 || vectors > 3) throw Error("probe_quotient_transform: 1 .. 3 vectors");
  if (!in || !out) throw Error("probe: null buffer");
  const size_t n = (size_t)1 << logn, rows = (size_t)vectors * n;
  if (rows * B > ((size_t)1 << 26)) throw Error("probe_quotient_transform: more than 2^26 elements in the layout");
  require_gpu();
  const NttTables T = ntt_tables(logn);
  const std::vector<NttPass> passes = ntt_pass_list(logn);
  DevBuf<Fr> tw_i(T.tw_i.size()), tw_f(T.tw_f.size()), coset(T.coset.size()), data(rows * B);
  DevBuf<uint32_t> din(rows * nb * 8), dout(rows * nb * 8), tw_i29, tw_f29, coset29;
  tw_i29.assign(T.tw_i29, 0);
  tw_f29.assign(T.tw_f29, 0);
  coset29.assign(T.coset29, 0);
  RLN_HIP(hipMemcpy(tw_i.p, T.tw_i.data(), T.tw_i.size() * sizeof(Fr), hipMemcpyHostToDevice));
  RLN_HIP(hipMemcpy(tw_f.p, T.tw_f.data(), T.tw_f.size() * sizeof(Fr), hipMemcpyHostToDevice));
  RLN_HIP(hipMemcpy(coset.p, T.coset.data(), T.coset.size() * sizeof(Fr), hipMemcpyHostToDevice));
  RLN_HIP(hipMemcpy(din.p, in, rows * nb * 32, hipMemcpyHostToDevice));
  RLN_HIP(hipMemset(data.p, 0, rows * B * sizeof(Fr)));
  const dim3 grid((uint32_t)div_up(rows * nb, 64));
  hipLaunchKernelGGL(k_probe_lanes_in, grid, dim3(64), 0, 0, (const uint32_t*)din.p, data.p, rows, B, nb);
  RLN_HIP(hipGetLastError());
  launch_quotient_transform(lds != 0, passes, data.p, {tw_i.p, tw_f.p, coset.p, tw_i29.p, tw_f29.p, coset29.p}, logn, B, nb,
                            vectors, 0);
  hipLaunchKernelGGL(k_probe_lanes_out, grid, dim3(64), 0, 0, (const Fr*)data.p, dout.p, rows, B, nb);
  RLN_HIP(hipGetLastError());
  RLN_HIP(hipMemcpy(out, dout.p, rows * nb * 32, hipMemcpyDeviceToHost));
}

void probe_witness_op(size_t n, const uint32_t* in, uint32_t* out) {
  probe_run(n, 17, 9, in, out, [&](dim3 g, dim3 b, const uint32_t* di, uint32_t* dq) {
    hipLaunchKernelGGL(k_probe_witness_op, g, b, 0, 0, n, di, dq);
  });
}

}  // namespace rlnamd
