// Groth16 verification for BN254 written for one GPU lane per proof (verify.hip) and for a plain g++ build
// (tests/host/verifymath.cpp): from the 128 compressed proof bytes and the public inputs to the final-exponentiated
// pairing product.  pairing.h stays the host verifier and the yardstick; this file restates the same mathematics
// without std::vector, function-local statics or runtime-indexed local arrays, and takes every constant through a
// pointer to a prepared key (verify_key.h builds it on the host, verify.hip keeps a copy on the device).
//
//   Fq12 = Fq2[w]/(w^6 - xi), xi = 9 + u, as the flat vector c[0..5] of w^0..w^5 (pairing.h's order), computed as
//   Fq6[w]/(w^2 - v) over Fq6 = Fq2[v]/(v^3 - xi) with Karatsuba at both levels.
//
// The Miller loop of the variable pair (A, B) keeps the running point of the twist in homogeneous projective
// coordinates (X : Y : Z), so a line costs no field inversion (the affine step of pairing.h inverts in Fq2 at each of
// its 102 lines).  Doubling and mixed-addition steps and their line coefficients follow Costello, Lange, Naehrig,
// "Faster Pairing Computations on Curves with High-Degree Twists" (PKC 2010), section 5 (D-type sextic twist, a = 0);
// each line is the affine one scaled by an element of Fq2, which the (q^6 - 1) part of the final exponentiation sends to
// 1: only the value after the final exponentiation is comparable with pairing.h, and that value is unique.
//
// On the device the Fq12-level routines are out of line (one body each, operands through memory): a verification is
// ~4 x 10^4 base-field products, and inlining them all at every call site would make a kernel of millions of
// instructions.  The base-field products inside them stay inlined (field.h's one-reduction dot products).
#pragma once
#include "curve.h"

#if defined(__HIPCC__)
#define VM_FN static __host__ __device__ __noinline__
#else
#define VM_FN static inline
#endif

namespace rlnamd {
namespace vm {

constexpr int N_LINES = 102;  // 64 doublings + 36 additions (set bits of 6u + 2 below the top one) + 2 Frobenius additions

struct F12 {
  Fq2 c[6];
};
struct F6 {
  Fq2 a, b, c;  // a + b v + c v^2
};
struct LineC {
  Fq2 lam, c;  // pairing.h's LineCoef: l(P) = P.y - lam P.x w + c w^3
};

// The prepared verifying key: plain data, read at wave-uniform addresses (every lane runs the same loop).
struct PreparedKey {
  uint32_t n_values;       // public inputs per proof = gamma_abc_g1.size() - 1
  uint32_t pad_[3];
  uint32_t sqrt_exp[8];    // (q + 1) / 4
  uint32_t six_u2[8];      // 6 u^2 of the G2 subgroup test
  Fq inv2;                 // 1 / 2
  Fq three;                // the curve's b
  Fq2 twist_b, twist_3b;   // b' = 3 / xi and 3 b'
  Fq2 frob1[6], frob2[6];  // q-power: c_i -> conj(c_i) frob1[i]; q^2-power: c_i -> c_i frob2[i]
  Fq2 g22, g23;            // xi^((q^2 - 1) / 3), xi^((q^2 - 1) / 2)
  F12 alpha_beta;          // miller(-alpha, beta)
  LineC gamma[N_LINES], delta[N_LINES];
  G1Affine ic0;
  const G1Affine* ic_mult;  // n_values rows of d * IC_i, d = 1..15 (pairing.h: PreparedVk::ic_mult)
};

// What the first stage hands to the Miller loop.
enum : uint32_t { P_REJECT = 1, P_VARYING = 2, P_GAMMA = 4, P_DELTA = 8 };
struct Prep {
  G1Affine A;
  G2Affine B;
  G1Affine icn, cn;  // -(IC_0 + sum x_i IC_i) and -C
  uint32_t flags;
};

// ---------------------------------------------------------------- tower
RLN_HD Fq2 vxi(const Fq2& x) {  // (9 + u) x
  const Fq2 x2 = x.dbl(), x4 = x2.dbl(), x9 = x4.dbl() + x;
  return {x9.c0 - x.c1, x9.c1 + x.c0};
}
RLN_HD F6 f6_add(const F6& x, const F6& y) { return {x.a + y.a, x.b + y.b, x.c + y.c}; }
RLN_HD F6 f6_sub(const F6& x, const F6& y) { return {x.a - y.a, x.b - y.b, x.c - y.c}; }
RLN_HD F6 f6_mul_v(const F6& x) { return {vxi(x.c), x.a, x.b}; }
RLN_HD F6 f6_mul(const F6& x, const F6& y) {
  const Fq2 v0 = x.a * y.a, v1 = x.b * y.b, v2 = x.c * y.c;
  const Fq2 t12 = (x.b + x.c) * (y.b + y.c) - v1 - v2;
  const Fq2 t01 = (x.a + x.b) * (y.a + y.b) - v0 - v1;
  const Fq2 t02 = (x.a + x.c) * (y.a + y.c) - v0 - v2;
  return {v0 + vxi(t12), t01 + vxi(v2), t02 + v1};
}
RLN_HD F6 f6_mul_01(const F6& x, const Fq2& y0, const Fq2& y1) {  // x (y0 + y1 v)
  const Fq2 v0 = x.a * y0, v1 = x.b * y1;
  const Fq2 t01 = (x.a + x.b) * (y0 + y1) - v0 - v1;
  return {v0 + vxi(x.c * y1), t01, x.c * y0 + v1};
}
RLN_HD F6 f6_even(const F12& f) { return {f.c[0], f.c[2], f.c[4]}; }
RLN_HD F6 f6_odd(const F12& f) { return {f.c[1], f.c[3], f.c[5]}; }
RLN_HD void f12_set(F12* r, const F6& A, const F6& B) {
  r->c[0] = A.a; r->c[2] = A.b; r->c[4] = A.c;
  r->c[1] = B.a; r->c[3] = B.b; r->c[5] = B.c;
}
RLN_HD void f12_one(F12* r) {
  r->c[0] = Fq2::one();
  r->c[1] = r->c[2] = r->c[3] = r->c[4] = r->c[5] = Fq2::zero();
}
RLN_HD bool f12_is_one(const F12& f) {
  return f.c[0] == Fq2::one() && f.c[1].is_zero() && f.c[2].is_zero() && f.c[3].is_zero() && f.c[4].is_zero() &&
         f.c[5].is_zero();
}
// r may alias x or y in all of these
VM_FN void f12_mul(F12* r, const F12* x, const F12* y) {
  const F6 A = f6_even(*x), B = f6_odd(*x), C = f6_even(*y), D = f6_odd(*y);
  const F6 ac = f6_mul(A, C), bd = f6_mul(B, D);
  const F6 cross = f6_sub(f6_sub(f6_mul(f6_add(A, B), f6_add(C, D)), ac), bd);
  f12_set(r, f6_add(ac, f6_mul_v(bd)), cross);
}
VM_FN void f12_sqr(F12* r, const F12* x) {
  const F6 A = f6_even(*x), B = f6_odd(*x);
  const F6 t = f6_mul(A, B);
  const F6 s = f6_mul(f6_add(A, B), f6_add(A, f6_mul_v(B)));
  f12_set(r, f6_sub(f6_sub(s, t), f6_mul_v(t)), f6_add(t, t));
}
// f * (l0 + l1 w + l3 w^3), l0 in Fq2: a projective line of the variable pair
VM_FN void f12_mul_line2(F12* f, const Fq2* l0, const Fq2* l1, const Fq2* l3) {
  const F6 A = f6_even(*f), B = f6_odd(*f);
  const F6 aa{A.a * *l0, A.b * *l0, A.c * *l0};
  const F6 bb = f6_mul_01(B, *l1, *l3);
  const F6 cross = f6_sub(f6_sub(f6_mul_01(f6_add(A, B), *l0 + *l1, *l3), aa), bb);
  f12_set(f, f6_add(aa, f6_mul_v(bb)), cross);
}
// the same with l0 in Fq: a precomputed line of gamma or delta at a G1 point (pairing.h: f12_mul_line)
VM_FN void f12_mul_line1(F12* f, const Fq* l0, const Fq2* l1, const Fq2* l3) {
  const F6 A = f6_even(*f), B = f6_odd(*f);
  const F6 aa{A.a.mul_fq(*l0), A.b.mul_fq(*l0), A.c.mul_fq(*l0)};
  const F6 bb = f6_mul_01(B, *l1, *l3);
  const Fq2 s0{l1->c0 + *l0, l1->c1};
  const F6 cross = f6_sub(f6_sub(f6_mul_01(f6_add(A, B), s0, *l3), aa), bb);
  f12_set(f, f6_add(aa, f6_mul_v(bb)), cross);
}
RLN_HD void f12_conj(F12* r, const F12& a) {  // w -> -w: the q^6-power
  r->c[0] = a.c[0]; r->c[2] = a.c[2]; r->c[4] = a.c[4];
  r->c[1] = a.c[1].neg(); r->c[3] = a.c[3].neg(); r->c[5] = a.c[5].neg();
}
VM_FN void f12_frob(const PreparedKey* vk, F12* r, const F12* a) {
  r->c[0] = a->c[0].conj();
  r->c[1] = a->c[1].conj() * vk->frob1[1];
  r->c[2] = a->c[2].conj() * vk->frob1[2];
  r->c[3] = a->c[3].conj() * vk->frob1[3];
  r->c[4] = a->c[4].conj() * vk->frob1[4];
  r->c[5] = a->c[5].conj() * vk->frob1[5];
}
VM_FN void f12_frob2(const PreparedKey* vk, F12* r, const F12* a) {  // frob2[i] lies in Fq
  r->c[0] = a->c[0];
  r->c[1] = a->c[1].mul_fq(vk->frob2[1].c0);
  r->c[2] = a->c[2].mul_fq(vk->frob2[2].c0);
  r->c[3] = a->c[3].mul_fq(vk->frob2[3].c0);
  r->c[4] = a->c[4].mul_fq(vk->frob2[4].c0);
  r->c[5] = a->c[5].mul_fq(vk->frob2[5].c0);
}
RLN_HD F6 f6_inv(const F6& x) {
  const Fq2 t0 = x.a.sqr() - vxi(x.b * x.c);
  const Fq2 t1 = vxi(x.c.sqr()) - x.a * x.b;
  const Fq2 t2 = x.b.sqr() - x.a * x.c;
  const Fq2 d = (x.a * t0 + vxi(x.c * t1 + x.b * t2)).inv();
  return {t0 * d, t1 * d, t2 * d};
}
VM_FN void f12_inv(F12* r, const F12* f) {  // (A - B w) / (A^2 - v B^2); 0 -> 0
  const F6 A = f6_even(*f), B = f6_odd(*f);
  const F6 d = f6_inv(f6_sub(f6_mul(A, A), f6_mul_v(f6_mul(B, B))));
  const F6 ra = f6_mul(A, d), rb = f6_mul(B, d);
  f12_set(r, ra, {rb.a.neg(), rb.b.neg(), rb.c.neg()});
}
// Granger, Scott, "Faster squaring in the cyclotomic subgroup of sixth degree extensions": valid after the easy part
RLN_HD void fp4_sqr(const Fq2& a, const Fq2& b, Fq2* c0, Fq2* c1) {
  const Fq2 t0 = a.sqr(), t1 = b.sqr();
  *c0 = vxi(t1) + t0;
  *c1 = (a + b).sqr() - t0 - t1;
}
RLN_HD Fq2 m3sub2(const Fq2& t, const Fq2& z) { return (t - z).dbl() + t; }  // 3 t - 2 z
RLN_HD Fq2 m3add2(const Fq2& t, const Fq2& z) { return (t + z).dbl() + t; }  // 3 t + 2 z
VM_FN void f12_cyclotomic_sqr(F12* r, const F12* x) {
  const Fq2 z0 = x->c[0], z4 = x->c[2], z3 = x->c[4], z2 = x->c[1], z1 = x->c[3], z5 = x->c[5];
  Fq2 t0, t1, t2, t3;
  fp4_sqr(z0, z1, &t0, &t1);
  r->c[0] = m3sub2(t0, z0);
  r->c[3] = m3add2(t1, z1);
  fp4_sqr(z2, z3, &t0, &t1);
  fp4_sqr(z4, z5, &t2, &t3);
  r->c[2] = m3sub2(t0, z4);
  r->c[5] = m3add2(t1, z5);
  r->c[1] = m3add2(vxi(t3), z2);
  r->c[4] = m3sub2(t2, z3);
}
VM_FN void f12_pow_u(F12* r, const F12* f) {  // f in the cyclotomic subgroup; r must not alias f
  const uint64_t u = 4965661367192848881ULL;  // 63 bits; the top bit is the initial value
  *r = *f;
  for (int i = 61; i >= 0; i--) {
    f12_cyclotomic_sqr(r, r);
    if ((u >> i) & 1) f12_mul(r, r, f);
  }
}
// f^((q^12 - 1) / r): easy part by conjugation, one inversion and Frobenius; hard part (q^4 - q^2 + 1) / r by the
// y0..y6 chain of Scott et al., "On the final exponentiation for calculating pairings on ordinary elliptic curves"
// (three exponentiations by u), as in pairing.h.  f == 0 gives 0.
VM_FN void final_exponentiation(const PreparedKey* vk, F12* out, const F12* f0) {
  F12 f, t, fx, fx2, fx3, y0, y4, y6, t0, t1;
  f12_inv(&t, f0);
  f12_conj(&f, *f0);
  f12_mul(&f, &f, &t);  // ^(q^6 - 1)
  f12_frob2(vk, &t, &f);
  f12_mul(&f, &t, &f);  // ^(q^2 + 1)
  f12_pow_u(&fx, &f);
  f12_pow_u(&fx2, &fx);
  f12_pow_u(&fx3, &fx2);
  // y0 = f^q f^(q^2) f^(q^3)
  f12_frob(vk, &y0, &f);
  f12_frob2(vk, &t, &f);
  f12_mul(&y0, &y0, &t);
  f12_frob(vk, &t, &t);
  f12_mul(&y0, &y0, &t);
  // y4 = conj(fx fx2^q), y6 = conj(fx3 fx3^q)
  f12_frob(vk, &t, &fx2);
  f12_mul(&y4, &fx, &t);
  f12_conj(&y4, y4);
  f12_frob(vk, &t, &fx3);
  f12_mul(&y6, &fx3, &t);
  f12_conj(&y6, y6);
  // t0 = y6^2 y4 y5, y5 = conj(fx2)
  f12_conj(&fx3, fx2);  // fx3 is free: y5
  f12_sqr(&t0, &y6);
  f12_mul(&t0, &t0, &y4);
  f12_mul(&t0, &t0, &fx3);
  // t1 = y3 y5 t0, y3 = conj(fx^q)
  f12_frob(vk, &t, &fx);
  f12_conj(&t, t);
  f12_mul(&t1, &t, &fx3);
  f12_mul(&t1, &t1, &t0);
  // t0 *= y2, y2 = fx2^(q^2)
  f12_frob2(vk, &t, &fx2);
  f12_mul(&t0, &t0, &t);
  f12_sqr(&t1, &t1);
  f12_mul(&t1, &t1, &t0);
  f12_sqr(&t1, &t1);
  f12_conj(&t, f);  // y1
  f12_mul(&t0, &t1, &t);
  f12_mul(&t1, &t1, &y0);
  f12_sqr(&t0, &t0);
  f12_mul(out, &t0, &t1);
}

// ---------------------------------------------------------------- Miller loop
struct G2Proj {
  Fq2 X, Y, Z;
};
// T <- 2 T; the line through T tangent to the twist, times 2 Y Z:  l0 = -2 Y Z (times y_P), l1 = 3 X^2 (times x_P),
// l3 = 3 b' Z^2 - Y^2.  All three coordinates of 2 T carry a common factor 4 (no halving needed).
RLN_HD void proj_double(const PreparedKey* vk, G2Proj* T, Fq2* l0, Fq2* l1, Fq2* l3) {
  const Fq2 B = T->Y.sqr(), C = T->Z.sqr();
  const Fq2 E = C * vk->twist_3b;          // 3 b' Z^2
  const Fq2 F = E.dbl() + E;               // 9 b' Z^2
  const Fq2 H = (T->Y * T->Z).dbl();       // 2 Y Z
  const Fq2 X2 = T->X.sqr();
  const Fq2 S = B + F;
  const Fq2 E2 = E.sqr();
  *l0 = H.neg();
  *l1 = X2.dbl() + X2;
  *l3 = E - B;
  const Fq2 XY = T->X * T->Y;
  T->X = (XY * (B - F)).dbl();                        // 4 (X Y / 2)(B - F)
  T->Y = S.sqr() - (E2.dbl() + E2).dbl().dbl();       // 4 (((B + F) / 2)^2 - 3 E^2)
  T->Z = (B * H).dbl().dbl();                         // 4 B H
}
// T <- T + Q, Q affine and T != +-Q (always so for points of prime order r inside the loop); the line through T and
// Q times lambda = X - x_Q Z:  l0 = lambda (times y_P), l1 = -theta (times x_P), l3 = theta x_Q - lambda y_Q
RLN_HD void proj_add(G2Proj* T, const Fq2& qx, const Fq2& qy, Fq2* l0, Fq2* l1, Fq2* l3) {
  const Fq2 theta = T->Y - qy * T->Z, lambda = T->X - qx * T->Z;
  const Fq2 C = theta.sqr(), D = lambda.sqr();
  const Fq2 E = lambda * D, F = T->Z * C, G = T->X * D;
  const Fq2 H = E + F - G.dbl();
  *l0 = lambda;
  *l1 = theta.neg();
  *l3 = theta * qx - lambda * qy;
  T->X = lambda * H;
  T->Y = theta * (G - H) - E * T->Y;
  T->Z = T->Z * E;
}
// one line of each of the three pairs into f.  KEY_LINES = false leaves out the lines of gamma and delta (and never
// reads icn / cn, so P may be a record without them: verify_agg_math.h's single pair)
template <bool KEY_LINES, class P>
RLN_HD void miller_step_t(const PreparedKey* vk, const P* p, F12* f, int k, const Fq2* l0, const Fq2* l1,
                          const Fq2* l3) {
  if (p->flags & P_VARYING) {
    const Fq2 a0 = l0->mul_fq(p->A.y), a1 = l1->mul_fq(p->A.x);
    f12_mul_line2(f, &a0, &a1, l3);
  }
  if constexpr (KEY_LINES) {
    if (p->flags & P_GAMMA) {
      const Fq2 g1 = vk->gamma[k].lam.mul_fq(p->icn.x).neg();
      f12_mul_line1(f, &p->icn.y, &g1, &vk->gamma[k].c);
    }
    if (p->flags & P_DELTA) {
      const Fq2 d1 = vk->delta[k].lam.mul_fq(p->cn.x).neg();
      f12_mul_line1(f, &p->cn.y, &d1, &vk->delta[k].c);
    }
  }
}
VM_FN void miller_step(const PreparedKey* vk, const Prep* p, F12* f, int k, const Fq2* l0, const Fq2* l1,
                       const Fq2* l3) {
  miller_step_t<true>(vk, p, f, k, l0, l1, l3);
}
struct ThreePairStep {
  RLN_HD void operator()(const PreparedKey* vk, const Prep* p, F12* f, int k, const Fq2* l0, const Fq2* l1,
                         const Fq2* l3) const {
    miller_step(vk, p, f, k, l0, l1, l3);
  }
};
// The loop over the running point of (A, B); STEP folds the lines of one step into f
template <class P, class STEP>
RLN_HD void miller_loop_t(const PreparedKey* vk, const P* p, F12* f, STEP step) {
  f12_one(f);
  G2Proj T{p->B.x, p->B.y, Fq2::one()};
  Fq2 l0, l1, l3;
  int k = 0;
  for (int i = ATE_LOOP_BITS - 2; i >= 0; i--) {
    f12_sqr(f, f);
    proj_double(vk, &T, &l0, &l1, &l3);
    step(vk, p, f, k++, &l0, &l1, &l3);
    const uint32_t word = i >= 32 ? ATE_LOOP[1] : ATE_LOOP[0];   // bit 64 is the start value
    if ((word >> (i & 31)) & 1) {
      proj_add(&T, p->B.x, p->B.y, &l0, &l1, &l3);
      step(vk, p, f, k++, &l0, &l1, &l3);
    }
  }
  const Fq2 q1x = p->B.x.conj() * vk->frob1[2], q1y = p->B.y.conj() * vk->frob1[3];   // pi(B)
  proj_add(&T, q1x, q1y, &l0, &l1, &l3);
  step(vk, p, f, k++, &l0, &l1, &l3);
  const Fq2 q2x = p->B.x * vk->g22, q2y = (p->B.y * vk->g23).neg();                   // -pi^2(B)
  proj_add(&T, q2x, q2y, &l0, &l1, &l3);
  step(vk, p, f, k++, &l0, &l1, &l3);
}
// miller(A, B) miller(-IC, gamma) miller(-C, delta), up to factors of proper subfields (the caller multiplies by
// vk->alpha_beta)
VM_FN void miller_loop(const PreparedKey* vk, const Prep* p, F12* f) {
  miller_loop_t(vk, p, f, ThreePairStep{});
}

// ---------------------------------------------------------------- decompression (zkey.cpp's rules), subgroup, IC
RLN_HD bool y_is_neg(const Fq& y) {  // y > (q - 1) / 2
  uint32_t c[8];
  y.to_canonical(c);
  bool gt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (!decided && c[i] != FqParams::HALF[i]) {
      gt = c[i] > FqParams::HALF[i];
      decided = true;
    }
  }
  return gt;
}
RLN_HD bool y2_is_neg(const Fq2& y) { return y.c1.is_zero() ? y_is_neg(y.c0) : y_is_neg(y.c1); }
// limbs >= modulus, limbs in registers (no pointer to a local array leaves the function)
template <class P>
RLN_HD bool words_geq_mod(const uint32_t (&c)[8]) {
  bool lt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (!decided && c[i] != P::MOD[i]) {
      lt = c[i] < P::MOD[i];
      decided = true;
    }
  }
  return !lt;
}
VM_FN bool fq_sqrt(const PreparedKey* vk, const Fq* a, Fq* r) {  // q = 3 mod 4: a^((q + 1) / 4)
  Fq x = Fq::one();
  for (int i = 253; i >= 0; i--) {
    x = x.sqr();
    if ((vk->sqrt_exp[i >> 5] >> (i & 31)) & 1) x = x * *a;
  }
  *r = x;
  return x.sqr() == *a;
}
// words: 8 little-endian words of an x coordinate; strip: the two flag bits sit in its top byte
RLN_HD bool load_x_checked(const uint32_t* words, bool strip, Fq* out) {
  uint32_t c[8];
#pragma unroll
  for (int i = 0; i < 8; i++) c[i] = words[i];
  if (strip) c[7] &= 0x3FFFFFFFu;
  const bool bad = words_geq_mod<FqParams>(c);
  Fq x, r2;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x.v[i] = bad ? 0 : c[i];
    r2.v[i] = FqParams::R2[i];
  }
  *out = x * r2;
  return !bad;
}
VM_FN bool g1_decompress(const PreparedKey* vk, const uint32_t* in, G1Affine* out) {
  if (in[7] & 0x40000000u) {
    *out = G1Affine::inf();
    return true;
  }
  Fq x, y;
  if (!load_x_checked(in, true, &x)) return false;
  const Fq rhs = x.sqr() * x + vk->three;
  if (!fq_sqrt(vk, &rhs, &y)) return false;
  if (y_is_neg(y) != ((in[7] & 0x80000000u) != 0)) y = y.neg();
  *out = {x, y};
  return true;
}
VM_FN bool fq2_sqrt(const PreparedKey* vk, const Fq2* a, Fq2* r) {  // norm method, as zkey.cpp
  Fq s;
  if (a->c1.is_zero()) {
    if (fq_sqrt(vk, &a->c0, &s)) {
      *r = {s, Fq::zero()};
      return true;
    }
    const Fq n0 = a->c0.neg();
    if (fq_sqrt(vk, &n0, &s)) {
      *r = {Fq::zero(), s};
      return true;
    }
    return false;
  }
  Fq n;
  const Fq norm = a->c0.sqr() + a->c1.sqr();
  if (!fq_sqrt(vk, &norm, &n)) return false;
  for (int k = 0; k < 2; k++) {
    const Fq t = (a->c0 + (k ? n.neg() : n)) * vk->inv2;
    Fq x0;
    if (!fq_sqrt(vk, &t, &x0) || x0.is_zero()) continue;
    const Fq x1 = a->c1 * x0.dbl().inv();
    const Fq2 cand{x0, x1};
    if (cand.sqr() == *a) {
      *r = cand;
      return true;
    }
  }
  return false;
}
VM_FN bool g2_decompress(const PreparedKey* vk, const uint32_t* in, G2Affine* out) {
  if (in[15] & 0x40000000u) {
    *out = G2Affine::inf();
    return true;
  }
  Fq x0, x1;
  if (!load_x_checked(in, false, &x0) || !load_x_checked(in + 8, true, &x1)) return false;
  const Fq2 x{x0, x1};
  const Fq2 rhs = x.sqr() * x + vk->twist_b;
  Fq2 y;
  if (!fq2_sqrt(vk, &rhs, &y)) return false;
  if (y2_is_neg(y) != ((in[15] & 0x80000000u) != 0)) y = y.neg();
  *out = {x, y};
  return true;
}
// psi(P) == [6 u^2] P (zkey.cpp: g2_in_subgroup)
VM_FN bool g2_in_subgroup(const PreparedKey* vk, const G2Affine* p) {
  if (p->is_inf()) return true;
  const Fq2 px = p->x.conj() * vk->frob1[2], py = p->y.conj() * vk->frob1[3];
  G2XYZZ acc = G2XYZZ::inf();
  bool started = false;
  for (int i = 127; i >= 0; i--) {
    if (started) acc = acc.dbl();
    if ((vk->six_u2[i >> 5] >> (i & 31)) & 1) {
      acc.madd(*p);
      started = true;
    }
  }
  if (acc.is_inf()) return false;
  return acc.X == px * acc.ZZ && acc.Y == py * acc.ZZZ;
}
// IC_0 + sum x_i IC_i by one Straus ladder over 4-bit digits (pairing.h: ic_combination); vals: n_values x 8 canonical
// words, each already known to be below r
VM_FN void ic_combination(const PreparedKey* vk, const uint32_t* vals, G1Affine* out) {
  G1XYZZ acc = G1XYZZ::inf();
  const uint32_t nv = vk->n_values;
  for (int w = 63; w >= 0; w--) {
    if (w != 63) acc = acc.dbl().dbl().dbl().dbl();
    for (uint32_t i = 0; i < nv; i++) {
      const uint32_t d = (vals[8 * i + (w >> 3)] >> ((w & 7) * 4)) & 15;
      if (d) acc.madd(vk->ic_mult[15 * i + d - 1]);
    }
  }
  acc.madd(vk->ic0);
  *out = acc.to_affine();
}

// Stage 1: proof bytes (32 little-endian words: A | B | C) and public inputs -> the operands of the Miller loop.
// A rejected proof (bad encoding, B outside the subgroup, an input >= r) gets P_REJECT and harmless operands, so that
// the later stages run the same instructions on it and its verdict is masked at the end.
// The reject rules, one text for both forms of the verifier (prepare below, verify_agg_math.h's prepare_agg):
// canonical encodings, points on their curves, B in the order-r subgroup, every input below r.  False: rejected; A, B
// and C are then unspecified.
VM_FN bool checked_points(const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, G1Affine* A, G2Affine* B,
                          G1Affine* C) {
  bool ok = g1_decompress(vk, proof, A);
  ok = ok && g2_decompress(vk, proof + 8, B);
  *C = G1Affine::inf();
  ok = ok && g1_decompress(vk, proof + 24, C);
  ok = ok && g2_in_subgroup(vk, B);
  for (uint32_t i = 0; ok && i < vk->n_values; i++) {
    bool lt = false, decided = false;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
      const uint32_t c = vals[8 * i + j], m = FrParams::MOD[j];
      if (!decided && c != m) {
        lt = c < m;
        decided = true;
      }
    }
    ok = lt;
  }
  return ok;
}
VM_FN void prepare(const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, Prep* out) {
  G1Affine C;
  const bool ok = checked_points(vk, proof, vals, &out->A, &out->B, &C);
  if (!ok) {
    out->A = G1Affine::inf();
    out->B = G2Affine::inf();
    out->icn = out->cn = G1Affine::inf();
    out->flags = P_REJECT;
    return;
  }
  G1Affine ic;
  ic_combination(vk, vals, &ic);
  out->icn = ic.neg();
  out->cn = C.neg();
  out->flags = ((out->A.is_inf() || out->B.is_inf()) ? 0 : P_VARYING) | (ic.is_inf() ? 0 : P_GAMMA) |
               (C.is_inf() ? 0 : P_DELTA);
}
// Stage 3 output: 96 canonical words, c[0].c0, c[0].c1, c[1].c0, ...; all zero for a rejected proof
RLN_HD void gt_words(const F12& f, bool rejected, uint32_t* out) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    uint32_t a[8], b[8];
    f.c[i].c0.to_canonical(a);
    f.c[i].c1.to_canonical(b);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      out[16 * i + j] = rejected ? 0 : a[j];
      out[16 * i + 8 + j] = rejected ? 0 : b[j];
    }
  }
}
// The whole verification of one proof: 1 accept, 0 reject; gt (optional) as gt_words
VM_FN int verify_one(const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, uint32_t* gt) {
  Prep p;
  F12 f;
  prepare(vk, proof, vals, &p);
  miller_loop(vk, &p, &f);
  f12_mul(&f, &f, &vk->alpha_beta);
  final_exponentiation(vk, &f, &f);
  const bool rejected = (p.flags & P_REJECT) != 0;
  if (gt) gt_words(f, rejected, gt);
  return (!rejected && f12_is_one(f)) ? 1 : 0;
}

}  // namespace vm
}  // namespace rlnamd
