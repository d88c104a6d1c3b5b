// Groth16 verification for BN254 written for a team of TEAM = 8 lanes per proof (verify_team.hip) and for a plain g++
// build that runs the eight lanes in a loop (tests/host/verifyteam.cpp).  The same verification as verify_math.h: the
// same prepared key, the same Prep and F12 records between the stages, the same accept / reject rules and the same GT
// value; verify_math.h stays the lane-per-proof path and the yardstick.
//
//   Lanes 0..5 own coefficient w^k of every Fq12 value.  A value lives in the team's exchange memory (a slot of six
//   Fq2); an operation is "lane k computes coefficient k from the published operands":
//     product      c_k = sum_i x'_i y_((k - i) mod 6), x'_i = xi x_i where i > k (the wrap w^6 = xi is applied to the
//                  operand, a predicated vxi, so that the row is one 6-term dot product: three 4-product sums with one
//                  reduction each per component -- Fq::dot4's bound, 4 p^2 < p 2^256 (curve.h), is not exceeded)
//     sparse line  c_k = x_k l0 + x'_(k-1) l1 + x'_(k-3) l3 (a product and one two-term sum)
//     cyclotomic   lanes 0, 2, 4 form a^2 + xi b^2, lanes 3, 5, 1 form 2 a b of one Fq4 square (one two-term sum each)
//     Frobenius    conj(c_k) frob1[k], c_k frob2[k]; conjugation negates the odd lanes
//     inverse      on lane 0 alone (vm::f12_inv: the Fq6 norm and the one Fq2 inversion are a serial chain)
//   Which operand a lane reads is an address into the exchange memory, never an index into a local array.
//
// The exchange is a policy type X, so that the kernels and the CPU emulation compile the same source:
//   X::f(slot, i)   coefficient i of Fq12 slot `slot`        X::s(i)   scratch Fq2 i (points, lines, candidates)
//   X::w(i)         scratch word i (flags)                   X::sync() everything written before is visible after
//   VT_LANES(x, k)  the lanes this instance runs: the one lane of the calling thread on the device (LDS behind it),
//                   all eight one after the other on the host (an array behind it)
// Every operation is two phases -- all lanes compute into a private value, sync, all lanes store, sync -- so that a
// destination may alias an operand and the host's serial order of lanes can never see a value the device would not.
// No lane leaves before the last exchange; a rejected proof runs the same instructions on harmless operands (identity
// lines) and its verdict is masked at the end.
#pragma once
#include "verify_math.h"

#if defined(__HIPCC__)
#define VT_FN static __host__ __device__ __noinline__
#else
#define VT_FN static inline
#endif
#define VT_LANES(x, k) for (int k = (x).lane_lo(); k < (x).lane_hi(); k++)

namespace rlnamd {
namespace vt {

using vm::F12;
using vm::Prep;
using vm::PreparedKey;
using vm::vxi;

constexpr int TEAM = 8;              // lanes per proof
constexpr int TEAMS_PER_WAVE = 8;    // a workgroup is one wave of 64 lanes
constexpr int N_WORDS = 32;          // flag words per team (two Fq2 units)

// Exchange memory of one team, in Fq2 units: [flag words: 2][Fq12 slots: 6 each][scratch]
RLN_HD constexpr int team_units(int n_slots, int n_scratch) { return 2 + 6 * n_slots + n_scratch; }
constexpr int MILLER_SLOTS = 2, MILLER_SCRATCH = 30;
constexpr int FINAL_SLOTS = 10, FINAL_SCRATCH = 0;
constexpr int PREP_SLOTS = 0, PREP_SCRATCH = 32;
// the optimistic form (verify_agg_team_math.h): no x_i IC_i places in its first stage; its Miller stage, without
// alpha_beta and the lines of gamma and delta, is PAIR_SLOTS / PAIR_SCRATCH below
constexpr int PREP_AGG_SCRATCH = 14;

// The host's exchange: an array, the eight lanes run one after the other.  (verify_team_lds.h has the device's.)
struct HostX {
  static constexpr int NL = TEAM;
  Fq2* mem;
  int n_slots;
  int lane_lo() const { return 0; }
  int lane_hi() const { return TEAM; }
  int li(int k) const { return k; }
  Fq2& f(int slot, int i) const { return mem[2 + 6 * slot + i]; }
  Fq2& s(int i) const { return mem[2 + 6 * n_slots + i]; }
  uint32_t& w(int i) const { return reinterpret_cast<uint32_t*>(mem)[i]; }
  void sync() const {}
};

// Which proof a team works on: teams past the end of the batch redo the last proof and skip only the final store.
struct TeamIndex {
  uint32_t i;
  bool live;
};
RLN_HD TeamIndex team_index(uint32_t wave, uint32_t team, uint32_t n) {
  const uint32_t i = wave * TEAMS_PER_WAVE + team;
  return {i < n ? i : n - 1, i < n};
}

RLN_HD Fq2 sel(bool c, const Fq2& a, const Fq2& b) {
  Fq2 r;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    r.c0.v[i] = c ? a.c0.v[i] : b.c0.v[i];
    r.c1.v[i] = c ? a.c1.v[i] : b.c1.v[i];
  }
  return r;
}
RLN_HD Fq sel(bool c, const Fq& a, const Fq& b) {
  Fq r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
// a b + c d: each component is a 4-term dot product over Fq, one reduction (operands reduced: 4 p^2 < p 2^256)
RLN_HD Fq2 dot2(const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) {
  return {Fq::dot4(a.c0, b.c0, a.c1.neg(), b.c1, c.c0, d.c0, c.c1.neg(), d.c1),
          Fq::dot4(a.c0, b.c1, a.c1, b.c0, c.c0, d.c1, c.c1, d.c0)};
}
RLN_HD Fq2 fq_as_fq2(const Fq& a) { return {a, Fq::zero()}; }
RLN_HD int coef_lane(int k) { return k < 6 ? k : k - 6; }  // lanes 6 and 7 redo rows 0 and 1 and store nothing

// ---------------------------------------------------------------- Fq12 on a team (d may alias a or b everywhere)
template <class X>
RLN_HD void store_row(const X& x, int d, const Fq2* r) {
  x.sync();
  VT_LANES(x, k) {
    if (k < 6) x.f(d, k) = r[x.li(k)];
  }
  x.sync();
}
template <class X>
RLN_HD Fq2 row_mul(const X& x, int a, int b, int kk) {
  Fq2 acc = Fq2::zero();
  for (int i = 0; i < 6; i += 2) {
    int j0 = kk - i, j1 = kk - i - 1;
    const bool w0 = j0 < 0, w1 = j1 < 0;
    j0 += w0 ? 6 : 0;
    j1 += w1 ? 6 : 0;
    const Fq2 x0 = x.f(a, i), x1 = x.f(a, i + 1);
    acc = acc + dot2(sel(w0, vxi(x0), x0), x.f(b, j0), sel(w1, vxi(x1), x1), x.f(b, j1));
  }
  return acc;
}
template <class X>
VT_FN void t_mul(X x, int d, int a, int b) {
  Fq2 r[X::NL];
  VT_LANES(x, k) r[x.li(k)] = row_mul(x, a, b, coef_lane(k));
  store_row(x, d, r);
}
// The symmetric row: the unordered pairs {i, j} with i + j = k (mod 6).  Even k: two squares and two doubled
// products; odd k: three doubled products and an empty fourth place.  Four products in two sums instead of six in three.
// Each entry packs four pairs as octal digits i j, low pair first.
RLN_HD uint32_t sqr_pairs(int kk) {
  const uint32_t t0 = 000 | (033 << 6) | (015 << 12) | (024 << 18);
  const uint32_t t1 = 001 | (025 << 6) | (034 << 12) | (000 << 18);
  const uint32_t t2 = 011 | (044 << 6) | (002 << 12) | (035 << 18);
  const uint32_t t3 = 003 | (012 << 6) | (045 << 12) | (000 << 18);
  const uint32_t t4 = 022 | (055 << 6) | (004 << 12) | (013 << 18);
  const uint32_t t5 = 005 | (014 << 6) | (023 << 12) | (000 << 18);
  return kk == 0 ? t0 : kk == 1 ? t1 : kk == 2 ? t2 : kk == 3 ? t3 : kk == 4 ? t4 : t5;
}
template <class X>
RLN_HD Fq2 sqr_operand(const X& x, int a, int i, int j, bool empty) {
  Fq2 v = x.f(a, i);
  v = sel(i != j, v.dbl(), v);
  v = sel(i + j >= 6, vxi(v), v);
  return sel(empty, Fq2::zero(), v);
}
template <class X>
RLN_HD Fq2 row_sqr(const X& x, int a, int kk) {
  const uint32_t t = sqr_pairs(kk);
  Fq2 acc = Fq2::zero();
  for (int s = 0; s < 4; s += 2) {
    const int i0 = (t >> (6 * s + 3)) & 7, j0 = (t >> (6 * s)) & 7;
    const int i1 = (t >> (6 * s + 9)) & 7, j1 = (t >> (6 * s + 6)) & 7;
    const bool empty = s == 2 && (kk & 1);   // the fourth place of an odd row
    acc = acc + dot2(sqr_operand(x, a, i0, j0, false), x.f(a, j0), sqr_operand(x, a, i1, j1, empty), x.f(a, j1));
  }
  return acc;
}
template <class X>
VT_FN void t_sqr(X x, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) r[x.li(k)] = row_sqr(x, a, coef_lane(k));
  store_row(x, d, r);
}
// f (l0 + l1 w + l3 w^3) with the line in scratch places i0, i1, i3
template <class X>
VT_FN void t_mul_line(X x, int d, int a, int i0, int i1, int i3) {
  Fq2 r[X::NL];
  VT_LANES(x, k) {
    const int kk = coef_lane(k);
    const bool w1 = kk < 1, w3 = kk < 3;
    const Fq2 x1 = x.f(a, kk - 1 + (w1 ? 6 : 0)), x3 = x.f(a, kk - 3 + (w3 ? 6 : 0));
    r[x.li(k)] = x.f(a, kk) * x.s(i0) + dot2(sel(w1, vxi(x1), x1), x.s(i1), sel(w3, vxi(x3), x3), x.s(i3));
  }
  store_row(x, d, r);
}
// Granger-Scott in the cyclotomic subgroup, vm::f12_cyclotomic_sqr's three Fq4 squares: the square of (a, b) =
// (x_m, x_(m+3)) gives a^2 + xi b^2 to lane 2 m and 2 a b to lane (2 m + 3) mod 6 (times xi on lane 1); every lane
// ends with 3 t -+ 2 x_k
template <class X>
VT_FN void t_cyclotomic_sqr(X x, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) {
    const int kk = coef_lane(k);
    const bool even = (kk & 1) == 0;
    const int m = even ? kk >> 1 : ((kk + 3) % 6) >> 1;
    const Fq2 p = x.f(a, m), q = x.f(a, m + 3), z = x.f(a, kk);
    Fq2 t = dot2(p, sel(even, p, q), sel(even, vxi(q), p), q);
    t = sel(kk == 1, vxi(t), t);
    r[x.li(k)] = sel(even, (t - z).dbl() + t, (t + z).dbl() + t);
  }
  store_row(x, d, r);
}
template <class X>
VT_FN void t_frob(X x, const PreparedKey* vk, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) {
    const int kk = coef_lane(k);
    const Fq2 c = x.f(a, kk).conj();
    r[x.li(k)] = sel(kk == 0, c, c * vk->frob1[kk]);
  }
  store_row(x, d, r);
}
template <class X>
VT_FN void t_frob2(X x, const PreparedKey* vk, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) {
    const int kk = coef_lane(k);
    const Fq2 c = x.f(a, kk);
    r[x.li(k)] = sel(kk == 0, c, c.mul_fq(vk->frob2[kk].c0));
  }
  store_row(x, d, r);
}
template <class X>
RLN_HD void t_conj(const X& x, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) {
    const int kk = coef_lane(k);
    const Fq2 c = x.f(a, kk);
    r[x.li(k)] = sel((kk & 1) != 0, c.neg(), c);
  }
  store_row(x, d, r);
}
template <class X>
RLN_HD void t_copy(const X& x, int d, int a) {
  Fq2 r[X::NL];
  VT_LANES(x, k) r[x.li(k)] = x.f(a, coef_lane(k));
  store_row(x, d, r);
}
template <class X>
RLN_HD void t_load(const X& x, int d, const F12* g) {  // a record in memory (the key, the stage buffers) into a slot
  Fq2 r[X::NL];
  VT_LANES(x, k) r[x.li(k)] = g->c[coef_lane(k)];
  store_row(x, d, r);
}
template <class X>
VT_FN void t_inv(X x, int d, int a) {  // lane 0 alone
  F12 r[X::NL];
  VT_LANES(x, k) {
    if (k == 0) {
      F12 v;
      for (int i = 0; i < 6; i++) v.c[i] = x.f(a, i);
      vm::f12_inv(&r[x.li(k)], &v);
    }
  }
  x.sync();
  VT_LANES(x, k) {
    if (k == 0)
      for (int i = 0; i < 6; i++) x.f(d, i) = r[x.li(k)].c[i];
  }
  x.sync();
}
template <class X>
VT_FN void t_pow_u(X x, int d, int a) {  // d must not alias a
  const uint64_t u = 4965661367192848881ULL;
  t_copy(x, d, a);
  for (int i = 61; i >= 0; i--) {
    t_cyclotomic_sqr(x, d, d);
    if ((u >> i) & 1) t_mul(x, d, d, a);
  }
}
// vm::final_exponentiation on team operations; the value is in slot 0 before and after.  Ten slots, all in the
// exchange memory.
template <class X>
VT_FN void t_final_exponentiation(X x, const PreparedKey* vk) {
  enum { F = 0, T, FX, FX2, FX3, Y0, Y4, Y6, T0, T1 };
  t_inv(x, T, F);
  t_conj(x, F, F);
  t_mul(x, F, F, T);
  t_frob2(x, vk, T, F);
  t_mul(x, F, T, F);
  t_pow_u(x, FX, F);
  t_pow_u(x, FX2, FX);
  t_pow_u(x, FX3, FX2);
  t_frob(x, vk, Y0, F);
  t_frob2(x, vk, T, F);
  t_mul(x, Y0, Y0, T);
  t_frob(x, vk, T, T);
  t_mul(x, Y0, Y0, T);
  t_frob(x, vk, T, FX2);
  t_mul(x, Y4, FX, T);
  t_conj(x, Y4, Y4);
  t_frob(x, vk, T, FX3);
  t_mul(x, Y6, FX3, T);
  t_conj(x, Y6, Y6);
  t_conj(x, FX3, FX2);  // y5
  t_sqr(x, T0, Y6);
  t_mul(x, T0, T0, Y4);
  t_mul(x, T0, T0, FX3);
  t_frob(x, vk, T, FX);
  t_conj(x, T, T);
  t_mul(x, T1, T, FX3);
  t_mul(x, T1, T1, T0);
  t_frob2(x, vk, T, FX2);
  t_mul(x, T0, T0, T);
  t_sqr(x, T1, T1);
  t_mul(x, T1, T1, T0);
  t_sqr(x, T1, T1);
  t_conj(x, T, F);  // y1
  t_mul(x, T0, T1, T);
  t_mul(x, T1, T1, Y0);
  t_sqr(x, T0, T0);
  t_mul(x, F, T0, T1);
}

// ---------------------------------------------------------------- Miller loop
// Scratch places of the Miller stage
enum {
  SX = 0, SY, SZ,            // the running point
  SB, SC, SYZ, SX2, SXY,     // doubling, level 1: Y^2, Z^2, Y Z, X^2, X Y
  SE,                        // 3 b' Z^2
  STH, SLA, SCC, SDD, SEE, SFF, SGG,   // addition: theta, lambda, theta^2, lambda^2, E, F, G
  SA0, SA1, SA3,             // the line of the variable pair at A
  SGY, SG1, SGC,             // the gamma line at -IC
  SDY, SD1, SDC,             // the delta line at -C
  SQX, SQY,                  // the point that an addition step adds
  S_END
};
static_assert(S_END <= MILLER_SCRATCH, "scratch places of the Miller stage");
// With one pair (KEY_LINES = false) the six places of the gamma and delta lines go: the added point moves down
constexpr int PAIR_SLOTS = 1, PAIR_SCRATCH = S_END - (SQX - SGY);
template <bool KEY_LINES>
RLN_HD constexpr int sq_place(int i) { return KEY_LINES ? i : i - (SQX - SGY); }
static_assert(sq_place<false>(SQY) + 1 <= PAIR_SCRATCH, "scratch places of the one-pair Miller stage");

// Lanes 2..5 of a step's level 3 form the four places of its lines that need one product each: l0 y_A and l1 x_A of
// the variable pair, -lam x of the gamma and of the delta line (an Fq factor as an Fq2, so that every lane of the level
// runs one product program).  A pair that is absent (flags) gets the line 1: the same instructions, f unchanged.
// KEY_LINES = false is the one pair of the optimistic form: lanes 4 and 5 have no line, P is a record without icn / cn
// (vm::PrepAgg) and the places of the gamma and delta lines are never touched.
template <bool KEY_LINES, class X, class P>
RLN_HD void line_factor(const X& x, const PreparedKey* vk, const P* p, int k, int step, const Fq2& l0,
                        const Fq2& l1, Fq2* a, Fq2* b) {
  if (k == 2) {
    *a = l0;
    *b = fq_as_fq2(p->A.y);
  } else if (k == 3) {
    *a = l1;
    *b = fq_as_fq2(p->A.x);
  } else if constexpr (KEY_LINES) {
    if (k == 4) {
      *a = vk->gamma[step].lam;
      *b = fq_as_fq2(p->icn.x.neg());
    } else if (k == 5) {
      *a = vk->delta[step].lam;
      *b = fq_as_fq2(p->cn.x.neg());
    }
  }
}
template <bool KEY_LINES, class X, class P>
RLN_HD void line_store(const X& x, const PreparedKey* vk, const P* p, int k, int step, const Fq2& v) {
  const bool va = (p->flags & vm::P_VARYING) != 0;
  if (k == 2) {
    x.s(SA0) = sel(va, v, Fq2::one());
  } else if (k == 3) {
    x.s(SA1) = sel(va, v, Fq2::zero());
  } else if constexpr (KEY_LINES) {
    const bool ga = (p->flags & vm::P_GAMMA) != 0, de = (p->flags & vm::P_DELTA) != 0;
    if (k == 4) {
      x.s(SG1) = sel(ga, v, Fq2::zero());
      x.s(SGC) = sel(ga, vk->gamma[step].c, Fq2::zero());
    } else if (k == 5) {
      x.s(SD1) = sel(de, v, Fq2::zero());
      x.s(SDC) = sel(de, vk->delta[step].c, Fq2::zero());
    }
  }
}
// T <- 2 T and the lines of step `step` (vm::proj_double dealt to the lanes: three levels of products)
template <bool KEY_LINES, class X, class P>
VT_FN void t_double_step_t(X x, const PreparedKey* vk, const P* p, int step) {
  Fq2 r[X::NL];
  // level 1: Y^2, Z^2, Y Z, X^2, X Y on lanes 0..4
  VT_LANES(x, k) {
    const int ia = k == 0 ? SY : k == 1 ? SZ : k == 2 ? SY : SX;
    const int ib = k == 0 ? SY : k == 1 ? SZ : k == 2 ? SZ : k == 3 ? SX : SY;
    r[x.li(k)] = x.s(ia) * x.s(ib);
  }
  x.sync();
  VT_LANES(x, k) {
    if (k < 5) x.s(SB + k) = r[x.li(k)];
  }
  x.sync();
  // level 2: E = 3 b' Z^2 on lane 0, Z' = 8 Y^2 (Y Z) on lane 1
  VT_LANES(x, k) {
    const Fq2 a = x.s(k == 0 ? SC : SB);
    const Fq2 b = sel(k == 0, vk->twist_3b, x.s(SYZ));
    r[x.li(k)] = a * b;
  }
  x.sync();
  VT_LANES(x, k) {
    if (k == 0) x.s(SE) = r[x.li(k)];
    if (k == 1) x.s(SZ) = r[x.li(k)].dbl().dbl().dbl();
  }
  x.sync();
  // level 3: X' = 2 X Y (B - F), Y' = S^2 - 12 E^2 (F = 3 E, S = B + F) on lanes 0, 1; the line factors on lanes 2..5
  VT_LANES(x, k) {
    const Fq2 B = x.s(SB), E = x.s(SE);
    const Fq2 F = E.dbl() + E;
    Fq2 a = Fq2::zero(), b = Fq2::zero(), c = Fq2::zero(), d = Fq2::zero();
    if (k == 0) {
      a = x.s(SXY).dbl();
      b = B - F;
    } else if (k == 1) {
      a = b = B + F;
      c = F.dbl().dbl().neg();
      d = E;
    } else {
      const Fq2 X2 = x.s(SX2);
      line_factor<KEY_LINES>(x, vk, p, k, step, x.s(SYZ).dbl().neg(), X2.dbl() + X2, &a, &b);
    }
    r[x.li(k)] = dot2(a, b, c, d);
  }
  x.sync();
  VT_LANES(x, k) {
    if (k == 0) x.s(SX) = r[x.li(k)];
    if (k == 1) x.s(SY) = r[x.li(k)];
    if (k == 6) x.s(SA3) = sel((p->flags & vm::P_VARYING) != 0, x.s(SE) - x.s(SB), Fq2::zero());
    line_store<KEY_LINES>(x, vk, p, k, step, r[x.li(k)]);
  }
  x.sync();
}
// T <- T + Q (Q in SQX, SQY) and the lines of step `step` (vm::proj_add: four levels)
template <bool KEY_LINES, class X, class P>
VT_FN void t_add_step_t(X x, const PreparedKey* vk, const P* p, int step) {
  constexpr int QX = sq_place<KEY_LINES>(SQX), QY = sq_place<KEY_LINES>(SQY);
  Fq2 r[X::NL];
  // level 1: theta = Y - y_Q Z, lambda = X - x_Q Z
  VT_LANES(x, k) r[x.li(k)] = x.s(k == 0 ? SY : SX) - x.s(k == 0 ? QY : QX) * x.s(SZ);
  x.sync();
  VT_LANES(x, k) {
    if (k < 2) x.s(STH + k) = r[x.li(k)];
  }
  x.sync();
  // level 2: theta^2, lambda^2, l3 = theta x_Q - lambda y_Q
  VT_LANES(x, k) {
    const Fq2 th = x.s(STH), la = x.s(SLA);
    const Fq2 a = sel(k == 1, la, th);
    const bool l3 = k == 2;
    r[x.li(k)] = dot2(a, sel(l3, x.s(QX), a), sel(l3, la.neg(), Fq2::zero()), x.s(QY));
  }
  x.sync();
  VT_LANES(x, k) {
    if (k < 2) x.s(SCC + k) = r[x.li(k)];
    if (k == 2) x.s(SA3) = sel((p->flags & vm::P_VARYING) != 0, r[x.li(k)], Fq2::zero());
  }
  x.sync();
  // level 3: E = lambda D, F = Z C, G = X D on lanes 0, 1, 6; the line factors on lanes 2..5
  VT_LANES(x, k) {
    Fq2 a = Fq2::zero(), b = Fq2::zero();
    if (k == 0) {
      a = x.s(SLA);
      b = x.s(SDD);
    } else if (k == 1) {
      a = x.s(SZ);
      b = x.s(SCC);
    } else if (k == 6) {
      a = x.s(SX);
      b = x.s(SDD);
    } else {
      line_factor<KEY_LINES>(x, vk, p, k, step, x.s(SLA), x.s(STH).neg(), &a, &b);
    }
    r[x.li(k)] = a * b;
  }
  x.sync();
  VT_LANES(x, k) {
    if (k == 0) x.s(SEE) = r[x.li(k)];
    if (k == 1) x.s(SFF) = r[x.li(k)];
    if (k == 6) x.s(SGG) = r[x.li(k)];
    line_store<KEY_LINES>(x, vk, p, k, step, r[x.li(k)]);
  }
  x.sync();
  // level 4: X' = lambda H, Y' = theta (G - H) - E Y, Z' = Z E with H = E + F - 2 G
  VT_LANES(x, k) {
    const Fq2 E = x.s(SEE), G = x.s(SGG);
    const Fq2 H = E + x.s(SFF) - G.dbl();
    Fq2 a = x.s(SLA), b = H, c = Fq2::zero(), d = Fq2::zero();
    if (k == 1) {
      a = x.s(STH);
      b = G - H;
      c = E.neg();
      d = x.s(SY);
    } else if (k == 2) {
      a = x.s(SZ);
      b = E;
    }
    r[x.li(k)] = dot2(a, b, c, d);
  }
  x.sync();
  VT_LANES(x, k) {
    if (k < 3) x.s(SX + k) = r[x.li(k)];
  }
  x.sync();
}
template <bool KEY_LINES, class X>
RLN_HD void t_step_lines(const X& x) {
  t_mul_line(x, 0, 0, SA0, SA1, SA3);
  if constexpr (KEY_LINES) {
    t_mul_line(x, 0, 0, SGY, SG1, SGC);
    t_mul_line(x, 0, 0, SDY, SD1, SDC);
  }
}
// The walk of the running point of (A, B) with the lines of each step folded into slot 0: all three pairs
// (vm::miller_loop), or with KEY_LINES = false the variable pair alone (vm::miller_loop_pair: no line of gamma or
// delta is formed or multiplied in, not even as the line 1)
template <bool KEY_LINES, class X, class P>
RLN_HD void t_miller_walk(const X& x, const PreparedKey* vk, const P* p) {
  constexpr int QX = sq_place<KEY_LINES>(SQX), QY = sq_place<KEY_LINES>(SQY);
  VT_LANES(x, k) {
    if (k < 6) x.f(0, k) = k == 0 ? Fq2::one() : Fq2::zero();
    if (k == 0) {
      x.s(SX) = x.s(QX) = p->B.x;
      x.s(SY) = x.s(QY) = p->B.y;
      x.s(SZ) = Fq2::one();
    }
    if constexpr (KEY_LINES) {
      if (k == 1) {
        x.s(SGY) = sel((p->flags & vm::P_GAMMA) != 0, fq_as_fq2(p->icn.y), Fq2::one());
        x.s(SDY) = sel((p->flags & vm::P_DELTA) != 0, fq_as_fq2(p->cn.y), Fq2::one());
      }
    }
  }
  x.sync();
  int step = 0;
  for (int i = ATE_LOOP_BITS - 2; i >= 0; i--) {
    t_sqr(x, 0, 0);
    t_double_step_t<KEY_LINES>(x, vk, p, step++);
    t_step_lines<KEY_LINES>(x);
    const uint32_t word = i >= 32 ? ATE_LOOP[1] : ATE_LOOP[0];
    if ((word >> (i & 31)) & 1) {
      t_add_step_t<KEY_LINES>(x, vk, p, step++);
      t_step_lines<KEY_LINES>(x);
    }
  }
  // pi(B) and -pi^2(B)
  Fq2 r[X::NL];
  for (int last = 0; last < 2; last++) {
    VT_LANES(x, k) {
      const bool y = (k & 1) != 0;
      const Fq2 c = sel(y, p->B.y, p->B.x);
      if (last == 0)
        r[x.li(k)] = c.conj() * sel(y, vk->frob1[3], vk->frob1[2]);
      else
        r[x.li(k)] = sel(y, (c * vk->g23).neg(), c * vk->g22);
    }
    x.sync();
    VT_LANES(x, k) {
      if (k < 2) x.s(QX + k) = r[x.li(k)];
    }
    x.sync();
    t_add_step_t<KEY_LINES>(x, vk, p, step++);
    t_step_lines<KEY_LINES>(x);
  }
}
// vm::miller_loop times vk->alpha_beta: the value is left in slot 0
template <class X>
VT_FN void t_miller_loop(X x, const PreparedKey* vk, const Prep* p) {
  t_miller_walk<true>(x, vk, p);
  t_load(x, 1, &vk->alpha_beta);
  t_mul(x, 0, 0, 1);
}

// ---------------------------------------------------------------- stage 3: verdict and GT value
// ok and gt may each be null; nothing is stored for a team past the end of the batch
template <class X>
VT_FN void t_finish(X x, const Prep* p, bool live, uint8_t* ok, uint32_t* gt) {
  const bool rejected = (p->flags & vm::P_REJECT) != 0;
  VT_LANES(x, k) {
    if (k < 6) {
      const Fq2 c = x.f(0, k);
      x.w(k) = (k == 0 ? c == Fq2::one() : c.is_zero()) ? 1 : 0;
      if (gt && live) {
        uint32_t a[8], b[8];
        c.c0.to_canonical(a);
        c.c1.to_canonical(b);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          gt[16 * k + j] = rejected ? 0 : a[j];
          gt[16 * k + 8 + j] = rejected ? 0 : b[j];
        }
      }
    }
  }
  x.sync();
  VT_LANES(x, k) {
    if (k == 0 && ok && live)
      *ok = (!rejected && (x.w(0) & x.w(1) & x.w(2) & x.w(3) & x.w(4) & x.w(5))) ? 1 : 0;
  }
  x.sync();
}

// ---------------------------------------------------------------- stage 1: decompression, subgroup, public inputs
// Scratch places and flag words of the first stage
enum {
  PX = 0,        // PX + k: the x coordinate read by lane k (A, C: in c0; B: the Fq2)
  PRHS = 3,      // x_B^3 + b'
  PROOT = 4,     // PROOT + k: lane k's square root (c0): y_A, y_C, the norm's
  PCAND = 7,     // PCAND + k: the candidate root of lane k = 0, 1
  PA = 9, PC, PBX, PBY,   // the decompressed points (a G1 point as one Fq2 unit: x | y)
  PACC = 14,     // PACC + 2 k: lane k's x_i IC_i (X Y | ZZ ZZZ)
  P_END = PACC + 2 * TEAM
};
static_assert(P_END <= PREP_SCRATCH, "scratch places of the first stage");
enum { WF = 0 /* + k: lanes 0..2 */, WCAND = 4 /* + k */, WOK = 8 /* + k: A, C, B */, WSUB = 11, WVAL = 16 /* + k */ };
enum : uint32_t { F_X = 1, F_ROOT = 2, F_INF = 4, F_SPECIAL = 8 };

RLN_HD G1XYZZ ld_xyzz(const Fq2& a, const Fq2& b) { return {a.c0, a.c1, b.c0, b.c1}; }
// The reject rules of the points, one text for both team forms (t_prepare below, verify_agg_team_math.h's
// t_prepare_agg), as vm::checked_points is for the lane forms: the decompression phases and the subgroup test.  With
// what is one program on different data run at once: the square-root chains of y_A, y_C and of the norm of B's
// right-hand side (lanes 0..2), then both candidates of vm::fq2_sqrt (lanes 0, 1).  The 128-step ladder of the subgroup
// test stays on lane 0.  Leaves A, C and B in PA, PC, PBX | PBY and the verdicts in WOK + 0..2 and WSUB; the bound on
// the public inputs is the caller's (val_below_r).
template <class X>
RLN_HD void t_checked_points(const X& x, const PreparedKey* vk, const uint32_t* proof) {
  // phase 1: read the three x coordinates, form the right-hand sides, one square root per lane
  {
    Fq in[X::NL], root[X::NL];
    Fq2 keep[X::NL], rhs2[X::NL];
    uint32_t fl[X::NL];
    VT_LANES(x, k) {
      const int l = x.li(k);
      in[l] = Fq::zero();
      keep[l] = rhs2[l] = Fq2::zero();
      fl[l] = 0;
      if (k < 2) {
        const uint32_t* g = proof + (k ? 24 : 0);
        Fq xx;
        const bool okx = vm::load_x_checked(g, true, &xx);
        in[l] = xx.sqr() * xx + vk->three;
        keep[l].c0 = xx;
        fl[l] = (okx ? F_X : 0) | ((g[7] & 0x40000000u) ? F_INF : 0);
      } else if (k == 2) {
        const uint32_t* g = proof + 8;
        Fq x0, x1;
        const bool ok0 = vm::load_x_checked(g, false, &x0), ok1 = vm::load_x_checked(g + 8, true, &x1);
        const Fq2 xx{x0, x1};
        const Fq2 rhs = xx.sqr() * xx + vk->twist_b;
        const bool special = rhs.c1.is_zero();
        in[l] = sel(special, rhs.c0, rhs.c0.sqr() + rhs.c1.sqr());
        keep[l] = xx;
        rhs2[l] = rhs;
        fl[l] = ((ok0 && ok1) ? F_X : 0) | ((g[15] & 0x40000000u) ? F_INF : 0) | (special ? F_SPECIAL : 0);
      }
    }
    VT_LANES(x, k) {
      const int l = x.li(k);
      if (vm::fq_sqrt(vk, &in[l], &root[l])) fl[l] |= F_ROOT;
    }
    VT_LANES(x, k) {
      const int l = x.li(k);
      if (k < 3) {
        x.s(PX + k) = keep[l];
        x.s(PROOT + k) = fq_as_fq2(root[l]);
        x.w(WF + k) = fl[l];
      }
      if (k == 2) x.s(PRHS) = rhs2[l];
    }
    x.sync();
  }
  // phase 2: the two candidates of the Fq2 root side by side (vm::fq2_sqrt; c1 == 0: the roots of c0 and of -c0)
  {
    Fq t[X::NL], x0[X::NL];
    bool okt[X::NL];
    VT_LANES(x, k) {
      const int l = x.li(k);
      const Fq2 a = x.s(PRHS);
      const Fq n = x.s(PROOT + 2).c0;
      const bool special = (x.w(WF + 2) & F_SPECIAL) != 0, second = (k & 1) != 0;
      t[l] = sel(special, sel(second, a.c0.neg(), a.c0), (a.c0 + sel(second, n.neg(), n)) * vk->inv2);
    }
    VT_LANES(x, k) {
      const int l = x.li(k);
      okt[l] = vm::fq_sqrt(vk, &t[l], &x0[l]);
    }
    VT_LANES(x, k) {
      const int l = x.li(k);
      const Fq2 a = x.s(PRHS);
      const bool special = (x.w(WF + 2) & F_SPECIAL) != 0, second = (k & 1) != 0;
      const Fq x1 = a.c1 * x0[l].dbl().inv();
      const Fq2 plain{x0[l], x1};
      const Fq2 cand = sel(special, sel(second, Fq2{Fq::zero(), x0[l]}, Fq2{x0[l], Fq::zero()}), plain);
      const bool valid = okt[l] && (special || (!x0[l].is_zero() && plain.sqr() == a));
      if (k < 2) {
        x.s(PCAND + k) = cand;
        x.w(WCAND + k) = valid ? 1 : 0;
      }
    }
    x.sync();
  }
  // phase 3: signs and the three points (zkey.cpp's rules, as vm::g1_decompress / g2_decompress)
  VT_LANES(x, k) {
    if (k < 2) {
      const uint32_t fl = x.w(WF + k), top = proof[(k ? 24 : 0) + 7];
      const Fq xx = x.s(PX + k).c0;
      Fq y = x.s(PROOT + k).c0;
      if (vm::y_is_neg(y) != ((top & 0x80000000u) != 0)) y = y.neg();
      const bool inf = (fl & F_INF) != 0;
      x.s(PA + k) = sel(inf, Fq2::zero(), Fq2{xx, y});
      x.w(WOK + k) = (inf || ((fl & F_X) && (fl & F_ROOT))) ? 1 : 0;
    } else if (k == 2) {
      const uint32_t fl = x.w(WF + 2), top = proof[8 + 15];
      const bool v0 = x.w(WCAND) != 0, v1 = x.w(WCAND + 1) != 0;
      Fq2 y = sel(v0, x.s(PCAND), x.s(PCAND + 1));
      if (vm::y2_is_neg(y) != ((top & 0x80000000u) != 0)) y = y.neg();
      const bool inf = (fl & F_INF) != 0;
      const bool ok = inf || ((fl & F_X) && ((fl & F_SPECIAL) || (fl & F_ROOT)) && (v0 || v1));
      x.s(PBX) = sel(inf || !ok, Fq2::zero(), x.s(PX + 2));
      x.s(PBY) = sel(inf || !ok, Fq2::zero(), y);
      x.w(WOK + 2) = ok ? 1 : 0;
    }
  }
  x.sync();
  // phase 4, first half: the subgroup test on lane 0
  VT_LANES(x, k) {
    if (k == 0) {
      const G2Affine B{x.s(PBX), x.s(PBY)};
      x.w(WSUB) = vm::g2_in_subgroup(vk, &B) ? 1 : 0;
    }
  }
}
// a public input (8 canonical words) is below r
RLN_HD bool val_below_r(const uint32_t* v) {
  bool lt = false, decided = false;
#pragma unroll
  for (int j = 7; j >= 0; j--) {
    const uint32_t c = v[j], m = FrParams::MOD[j];
    if (!decided && c != m) {
      lt = c < m;
      decided = true;
    }
  }
  return lt;
}
// vm::prepare: t_checked_points, then a lane per public input for x_i IC_i, summed on lane 0
template <class X>
VT_FN void t_prepare(X x, const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, Prep* out, bool live) {
  t_checked_points(x, vk, proof);
  // phase 4: a lane per public input, eight at a time
  G1XYZZ total[X::NL];
  VT_LANES(x, k) {
    total[x.li(k)] = G1XYZZ::inf();
    x.w(WVAL + k) = 1;
  }
  const uint32_t nv = vk->n_values;
  for (uint32_t base = 0; base < nv; base += TEAM) {
    G1XYZZ acc[X::NL];
    VT_LANES(x, k) {
      const int l = x.li(k);
      const bool active = base + k < nv;
      const uint32_t i = active ? base + k : 0;
      const uint32_t* v = vals + 8 * i;
      const bool lt = val_below_r(v);
      if (active && !lt) x.w(WVAL + k) = 0;
      acc[l] = G1XYZZ::inf();
      for (int w = 63; w >= 0; w--) {
        if (w != 63) acc[l] = acc[l].dbl().dbl().dbl().dbl();
        const uint32_t d = active ? (v[w >> 3] >> ((w & 7) * 4)) & 15 : 0;
        if (d) acc[l].madd(vk->ic_mult[15 * i + d - 1]);
      }
    }
    x.sync();
    VT_LANES(x, k) {
      const int l = x.li(k);
      x.s(PACC + 2 * k) = {acc[l].X, acc[l].Y};
      x.s(PACC + 2 * k + 1) = {acc[l].ZZ, acc[l].ZZZ};
    }
    x.sync();
    VT_LANES(x, k) {
      if (k == 0)
        for (int j = 0; j < TEAM; j++) total[x.li(k)].add(ld_xyzz(x.s(PACC + 2 * j), x.s(PACC + 2 * j + 1)));
    }
    x.sync();
  }
  // phase 5: the record (lane 0)
  VT_LANES(x, k) {
    if (k == 0) {
      bool ok = x.w(WOK) && x.w(WOK + 1) && x.w(WOK + 2) && x.w(WSUB);
      for (int j = 0; j < TEAM; j++) ok = ok && x.w(WVAL + j);
      G1XYZZ t = total[x.li(k)];
      t.madd(vk->ic0);
      const G1Affine ic = t.to_affine();
      const Fq2 a = x.s(PA), c = x.s(PC);
      const G1Affine A{a.c0, a.c1}, C{c.c0, c.c1};
      const G2Affine B{x.s(PBX), x.s(PBY)};
      Prep r;
      if (ok) {
        r.A = A;
        r.B = B;
        r.icn = ic.neg();
        r.cn = C.neg();
        r.flags = ((A.is_inf() || B.is_inf()) ? 0 : vm::P_VARYING) | (ic.is_inf() ? 0 : vm::P_GAMMA) |
                  (C.is_inf() ? 0 : vm::P_DELTA);
      } else {
        r.A = G1Affine::inf();
        r.B = G2Affine::inf();
        r.icn = r.cn = G1Affine::inf();
        r.flags = vm::P_REJECT;
      }
      if (live) *out = r;
    }
  }
  x.sync();
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole verification of one proof by one team, stage by stage with the records the kernels pass through HBM
// (tests/host/verifyteam.cpp; the kernels call the three stages).  mem: team_units(FINAL_SLOTS, PREP_SCRATCH) Fq2.
inline void host_verify_team(const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, bool live, Fq2* mem,
                             uint8_t* ok, uint32_t* gt) {
  Prep p;
  F12 f;
  t_prepare(HostX{mem, PREP_SLOTS}, vk, proof, vals, &p, true);
  const HostX xm{mem, MILLER_SLOTS};
  t_miller_loop(xm, vk, &p);
  for (int i = 0; i < 6; i++) f.c[i] = xm.f(0, i);
  const HostX xf{mem, FINAL_SLOTS};
  t_load(xf, 0, &f);
  t_final_exponentiation(xf, vk);
  t_finish(xf, &p, live, ok, gt);
}
// n proofs as waves of eight teams, the way the kernels index them
inline void host_verify_waves(const PreparedKey* vk, size_t n, const uint32_t* proofs, const uint32_t* vals,
                              uint8_t* ok, uint32_t* gt, Fq2* mem) {
  const uint32_t waves = (uint32_t)((n + TEAMS_PER_WAVE - 1) / TEAMS_PER_WAVE);
  for (uint32_t wv = 0; wv < waves; wv++)
    for (uint32_t t = 0; t < (uint32_t)TEAMS_PER_WAVE; t++) {
      const TeamIndex ti = team_index(wv, t, (uint32_t)n);
      host_verify_team(vk, proofs + (size_t)32 * ti.i, vals + (size_t)8 * vk->n_values * ti.i, ti.live, mem,
                       ok ? ok + ti.i : nullptr, gt ? gt + (size_t)96 * ti.i : nullptr);
    }
}
#endif

}  // namespace vt
}  // namespace rlnamd
