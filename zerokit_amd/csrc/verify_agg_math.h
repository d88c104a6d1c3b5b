// The optimistic form of the device verifier: one combined pairing check for all proofs of a chunk, written like
// verify_math.h for one GPU lane per proof (verify_agg.hip) and for a plain g++ build that runs the lanes in a loop
// (tests/host/verifyagg.cpp).  No HIP call.
//
// Each proof i that the shared reject rules (vm::checked_points) let through gets a scalar r_i in [1, 2^128), drawn by
// the caller after the proofs are fixed.  With
//
//     R = sum r_i,   S_j = sum_i r_i x_ij  (mod r),   L = R IC_0 + sum_j S_j IC_j,   C* = sum_i r_i C_i
//
// the chunk is accepted when
//
//     prod_i e(r_i A_i, B_i) . e(-R alpha, beta) . e(-L, gamma) . e(-C*, delta) == 1,
//
// which is prod_i GT_i^(r_i) for the per-proof pairing products GT_i of verify_math.h.  Every GT_i lies in the
// order-r group (the per-proof checks put A, C on G1 and B in the order-r subgroup of the twist), so a chunk with a
// GT_i != 1 passes for at most one value of r_i given the others: probability at most 2^-128 over the scalars.
//
// A lane does prepare_agg (the shared checks, r A, r C, r x_j) and the Miller loop of its one pair (r A, B) -- no
// lines of gamma or delta, no public-input ladder, no final exponentiation.  The partials {Fq12 product, G1 sum,
// n_values + 1 Fr sums} are then folded 64 to 1 per level (fold_step, sum_column) and finish_host, on the host, does
// the three fixed pairs and the one final exponentiation with pairing.h.  The device's Miller value differs from
// pairing.h's by factors of proper subfields, which the final exponentiation removes.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "pairing.h"
#include "verify_math.h"

namespace rlnamd {
namespace vm {

constexpr int FOLD = 64;  // partials folded into one per level: a workgroup of one wave

// What prepare_agg hands to the single-pair Miller loop (the fields miller_loop_t reads)
struct PrepAgg {
  G1Affine A;  // r A
  G2Affine B;
  uint32_t flags;  // P_REJECT | P_VARYING
};
// A partial aggregate; its n_values + 1 Fr sums (R, S_1 ..) travel in a separate array, one row per partial
struct Partial {
  F12 f;
  G1XYZZ c;
};
RLN_HD void partial_identity(Partial* p) {
  f12_one(&p->f);
  p->c = G1XYZZ::inf();
}

// k P, k of 128 bits (4 words), by double-and-add from the top bit, as g2_in_subgroup walks its 6 u^2
VM_FN void g1_mul128(const G1Affine* p, const uint32_t* k, G1XYZZ* out) {
  G1XYZZ acc = G1XYZZ::inf();
  bool started = false;
  for (int i = 127; i >= 0; i--) {
    if (started) acc = acc.dbl();
    if ((k[i >> 5] >> (i & 31)) & 1) {
      acc.madd(*p);
      started = true;
    }
  }
  *out = acc;
}

// Stage 1 of the optimistic form.  scalar: 4 little-endian words, not all zero.  sums: n_values + 1 entries, r and the
// r x_j.  A rejected proof contributes the identity to every part (its r counts as 0); an infinite A or B leaves the
// pair out (it contributes 1, as in miller_loop_3) while r, r x_j and r C still count.
VM_FN void prepare_agg(const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, const uint32_t* scalar,
                       PrepAgg* out, G1XYZZ* rc, Fr* sums) {
  G1Affine A, C;
  const bool ok = checked_points(vk, proof, vals, &A, &out->B, &C);
  if (!ok) {
    out->A = G1Affine::inf();
    out->B = G2Affine::inf();
    out->flags = P_REJECT;
    *rc = G1XYZZ::inf();
    for (uint32_t j = 0; j <= vk->n_values; j++) sums[j] = Fr::zero();
    return;
  }
  G1XYZZ ra;
  g1_mul128(&A, scalar, &ra);
  out->A = ra.to_affine();
  g1_mul128(&C, scalar, rc);
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = i < 4 ? scalar[i] : 0;
  const Fr r = Fr::from_canonical(k);
  sums[0] = r;
  for (uint32_t j = 0; j < vk->n_values; j++) {
    uint32_t x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = vals[8 * j + i];
    sums[1 + j] = Fr::from_canonical(x) * r;
  }
  out->flags = (out->A.is_inf() || out->B.is_inf()) ? 0 : P_VARYING;
}

// miller(r A, B) alone: vm::miller_loop's walk of the running point without the lines of gamma and delta, and not
// multiplied by alpha_beta
struct OnePairStep {
  RLN_HD void operator()(const PreparedKey* vk, const PrepAgg* p, F12* f, int k, const Fq2* l0, const Fq2* l1,
                         const Fq2* l3) const {
    miller_step_t<false>(vk, p, f, k, l0, l1, l3);
  }
};
VM_FN void miller_loop_pair(const PreparedKey* vk, const PrepAgg* p, F12* f) {
  miller_loop_t(vk, p, f, OnePairStep{});
}

// a <- a (+) b.  The G1 addition is complete: equal points double (identical proofs under equal scalars), P + (-P)
// is infinity, infinity is neutral (XYZZ::add).
VM_FN void combine(Partial* a, const Partial* b) {
  f12_mul(&a->f, &a->f, &b->f);
  a->c.add(b->c);
}
// One level of the tree over FOLD slots: lane < stride takes slot lane + stride into its own.  The caller runs stride =
// FOLD / 2 .. 1 with a barrier (device) or a loop over the lanes (host) between the steps; the order is fixed, and
// since the arithmetic is exact the folded value depends on the inputs alone.
RLN_HD void fold_step(Partial* slots, uint32_t lane, uint32_t stride) {
  if (lane < stride) combine(&slots[lane], &slots[lane + stride]);
}
// column j of `count` rows of n1 Fr sums
RLN_HD Fr sum_column(const Fr* rows, uint32_t count, uint32_t n1, uint32_t j) {
  Fr s = Fr::zero();
  for (uint32_t i = 0; i < count; i++) s = s + rows[(size_t)i * n1 + j];
  return s;
}

// ---------------------------------------------------------------- host only (plain functions: no device form)
// What finish_host reads of the key
struct AggKey {
  G1Affine alpha;
  G2Affine beta;
  std::vector<G1Affine> ic;  // gamma_abc_g1
  std::vector<LineCoef> gamma, delta;
};
inline AggKey agg_key(const Zkey& zk) {
  const PreparedVk& pv = prepared(zk);
  return {zk.alpha_g1, zk.beta_g2, zk.gamma_abc_g1, pv.gamma, pv.delta};
}
inline G1XYZZ g1_mul_fr(const G1Affine& p, const Fr& k) {
  uint32_t c[8];
  k.to_canonical(c);
  return scalar_mul(p, c);
}
// The last partial -> the final-exponentiated combined value in pairing.h's form (one() = accept).  sums:
// ic.size() entries
inline Fq12 finish_host(const AggKey& K, const Partial& last, const Fr* sums) {
  G1XYZZ L = g1_mul_fr(K.ic[0], sums[0]);
  for (size_t j = 1; j < K.ic.size(); j++) L.add(g1_mul_fr(K.ic[j], sums[j]));
  const G1Affine nra = g1_mul_fr(K.alpha, sums[0]).to_affine().neg();
  Fq12 dev;  // gt_words' mapping: coefficient i of the device's flat vector is coefficient i of pairing.h's
  for (int i = 0; i < 6; i++) dev.c[i] = last.f.c[i];
  const Fq12 fixed = miller_loop_3(nra, K.beta, L.to_affine().neg(), K.gamma, last.c.to_affine().neg(), K.delta);
  return final_exponentiation(f12_mul(fixed, dev));
}
inline void fq12_words(const Fq12& f, uint8_t out[384]) {   // gt_words' order
  for (int i = 0; i < 6; i++) {
    uint32_t a[8], b[8];
    f.c[i].c0.to_canonical(a);
    f.c[i].c1.to_canonical(b);
    memcpy(out + 64 * i, a, 32);
    memcpy(out + 64 * i + 32, b, 32);
  }
}

// The levels of k_verify_reduce with their lanes in a loop: cur (at least one partial) and its rows of n1 sums are
// folded FOLD to 1 until one partial is left; both vectors are used up.  Shared by the lane and the team form
// (verify_agg_team_math.h).
inline void host_fold_levels(uint32_t n1, std::vector<Partial>* cur_in, std::vector<Fr>* sums_in, Partial* last,
                             std::vector<Fr>* last_sums) {
  std::vector<Partial>& cur = *cur_in;
  std::vector<Fr>& sums = *sums_in;
  while (cur.size() > 1) {
    const size_t groups = (cur.size() + FOLD - 1) / FOLD;
    std::vector<Partial> next(groups);
    std::vector<Fr> next_sums(groups * n1);
    for (size_t g = 0; g < groups; g++) {
      Partial slots[FOLD];
      const uint32_t count = (uint32_t)std::min<size_t>(FOLD, cur.size() - g * FOLD);
      for (uint32_t l = 0; l < FOLD; l++) {
        if (l < count) slots[l] = cur[g * FOLD + l];
        else partial_identity(&slots[l]);
      }
      for (uint32_t stride = FOLD / 2; stride; stride >>= 1)
        for (uint32_t l = 0; l < FOLD; l++) fold_step(slots, l, stride);
      next[g] = slots[0];
      for (uint32_t j = 0; j < n1; j++) next_sums[g * n1 + j] = sum_column(&sums[g * FOLD * n1], count, n1, j);
    }
    cur.swap(next);
    sums.swap(next_sums);
  }
  *last = cur[0];
  last_sums->assign(sums.begin(), sums.begin() + n1);
}
// The kernels of verify_agg.hip with their lanes in a loop: n proofs -> the last partial and its sums (levels of FOLD
// until one partial is left), rejected[i] = 1 where the shared checks refuse proof i.  For the CPU suite.
inline void host_aggregate_lanes(const PreparedKey* vk, size_t n, const uint32_t* proofs, const uint32_t* vals,
                                 const uint32_t* scalars, uint8_t* rejected, Partial* last, std::vector<Fr>* last_sums) {
  const uint32_t n1 = vk->n_values + 1;
  std::vector<Partial> cur(n ? n : 1);
  std::vector<Fr> sums((n ? n : 1) * n1, Fr::zero());
  if (!n) partial_identity(&cur[0]);
  for (size_t i = 0; i < n; i++) {
    PrepAgg pa;
    prepare_agg(vk, proofs + 32 * i, vals + (size_t)8 * vk->n_values * i, scalars + 4 * i, &pa, &cur[i].c, &sums[i * n1]);
    miller_loop_pair(vk, &pa, &cur[i].f);
    rejected[i] = (pa.flags & P_REJECT) ? 1 : 0;
  }
  host_fold_levels(n1, &cur, &sums, last, last_sums);
}

}  // namespace vm
}  // namespace rlnamd
