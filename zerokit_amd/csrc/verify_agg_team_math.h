// The optimistic form of the device verifier (verify_agg_math.h) for a team of 8 lanes per proof: the two stages that
// produce a proof's part of the combined check, written over the exchange policy X of verify_team_math.h so that the
// kernels (verify_agg_team.hip) and a plain g++ build (tests/host/verifyaggteam.cpp, vt::HostX) compile the same
// source.  The records between the stages (vm::PrepAgg, vm::Partial, the rows of Fr sums), the fold and finish_host are
// verify_agg_math.h's, unchanged.
//
// What is left of a team's program: the decompression and subgroup phases it shares with t_prepare
// (t_checked_points), one 128-step ladder run on two lanes at once (r A and r C: one scalar, so one branch pattern), a
// product per public input, and the Miller loop's walk with one line per step.  The per-proof Fq12 may differ from the
// lane form's by factors of proper subfields (the two exact forms' Miller values already do): values are comparable
// after finish_host only.
#pragma once
#include "verify_agg_math.h"
#include "verify_team_math.h"

namespace rlnamd {
namespace vt {

using vm::Partial;
using vm::PrepAgg;

static_assert(PA + 4 <= PREP_AGG_SCRATCH, "scratch places of the optimistic form's first stage");

// vm::prepare_agg by a team.  scalar: 4 little-endian words, not all zero.  A rejected proof contributes the identity
// to every part and sets *rejected = 1; an infinite A or B leaves the pair out (flags without P_VARYING) while r, the
// r x_j and r C still count.  Nothing is stored unless `live`.
template <class X>
VT_FN void t_prepare_agg(X x, const PreparedKey* vk, const uint32_t* proof, const uint32_t* vals,
                         const uint32_t* scalar, PrepAgg* out, G1XYZZ* rc, Fr* sums, uint8_t* rejected, bool live) {
  t_checked_points(x, vk, proof);
  const uint32_t nv = vk->n_values;
  // every input below r: a lane per input, eight at a time
  VT_LANES(x, k) x.w(WVAL + k) = 1;
  for (uint32_t base = 0; base < nv; base += TEAM) {
    VT_LANES(x, k) {
      if (base + k < nv && !val_below_r(vals + 8 * (base + k))) x.w(WVAL + k) = 0;
    }
  }
  x.sync();
  bool ok[X::NL];
  VT_LANES(x, k) {
    bool all = x.w(WOK) && x.w(WOK + 1) && x.w(WOK + 2) && x.w(WSUB);
    for (int j = 0; j < TEAM; j++) all = all && x.w(WVAL + j);
    ok[x.li(k)] = all;
  }
  uint32_t kw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kw[i] = i < 4 ? scalar[i] : 0;
  const Fr r = Fr::from_canonical(kw);
  // r A on lane 0 and r C on lane 1: one program (a rejected proof's points are harmless operands, masked below)
  G1XYZZ acc[X::NL];
  VT_LANES(x, k) {
    if (k < 2) {
      const Fq2 c = x.s(PA + k);
      const G1Affine pt{c.c0, c.c1};
      vm::g1_mul128(&pt, scalar, &acc[x.li(k)]);
    }
  }
  VT_LANES(x, k) {
    const bool good = ok[x.li(k)];
    if (k == 0) {
      const G1Affine ra = acc[x.li(k)].to_affine();
      PrepAgg rec;
      rec.A = good ? ra : G1Affine::inf();
      rec.B = good ? G2Affine{x.s(PBX), x.s(PBY)} : G2Affine::inf();
      rec.flags = good ? ((rec.A.is_inf() || rec.B.is_inf()) ? 0 : vm::P_VARYING) : vm::P_REJECT;
      if (live) {
        *out = rec;
        *rejected = good ? 0 : 1;
      }
    } else if (k == 1) {
      if (live) *rc = good ? acc[x.li(k)] : G1XYZZ::inf();
    } else if (k == 2) {
      if (live) sums[0] = good ? r : Fr::zero();
    }
  }
  // the r x_j: a lane per public input, eight at a time
  for (uint32_t base = 0; base < nv; base += TEAM) {
    VT_LANES(x, k) {
      const bool active = base + k < nv;
      const uint32_t j = active ? base + k : 0;
      uint32_t xw[8];
#pragma unroll
      for (int i = 0; i < 8; i++) xw[i] = vals[8 * j + i];
      const Fr s = Fr::from_canonical(xw) * r;
      if (live && active) sums[1 + j] = ok[x.li(k)] ? s : Fr::zero();
    }
  }
  x.sync();
}

// vm::miller_loop_pair by a team: t_miller_loop's walk of the running point with the lines of gamma and delta left out
// of the program, not multiplied by alpha_beta.  The value is left in slot 0.
template <class X>
VT_FN void t_miller_loop_pair(X x, const PreparedKey* vk, const PrepAgg* p) {
  t_miller_walk<false>(x, vk, p);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The two kernels of verify_agg_team.hip, one after the other, with their teams run as waves of eight (clamped index,
// masked store): part, sums (rows of n_values + 1) and rejected get entries [0, n).  n > 0.  mem:
// team_units(MILLER_SLOTS, MILLER_SCRATCH) Fq2.
inline void host_partials_teams(const PreparedKey* vk, size_t n, const uint32_t* proofs, const uint32_t* vals,
                                const uint32_t* scalars, Partial* part, Fr* sums, uint8_t* rejected, Fq2* mem) {
  const uint32_t n1 = vk->n_values + 1;
  const uint32_t waves = (uint32_t)((n + TEAMS_PER_WAVE - 1) / TEAMS_PER_WAVE);
  std::vector<PrepAgg> prep(n);
  for (uint32_t wv = 0; wv < waves; wv++)
    for (uint32_t t = 0; t < (uint32_t)TEAMS_PER_WAVE; t++) {
      const TeamIndex ti = team_index(wv, t, (uint32_t)n);
      t_prepare_agg(HostX{mem, PREP_SLOTS}, vk, proofs + (size_t)32 * ti.i, vals + (size_t)8 * vk->n_values * ti.i,
                    scalars + (size_t)4 * ti.i, &prep[ti.i], &part[ti.i].c, sums + (size_t)n1 * ti.i, &rejected[ti.i],
                    ti.live);
    }
  for (uint32_t wv = 0; wv < waves; wv++)
    for (uint32_t t = 0; t < (uint32_t)TEAMS_PER_WAVE; t++) {
      const TeamIndex ti = team_index(wv, t, (uint32_t)n);
      const HostX xm{mem, PAIR_SLOTS};
      t_miller_loop_pair(xm, vk, &prep[ti.i]);
      if (ti.live)
        for (int k = 0; k < 6; k++) part[ti.i].f.c[k] = xm.f(0, k);
    }
}
// host_aggregate_lanes in team form: the partials above, then the same fold levels
inline void host_aggregate_teams(const PreparedKey* vk, size_t n, const uint32_t* proofs, const uint32_t* vals,
                                 const uint32_t* scalars, uint8_t* rejected, Partial* last, std::vector<Fr>* last_sums) {
  const uint32_t n1 = vk->n_values + 1;
  std::vector<Partial> cur(n ? n : 1);
  std::vector<Fr> sums((n ? n : 1) * n1, Fr::zero());
  if (!n) vm::partial_identity(&cur[0]);
  std::vector<Fq2> mem(team_units(MILLER_SLOTS, MILLER_SCRATCH));
  if (n) host_partials_teams(vk, n, proofs, vals, scalars, cur.data(), sums.data(), rejected, mem.data());
  vm::host_fold_levels(n1, &cur, &sums, last, last_sums);
}
#endif

}  // namespace vt
}  // namespace rlnamd
