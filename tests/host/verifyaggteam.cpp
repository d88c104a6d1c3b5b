// CPU build of the optimistic verifier's team form (zerokit_amd/csrc/verify_agg_team_math.h: eight lanes per proof, run
// one after the other over an array in place of LDS) next to what it must reproduce: the plain product over pairing.h
// (vah_twin) and the lane form (vah_aggregate), both from tests/host/verifyagg.cpp, which this file includes.  Behind a
// tiny C interface for tests/test_verify_agg_team_host.py, and linked into tests/host/verifyaggteam_main.cpp for the
// sanitizer run.  Test infrastructure only: nothing in the product links this.  Built with g++ against the HIP headers
// (host declarations only; no HIP call is reached).
#include "verifyagg.cpp"

#include "verify_agg_team_math.h"

static void st_fq(const Fq& x, uint8_t* out) {
  uint32_t c[8];
  x.to_canonical(c);
  memcpy(out, c, 32);
}
struct Words {
  std::vector<uint32_t> pw, vw, sw;
  Words(size_t n, size_t nv, const uint8_t* proofs, const uint8_t* vals, const uint8_t* scalars)
      : pw(32 * n + 1), vw(8 * nv * n + 1), sw(4 * n + 1) {
    memcpy(pw.data(), proofs, 128 * n);
    memcpy(vw.data(), vals, 32 * nv * n);
    memcpy(sw.data(), scalars, 16 * n);
  }
};

extern "C" {
// The last partial of either form (team != 0: host_aggregate_teams, else host_aggregate_lanes) and what finish_host
// makes of it.  gt384 in gt_words order; c65: the G1 sum in affine form, x | y canonical and a byte that is 1 at
// infinity; sums: (n_values + 1) x 32 canonical bytes; rejected: n bytes.  0 ok, -1 error
int vat_last(int team, size_t n, const uint8_t* proofs, const uint8_t* vals, const uint8_t* scalars, uint8_t* gt384,
             uint8_t* c65, uint8_t* sums32, uint8_t* rejected) {
  if (!g_have) return -1;
  const size_t nv = g_key.n_values;
  Words w(n, nv, proofs, vals, scalars);
  vm::Partial last;
  std::vector<Fr> sums;
  if (team)
    vt::host_aggregate_teams(&g_key, n, w.pw.data(), w.vw.data(), w.sw.data(), rejected, &last, &sums);
  else
    vm::host_aggregate_lanes(&g_key, n, w.pw.data(), w.vw.data(), w.sw.data(), rejected, &last, &sums);
  vm::fq12_words(vm::finish_host(g_agg, last, sums.data()), gt384);
  if (c65) {
    const G1Affine c = last.c.to_affine();
    st_fq(c.x, c65);
    st_fq(c.y, c65 + 32);
    c65[64] = c.is_inf() ? 1 : 0;
  }
  for (size_t j = 0; sums32 && j <= nv; j++) {
    uint32_t c[8];
    sums[j].to_canonical(c);
    memcpy(sums32 + 32 * j, c, 32);
  }
  return 0;
}
// The waves driver over arrays of n + extra entries filled with the byte 0xA5: 0 when every entry of rows [0, n) of the
// partials (f and c), the sums and the reject flags was written and no byte beyond row n - 1 changed; otherwise a mask:
// 1 an f unwritten, 2 a c unwritten, 4 a sum unwritten, 8 a flag unwritten, 16 a byte past the end changed; -1 error
int vat_waves_bounds(size_t n, size_t extra, const uint8_t* proofs, const uint8_t* vals, const uint8_t* scalars) {
  if (!g_have || !n) return -1;
  const size_t nv = g_key.n_values, n1 = nv + 1, cap = n + extra;
  Words w(n, nv, proofs, vals, scalars);
  std::vector<vm::Partial> part(cap);
  std::vector<Fr> sums(cap * n1);
  std::vector<uint8_t> rej(cap, 0xA5);
  memset((void*)part.data(), 0xA5, cap * sizeof(vm::Partial));
  memset((void*)sums.data(), 0xA5, cap * n1 * sizeof(Fr));
  std::vector<Fq2> mem(vt::team_units(vt::MILLER_SLOTS, vt::MILLER_SCRATCH));
  vt::host_partials_teams(&g_key, n, w.pw.data(), w.vw.data(), w.sw.data(), part.data(), sums.data(), rej.data(),
                          mem.data());
  uint8_t mark[sizeof(vm::Partial)];
  memset(mark, 0xA5, sizeof(mark));
  int bad = 0;
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 6; k++)
      if (!memcmp(&part[i].f.c[k], mark, sizeof(Fq2))) bad |= 1;
    if (!memcmp(&part[i].c, mark, sizeof(G1XYZZ))) bad |= 2;
    for (size_t j = 0; j < n1; j++)
      if (!memcmp(&sums[i * n1 + j], mark, sizeof(Fr))) bad |= 4;
    if (rej[i] > 1) bad |= 8;
  }
  for (size_t i = n; i < cap; i++) {
    if (memcmp(&part[i], mark, sizeof(vm::Partial))) bad |= 16;
    for (size_t j = 0; j < n1; j++)
      if (memcmp(&sums[i * n1 + j], mark, sizeof(Fr))) bad |= 16;
    if (rej[i] != 0xA5) bad |= 16;
  }
  return bad;
}
// The exact team form, whose t_prepare now shares t_checked_points with the optimistic one.  proof: 128 bytes, pub:
// n_values x 32.  1 accept, 0 reject, -1 error; gt384: the final-exponentiated pairing product, zero when the proof is
// rejected before the pairing
int vat_team_verify(const uint8_t* proof, const uint8_t* pub, uint8_t* gt384) {
  if (!g_have) return -1;
  const size_t nv = g_key.n_values;
  uint32_t pw[32], gt[96];
  std::vector<uint32_t> vw(8 * nv + 1);
  memcpy(pw, proof, 128);
  memcpy(vw.data(), pub, 32 * nv);
  std::vector<Fq2> mem(vt::team_units(vt::FINAL_SLOTS, vt::PREP_SCRATCH));
  uint8_t ok = 2;
  vt::host_verify_team(&g_key, pw, vw.data(), true, mem.data(), &ok, gt);
  memcpy(gt384, gt, 384);
  return ok;
}
// the host verifier (capi.cpp: verify_common) with the same outputs
int vat_host_verify(const uint8_t* proof, const uint8_t* pub, uint8_t* gt384) {
  if (!g_have) return -1;
  const size_t nv = g_key.n_values;
  memset(gt384, 0, 384);
  try {
    G1Affine A, C;
    G2Affine B;
    if (!g1_decompress(proof, &A) || !g2_decompress(proof + 32, &B) || !g1_decompress(proof + 96, &C) ||
        !g2_in_subgroup(B))
      return 0;
    std::vector<Fr> x(nv);
    for (size_t i = 0; i < nv; i++) {
      uint32_t c[8];
      memcpy(c, pub + 32 * i, 32);
      if (limbs_geq(c, FrParams::MOD)) return 0;
      x[i] = Fr::from_canonical(c);
    }
    const PreparedVk& pv = prepared(g_zk);
    const G1Affine ic = ic_combination(g_zk, pv, x).to_affine();
    const Fq12 f = miller_loop_3(A, B, ic.neg(), pv.gamma, C.neg(), pv.delta);
    vm::fq12_words(final_exponentiation(f12_mul(f, pv.alpha_beta)), gt384);
    return groth16_verify(g_zk, A, B, C, x) ? 1 : 0;
  } catch (const std::exception&) {
    return -1;
  }
}
}
