// CPU build of the optimistic verifier's mathematics (zerokit_amd/csrc/verify_agg_math.h), its lanes run in a loop,
// next to the value it must reproduce: prod_i GT_i^(r_i) over the exact per-proof pairing products of pairing.h.  Behind
// a tiny C interface for tests/test_verify_agg_host.py, and linked into tests/host/verifyagg_main.cpp for the
// sanitizer run.  Test infrastructure only: nothing in the product links this.  Built with g++ against the HIP
// headers (host declarations only; no HIP call is reached).
#include <string.h>

#include <vector>

#include "../../zerokit_amd/csrc/zkey.cpp"
#include "verify_agg_math.h"
#include "verify_key.h"
using namespace rlnamd;

static Zkey g_zk;
static vm::PreparedKey g_key;
static vm::AggKey g_agg;
static std::vector<G1Affine> g_ic;
static bool g_have = false;

// vm::prepare as it stood before its reject rules moved into vm::checked_points, kept word for word: the refactored
// one must fill the same Prep
static void prepare_before(const vm::PreparedKey* vk, const uint32_t* proof, const uint32_t* vals, vm::Prep* out) {
  using namespace vm;
  bool ok = g1_decompress(vk, proof, &out->A);
  ok = ok && g2_decompress(vk, proof + 8, &out->B);
  G1Affine C = G1Affine::inf();
  ok = ok && g1_decompress(vk, proof + 24, &C);
  ok = ok && g2_in_subgroup(vk, &out->B);
  for (uint32_t i = 0; ok && i < vk->n_values; i++) {
    bool lt = false, decided = false;
    for (int j = 7; j >= 0; j--) {
      const uint32_t c = vals[8 * i + j], m = FrParams::MOD[j];
      if (!decided && c != m) {
        lt = c < m;
        decided = true;
      }
    }
    ok = lt;
  }
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

extern "C" {
int vah_load_zkey(const uint8_t* data, size_t len) {
  try {
    g_zk = parse_arkzkey(data, len);
    vm::prepare_key(g_zk, &g_key, &g_ic);
    g_agg = vm::agg_key(g_zk);
    g_have = true;
    return 0;
  } catch (const std::exception&) {
    return 1;
  }
}
size_t vah_n_values() { return g_have ? g_key.n_values : 0; }

// The header's path: prepare_agg -> single-pair Miller loop -> fold tree -> finish_host.  proofs n x 128 bytes, vals
// n x n_values x 32, scalars n x 16; gt384 in gt_words order, rejected n bytes.  0 ok, -1 error
int vah_aggregate(size_t n, const uint8_t* proofs, const uint8_t* vals, const uint8_t* scalars, uint8_t* gt384,
                  uint8_t* rejected) {
  if (!g_have) return -1;
  const size_t nv = g_key.n_values;
  std::vector<uint32_t> pw(32 * n + 1), vw(8 * nv * n + 1), sw(4 * n + 1);
  memcpy(pw.data(), proofs, 128 * n);
  memcpy(vw.data(), vals, 32 * nv * n);
  memcpy(sw.data(), scalars, 16 * n);
  vm::Partial last;
  std::vector<Fr> sums;
  vm::host_aggregate_lanes(&g_key, n, pw.data(), vw.data(), sw.data(), rejected, &last, &sums);
  vm::fq12_words(vm::finish_host(g_agg, last, sums.data()), gt384);
  return 0;
}
// The same value from pairing.h alone, one proof after the other
int vah_twin(size_t n, const uint8_t* proofs, const uint8_t* vals, const uint8_t* scalars, uint8_t* gt384,
             uint8_t* rejected) {
  if (!g_have) return -1;
  const size_t nv = g_key.n_values;
  const PreparedVk& pv = prepared(g_zk);
  Fq12 all = Fq12::one();
  for (size_t i = 0; i < n; i++) {
    const uint8_t* proof = proofs + 128 * i;
    G1Affine A, C;
    G2Affine B;
    bool ok = g1_decompress(proof, &A) && g2_decompress(proof + 32, &B) && g1_decompress(proof + 96, &C) &&
              g2_in_subgroup(B);
    std::vector<Fr> x(nv);
    for (size_t j = 0; ok && j < nv; j++) {
      uint32_t c[8];
      memcpy(c, vals + 32 * (nv * i + j), 32);
      ok = !limbs_geq(c, FrParams::MOD);
      if (ok) x[j] = Fr::from_canonical(c);
    }
    rejected[i] = ok ? 0 : 1;
    if (!ok) continue;
    const G1Affine ic = ic_combination(g_zk, pv, x).to_affine();
    const Fq12 g =
        final_exponentiation(f12_mul(miller_loop_3(A, B, ic.neg(), pv.gamma, C.neg(), pv.delta), pv.alpha_beta));
    uint32_t k[4];
    memcpy(k, scalars + 16 * i, 16);
    Fq12 r = Fq12::one();
    for (int b = 127; b >= 0; b--) {
      r = f12_sqr(r);
      if ((k[b >> 5] >> (b & 31)) & 1) r = f12_mul(r, g);
    }
    all = f12_mul(all, r);
  }
  vm::fq12_words(all, gt384);
  return 0;
}
// 1: vm::prepare fills the Prep that the text before the refactor fills, field for field; 0: not; -1 error
int vah_prep_same(const uint8_t* proof, const uint8_t* vals) {
  if (!g_have) return -1;
  uint32_t pw[32];
  std::vector<uint32_t> vw(8 * g_key.n_values + 1);
  memcpy(pw, proof, 128);
  memcpy(vw.data(), vals, 32 * g_key.n_values);
  vm::Prep a, b;
  memset(&a, 0, sizeof(a));
  memset(&b, 0, sizeof(b));
  vm::prepare(&g_key, pw, vw.data(), &a);
  prepare_before(&g_key, pw, vw.data(), &b);
  return memcmp(&a, &b, sizeof(a)) == 0 ? 1 : 0;
}
}
