// CPU build of the device verifier's mathematics (zerokit_amd/csrc/verify_math.h) next to the host verifier it must
// agree with (zkey.cpp + pairing.h), behind a tiny C interface for tests/test_verify_math_host.py.  Test
// infrastructure only: nothing in the product links this.  Built with g++ against the HIP headers (host declarations
// only; no HIP call is reached).  Field elements cross the interface as 32-byte canonical little-endian values, an
// Fq12 as 12 of them in pairing.h's coefficient order (c[0].c0, c[0].c1, c[1].c0, ...).
#include <string.h>

#include <vector>

#include "../../zerokit_amd/csrc/zkey.cpp"
#include "verify_key.h"
using namespace rlnamd;

static Zkey g_zk;
static vm::PreparedKey g_key;
static std::vector<G1Affine> g_ic;
static bool g_have = false;

static Fq ld_fq(const uint8_t* in) {
  uint32_t c[8];
  memcpy(c, in, 32);
  return Fq::from_canonical(c);
}
static void st_fq(const Fq& x, uint8_t* out) {
  uint32_t c[8];
  x.to_canonical(c);
  memcpy(out, c, 32);
}
static vm::F12 ld_f12(const uint8_t* in) {
  vm::F12 f;
  for (int i = 0; i < 6; i++) f.c[i] = {ld_fq(in + 64 * i), ld_fq(in + 64 * i + 32)};
  return f;
}
static void st_f12(const vm::F12& f, uint8_t* out) {
  for (int i = 0; i < 6; i++) {
    st_fq(f.c[i].c0, out + 64 * i);
    st_fq(f.c[i].c1, out + 64 * i + 32);
  }
}
static void st_host_f12(const Fq12& f, uint8_t* out) {
  for (int i = 0; i < 6; i++) {
    st_fq(f.c[i].c0, out + 64 * i);
    st_fq(f.c[i].c1, out + 64 * i + 32);
  }
}

extern "C" {
int vmh_load_zkey(const uint8_t* data, size_t len) {
  try {
    g_zk = parse_arkzkey(data, len);
    vm::prepare_key(g_zk, &g_key, &g_ic);
    g_have = true;
    return 0;
  } catch (const std::exception&) {
    return 1;
  }
}
size_t vmh_n_values() { return g_have ? g_key.n_values : 0; }

// op: 0 a*b, 1 a^2, 2 1/a, 3 a^q, 4 a^(q^2), 5 cyclotomic square, 6 final exponentiation, 7 a^u (cyclotomic a)
int vmh_f12_op(int op, const uint8_t* a384, const uint8_t* b384, uint8_t* out384) {
  if (!g_have) return -1;
  vm::F12 a = ld_f12(a384), b = ld_f12(b384 ? b384 : a384), r;
  switch (op) {
    case 0: vm::f12_mul(&r, &a, &b); break;
    case 1: vm::f12_sqr(&r, &a); break;
    case 2: vm::f12_inv(&r, &a); break;
    case 3: vm::f12_frob(&g_key, &r, &a); break;
    case 4: vm::f12_frob2(&g_key, &r, &a); break;
    case 5: vm::f12_cyclotomic_sqr(&r, &a); break;
    case 6: vm::final_exponentiation(&g_key, &r, &a); break;
    case 7: vm::f12_pow_u(&r, &a); break;
    default: return -1;
  }
  st_f12(r, out384);
  return 0;
}
// g1: x | y, g2: x.c0 | x.c1 | y.c0 | y.c1 (affine, finite).  out = final_exp(miller(P, Q)) by the projective loop
int vmh_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out384) {
  if (!g_have) return -1;
  vm::Prep p;
  p.A = {ld_fq(g1), ld_fq(g1 + 32)};
  p.B = {{ld_fq(g2), ld_fq(g2 + 32)}, {ld_fq(g2 + 64), ld_fq(g2 + 96)}};
  p.icn = p.cn = G1Affine::inf();
  p.flags = vm::P_VARYING;
  vm::F12 f;
  vm::miller_loop(&g_key, &p, &f);
  vm::final_exponentiation(&g_key, &f, &f);
  st_f12(f, out384);
  return 0;
}
// the same pair through pairing.h: final_exponentiation(miller_loop(P, Q)) with its affine lines
int vmh_host_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out384) {
  G1Affine P{ld_fq(g1), ld_fq(g1 + 32)};
  G2Affine Q{{ld_fq(g2), ld_fq(g2 + 32)}, {ld_fq(g2 + 64), ld_fq(g2 + 96)}};
  st_host_f12(final_exponentiation(miller_loop(P, Q)), out384);
  return 0;
}
// proof: 128 bytes compressed; pub: n canonical 32-byte LE values.  1 accept, 0 reject, -1 error.  gt384 (optional):
// the final-exponentiated pairing product, zero when the proof is rejected before the pairing
int vmh_verify(const uint8_t* proof, const uint8_t* pub, size_t n, uint8_t* gt384) {
  if (!g_have || n != g_key.n_values) return -1;
  uint32_t pw[32], gt[96];
  std::vector<uint32_t> vals(8 * n + 1);
  memcpy(pw, proof, 128);
  memcpy(vals.data(), pub, 32 * n);
  const int v = vm::verify_one(&g_key, pw, vals.data(), gt384 ? gt : nullptr);
  if (gt384) memcpy(gt384, gt, 384);
  return v;
}
// the host verifier (capi.cpp: verify_common) with the same outputs
int vmh_host_verify(const uint8_t* proof, const uint8_t* pub, size_t n, uint8_t* gt384) {
  if (!g_have || n != g_key.n_values) return -1;
  if (gt384) memset(gt384, 0, 384);
  try {
    G1Affine A, C;
    G2Affine B;
    if (!g1_decompress(proof, &A) || !g2_decompress(proof + 32, &B) || !g1_decompress(proof + 96, &C) ||
        !g2_in_subgroup(B))
      return 0;
    std::vector<Fr> x(n);
    for (size_t i = 0; i < n; i++) {
      uint32_t c[8];
      memcpy(c, pub + 32 * i, 32);
      if (limbs_geq(c, FrParams::MOD)) return 0;
      x[i] = Fr::from_canonical(c);
    }
    if (gt384) {
      const PreparedVk& pv = prepared(g_zk);
      G1Affine ic = ic_combination(g_zk, pv, x).to_affine();
      Fq12 f = miller_loop_3(A, B, ic.neg(), pv.gamma, C.neg(), pv.delta);
      st_host_f12(final_exponentiation(f12_mul(f, pv.alpha_beta)), gt384);
    }
    return groth16_verify(g_zk, A, B, C, x) ? 1 : 0;
  } catch (const std::exception&) {
    return -1;
  }
}
}
