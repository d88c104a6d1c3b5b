// CPU build of the team form of the device verifier (zerokit_amd/csrc/verify_team_math.h: eight lanes per proof, here
// run one after the other over an array in place of LDS) next to the host verifier it must agree with (zkey.cpp +
// pairing.h), behind a tiny C interface for tests/test_verify_team_host.py.  Test infrastructure only: nothing in the
// product links this.  Built with g++ against the HIP headers (host declarations only; no HIP call is reached).  Field
// elements cross the interface as 32-byte canonical little-endian values, an Fq12 as 12 of them in pairing.h's
// coefficient order (c[0].c0, c[0].c1, c[1].c0, ...).
#include <string.h>

#include <vector>

#include "../../zerokit_amd/csrc/zkey.cpp"
#include "verify_key.h"
#include "verify_team_math.h"
using namespace rlnamd;

static Zkey g_zk;
static vm::PreparedKey g_key;
static std::vector<G1Affine> g_ic;
static bool g_have = false;
static Fq2 g_mem[vt::team_units(vt::FINAL_SLOTS, vt::PREP_SCRATCH)];

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
template <class X>
static void ld_slot(const X& x, int slot, const uint8_t* in) {
  for (int i = 0; i < 6; i++) x.f(slot, i) = {ld_fq(in + 64 * i), ld_fq(in + 64 * i + 32)};
}
template <class X>
static void st_slot(const X& x, int slot, uint8_t* out) {
  for (int i = 0; i < 6; i++) {
    st_fq(x.f(slot, i).c0, out + 64 * i);
    st_fq(x.f(slot, i).c1, out + 64 * i + 32);
  }
}
static void st_host_f12(const Fq12& f, uint8_t* out) {
  for (int i = 0; i < 6; i++) {
    st_fq(f.c[i].c0, out + 64 * i);
    st_fq(f.c[i].c1, out + 64 * i + 32);
  }
}

extern "C" {
int vth_load_zkey(const uint8_t* data, size_t len) {
  try {
    g_zk = parse_arkzkey(data, len);
    vm::prepare_key(g_zk, &g_key, &g_ic);
    g_have = true;
    return 0;
  } catch (const std::exception&) {
    return 1;
  }
}
size_t vth_n_values() { return g_have ? g_key.n_values : 0; }

// op: 0 a*b, 1 a^2, 2 1/a, 3 a^q, 4 a^(q^2), 5 cyclotomic square, 6 final exponentiation, 7 a^u (cyclotomic a),
// 8 conjugate.  in_place != 0: the destination is the slot of a (every team operation allows it)
int vth_f12_op(int op, const uint8_t* a384, const uint8_t* b384, int in_place, uint8_t* out384) {
  if (!g_have) return -1;
  const vt::HostX x{g_mem, vt::FINAL_SLOTS};
  const int A = op == 6 ? 0 : 3, B = 4, D = (in_place || op == 6) ? A : 5;
  ld_slot(x, A, a384);
  ld_slot(x, B, b384 ? b384 : a384);
  switch (op) {
    case 0: vt::t_mul(x, D, A, B); break;
    case 1: vt::t_sqr(x, D, A); break;
    case 2: vt::t_inv(x, D, A); break;
    case 3: vt::t_frob(x, &g_key, D, A); break;
    case 4: vt::t_frob2(x, &g_key, D, A); break;
    case 5: vt::t_cyclotomic_sqr(x, D, A); break;
    case 6: vt::t_final_exponentiation(x, &g_key); break;
    case 7:
      if (in_place) return -1;
      vt::t_pow_u(x, D, A);
      break;
    case 8: vt::t_conj(x, D, A); break;
    default: return -1;
  }
  st_slot(x, D, out384);
  return 0;
}
// a (l0 + l1 w + l3 w^3): line192 = l0 | l1 | l3, each an Fq2 of 64 bytes
int vth_line_op(const uint8_t* a384, const uint8_t* line192, uint8_t* out384) {
  if (!g_have) return -1;
  const vt::HostX x{g_mem, vt::MILLER_SLOTS};
  ld_slot(x, 0, a384);
  for (int i = 0; i < 3; i++) x.s(vt::SA0 + i) = {ld_fq(line192 + 64 * i), ld_fq(line192 + 64 * i + 32)};
  vt::t_mul_line(x, 0, 0, vt::SA0, vt::SA1, vt::SA3);
  st_slot(x, 0, out384);
  return 0;
}
// proof: 128 bytes compressed; pub: n canonical 32-byte LE values.  1 accept, 0 reject, -1 error.  gt384 (optional):
// the final-exponentiated pairing product, zero when the proof is rejected before the pairing
int vth_verify(const uint8_t* proof, const uint8_t* pub, size_t n, uint8_t* gt384) {
  if (!g_have || n != g_key.n_values) return -1;
  uint32_t pw[32], gt[96];
  std::vector<uint32_t> vals(8 * n + 1);
  memcpy(pw, proof, 128);
  memcpy(vals.data(), pub, 32 * n);
  uint8_t ok = 2;
  vt::host_verify_team(&g_key, pw, vals.data(), true, g_mem, &ok, gt384 ? gt : nullptr);
  if (gt384) memcpy(gt384, gt, 384);
  return ok;
}
// n proofs as waves of eight teams (clamped index, masked store); ok: n bytes, gt: n x 384 bytes, each may be null
int vth_verify_waves(size_t n, const uint8_t* proofs, const uint8_t* pub, size_t n_values, uint8_t* ok, uint8_t* gt384) {
  if (!g_have || n_values != g_key.n_values) return -1;
  if (n == 0) return 0;
  std::vector<uint32_t> pw(32 * n), vals(8 * n_values * n + 1), gt(gt384 ? 96 * n : 0);
  memcpy(pw.data(), proofs, 128 * n);
  memcpy(vals.data(), pub, 32 * n_values * n);
  vt::host_verify_waves(&g_key, n, pw.data(), vals.data(), ok, gt384 ? gt.data() : nullptr, g_mem);
  if (gt384) memcpy(gt384, gt.data(), 384 * n);
  return 0;
}
// the host verifier (capi.cpp: verify_common) with the same outputs
int vth_host_verify(const uint8_t* proof, const uint8_t* pub, size_t n, uint8_t* gt384) {
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
