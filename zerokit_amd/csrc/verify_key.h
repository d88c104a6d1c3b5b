// Host side of verify_math.h: fills a vm::PreparedKey from a parsed zkey with pairing.h's own precomputation (the
// Miller value of (-alpha, beta), the line coefficients of gamma and delta, the d * IC_i rows), so that the device
// verifier and the host verifier read the same constants.
#pragma once
#include <vector>

#include "pairing.h"
#include "verify_math.h"

namespace rlnamd {
namespace vm {

// ic_rows receives the n_values x 15 rows; key->ic_mult points into it (verify.hip re-points it at its device copy)
inline void prepare_key(const Zkey& zk, PreparedKey* key, std::vector<G1Affine>* ic_rows) {
  const PreparedVk& pv = prepared(zk);
  if (pv.gamma.size() != (size_t)N_LINES || pv.delta.size() != (size_t)N_LINES) throw Error("MalformedVerifyingKey");
  PreparedKey& K = *key;
  K.n_values = (uint32_t)(zk.gamma_abc_g1.size() - 1);
  K.pad_[0] = K.pad_[1] = K.pad_[2] = 0;
  uint64_t c = 1;   // (q + 1) / 4
  uint32_t q1[8];
  for (int i = 0; i < 8; i++) {
    const uint64_t s = (uint64_t)FqParams::MOD[i] + c;
    q1[i] = (uint32_t)s;
    c = s >> 32;
  }
  for (int i = 0; i < 8; i++) K.sqrt_exp[i] = (q1[i] >> 2) | (i < 7 ? q1[i + 1] << 30 : 0);
  const uint32_t SIX_U2[8] = {0xe87cfd46u, 0xf83e9682u, 0xeeb859fbu, 0x6f4d8248u, 0, 0, 0, 0};   // zkey.cpp: g2_in_subgroup
  for (int i = 0; i < 8; i++) K.six_u2[i] = SIX_U2[i];
  K.inv2 = Fq::from_u32(2).inv();
  K.three = Fq::from_u32(3);
  K.twist_b = Fq2{Fq::from_u32(9), Fq::one()}.inv().mul_fq(K.three);
  K.twist_3b = K.twist_b.dbl() + K.twist_b;
  const FrobeniusCoeffs& fc = frob_coeffs();
  for (int i = 0; i < 6; i++) {
    K.frob1[i] = fc.g1[i];
    K.frob2[i] = fc.g2[i];
  }
  K.g22 = fq2_from_limbs(FROB_G22);
  K.g23 = fq2_from_limbs(FROB_G23);
  for (int i = 0; i < 6; i++) K.alpha_beta.c[i] = pv.alpha_beta.c[i];
  for (int k = 0; k < N_LINES; k++) {
    K.gamma[k] = {pv.gamma[k].lam, pv.gamma[k].c};
    K.delta[k] = {pv.delta[k].lam, pv.delta[k].c};
  }
  K.ic0 = zk.gamma_abc_g1[0];
  ic_rows->clear();
  for (const auto& row : pv.ic_mult) ic_rows->insert(ic_rows->end(), row.begin(), row.end());
  K.ic_mult = ic_rows->data();
}

}  // namespace vm
}  // namespace rlnamd
