// The scalars of a combined pairing check (verify_agg.hip) derived from one 32-byte seed per chunk: Keccak-f[1600] as a
// keyed function, one permutation per 8 proofs.  Everything the kernel k_verify_agg_scalars inlines is here, and there
// is no HIP call in here: a plain C++ compiler builds the same source for the host entry rlnamd_verify_agg_scalars and
// for the CPU tests (tests/host/aggscalars_main.cpp).  The byte layout is stated in include/rln_amd.h.
//
// Group g of chunk c covers proofs 8 g .. 8 g + 7 of the chunk.  Its state before the permutation is the one padded
// rate block of the 64-byte message  seed | "RLNAMD-AGG-SCAL1" | c | g  (c and g little-endian 64-bit) under the
// original Keccak pad (0x01 ... 0x80, as hash_to_field's), the capacity zero:
//   words 0-3 seed, 4-5 the domain string, 6 c, 7 g, 8 = 1, 9-15 = 0, 16 = 2^63, 17-24 = 0
// and behind it words 2 j and 2 j + 1 are the scalar of proof 8 g + j, little-endian; a scalar of zero becomes 1.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "keccak_batch.h"

namespace rlnamd {
namespace aggsc {

constexpr uint32_t GROUP = 8;   // proofs per permutation: 128 of the 136 rate bytes
// "RLNAMD-AGG-SCAL1", bytes 0-7 and 8-15 read little-endian
constexpr uint64_t DOMAIN_LO = 0x412D444D414E4C52ULL, DOMAIN_HI = 0x314C4143532D4747ULL;

// seed: the 32 bytes as 4 little-endian words; out: 8 scalars as (low, high) word pairs, none zero
RLN_HD void derive_group(const uint64_t (&seed)[4], uint64_t chunk, uint64_t group, uint64_t (&out)[16]) {
  uint64_t a[25];
#pragma unroll
  for (int k = 0; k < 25; k++) a[k] = 0;
  a[0] = seed[0]; a[1] = seed[1]; a[2] = seed[2]; a[3] = seed[3];
  a[4] = DOMAIN_LO;
  a[5] = DOMAIN_HI;
  a[6] = chunk;
  a[7] = group;
  a[8] = 0x01;                     // the pad's first byte, at byte 64
  a[16] = 0x8000000000000000ULL;   // and its last, at byte 135
  kbatch::permute(a);
#define RLN_AGGSC_OUT(j)                          \
  {                                               \
    uint64_t lo = a[2 * j];                       \
    const uint64_t hi = a[2 * j + 1];             \
    if ((lo | hi) == 0) lo = 1;                   \
    out[2 * j] = lo;                              \
    out[2 * j + 1] = hi;                          \
  }
  RLN_AGGSC_OUT(0) RLN_AGGSC_OUT(1) RLN_AGGSC_OUT(2) RLN_AGGSC_OUT(3)
  RLN_AGGSC_OUT(4) RLN_AGGSC_OUT(5) RLN_AGGSC_OUT(6) RLN_AGGSC_OUT(7)
#undef RLN_AGGSC_OUT
}

// the host's loop over the groups: out16 = n x 16 bytes (a little-endian host, as everywhere in this library)
inline void scalars_host(const uint8_t seed32[32], uint64_t chunk, size_t n, uint8_t* out16) {
  uint64_t seed[4], out[16];
  memcpy(seed, seed32, 32);
  for (size_t g = 0; GROUP * g < n; g++) {
    derive_group(seed, chunk, (uint64_t)g, out);
    const size_t left = n - GROUP * g;
    memcpy(out16 + 16 * GROUP * g, out, 16 * (left < GROUP ? left : GROUP));
  }
}

}  // namespace aggsc
}  // namespace rlnamd
