// CPU build of the index arithmetic the device gather shares with the host (zerokit_amd/csrc/merkle_paths.h), for
// tests/test_merkle_paths_host.py.  Built with g++: the header makes no HIP call.
#include <stdint.h>

#include "merkle_paths.h"

extern "C" {

// every level of one leaf's path: ancestor, sibling (0-based heap indices) and bit, `depth` entries each
void mp_path(uint32_t depth, uint64_t leaf, uint64_t* ancestors, uint64_t* siblings, uint32_t* bits) {
  for (uint32_t l = 0; l < depth; l++) {
    const rlnamd::PathStep s = rlnamd::merkle_path_step(depth, leaf, l);
    ancestors[l] = s.ancestor;
    siblings[l] = s.sibling;
    bits[l] = s.bit;
  }
}

// byte offsets (from the bases) at which the gather writes element / bit `level` of proof `i` under a destination's strides
void mp_dest_offsets(uint64_t proof_stride, uint64_t elem_stride, uint64_t bit_proof_stride, uint64_t bit_stride, uint64_t i,
                     uint64_t level, uint64_t out[2]) {
  const rlnamd::PathDest d{nullptr, nullptr, proof_stride, elem_stride, bit_proof_stride, bit_stride, 0};
  out[0] = rlnamd::path_elem_offset(d, i, level);
  out[1] = rlnamd::path_bit_offset(d, i, level);
}

}  // extern "C"
