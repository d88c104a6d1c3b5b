// Index arithmetic of one Merkle path step, shared by the device gather (merkle.hip: k_proofs_at) and the host.
// No HIP call in here: a plain C++ compiler builds it for the CPU test (tests/host/merklepaths.cpp).
//
// Heap layout of FullMerkleTree (utils/src/merkle_tree/full_merkle_tree.rs:20-40): node i has children 2i + 1 and
// 2i + 2, leaf `idx` of a tree of depth d sits at 2^d - 1 + idx.  A proof (:288-304) walks from the leaf to the root:
// at level l (0 = the leaf's own level) it records the sibling of the leaf's ancestor and 1 when that ancestor is a
// right child (an even heap index), else 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLN_PATHS_HD __host__ __device__
#else
#define RLN_PATHS_HD
#endif

namespace rlnamd {

struct PathStep {
  uint64_t ancestor;   // 0-based heap index of the leaf's ancestor at this level
  uint64_t sibling;    // 0-based heap index of that ancestor's sibling: the path element
  uint32_t bit;        // 1: the ancestor is a right child
};

// depth in [1, 63), leaf < 2^depth, level in [0, depth)
RLN_PATHS_HD inline PathStep merkle_path_step(uint32_t depth, uint64_t leaf, uint32_t level) {
  const uint64_t a1 = ((((uint64_t)1) << depth) + leaf) >> level;   // 1-based: the sibling is a1 ^ 1, odd == right child
  PathStep s;
  s.ancestor = a1 - 1;
  s.sibling = (a1 ^ 1) - 1;
  s.bit = (uint32_t)(a1 & 1);
  return s;
}

// Where a gather writes: path element l of proof i goes to elem_base + i * proof_stride + l * elem_stride (32 bytes,
// 16-byte aligned) and its bit to bit_base + i * bit_proof_stride + l * bit_stride -- as one byte (bit_as_field = 0) or as
// the field element 0 / 1, 32 bytes little-endian (bit_as_field = 1, 16-byte aligned).  Strides in bytes.
//   packed:  [k][depth][32] + [k][depth]        : proof_stride = depth * 32, elem_stride = 32, bit strides depth and 1
//   staged:  a prover's inputs [p][inputs_size][32]: both bases inside the inputs, proof strides inputs_size * 32,
//            level strides 32, bit_as_field = 1
struct PathDest {
  uint8_t* elem_base;
  uint8_t* bit_base;
  uint64_t proof_stride, elem_stride, bit_proof_stride, bit_stride;
  uint32_t bit_as_field;
};

// byte offsets from the two bases (64-bit: proof 2^27 of a packed depth-30 buffer lies past 2^32)
RLN_PATHS_HD inline uint64_t path_elem_offset(const PathDest& d, uint64_t i, uint64_t level) {
  return i * d.proof_stride + level * d.elem_stride;
}
RLN_PATHS_HD inline uint64_t path_bit_offset(const PathDest& d, uint64_t i, uint64_t level) {
  return i * d.bit_proof_stride + level * d.bit_stride;
}

}  // namespace rlnamd
