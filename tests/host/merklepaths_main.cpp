// Stand-alone program over zerokit_amd/csrc/merkle_paths.h for a sanitizer build (-fsanitize=address,undefined): every
// level of the first, the last and a few thousand pseudo-random leaves at depths 1 .. 62, checked against the parent /
// child relations of the heap layout.  Prints "ok <steps>" and exits 0, or names the first step that is wrong.
#include <stdint.h>
#include <stdio.h>

#include "merkle_paths.h"

int main() {
  uint64_t st = 0x9E3779B97F4A7C15ull, steps = 0;
  for (uint32_t depth = 1; depth <= 62; depth++) {
    const uint64_t cap = (uint64_t)1 << depth;
    for (int k = 0; k < 2048; k++) {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t leaf = k == 0 ? 0 : k == 1 ? cap - 1 : (st >> 1) % cap;
      uint64_t node = cap - 1 + leaf;
      for (uint32_t l = 0; l < depth; l++, steps++) {
        const rlnamd::PathStep s = rlnamd::merkle_path_step(depth, leaf, l);
        const uint64_t parent = (node - 1) / 2;
        const bool right = node == 2 * parent + 2;
        const uint64_t sib = right ? node - 1 : node + 1;
        if (s.ancestor != node || s.sibling != sib || s.bit != (right ? 1u : 0u)) {
          printf("wrong step: depth %u leaf %llu level %u\n", depth, (unsigned long long)leaf, l);
          return 1;
        }
        node = parent;
      }
      if (node != 0) return 2;
    }
  }
  const rlnamd::PathDest d{nullptr, nullptr, 30 * 32, 32, 30, 1, 0};
  if (rlnamd::path_elem_offset(d, (uint64_t)1 << 27, 29) != (((uint64_t)1 << 27) * 30 + 29) * 32) return 3;
  if (rlnamd::path_bit_offset(d, (uint64_t)1 << 27, 29) != ((uint64_t)1 << 27) * 30 + 29) return 3;
  printf("ok %llu\n", (unsigned long long)steps);
  return 0;
}
