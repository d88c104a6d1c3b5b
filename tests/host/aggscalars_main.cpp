// Stand-alone run of zerokit_amd/csrc/verify_agg_scalars.h for the sanitizers (g++ -fsanitize=address,undefined; never
// loaded into python): aggscalars_main <seed: 64 hex digits> <chunk> <n>...  For every n the scalars go into a heap
// buffer of exactly 16 n bytes, so that a store past a partial last group is an error the sanitizer reports; the
// program checks that no scalar is zero and that the n scalars are the first n of the next multiple of 8, and prints
// them as one line of hex per n.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "verify_agg_scalars.h"

int main(int argc, char** argv) {
  if (argc < 4 || strlen(argv[1]) != 64) return 2;
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) {
    unsigned v = 0;
    if (sscanf(argv[1] + 2 * i, "%2x", &v) != 1) return 2;
    seed[i] = (uint8_t)v;
  }
  const uint64_t chunk = strtoull(argv[2], nullptr, 10);
  int failures = 0;
  for (int a = 3; a < argc; a++) {
    const size_t n = (size_t)strtoull(argv[a], nullptr, 10), whole = (n + 7) / 8 * 8;
    uint8_t* exact = (uint8_t*)malloc(16 * n ? 16 * n : 1);
    std::vector<uint8_t> full(16 * whole);
    rlnamd::aggsc::scalars_host(seed, chunk, n, exact);
    rlnamd::aggsc::scalars_host(seed, chunk, whole, full.data());
    if (n && memcmp(exact, full.data(), 16 * n) != 0) failures++;
    static const uint8_t zero[16] = {0};
    for (size_t i = 0; i < n; i++) failures += memcmp(exact + 16 * i, zero, 16) == 0;
    for (size_t i = 0; i < 16 * n; i++) printf("%02x", exact[i]);
    printf("\n");
    free(exact);
  }
  fprintf(stderr, "%d sizes, %d failures\n", argc - 3, failures);
  return failures ? 1 : 0;
}
