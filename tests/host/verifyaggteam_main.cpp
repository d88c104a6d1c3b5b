// Stand-alone run of tests/host/verifyaggteam.cpp for the sanitizers (g++ -fsanitize=address,undefined; never loaded
// into python): verifyaggteam_main <arkzkey> <rows.bin> <n>, rows.bin = k rows of 128 proof bytes + n_values x 32 value
// bytes.  n rows tiled from the file, under scalars 1, 2^128 - 1 and a counter pattern: the team form's path
// (host_aggregate_teams + finish_host) must give the bytes and the reject flags of the plain product over pairing.h.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>

#include "verifyaggteam.cpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<uint8_t> zkey = slurp(argv[1]), rows = slurp(argv[2]);
  const size_t n = (size_t)atoi(argv[3]);
  if (!n || vah_load_zkey(zkey.data(), zkey.size()) != 0) return 2;
  const size_t nv = vah_n_values(), row = 128 + 32 * nv, k = rows.size() / row;
  if (!k || rows.size() != k * row) return 2;
  int failures = 0, runs = 0, ones = 0;
  std::vector<uint8_t> proofs(128 * n), vals(32 * nv * n), scalars(16 * n);
  for (size_t i = 0; i < n; i++) {
    memcpy(&proofs[128 * i], &rows[row * (i % k)], 128);
    memcpy(&vals[32 * nv * i], &rows[row * (i % k) + 128], 32 * nv);
  }
  for (int pattern = 0; pattern < 3; pattern++) {
    for (size_t i = 0; i < n; i++)
      for (int b = 0; b < 16; b++)
        scalars[16 * i + b] = pattern == 0 ? (b == 0) : pattern == 1 ? 0xff : (uint8_t)(37 * i + 11 * b + 1);
    std::vector<uint8_t> ra(n), rb(n);
    uint8_t ga[384], gb[384];
    if (vat_last(1, n, proofs.data(), vals.data(), scalars.data(), ga, nullptr, nullptr, ra.data()) != 0 ||
        vah_twin(n, proofs.data(), vals.data(), scalars.data(), gb, rb.data()) != 0 || memcmp(ga, gb, 384) != 0 ||
        ra != rb) {
      printf("mismatch at n = %zu, pattern %d\n", n, pattern);
      failures++;
    }
    bool one = ga[0] == 1;
    for (int b = 1; b < 384; b++) one = one && ga[b] == 0;
    ones += one ? 1 : 0;
    runs++;
  }
  printf("%d runs, %d failures, %d ones\n", runs, failures, ones);
  return failures ? 1 : 0;
}
