// Stand-alone program over tests/host/sharedrows.cpp for the sanitizer build of tests/test_shared_rows_host.py
// (-fsanitize=address,undefined): sharedrows_main <arkzkey> <graph.bin> <wires file> <seed>.  The wires file, written by the
// test from its own reading of the key: 2 x uint32 (wires of E+, wires of E-), then the two lists as uint32.
// Prints "ok <E+> <E-> <plans> <identities> <checksum>" and exits 0, or says what is wrong.
#include <stdio.h>
#include <stdlib.h>

#include "sharedrows.cpp"

static bool slurp(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out->insert(out->end(), buf, buf + got);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: sharedrows_main <arkzkey> <graph.bin> <wires file> <seed>\n");
    return 2;
  }
  std::vector<uint8_t> zkey, graph, wires;
  if (!slurp(argv[1], &zkey) || !slurp(argv[2], &graph) || !slurp(argv[3], &wires)) {
    printf("cannot read the input files\n");
    return 2;
  }
  uint32_t head[2] = {0, 0};
  if (wires.size() < sizeof head) {
    printf("the wires file is too short\n");
    return 2;
  }
  memcpy(head, wires.data(), sizeof head);
  if (wires.size() != sizeof head + 4 * ((size_t)head[0] + head[1])) {
    printf("the wires file has the wrong size\n");
    return 2;
  }
  std::vector<uint32_t> eq(head[0]), opp(head[1]);
  if (head[0]) memcpy(eq.data(), wires.data() + sizeof head, 4 * (size_t)head[0]);
  if (head[1]) memcpy(opp.data(), wires.data() + sizeof head + 4 * (size_t)head[0], 4 * (size_t)head[1]);
  char log[8192] = "";
  uint64_t stats[8] = {0}, sum = 0;
  const int failures = sharedrows_check(zkey.data(), zkey.size(), graph.data(), graph.size(), eq.data(), eq.size(), opp.data(), opp.size(),
                                        strtoull(argv[4], nullptr, 10), log, sizeof log, stats);
  if (failures != 0) {
    printf("%d failures\n%s%s\n", failures, log, failures < 0 ? sharedrows_error() : "");
    return 1;
  }
  if (sharedrows_legacy_checksum(zkey.data(), zkey.size(), graph.data(), graph.size(), &sum) != 0) {
    printf("checksum: %s\n", sharedrows_error());
    return 1;
  }
  printf("ok %llu %llu %llu %llu %016llx\n", (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[4],
         (unsigned long long)stats[7], (unsigned long long)sum);
  return 0;
}
