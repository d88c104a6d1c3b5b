// Stand-alone program over zerokit_amd/csrc/keccak_batch.h for the sanitizer build of tests/test_keccak_batch_host.py
// (-fsanitize=address,undefined): the cases of kb_selfcheck (tests/host/keccakbatch.cpp) -- ragged calls planned, packed
// into halves of exactly their size and hashed on the host, a half filled exactly, zero-length messages at both ends,
// offsets[0] > 0, the refusals -- every row judged by keccak.h.  Prints "ok <digest of all rows>" and exits 0, or names
// the case that went wrong.
#include "keccakbatch.cpp"

int main() {
  uint64_t digest = 0;
  const int bad = kb_selfcheck(&digest);
  if (bad) {
    printf("case %d went wrong\n", bad);
    return 1;
  }
  printf("ok %016llx\n", (unsigned long long)digest);
  return 0;
}
