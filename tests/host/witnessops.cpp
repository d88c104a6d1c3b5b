// CPU build of zerokit_amd/csrc/witness_ops.h behind the layout of rlnamd_probe_witness_op (tests/test_field_ops_host.py):
// the same operand table that tests/test_gpu_field_ops.py sends to the device, so that a failure of the device alone can
// be told from an error in the operations' logic.
#include <stddef.h>
#include <stdint.h>

#include "witness_ops.h"

using namespace rlnamd;

extern "C" {

// in: n x 17 words (opcode, a, b: Fr in the 8 x 32 Montgomery form), out: n x 9 (value, error word)
void wo_probe(size_t n, const uint32_t* in, uint32_t* out) {
  for (size_t t = 0; t < n; t++) {
    const uint32_t* s = in + t * 17;
    Fr a, b, r;
    for (int j = 0; j < 8; j++) {
      a.v[j] = s[1 + j];
      b.v[j] = s[9 + j];
    }
    uint32_t err = WERR_NONE;
    const uint32_t op = s[0];
    if (op == G_MUL) r = a * b;          // the interpreters' fast path, as in the device probe
    else if (op == G_ADD) r = a + b;
    else if (op == G_SUB) r = a - b;
    else r = witness_slow_op(op, a, b, &err);
    for (int j = 0; j < 8; j++) out[t * 9 + j] = r.v[j];
    out[t * 9 + 8] = err;
  }
}

}  // extern "C"
