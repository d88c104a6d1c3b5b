// Test support (include/rln_amd.h: rlnamd_probe_*): single device functions of field.h, fq29.h, poseidon.h and
// witness_ops.h run on operand tuples the caller supplies, one lane per tuple, results copied back raw.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rlnamd {

// in: n x in_words, out: n x out_words (host memory); in_words / out_words must be the operation's own counts
void probe_field(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
void probe_f29(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
// in: n x 17 (op, a[8], b[8]), out: n x 9 (value[8], error word)
void probe_witness_op(size_t n, const uint32_t* in, uint32_t* out);

}  // namespace rlnamd
