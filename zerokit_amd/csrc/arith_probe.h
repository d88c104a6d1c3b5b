// Test support (include/rln_amd.h: rlnamd_probe_*): single device functions of field.h, fq29.h, poseidon.h and
// witness_ops.h run on operand tuples the caller supplies, one lane per tuple, results copied back raw.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rlnamd {

// in: n x in_words, out: n x out_words (host memory); in_words / out_words must be the operation's own counts
void probe_field(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
void probe_f29(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
// The quotient's transforms as the prover launches them (prover_kernels.h: launch_quotient_transform): iNTT, coset scaling
// and NTT of vectors x 2^logn x nb canonical values (dense, [vector][index][lane]; out the same), run in the [index][B]
// layout.  lds: the edge / mid / edge kernels (logn 9 .. 18), else the pass list.  Throws before any launch on logn
// outside 1 .. 18, nb outside 1 .. B, vectors outside 1 .. 3.
void probe_quotient_transform(int logn, int lds, uint32_t B, uint32_t nb, uint32_t vectors, const uint32_t* in, uint32_t* out);
// in: n x 17 (op, a[8], b[8]), out: n x 9 (value[8], error word)
void probe_witness_op(size_t n, const uint32_t* in, uint32_t* out);

}  // namespace rlnamd
