// prover_desc.h -- the plain descriptors and constants that the prover's host planning (prover_plan.h) and its kernels
// (prover_kernels.h, walk29.h) share.  No HIP here: the planning unit and its CPU tests compile with a plain C++ compiler.
#pragma once
#include <stdint.h>

namespace rlnamd {

// ---- witness interpreters (prover_front.hip)
constexpr uint32_t OPK_RING = 0u << 30, OPK_CONST = 1u << 30, OPK_FAR = 2u << 30, OPK_MASK = 3u << 30;
constexpr uint32_t W29_STORE = 1u << 8, W29_RED = 1u << 9, W29_RARE = 1u << 10;  // flags in descriptor word 0
constexpr uint32_t W29_FMA = 25;             // program-only operation: a * b + c (an Add fused with its single-use product)
constexpr uint32_t WIT29_RING = 32;          // node values kept in LDS: 32 x 64 x 48 B = 96 KiB
constexpr uint32_t WIT29_LDS_CONSTS = 1024;  // constants kept in LDS: 48 KiB
constexpr uint32_t WIT29_CH = 256;           // descriptors per program chunk: 64 lanes x 64 B; two chunks in LDS (8 KiB)
constexpr uint32_t WIT29_LDS_BYTES = WIT29_RING * 64 * 48 + WIT29_LDS_CONSTS * 48 + 2 * WIT29_CH * 16;
constexpr double WIT29_BMAX = 7.5;
struct GNode29 {
  uint32_t w0;       // op | flags | slot << 16 (slot: index into the compact array of stored values)
  uint32_t a, b, c;  // operands as in GNode: OPK_RING | node, OPK_CONST | index, OPK_FAR | slot
};

constexpr uint32_t MV_LONG = 8;   // mat-vec: rows with more entries in A or B get a wave each (k_matvec)
constexpr uint32_t SUM_TREE_LANES = 512;
constexpr int NTT_MAX_K = 3;      // levels of one k_ntt_pass: eight points per lane (a 16-point block spills; measured 6.7 -> 5.0 ms)
struct InputSlots {
  uint32_t secret, limit, msg_id, path, path_idx, x, ext, depth;
};

// Window schedule of the comb tables.  Window j covers cw[j] scalar bits starting at bit bo[j]; its table row holds
// the 2^(cw[j]-1) multiples d 2^bo[j] P (signed digits) at entry offset ro[j] inside the point's block of `stride`
// entries.  Uniform widths (c, c, ...) are the classical comb; with 288 GB of HBM the first `wide` windows take one
// more bit so that W drops from 20 to 19 at c = 13 (8 x 14 + 11 x 13 = 255 bits, table x 1.35).  Passed by value:
// the kernels index it with wave-uniform j (scalar loads from the kernarg segment).
struct WinSched {
  int W;
  uint32_t stride;
  uint8_t cw[32];
  uint16_t bo[32];
  uint32_t ro[32];
};

struct ChunkDesc {
  uint32_t pt_begin, pt_end;  // compact point range
};

// A row word (the `rows` lists of the walk plans) = table point index | flags.
//   ROW_HALF2   bit 31: the second GLV half of the scalar (k2; the sum goes through phi afterwards)
//   ROW_PAIRED  bit 30: the point is a member of a PAIR (two points whose rows are walked under the SAME scalar: A_i and
//               B1_i, or one of them and L_i).  The two members sit at consecutive point indices 2 q, 2 q + 1 and their
//               tables are interleaved entry by entry: entry x of member m at ((2 q) stride + 2 x + m) -- the two entries a
//               digit selects share one 128-byte line.  Any walk may read a paired point by itself (a strided row); the
//               pair chunks of the throughput plan read both with a lane pair and halve the HBM requests of those rows.
constexpr uint32_t ROW_HALF2 = 1u << 31, ROW_PAIRED = 1u << 30, ROW_INDEX = ROW_PAIRED - 1;

// Output segments of the G1 walk.  Every family of rows has A, B1 and Cpart; the shared family of the throughput plan
// (prover_plan.h: G1Rows::shared) has two more: the A rows of the wires whose B1 row is the same point (SEG_SHARED_EQ) or
// its negative (SEG_SHARED_OPP).  k_shared_join, behind the fold, adds their sums to A and B1.
constexpr uint32_t G1_SEGS = 3, G1_SHARED_SEGS = 5, SEG_SHARED_EQ = 3, SEG_SHARED_OPP = 4;

}  // namespace rlnamd
