// prover_front.hip -- front end of the prover pipeline: the witness-graph interpreters, the QAP mat-vec, the NTT passes
// and the quotient, the digit recoding.  Declarations: prover_kernels.h; shared descriptors: prover_desc.h; host side: prover.hip, prover_plan.cpp.
//
// The 256-bit multiply is inlined (measured on MI355X: G1 MSM 44.5 -> 41.7 ms, G2 MSM 30.7 -> 22.5 ms per 1024
// proofs against the out-of-line form, which costs call overhead and a VGPR-hungry calling convention);
// -DRLN_NOINLINE_MUL restores the shared 2.5 KB body.
#include "prover_kernels.h"

#include "glv.h"

namespace rlnamd {

// =====================================================================================================
// 1. witness: one lane per proof interprets the straight-line graph (graph.rs:246-272)
// =====================================================================================================
// Node values are in the 9 x 29-bit form of fq29.h.  The device program is built once on the host (Prover::Prover); the
// top two bits of an operand say where its value lives -- RING: produced fewer than WIT29_RING program nodes earlier,
// read from the LDS ring; CONST: index into the constant table; FAR: anything else, read from the compact array of
// stored values in HBM.  One wave per SIMD is all this kernel ever has, so its time is latency, and
// tools/microbench_lonewave.hip shows what a lone wave pays on gfx950: ~12 cycles per LDS instruction issued (a
// 9 x ds_read_b32 operand is a 118-cycle round trip, two of them 225), 25 - 70 cycles per uniform branch hop, ~5.7 cycles
// per dependent multiply-add.  An earlier interpreter with values as 8 x 32 bits spent two thirds of its 1 950 cycles per
// node on exactly that (profiled: an ADD node of 30 instructions took 1 250 - 1 750 cycles).  Hence:
//   * values live in LDS as [slot][lane][12 words]: an operand is ds_read_b128 x 2 + ds_read_b32, conflict-free at
//     the 48-byte lane stride; constants as [id][12 words] are the SAME address form with lane multiplier 0, so both
//     operands of a node are read without a branch and share one round trip;
//   * the descriptor is 16 bytes (one broadcast ds_read_b128, issued one node ahead, made wave-uniform when its turn
//     comes); the program reaches LDS through coalesced vector loads, a chunk ahead (a scalar load in flight would turn
//     every LDS wait into s_waitcnt lgkmcnt(0));
//   * no register forwarding (a node waits for an LDS read anyway; the previous node's value comes back from the ring);
//     the rare sources (a value further back than the ring, a constant beyond the LDS table), the reduction flag and the
//     slow operations hide behind ONE flag test, taken before any operand is read;
//   * a product is ~200 instructions against ~375 in the 8 x 32 form, and the ~6 000 witness signals leave in the limb
//     form ([slot][proof][12 words], three 16-byte stores) for a throughput kernel to convert (k_v29_to_fr).
//
// Value discipline: every node value is normalised (limbs < 2^29) with a STATIC bound, computed on the host when the
// device program is built (Prover::Prover): products < 1 + 0.006 a b (in units of r), sums a + b, differences
// a + 8 (K8 - b, b < 7.9 r), inputs / constants / slow operations ~ 1.  A node whose bound would pass WIT29_BMAX
// carries W29_RED: its value is multiplied by the Montgomery one (result < 1.1 r).  Every operand is therefore below
// 7.5 r, inside what fq29.h's products (check_fq29_bounds.py: N(10)), K8 - b and the exact zero test (k r, k < 8) take.
// LDS byte address of an operand for this lane, without a branch (a uniform branch hop costs a lone wave 25 - 70
// cycles): ring value (id % RING) * 64 * 48 + lane * 48, LDS constant RING * 64 * 48 + id * 48.  Only valid for the
// operands of the fast path (ring or LDS constant); the rare path re-reads what else it needs.
__device__ __forceinline__ uint32_t wit29_addr(uint32_t enc, uint32_t lane48) {
  const uint32_t id = enc & ~OPK_MASK;
  const uint32_t cm = 0u - ((enc >> 30) & 1u);   // all ones for OPK_CONST
  const uint32_t ring_a = (id % WIT29_RING) * (64 * 48), const_a = WIT29_RING * 64 * 48 + id * 48;
  return ((const_a & cm) | (ring_a & ~cm)) + (lane48 & ~cm);
}
__device__ __forceinline__ void wit29_read(Fr29& r, uint32_t addr, const uint32_t* ring) {
  const char* a = (const char*)ring + addr;
  const uint4 x = *(const uint4*)a, y = *(const uint4*)(a + 16);
  r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
  r.v[4] = y.x; r.v[5] = y.y; r.v[6] = y.z; r.v[7] = y.w;
  r.v[8] = *(const uint32_t*)(a + 32);
}
struct Wit29Out {
  Fr29 v;
  uint32_t e;
};
// Everything that is not Mul / Add on ring / LDS-constant / forwarded operands.  Out of line and by value on purpose:
// inlined, its slow operations (calls with stack arguments) made the compiler keep the hot path's operands in scratch.
__device__ __noinline__ Wit29Out wit29_rare(uint32_t w0, uint32_t ea, uint32_t eb, uint32_t ec, const uint32_t* ring,
                                            uint32_t lane,
                                            const uint32_t* __restrict__ consts29, const uint32_t* __restrict__ inputs,
                                            uint32_t n_inputs, const uint4* __restrict__ V29, uint32_t B, uint32_t p) {
  Wit29Out o;
  o.e = WERR_NONE;
  const uint32_t op = w0 & 0xFF;
  auto src = [&](Fr29& r, uint32_t enc) {   // any source, from scratch
    const uint32_t kind = enc >> 30, id = enc & ~OPK_MASK;
    if (kind == (OPK_FAR >> 30)) {
      const uint4* g = V29 + ((size_t)id * B + p) * 3;
      const uint4 x = g[0], y = g[1], z = g[2];
      r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
      r.v[4] = y.x; r.v[5] = y.y; r.v[6] = y.z; r.v[7] = y.w;
      r.v[8] = z.x;
    } else if (kind == (OPK_CONST >> 30) && id >= WIT29_LDS_CONSTS) {
      const uint32_t* c = consts29 + (size_t)id * 9;
#pragma unroll
      for (int k = 0; k < 9; k++) r.v[k] = c[k];
    } else {
      wit29_read(r, wit29_addr(enc, lane * 48), ring);
    }
  };
  Fr29 v, va, vb;
  if (op == G_CONST) {
    src(v, OPK_CONST | ea);
  } else if (op == G_INPUT) {
    const uint32_t* in = inputs + ((size_t)p * n_inputs + ea) * 8;
    if (limbs_geq(in, FrParams::MOD)) o.e = WERR_INPUT_RANGE;  // u256_to_fr fails (graph.rs:42-45)
    Fr x;
#pragma unroll
    for (int k = 0; k < 8; k++) x.v[k] = in[k];
    v = Fr29::mul(Fr29::slice(x), Fr29::from_const(Fr29C::FROM_CANON));
  } else {
    src(va, ea);
    if (op != G_NEG && op != G_ID) src(vb, eb);
    if (op == G_MUL) {
      v = Fr29::mul(va, vb);
    } else if (op == W29_FMA) {
      Fr29 vc;
      src(vc, ec);
      v = Fr29::mul_add(va, vb, vc);
    } else if (op == G_ADD) {
#pragma unroll
      for (int k = 0; k < 9; k++) v.v[k] = va.v[k] + vb.v[k];
      v.normalize();
    } else if (op == G_SUB) {
      v = Fr29::sub(va, Fr29C::K8, vb);
    } else if (op == G_NEG) {
      v = Fr29::neg_lazy(Fr29C::K8, va);
      v.normalize();
    } else if (op == G_ID) {
      (void)witness_slow_op(G_ID, Fr::zero(), Fr::zero(), &o.e);
      v = Fr29::zero();
    } else if (op == G_TERN) {
      Fr29 vc;
      src(vc, ec);
      const bool z = va.is_zero_mod_q();  // graph.rs:214-224
#pragma unroll
      for (int k = 0; k < 9; k++) v.v[k] = z ? vc.v[k] : vb.v[k];
    } else {  // comparisons, shifts, bit operations, division ...: on canonical integers, in the 8 x 32 form
      v = Fr29::from_fq(witness_slow_op(op, va.to_fq(), vb.to_fq(), &o.e));
    }
  }
  if (w0 & W29_RED) v = Fr29::mul(v, Fr29::from_const(Fr29C::ONE));
  o.v = v;
  return o;
}
template <bool PROF>
__global__ void __launch_bounds__(64) k_witness29(const GNode29* __restrict__ nodes, uint32_t n_nodes,
                                                  const uint32_t* __restrict__ consts29, uint32_t n_consts,
                                                  const uint32_t* __restrict__ inputs, uint32_t n_inputs,
                                                  uint4* __restrict__ V29, uint32_t* __restrict__ err, uint32_t B,
                                                  uint32_t nb, unsigned long long* __restrict__ prof) {
  unsigned long long pc[4] = {0, 0, 0, 0}, pn[4] = {0, 0, 0, 0}, pw0 = 0, pc0 = 0;
  if (PROF) { pc0 = clock64(); pw0 = wall_clock64(); }
  // LDS: [WIT29_RING][64][12] node values, [WIT29_LDS_CONSTS][12] constants, [2 WIT29_CH][4] program words
  extern __shared__ __attribute__((aligned(16))) uint32_t ring[];
  __builtin_amdgcn_s_setprio(3);  // few, latency-bound waves: issue ahead of the MSM waves sharing the SIMD
  const uint32_t lane = threadIdx.x, lane48 = lane * 48;
  uint32_t p = blockIdx.x * 64 + lane;
  if (p >= nb) return;
  uint32_t e = WERR_NONE;
  uint32_t* const lconsts = ring + WIT29_RING * 64 * 12;
  uint32_t* const prog = lconsts + WIT29_LDS_CONSTS * 12;
  {
    const uint32_t nc = n_consts < WIT29_LDS_CONSTS ? n_consts : WIT29_LDS_CONSTS;
    for (uint32_t i = lane; i < nc * 9; i += 64) lconsts[(i / 9) * 12 + i % 9] = consts29[i];
  }
  const uint4* const gsrc = (const uint4*)nodes;   // lane l of chunk k: descriptors [k CH + 4 l, + 4)
  uint4 pf[4];
#pragma unroll
  for (int k = 0; k < 4; k++) pf[k] = gsrc[lane * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; k++) ((uint4*)prog)[lane * 4 + k] = pf[k];
#pragma unroll
  for (int k = 0; k < 4; k++) pf[k] = gsrc[(size_t)WIT29_CH + lane * 4 + k];   // chunk 1
  __syncthreads();
  uint4 d_next = ((const uint4*)prog)[0];
  const uint32_t n_chunks = (n_nodes + WIT29_CH - 1) / WIT29_CH;
#pragma unroll 1
  for (uint32_t ch = 0; ch < n_chunks; ch++) {
    {   // chunk ch is in LDS; park chunk + 1, start loading chunk + 2
#pragma unroll
      for (int k = 0; k < 4; k++) ((uint4*)prog)[((ch + 1) & 1) * WIT29_CH + lane * 4 + k] = pf[k];
#pragma unroll
      for (int k = 0; k < 4; k++) pf[k] = gsrc[(size_t)(ch + 2) * WIT29_CH + lane * 4 + k];
    }
    const uint32_t n_end = (ch + 1) * WIT29_CH < n_nodes ? (ch + 1) * WIT29_CH : n_nodes;
#pragma unroll 1
    for (uint32_t n = ch * WIT29_CH; n < n_end; n++) {
      const uint32_t w0 = __builtin_amdgcn_readfirstlane(d_next.x), ea = __builtin_amdgcn_readfirstlane(d_next.y),
                     eb = __builtin_amdgcn_readfirstlane(d_next.z), ec = __builtin_amdgcn_readfirstlane(d_next.w);
      unsigned long long tn = 0;
      if (PROF) tn = clock64();
      Fr29 v;
      if (!(w0 & W29_RARE)) {
        // Mul / Add on ring values and LDS constants: both operand reads and the next descriptor go out together and
        // cost one LDS round trip.  The previous node's value is read back from the ring like any other (its write
        // was issued a few instructions earlier and LDS is in order): forwarding it in registers cost 18 selects and
        // saved nothing, because a node waits for at least one LDS read anyway.
        Fr29 va, vb, vc;
        wit29_read(va, wit29_addr(ea, lane48), ring);
        wit29_read(vb, wit29_addr(eb, lane48), ring);
        wit29_read(vc, wit29_addr(ec, lane48), ring);   // the addend of a * b + c (a harmless ring slot otherwise)
        d_next = ((const uint4*)prog)[(n + 1) % (2 * WIT29_CH)];
        if ((w0 & 0xFF) == W29_FMA) {
          v = Fr29::mul_add(va, vb, vc);
        } else if ((w0 & 0xFF) == G_MUL) {
          v = Fr29::mul(va, vb);
        } else {  // G_ADD
#pragma unroll
          for (int k = 0; k < 9; k++) v.v[k] = va.v[k] + vb.v[k];
          v.normalize();
        }
      } else {
        d_next = ((const uint4*)prog)[(n + 1) % (2 * WIT29_CH)];
        const Wit29Out o = wit29_rare(w0, ea, eb, ec, ring, lane, consts29, inputs, n_inputs, V29, B, p);
        v = o.v;
        if (o.e && !e) e = o.e;
      }
      {  // every value goes to the ring (three LDS instructions: cheaper than asking whether anybody reads it)
        char* a = (char*)ring + (n % WIT29_RING) * 64 * 48 + lane48;
        *(uint4*)a = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
        *(uint4*)(a + 16) = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
        *(uint32_t*)(a + 32) = v.v[8];
      }
      if (w0 & W29_STORE) {
        uint4* g = V29 + ((size_t)(w0 >> 16) * B + p) * 3;
        g[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
        g[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
        g[2] = make_uint4(v.v[8], 0, 0, 0);
      }
      if (PROF) {
        const uint32_t op = w0 & 0xFF;
        const int cls = (op == G_MUL || op == W29_FMA) ? 0 : op == G_ADD ? 1 : (op == G_CONST || op == G_INPUT) ? 2 : 3;
        pc[cls] += clock64() - tn;
        pn[cls]++;
      }
    }
  }
  err[p] = e;
  if (PROF && blockIdx.x == 0 && lane == 0) {
    for (int k = 0; k < 4; k++) { prof[k] = pc[k]; prof[4 + k] = pn[k]; }
    prof[8] = clock64() - pc0;
    prof[9] = wall_clock64() - pw0;
  }
}
// stored node values of the Fr29 interpreter -> the 8 x 32 Montgomery values every later kernel reads (V[node][proof])
// lg (small batches): lanes = stored values of ONE proof (blockIdx.y) instead of lanes = proofs
__global__ void __launch_bounds__(64) k_v29_to_fr(const uint4* __restrict__ V29, const uint32_t* __restrict__ slot2node,
                                                  uint32_t nslots, Fr* __restrict__ V, uint32_t B, uint32_t nb,
                                                  uint32_t lg) {
  const uint32_t p = lg ? blockIdx.y : blockIdx.x * 64 + threadIdx.x, sl = lg ? blockIdx.x * 64 + threadIdx.x : blockIdx.y;
  if (p >= nb || sl >= nslots) return;
  const uint4* g = V29 + ((size_t)sl * B + p) * 3;
  const uint4 x = g[0], y = g[1], z = g[2];
  Fr29 v;
  v.v[0] = x.x; v.v[1] = x.y; v.v[2] = x.z; v.v[3] = x.w;
  v.v[4] = y.x; v.v[5] = y.y; v.v[6] = y.z; v.v[7] = y.w;
  v.v[8] = z.x;
  V[(size_t)slot2node[sl] * B + p] = v.to_fq();
}

// =====================================================================================================
// 2. a = A.w, b = B.w, c = a o b on the padded domain (qap.rs:40-67)
// =====================================================================================================
// LG (small batches): lanes = rows of ONE proof (blockIdx.y) instead of lanes = proofs -- with lanes = proofs a single
// proof launches 8 192 waves with one useful lane each, which also crowd the walks that run beside them
// Long rows (LG): the circuit's matrices hold 2 entries in most rows and 60 + 60 in ninety of them (Poseidon's mix
// layers), and a lane that walks 120 entries alone -- two dependent loads and a product each -- is the whole kernel
// (0.40 ms for one proof).  Rows with more than MV_LONG entries in A or B are therefore taken out of the lanes = rows
// part and given a wave each (blocks >= nshort): a lane per entry, then a shuffle tree of field additions (exact, so the
// order of the sum does not matter).
__device__ __forceinline__ Fr fr_shfl_down(const Fr& x, int off) {
  Fr r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] = (uint32_t)__shfl_down((int)x.v[k], off, 64);
  return r;
}
template <bool LG>
__global__ void __launch_bounds__(256) k_matvec(CsrView A, CsrView Bm, const Fr* __restrict__ V,
                                                const uint32_t* __restrict__ sig2node, uint32_t nc, uint32_t ni,
                                                uint32_t n, Fr* __restrict__ abc, uint32_t B, uint32_t nb,
                                                const uint32_t* __restrict__ long_rows, uint32_t nshort) {
  if (LG) __builtin_amdgcn_s_setprio(3);   // small batches: a link of the latency chain (see k_ntt_mid)
  uint32_t p = LG ? blockIdx.y : blockIdx.x * 64 + threadIdx.x;
  if (LG && blockIdx.x >= nshort) {   // a wave per long row
    const uint32_t row = long_rows[blockIdx.x - nshort], lane = threadIdx.x;
    Fr a = Fr::zero(), b = Fr::zero();
    for (uint32_t k = A.ptr[row] + lane; k < A.ptr[row + 1]; k += 64) a = a + A.coef[k] * V[(size_t)A.col[k] * B + p];
    for (uint32_t k = Bm.ptr[row] + lane; k < Bm.ptr[row + 1]; k += 64) b = b + Bm.coef[k] * V[(size_t)Bm.col[k] * B + p];
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      a = a + fr_shfl_down(a, off);
      b = b + fr_shfl_down(b, off);
    }
    if (lane == 0) {
      const size_t o = (size_t)row * B + p;
      abc[o] = a;
      abc[(size_t)n * B + o] = b;
      abc[2 * (size_t)n * B + o] = a * b;
    }
    return;
  }
  uint32_t row = LG ? blockIdx.x * 64 + threadIdx.x
                    : __builtin_amdgcn_readfirstlane(blockIdx.y * blockDim.y + threadIdx.y);  // wave-uniform
  if (row >= n) return;
  if (p >= nb) return;
  Fr a = Fr::zero(), b = Fr::zero();
  if (row < nc) {
    if (LG && long_rows && (A.ptr[row + 1] - A.ptr[row] > MV_LONG || Bm.ptr[row + 1] - Bm.ptr[row] > MV_LONG)) return;
    for (uint32_t k = A.ptr[row]; k < A.ptr[row + 1]; k++) a = a + A.coef[k] * V[(size_t)A.col[k] * B + p];
    for (uint32_t k = Bm.ptr[row]; k < Bm.ptr[row + 1]; k++) b = b + Bm.coef[k] * V[(size_t)Bm.col[k] * B + p];
  } else if (row < nc + ni) {
    a = V[(size_t)sig2node[row - nc] * B + p];  // a[nc..nc+ni] = w[0..ni] (qap.rs:54-58)
  }
  size_t o = (size_t)row * B + p;
  abc[o] = a;
  abc[(size_t)n * B + o] = b;
  abc[2 * (size_t)n * B + o] = (row < nc) ? a * b : Fr::zero();
}

// =====================================================================================================
// 3. radix-2^K register-blocked NTT passes over [index][proof] data (ark-poly Radix2EvaluationDomain
//    fft/ifft semantics; call sites qap.rs:69-90).  DIF takes natural order to bit-reversed, DIT takes
//    bit-reversed back to natural, so iNTT(DIF) -> coset scale -> NTT(DIT) needs no reordering pass.
// =====================================================================================================
__device__ __forceinline__ Fr29 load_fr29(const uint32_t* __restrict__ p) {
  Fr29 w;
#pragma unroll
  for (int k = 0; k < 9; k++) w.v[k] = p[k];
  return w;
}
// constants for Fr29::mul_mont: the Fr29 image (x 2^261, normalised) of 8 x 32 Montgomery values
__global__ void __launch_bounds__(256) k_consts_to29(const Fr* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr29 v = Fr29::from_fq(src[t]);
  v.normalize();
#pragma unroll
  for (int k = 0; k < 9; k++) dst[(size_t)t * 9 + k] = v.v[k];
}
// (Small batches do not come here: k_ntt_edge / k_ntt_mid below; a circuit with fewer than 512 constraints would, with its
// proofs in the lanes like any batch.)
// Which pass takes which levels: ntt_pass_list (prover_plan.h).  The lowest levels of both directions and the scaling
// between them are k_ntt_turn's, so a pass here never has stride 1 and never scales.
//
// ---- the arithmetic: 9 x 29 limbs, lazy, with NO change of radix
// A canonical Fr word string is the integer X = x 2^256 mod r.  Cut into 29-bit limbs (Fr29::slice: no arithmetic) the same
// integer is a valid Fr29 representative: of x 2^256 / 2^261 = x 2^-5 in the 2^261 radix.  The transform is linear, so a
// constant factor on every input is the same factor on every output: nobody has to know about the 2^-5.  The twiddles and
// the coset / (1/n) factors are held in Fr29's Montgomery form T = t 2^261 mod r (NttTables::tw_i29, tw_f29, coset29), and
// Fr29::mul(D, T) = D T / 2^261 = D t mod r for ANY integer D: if D = X + k r then the product is X t + k' r.  Sums and
// K r - v differences keep "X up to a multiple of r" as well, so from the first load to the last store the data integers
// are the 8 x 32 Montgomery values up to a multiple of r, and the only conversions are the limb cuts at load (slice) and
// store (ntt29_pack): no multiplication by a radix constant anywhere.
// Inside a launch sums are nine 32-bit adds, differences u + K - v with a multiple K of r whose every limb dominates v's
// (Fr29C::K2 / K6, Ntt29C below), products Fr29::mul with the table entry -- the same for all 64 lanes, so in SGPRs -- as the
// normalised operand.  Which K, and where a normalize() is needed, follows from how an element got where it is, which the
// unrolled loops know at compile time (ntt29_dif_sums); tools/check_fq29_bounds.py replays every level of every
// instantiation with all limbs and values at their maxima (no limb sum reaches 2^32, no column 2^64, every K dominates).
// Between launches the buffer holds ANY representative below 2^256, in place, 32 bytes as before: products are below
// 1.5 r and are stored as they are; a sum that can exceed 2^256 first loses floor(top limb / ceil(r / 2^232)) times r
// (ntt29_reduce: one v_mul_hi for the estimate, nine multiply-adds; leaves less than r + 2^240).  The last launch of a
// transform (LAST) reduces every value that way and then subtracts r once more where needed (pack_reduced): the canonical
// Fr, bit for bit what sums, differences and products of Fr gave.
// A butterfly whose twiddle index j is 0 multiplies by the one and is left out as before (the tables' entry 0 is checked
// against Fr29C::ONE where they are built): 8 191 of a 2^13-point transform's 53 248 products.  j = (m & (half - 1)) stride
// + lo: the first term is known at compile time, lo is the same for the whole wave (a scalar branch).
// (A variant that went through Fr29::mul_mont per PRODUCT -- both cuts around every product, canonical 8 x 32 sums -- was
// measured neutral twice in earlier rounds and is gone.  This form, measured against the 8 x 32 passes on one box
// (profiles/quotient_chain_29.md): 1.80 -> 1.43 G VALU wave-instructions per 1 024-proof batch, of which the 64-bit
// multiply-adds are 0.61 -> 0.89 G; the nine launches alone 4.00 -> 3.81 ms; the 20-second rate +1.4 % in every run of
// three, the 20-step headline rate unchanged within its spread -- by the condition set for it, not a speed-up.)
struct Ntt29C {   // tools/check_fq29_bounds.py computes these and compares
  static constexpr uint32_t K12[9] = {0x2000000cu, 0x34bc1779u, 0x2c51b3cau, 0x3dc6cb68u, 0x2245de25u, 0x22470907u, 0x27d28f0cu, 0x2c51ca6fu, 0x0244b3acu};  // 12 r, limbs >= 2^29
  static constexpr uint32_t K24[9] = {0x20000018u, 0x29782ef3u, 0x38a36796u, 0x3b8d96d1u, 0x248bbc4cu, 0x248e120fu, 0x2fa51e19u, 0x38a394dfu, 0x04896759u};  // 24 r, limbs >= 2^29
  static constexpr uint32_t K12B2[9] = {0x4000000cu, 0x54bc1778u, 0x4c51b3c9u, 0x5dc6cb67u, 0x4245de24u, 0x42470906u, 0x47d28f0bu, 0x4c51ca6eu, 0x0244b3abu};  // 12 r, limbs >= 2^30: a sum of two loads
  static constexpr uint32_t K4B2[9] = {0x40000004u, 0x5c3eb27cu, 0x59709141u, 0x5f4243cbu, 0x56174a0au, 0x4b6d0300u, 0x429b8502u, 0x597098ceu, 0x00c19137u};  // 4 r, limbs >= 2^30: a sum of two products
  static constexpr uint32_t NEGR[9] = {0x0fffffffu, 0x00f05360u, 0x11a3dbafu, 0x182f6f0cu, 0x0a7a2d7cu, 0x1d24bf3fu, 0x1f591ebeu, 0x11a3d9cbu, 0x1fcf9bb1u};  // 2^261 - r
  static constexpr uint32_t MAGIC = 0xa948e6d7u;  // floor(2^53 / ceil(r / 2^232))
};
enum Ntt29K { NK_2, NK_6, NK_12, NK_24, NK_12B2, NK_4B2 };
// how many of the DIF levels t - 1, t - 2, ... of a 2^K-point block left element m on the sum side, consecutively
__host__ __device__ constexpr int ntt29_dif_sums(int K, int m, int t) {
  int c = 0;
  for (int l = t - 1; l >= 0; l--) {
    if (m & ((1 << K) >> (l + 1))) break;
    c++;
  }
  return c;
}
__device__ __forceinline__ Fr29 ntt29_add(const Fr29& a, const Fr29& b) {
  Fr29 r;
#pragma unroll
  for (int j = 0; j < 9; j++) r.v[j] = a.v[j] + b.v[j];
  return r;
}
__device__ __forceinline__ Fr29 ntt29_sub_k(const Fr29& u, const uint32_t (&K)[9], const Fr29& v) {
  Fr29 r;
#pragma unroll
  for (int j = 0; j < 9; j++) r.v[j] = u.v[j] + K[j] - v.v[j];
  return r;
}
// u + K - v, limbs left as they fall
__device__ __forceinline__ Fr29 ntt29_sub(const Fr29& u, int k, const Fr29& v) {
  switch (k) {
    case NK_2: return ntt29_sub_k(u, Fr29C::K2, v);
    case NK_6: return ntt29_sub_k(u, Fr29C::K6, v);
    case NK_12: return ntt29_sub_k(u, Ntt29C::K12, v);
    case NK_24: return ntt29_sub_k(u, Ntt29C::K24, v);
    case NK_12B2: return ntt29_sub_k(u, Ntt29C::K12B2, v);
    default: return ntt29_sub_k(u, Ntt29C::K4B2, v);
  }
}
// a normalised x -> x - q r with q = floor(x[8] / ceil(r / 2^232)) (or one less): in [0, r + 2^240), normalised
__device__ __forceinline__ void ntt29_reduce(Fr29& x) {
  const uint32_t q = __umulhi(x.v[8], Ntt29C::MAGIC) >> 21;
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const uint64_t t = (uint64_t)q * Ntt29C::NEGR[j] + x.v[j] + c;   // x + q (2^261 - r): the 2^261 q leaves with the top limb's mask
    x.v[j] = (uint32_t)t & Fr29::M;
    c = t >> 29;
  }
}
// a normalised integer below 2^256 as eight words (the inverse of Fr29::slice)
__device__ __forceinline__ Fr ntt29_pack(const Fr29& x) {
  const uint32_t r0 = x.v[0], r1 = x.v[1], r2 = x.v[2], r3 = x.v[3], r4 = x.v[4], r5 = x.v[5], r6 = x.v[6], r7 = x.v[7], r8 = x.v[8];
  Fr o;
  o.v[0] = r0 | (r1 << 29);
  o.v[1] = (r1 >> 3) | (r2 << 26);
  o.v[2] = (r2 >> 6) | (r3 << 23);
  o.v[3] = (r3 >> 9) | (r4 << 20);
  o.v[4] = (r4 >> 12) | (r5 << 17);
  o.v[5] = (r5 >> 15) | (r6 << 14);
  o.v[6] = (r6 >> 18) | (r7 << 11);
  o.v[7] = (r7 >> 21) | (r8 << 8);
  return o;
}
// DIF level t of a 2^K-point block.  Only differences are multiplied; the subtrahend v is never a unit butterfly's
// difference (those land where all lower index bits are zero: the u side of every later level), so it is a load, a
// product, or a sum of 2^c of either -- which picks K.  A sum of four is normalised before it is used again.
template <int K, class UNIT, class TW>
__device__ __forceinline__ void ntt29_dif_level(Fr29 (&e)[1 << K], int t, UNIT unit, TW twiddle) {
  constexpr int R = 1 << K;
  const int half = R >> (t + 1);
#pragma unroll
  for (int m = 0; m < R; m++) {
    if (m & half) continue;
    const int c = ntt29_dif_sums(K, m + half, t);
    Fr29 u = e[m], v = e[m + half];
    if (c == 2) {
      u.normalize();
      v.normalize();
    }
    const int k = t == 0 ? NK_6 : c == 0 ? NK_2 : c == 1 ? (t == 1 ? NK_12B2 : NK_4B2) : NK_24;
    e[m] = ntt29_add(u, v);
    Fr29 d = ntt29_sub(u, k, v);
    if (unit(m & (half - 1))) d.normalize(); else d = Fr29::mul(d, twiddle(m & (half - 1), t));
    e[m + half] = d;
    // one butterfly at a time: with the products of neighbouring butterflies interleaved the eight-point turn takes 166
    // registers instead of 139
    __builtin_amdgcn_sched_barrier(0);
  }
}
// DIT level t.  The product is below 1.2 r: K2.  A unit butterfly subtracts v itself: a load (FROM_LOADS) or a scaled
// value at level 0, a sum of two / four of them above -- normalised first, K by the level.
template <int K, bool FROM_LOADS, class UNIT, class TW>
__device__ __forceinline__ void ntt29_dit_level(Fr29 (&e)[1 << K], int t, UNIT unit, TW twiddle) {
  constexpr int R = 1 << K;
  const int half = 1 << t;
#pragma unroll
  for (int m = 0; m < R; m++) {
    if (m & half) continue;
    Fr29 u = e[m], v = e[m + half];
    if (unit(m & (half - 1))) {
      if (t > 0) v.normalize();
      const int k = FROM_LOADS ? (t == 0 ? NK_6 : t == 1 ? NK_12 : NK_24) : (t == 0 ? NK_2 : t == 1 ? NK_6 : NK_12);
      e[m] = ntt29_add(u, v);
      e[m + half] = ntt29_sub(u, k, v);
    } else {
      v = Fr29::mul(v, twiddle(m & (half - 1), t));
      e[m] = ntt29_add(u, v);
      e[m + half] = ntt29_sub(u, NK_2, v);
    }
    __builtin_amdgcn_sched_barrier(0);   // (see ntt29_dif_level)
  }
}

template <int K, bool DIF, bool LAST>
__global__ void __launch_bounds__(256, RLN_NTT_WAVES) k_ntt_pass(Fr* __restrict__ data, const uint32_t* __restrict__ tw29, int logn,
                                                  int s0, uint32_t B, uint32_t nb) {
  static_assert(K == 3, "the K / normalize() choices are replayed for three levels (tools/check_fq29_bounds.py)");
  static_assert(!(DIF && LAST), "a transform ends with a DIT pass or with the turn");
  constexpr int R = 1 << K;
  const uint32_t n = 1u << logn;
  auto uni = [](uint32_t v) -> uint32_t { return __builtin_amdgcn_readfirstlane(v); };
  uint32_t p = blockIdx.x * 64 + threadIdx.x;
  uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.y * blockDim.y + threadIdx.y);  // one group per wave
  if (g >= (n >> K)) return;
  if (p >= nb) return;
  Fr* x = data + (size_t)blockIdx.z * n * B + p;
  uint32_t stride, base;
  if (DIF) {
    stride = n >> (s0 + K);  // h_last
    uint32_t blk = g / stride, lo = g % stride;
    base = blk * (n >> s0) + lo;
  } else {
    stride = 1u << s0;  // h_first
    uint32_t blk = g / stride, lo = g % stride;
    base = blk * (stride << K) + lo;
  }
  const uint32_t lo = g % stride;
  const bool lo0 = lo == 0;   // wave-uniform
  Fr29 e[R];
#pragma unroll
  for (int m = 0; m < R; m++) e[m] = Fr29::slice(x[(size_t)(base + m * stride) * B]);
  auto unit = [&](int jm) -> bool { return jm == 0 && lo0; };   // j == 0
  // the twiddle index is the same for all 64 lanes (lanes = proofs): force the scalar path so the twiddle rides in SGPRs
  // instead of VGPRs
  auto twiddle = [&](int jm, int t) -> Fr29 {
    const uint32_t j = (uint32_t)jm * stride + lo;
    const uint32_t ti = DIF ? (j << (s0 + t)) : (j << (logn - 1 - (s0 + t)));
    return load_fr29(tw29 + (size_t)uni(ti) * 9);
  };
#pragma unroll
  for (int t = 0; t < K; t++) {
    if (DIF) ntt29_dif_level<K>(e, t, unit, twiddle); else ntt29_dit_level<K, true>(e, t, unit, twiddle);
  }
  // the eight store addresses are computed again from here: kept from the loads they are sixteen registers held through
  // every level (DIF 169 -> 155 registers, the third wave per SIMD; DIT 140 -> 128)
  asm volatile("" : "+s"(base));
#pragma unroll
  for (int m = 0; m < R; m++) {
    Fr29 y = e[m];
    if (DIF) {
      // products (and the normalised differences of unit butterflies) are normalised already; without a unit butterfly
      // only the sum of all eight loads can reach 2^256, with them (lo == 0) anything can
      if (ntt29_dif_sums(K, m, K) > 0) y.normalize();
      if (m == 0 || lo0) ntt29_reduce(y);
      x[(size_t)(base + m * stride) * B] = ntt29_pack(y);
    } else {
      y.normalize();
      ntt29_reduce(y);
      x[(size_t)(base + m * stride) * B] = LAST ? y.pack_reduced() : ntt29_pack(y);
    }
  }
}

// The turn: the lowest KT levels of the inverse transform (DIF levels logn - KT .. logn - 1), the coset / 1/n scaling and
// the lowest KT levels of the forward one (DIT levels 0 .. KT - 1) over the same 2^KT contiguous points -- DIF leaves
// bit-reversed order and DIT starts from it, so both close over the positions (g << KT) + m, as in k_ntt_mid.  One trip
// through HBM where two one-level passes around the scaling made two.  Same butterflies, same twiddles, same products per
// point as k_ntt_pass over those levels (stride 1, lo 0): j = m & (half - 1) is known at compile time and the products by
// the one are left out -- KT = 1 has no twiddle product at all, and what it stores (a sum or a K2 difference of two scaled
// values, below 3.1 r) needs no reduction.  LAST: the turn is the whole transform (logn <= 3) and stores canonical values.
template <int KT, bool LAST>
__global__ void __launch_bounds__(256, RLN_NTT_WAVES) k_ntt_turn(Fr* __restrict__ data, const uint32_t* __restrict__ tw_i29,
                                                  const uint32_t* __restrict__ tw_f29, int logn,
                                                  const uint32_t* __restrict__ scale29, uint32_t B, uint32_t nb) {
  static_assert(KT >= 1 && KT <= 3, "replayed for one to three levels (tools/check_fq29_bounds.py)");
  constexpr int R = 1 << KT;
  const uint32_t n = 1u << logn;
  uint32_t p = blockIdx.x * 64 + threadIdx.x;
  uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.y * blockDim.y + threadIdx.y);  // one group per wave
  if (g >= (n >> KT)) return;
  if (p >= nb) return;
  const uint32_t base = g << KT;
  Fr* x = data + ((size_t)blockIdx.z * n + base) * B + p;
  Fr29 e[R];
#pragma unroll
  for (int m = 0; m < R; m++) e[m] = Fr29::slice(x[(size_t)m * B]);
  auto unit = [](int jm) -> bool { return jm == 0; };
  auto tw_inv = [&](int jm, int t) -> Fr29 { return load_fr29(tw_i29 + ((size_t)jm << (logn - KT + t)) * 9); };   // inverse level logn - KT + t
  auto tw_fwd = [&](int jm, int t) -> Fr29 { return load_fr29(tw_f29 + ((size_t)jm << (logn - 1 - t)) * 9); };    // forward level t
#pragma unroll
  for (int t = 0; t < KT; t++) ntt29_dif_level<KT>(e, t, unit, tw_inv);
#pragma unroll
  for (int m = 0; m < R; m++) e[m] = Fr29::mul(e[m], load_fr29(scale29 + (size_t)(base + m) * 9));   // (wave-uniform index: the factor rides in SGPRs)
#pragma unroll
  for (int t = 0; t < KT; t++) ntt29_dit_level<KT, false>(e, t, unit, tw_fwd);
#pragma unroll
  for (int m = 0; m < R; m++) {
    Fr29 y = e[m];
    y.normalize();
    if (LAST || KT > 1) ntt29_reduce(y);
    x[(size_t)m * B] = LAST ? y.pack_reduced() : ntt29_pack(y);
  }
}

// Small batches (lanes = groups), logn >= 9: the three transforms of the quotient in THREE kernels, one butterfly per lane
// per level.  A lone proof's transform is all latency: with eight points per lane (k_ntt_pass, and the nine-level kernel
// that stood here until round 4) a lane's chain is 12 twiddle products per pass -- 38 + 15 + 10 us inverse,
// 57 + 15 + 42 us forward for 6 us of arithmetic.  Here a workgroup of 256 lanes (a wave per SIMD) owns 512 points in 16 KB
// of LDS and every level costs a lane ONE product:
//   k_ntt_edge<true>   inverse (DIF) levels 0 .. E-1, E = logn - 9: the sets {lo + 512 m}, 512 >> E of them per workgroup
//   k_ntt_mid          inverse levels E .. logn-1 over 512 CONTIGUOUS points, the coset / 1/n scaling, and forward (DIT)
//                      levels 0 .. 8 over the same points (DIF leaves bit-reversed order, DIT starts from it: the low
//                      nine levels of both close over the same 512 positions) -- eighteen levels, one kernel
//   k_ntt_edge<false>  forward levels 9 .. logn-1
// Same butterflies, same twiddles, same products per point as the passes: bit-identical (Fr products are canonical).
__global__ void __launch_bounds__(256) k_ntt_mid(Fr* __restrict__ data, const Fr* __restrict__ tw_i,
                                                 const Fr* __restrict__ tw_f, int logn, const Fr* __restrict__ scale,
                                                 uint32_t B, uint32_t nb) {
  __shared__ Fr buf[512];
  __builtin_amdgcn_s_setprio(3);   // the quotient chain is short and the h rows wait for it: issue ahead of the walks' waves
  const uint32_t p = blockIdx.x, l = threadIdx.x;
  const uint32_t n = 1u << logn, base = blockIdx.y * 512;
  if (p >= nb) return;
  Fr* x = data + (size_t)blockIdx.z * n * B + p;
  buf[l] = x[(size_t)(base + l) * B];
  buf[l + 256] = x[(size_t)(base + l + 256) * B];
  __syncthreads();
  const int E = logn - 9;
#pragma unroll 1
  for (int t = 0; t < 8; t++) {   // inverse level E + t: half = 256 >> t
    const uint32_t hl = 256u >> t, jl = l & (hl - 1), i0 = ((l >> (8 - t)) << (9 - t)) | jl, i1 = i0 + hl;
    const Fr u = buf[i0], v = buf[i1];
    buf[i0] = u + v;
    buf[i1] = (u - v) * tw_i[(size_t)jl << (E + t)];
    __syncthreads();
  }
  {   // the last inverse level (half = 1), the scaling and the first forward level (half = 1): the same two points
    const uint32_t i0 = 2 * l, i1 = i0 + 1;
    const Fr u = buf[i0], v = buf[i1];
    Fr a = u + v, b = u - v;   // (both levels' twiddle is tw[0] = 1: the product would return its operand)
    if (scale) {
      a = a * scale[base + i0];
      b = b * scale[base + i1];
    }
    buf[i0] = a + b;
    buf[i1] = a - b;
    __syncthreads();
  }
#pragma unroll 1
  for (int s = 1; s < 9; s++) {   // forward level s: half = 1 << s
    const uint32_t hl = 1u << s, jl = l & (hl - 1), i0 = ((l >> s) << (s + 1)) | jl, i1 = i0 + hl;
    const Fr u = buf[i0], v = buf[i1] * tw_f[(size_t)jl << (logn - 1 - s)];
    buf[i0] = u + v;
    buf[i1] = u - v;
    __syncthreads();
  }
  x[(size_t)(base + l) * B] = buf[l];
  x[(size_t)(base + l + 256) * B] = buf[l + 256];
}

template <bool DIF>
__global__ void __launch_bounds__(256) k_ntt_edge(Fr* __restrict__ data, const Fr* __restrict__ tw, int logn, uint32_t B,
                                                  uint32_t nb) {
  __shared__ Fr buf[512];
  __builtin_amdgcn_s_setprio(3);
  const uint32_t p = blockIdx.x, l = threadIdx.x;
  const uint32_t n = 1u << logn;
  if (p >= nb) return;
  const int E = logn - 9;                       // 1 .. 9
  const uint32_t cl = 512u >> E, lo0 = blockIdx.y * cl;   // local point i = m cl + c  <->  position lo0 + c + 512 m
  Fr* x = data + (size_t)blockIdx.z * n * B + p;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t i = l + 256 * k;
    buf[i] = x[(size_t)(lo0 + (i & (cl - 1)) + 512 * (i >> (9 - E))) * B];
  }
  __syncthreads();
  const uint32_t c = l & (cl - 1), q = l >> (9 - E);
#pragma unroll 1
  for (int t = 0; t < E; t++) {
    const int lh = DIF ? E - 1 - t : t;         // log2 of the level's half in units of m
    const uint32_t hm = 1u << lh, jm = q & (hm - 1), m0 = ((q >> lh) << (lh + 1)) | jm;
    const uint32_t i0 = m0 * cl + c, i1 = i0 + hm * cl;
    const size_t j = (size_t)jm * 512 + lo0 + c;
    if (DIF) {
      const Fr u = buf[i0], v = buf[i1];
      buf[i0] = u + v;
      buf[i1] = (u - v) * tw[j << t];
    } else {
      const Fr u = buf[i0], v = buf[i1] * tw[j << (logn - 1 - (9 + t))];
      buf[i0] = u + v;
      buf[i1] = u - v;
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t i = l + 256 * k;
    x[(size_t)(lo0 + (i & (cl - 1)) + 512 * (i >> (9 - E))) * B] = buf[i];
  }
}

// =====================================================================================================
// 4. scalars -> signed digits (window j: cw[j] bits), layout [scalar][half][window][proof] (int16)
// =====================================================================================================
// Digits of the magnitude `l` (NL limbs, destroyed) under schedule ws; the scalar's sign flips every digit.  A window
// of c bits yields d in [-2^(c-1), 2^(c-1)]; both ends select table entry 2^(c-1) - 1, but only one of them fits an
// int16 at c = 16, so a window value of exactly 2^(c-1) goes to the end the sign leaves representable.
template <int NL>
__device__ __forceinline__ void emit_digits(uint32_t* l, bool neg, const WinSched& ws, int16_t* __restrict__ out, uint32_t B) {
  uint32_t carry = 0;
#pragma unroll 1
  for (int j = 0; j < ws.W; j++) {
    const int c = ws.cw[j];
    const uint32_t mask = (c >= 32) ? 0xFFFFFFFFu : ((1u << c) - 1), E = 1u << (c - 1);
    uint32_t raw = (l[0] & mask) + carry;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) l[i] = (l[i] >> c) | (l[i + 1] << (32 - c));
    l[NL - 1] >>= c;
    int d;
    if (raw > E || (raw == E && !neg)) {
      d = (int)raw - (int)(mask + 1);
      carry = 1;
    } else {
      d = (int)raw;
      carry = 0;
    }
    out[(size_t)j * B] = (int16_t)(neg ? -d : d);
  }
}
// Scalar ids: [0, ns) witness signals (id 0: the constant one, not w_0), [ns, ns + n) quotient coefficients h, then
// r, s, -(r s).  dig1 holds the G1 schedule for all of them; dig2 the G2 schedule for the ones the G2 walk uses
// (witness, r, s, -(r s): id - n).
// Every scalar is split as k1 + lambda k2 (glv.h) and both halves are recoded.
__global__ void __launch_bounds__(256) k_recode(const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node,
                                                uint32_t ns, const Fr* H, uint32_t n,
                                                const uint32_t* __restrict__ rs, WinSched ws1, WinSched ws2,
                                                int16_t* __restrict__ dig1, int16_t* __restrict__ dig2, uint32_t B,
                                                uint32_t nb, uint32_t part, uint32_t lg, uint32_t hq, uint32_t dB) {
  // dB: the proof stride of the digit arrays ([scalar][half][window][dB]).  The batch capacity B in the throughput
  // shapes; the batch SIZE for small batches -- with B = 64 a lone proof's digits sat one per 128-byte line (64 scattered
  // two-byte stores per lane here, a miss per step in the walks); compact, a scalar's windows share one line.
  // part 0: every scalar; 1: the witness scalars and r, s, -(r s) (all the G2 walk needs: it can start before the
  // quotient h exists); 2: the coefficients of h only
  // part 3 (small full proofs, fused plan): the products s w_i, r w_i and r s under the ids ns + n + 3 + ..., G1 only
  if (lg) __builtin_amdgcn_s_setprio(3);   // small batches: a link of the latency chain (see k_ntt_mid)
  uint32_t p = lg ? blockIdx.y : blockIdx.x * 64 + threadIdx.x;   // lg (small batches): lanes = scalars of one proof
  uint32_t sid = lg ? blockIdx.x * 64 + threadIdx.x : blockIdx.y * blockDim.y + threadIdx.y;
  if (part == 1) {
    if (sid >= ns + 3) return;
    if (sid >= ns) sid += n;
  } else if (part == 2) {
    if (sid >= n) return;
    sid += ns;
  } else if (part == 3) {
    if (sid >= 2 * ns + 1) return;
    sid += ns + n + 3;
  }
  if (p >= nb || sid >= 3 * ns + n + 4) return;
  Fr x;
  if (sid >= ns + n + 3) {
    const uint32_t q = sid - (ns + n + 3);
    const Fr r = Fr::from_canonical(rs + (size_t)p * 16), s = Fr::from_canonical(rs + (size_t)p * 16 + 8);
    // (id 0: the constant row, see below -- s and r themselves)
    if (q < ns)
      x = q == 0 ? s : s * V[(size_t)sig2node[q] * B + p];
    else if (q < 2 * ns)
      x = q == ns ? r : r * V[(size_t)sig2node[q - ns] * B + p];
    else
      x = r * s;
  } else if (sid < ns) {
    // id 0 is the scalar of the constant row -- query[0], alpha, beta -- which the reference adds unconditionally
    // (ark-groth16 create_proof_with_reduction_and_matrices): ONE, whatever a supplied witness holds in w_0.  The mat-vec
    // reads w_0 from the witness as given (the witness map's full_assignment[0]).
    x = sid == 0 ? Fr::one() : V[(size_t)sig2node[sid] * B + p];
  } else if (sid < ns + n) {
    const size_t o = (size_t)(sid - ns) * B + p;
    // hq (every full proof and finish; a flag of its own: lg also selects the lane mapping): the quotient on the fly,
    // h = a o b - c (qap.rs:84-95), from the three transformed vectors -- no kernel of its own that reads a, b, c and
    // writes h for this one to read back, and for small batches one boundary less on the chain the h rows wait for.
    // Without it (a partial proof: no quotient, its h rows are not walked) the row is read as it is.
    x = hq ? H[o] * H[(size_t)n * B + o] - H[2 * (size_t)n * B + o] : H[o];
    if (hq) const_cast<Fr*>(H)[o] = x;   // over the `a` vector, where Prover::fetch_h reads it; one lane per element
  } else {
    Fr r = Fr::from_canonical(rs + (size_t)p * 16);
    Fr s = Fr::from_canonical(rs + (size_t)p * 16 + 8);
    uint32_t which = sid - ns - n;  // 0: r, 1: s, 2: -(r s)
    x = which == 0 ? r : which == 1 ? s : (r * s).neg();
  }
  uint32_t l[8];
  x.to_canonical(l);
  const bool g2 = sid < ns || (sid >= ns + n && sid < ns + n + 3);
  const uint32_t sid2 = sid < ns ? sid : sid - n;
  uint32_t k[2][4], neg[2];
  glv_split(l, k[0], &neg[0], k[1], &neg[1]);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    uint32_t t[4];
    if (g2) {
#pragma unroll
      for (int i = 0; i < 4; i++) t[i] = k[h][i];
      emit_digits<4>(t, neg[h] != 0, ws2, dig2 + ((size_t)sid2 * 2 + h) * ws2.W * dB + p, dB);
    }
    emit_digits<4>(k[h], neg[h] != 0, ws1, dig1 + ((size_t)sid * 2 + h) * ws1.W * dB + p, dB);
  }
}


// ---- explicit instantiations: every form the host launches
template __global__ void k_witness29<false>(const GNode29* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ consts29, uint32_t n_consts, const uint32_t* __restrict__ inputs, uint32_t n_inputs, uint4* __restrict__ V29, uint32_t* __restrict__ err, uint32_t B, uint32_t nb, unsigned long long* __restrict__ prof);
template __global__ void k_matvec<true>(CsrView A, CsrView Bm, const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node, uint32_t nc, uint32_t ni, uint32_t n, Fr* __restrict__ abc, uint32_t B, uint32_t nb, const uint32_t* __restrict__ long_rows, uint32_t nshort);
template __global__ void k_matvec<false>(CsrView A, CsrView Bm, const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node, uint32_t nc, uint32_t ni, uint32_t n, Fr* __restrict__ abc, uint32_t B, uint32_t nb, const uint32_t* __restrict__ long_rows, uint32_t nshort);
template __global__ void k_ntt_pass<NTT_MAX_K, true, false>(Fr* __restrict__ data, const uint32_t* __restrict__ tw29, int logn, int s0, uint32_t B, uint32_t nb);
template __global__ void k_ntt_pass<NTT_MAX_K, false, false>(Fr* __restrict__ data, const uint32_t* __restrict__ tw29, int logn, int s0, uint32_t B, uint32_t nb);
template __global__ void k_ntt_pass<NTT_MAX_K, false, true>(Fr* __restrict__ data, const uint32_t* __restrict__ tw29, int logn, int s0, uint32_t B, uint32_t nb);
#define RLN_NTT_TURN(KT, LAST)                                                                                                       \
  template __global__ void k_ntt_turn<KT, LAST>(Fr* __restrict__ data, const uint32_t* __restrict__ tw_i29, const uint32_t* __restrict__ tw_f29, \
                                                int logn, const uint32_t* __restrict__ scale29, uint32_t B, uint32_t nb);
RLN_NTT_TURN(1, false) RLN_NTT_TURN(2, false) RLN_NTT_TURN(3, false) RLN_NTT_TURN(1, true) RLN_NTT_TURN(2, true) RLN_NTT_TURN(3, true)
#undef RLN_NTT_TURN
template __global__ void k_ntt_edge<true>(Fr* __restrict__ data, const Fr* __restrict__ tw, int logn, uint32_t B, uint32_t nb);
template __global__ void k_ntt_edge<false>(Fr* __restrict__ data, const Fr* __restrict__ tw, int logn, uint32_t B, uint32_t nb);

}  // namespace rlnamd
