// prover_kernels.h -- internal to the prover: what the host pipeline (prover.hip) and the kernel translation units
// (prover_front.hip: witness interpreters, mat-vec, NTT, recoding; prover_walks.hip: table build, table walks, partial-sum
// reductions; prover_back.hip: finalize, proof values, taps, staging, wipes) share -- the kernel DECLARATIONS and the
// descriptors only kernels and launches need.  The descriptors the host planning builds (GNode29, the W29_* / WIT29_*
// constants, InputSlots, ...) are in prover_desc.h, which has no HIP in it.  The kernels are defined (and their templates explicitly instantiated) in exactly one unit each, so
// a change to one kernel recompiles one unit, and the units compile in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "fq29.h"
#include "poseidon.h"
#include "prover.h"
#include "prover_desc.h"
#include "prover_plan.h"
#include "walk29.h"
#include "witness_ops.h"

namespace rlnamd {

// ---- mat-vec
struct CsrView {
  const uint32_t* ptr;
  const uint32_t* col;  // already mapped to graph node ids
  const Fr* coef;
};

// ---- partial-sum reductions and the back end
struct TaskSel {
  uint8_t id[8];
};
inline TaskSel task_sel(std::initializer_list<uint32_t> ids) {
  TaskSel t{};
  uint32_t k = 0;
  for (uint32_t v : ids) t.id[k++] = (uint8_t)v;
  return t;
}
// dynamic LDS of k_sum_tree / k_sum_blocks: the upper half of a level, one point in the 9 x 29 form per lane
constexpr uint32_t SUM_TREE_LDS_G1 = SUM_TREE_LANES / 2 * 4 * 9 * 4, SUM_TREE_LDS_G2 = 2 * SUM_TREE_LDS_G1;

#ifndef RLN_NTT_WAVES
#define RLN_NTT_WAVES 1
#endif

// ---- the quotient's transforms (prover.hip): iNTT, coset scaling, NTT over `vectors` vectors of 2^logn points in the
// [index][B] layout, nb live lanes -- lds: k_ntt_edge / k_ntt_mid / k_ntt_edge (2^9 .. 2^18 points); otherwise the pass list
// (ntt_pass_list(logn)) through k_ntt_pass / k_ntt_turn.  The one place either form is launched from.
// The tables of NttTables on the device: the LDS kernels read the 8 x 32 ones, the passes the 9 x 29 ones.
struct NttDeviceTables {
  const Fr *tw_i, *tw_f, *coset;
  const uint32_t *tw_i29, *tw_f29, *coset29;
};
void launch_quotient_transform(bool lds, const std::vector<NttPass>& passes, Fr* data, const NttDeviceTables& T, int logn,
                               uint32_t B, uint32_t nb, uint32_t vectors, hipStream_t s);

// ---- kernels of prover_front.hip
template <bool PROF>
__global__ void __launch_bounds__(64) k_witness29(const GNode29* __restrict__ nodes, uint32_t n_nodes,
                                                  const uint32_t* __restrict__ consts29, uint32_t n_consts,
                                                  const uint32_t* __restrict__ inputs, uint32_t n_inputs,
                                                  uint4* __restrict__ V29, uint32_t* __restrict__ err, uint32_t B,
                                                  uint32_t nb, unsigned long long* __restrict__ prof);
__global__ void __launch_bounds__(64) k_v29_to_fr(const uint4* __restrict__ V29, const uint32_t* __restrict__ slot2node,
                                                  uint32_t nslots, Fr* __restrict__ V, uint32_t B, uint32_t nb,
                                                  uint32_t lg = 0);
template <bool LG>
__global__ void __launch_bounds__(256) k_matvec(CsrView A, CsrView Bm, const Fr* __restrict__ V,
                                                const uint32_t* __restrict__ sig2node, uint32_t nc, uint32_t ni,
                                                uint32_t n, Fr* __restrict__ abc, uint32_t B, uint32_t nb,
                                                const uint32_t* __restrict__ long_rows = nullptr, uint32_t nshort = 0);
__global__ void __launch_bounds__(256) k_consts_to29(const Fr* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n);
// (tables in the 9 x 29 form, nine words an entry: NttTables::tw_i29 / tw_f29 / coset29.  LAST: the launch that ends a
// transform and stores canonical values)
template <int K, bool DIF, bool LAST>
__global__ void __launch_bounds__(256, RLN_NTT_WAVES) k_ntt_pass(Fr* __restrict__ data, const uint32_t* __restrict__ tw29, int logn,
                                                  int s0, uint32_t B, uint32_t nb);
template <int KT, bool LAST>
__global__ void __launch_bounds__(256, RLN_NTT_WAVES) k_ntt_turn(Fr* __restrict__ data, const uint32_t* __restrict__ tw_i29,
                                                  const uint32_t* __restrict__ tw_f29, int logn,
                                                  const uint32_t* __restrict__ scale29, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(256) k_ntt_mid(Fr* __restrict__ data, const Fr* __restrict__ tw_i,
                                                 const Fr* __restrict__ tw_f, int logn, const Fr* __restrict__ scale,
                                                 uint32_t B, uint32_t nb);
template <bool DIF>
__global__ void __launch_bounds__(256) k_ntt_edge(Fr* __restrict__ data, const Fr* __restrict__ tw, int logn, uint32_t B,
                                                  uint32_t nb);
__global__ void __launch_bounds__(256) k_recode(const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node,
                                                uint32_t ns, const Fr* H, uint32_t n,
                                                const uint32_t* __restrict__ rs, WinSched ws1, WinSched ws2,
                                                int16_t* __restrict__ dig1, int16_t* __restrict__ dig2, uint32_t B,
                                                uint32_t nb, uint32_t part, uint32_t lg, uint32_t hq, uint32_t dB);

// ---- kernels of prover_walks.hip (k_msm29 itself is declared in walk29.h)
template <class A, class E>
__global__ void __launch_bounds__(256) k_table_to29(const A* __restrict__ src, E* __restrict__ dst, size_t n, uint32_t stride,
                                                    uint32_t k0, uint32_t npaired);
template <class F>
__global__ void __launch_bounds__(64) k_sum_ranges(const XYZZ<F>* __restrict__ src, const ChunkDesc* __restrict__ ranges,
                                                   uint32_t nranges, XYZZ<F>* __restrict__ dst, uint32_t B, uint32_t nb);
template <class F, class Acc>
__global__ void __launch_bounds__(SUM_TREE_LANES) k_sum_tree(const XYZZ<F>* __restrict__ part, const ChunkDesc* __restrict__ segchunks,
                                                  XYZZ<F>* __restrict__ dst, uint32_t B, uint32_t PB, TaskSel sel);
template <class F, class Acc>
__global__ void __launch_bounds__(SUM_TREE_LANES) k_sum_blocks(const XYZZ<F>* __restrict__ part, const ChunkDesc* __restrict__ segchunks,
                                                    const ChunkDesc* __restrict__ segblocks, XYZZ<F>* __restrict__ dst, uint32_t PB,
                                                    TaskSel sel);
__global__ void __launch_bounds__(64) k_glv_fold(G1XYZZ* __restrict__ sums1, G2XYZZ* __restrict__ sums2, uint32_t nseg1,
                                                 uint32_t B, uint32_t nb, TaskSel sel);
__global__ void __launch_bounds__(64) k_shared_join(G1XYZZ* __restrict__ sums1, uint32_t B, uint32_t nb);
template <class F>
__global__ void __launch_bounds__(64) k_table_build(const Affine<F>* __restrict__ pts, uint32_t npts, WinSched ws,
                                                    Affine<F>* __restrict__ table, F* __restrict__ scratch);

// ---- kernels of prover_back.hip
__global__ void __launch_bounds__(64) k_partial_out(const G1XYZZ* __restrict__ sums1, const G2XYZZ* __restrict__ sums2,
                                                    uint32_t* __restrict__ out, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(64) k_add_partial(G1XYZZ* __restrict__ sums1, G2XYZZ* __restrict__ sums2,
                                                    const uint32_t* __restrict__ pp, uint32_t B, uint32_t nb, TaskSel sel,
                                                    const G1XYZZ* __restrict__ extra);
__global__ void __launch_bounds__(64) k_fin_affine(const G1XYZZ* __restrict__ sums1, const G2XYZZ* __restrict__ sums2,
                                                   G1Affine* __restrict__ affA, G1Affine* __restrict__ affB1,
                                                   G2Affine* __restrict__ affB2, uint32_t B, uint32_t nb, TaskSel sel);
__global__ void __launch_bounds__(64) k_fin_smul(const G1Affine* __restrict__ affA, const G1Affine* __restrict__ affB1,
                                                 const uint32_t* __restrict__ rs, G1XYZZ* __restrict__ tbl,
                                                 G1XYZZ* __restrict__ prod, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(64) k_fin_out(const G1XYZZ* __restrict__ sums1, const G1XYZZ* __restrict__ prod,
                                                const G1Affine* __restrict__ affA, const G2Affine* __restrict__ affB2,
                                                uint32_t* __restrict__ coords, uint8_t* __restrict__ comp, uint32_t B,
                                                uint32_t nb);
__global__ void __launch_bounds__(64) k_fin_out_b2(const G2XYZZ* __restrict__ sums2, uint32_t* __restrict__ coords,
                                                   uint8_t* __restrict__ comp, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(64) k_fin_out_ac(const G1XYZZ* __restrict__ sums1, const G1XYZZ* __restrict__ prod,
                                                   const G1Affine* __restrict__ affA, uint32_t* __restrict__ coords,
                                                   uint8_t* __restrict__ comp, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(64) k_fin_out_ac_fused(const G1XYZZ* __restrict__ sums1, G1Affine* __restrict__ affA,
                                                         uint32_t* __restrict__ coords, uint8_t* __restrict__ comp, uint32_t B,
                                                         uint32_t nb);
__global__ void __launch_bounds__(64) k_proof_values(const uint32_t* __restrict__ inputs, uint32_t n_inputs,
                                                     InputSlots sl, PoseidonView p2, PoseidonView p3, PoseidonView p4,
                                                     uint32_t* __restrict__ values, uint32_t nb);
__global__ void __launch_bounds__(256) k_public_signals(const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node,
                                                        uint32_t npub, uint32_t B, uint32_t nb, uint32_t* __restrict__ out);
__global__ void __launch_bounds__(64) k_values_from_witness(const Fr* __restrict__ V, const uint32_t* __restrict__ sig2node,
                                                            uint32_t B, uint32_t nb, uint32_t* __restrict__ values);
__global__ void k_gather_col(const Fr* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t count, uint32_t B,
                             uint32_t p, uint32_t* __restrict__ out);
__global__ void k_scatter_witness(const uint32_t* __restrict__ given, const uint32_t* __restrict__ sig2node,
                                  uint32_t NS, Fr* __restrict__ V, uint32_t* __restrict__ err, uint32_t B, uint32_t nb);
__global__ void __launch_bounds__(64) k_alias_rows(Fr* __restrict__ V, const uint32_t* __restrict__ src,
                                                   const uint32_t* __restrict__ dst, uint32_t count, uint32_t B, uint32_t nb);
// partial-proof cache (Prover::collect_partial_cached / submit_finish): rows[k] = stored slot of the k-th known value;
// entry_of[p] (pinned host memory) = cache entry of proof p; an entry is [nk][3] uint4 in the 9 x 29 form of V29
__global__ void __launch_bounds__(64) k_hint_check(const Fr* __restrict__ V, const uint32_t* __restrict__ cut_node,
                                                   const uint32_t* __restrict__ cut_hint, uint32_t n_cut,
                                                   const uint32_t* __restrict__ hints, uint32_t n_hints, uint32_t B,
                                                   uint32_t* __restrict__ err);
__global__ void __launch_bounds__(256) k_cone_save(const uint4* __restrict__ V29, const uint32_t* __restrict__ rows, uint32_t nk,
                                                   uint32_t B, const uint32_t* __restrict__ entry_of, uint4* __restrict__ cache, uint32_t stride16);
__global__ void __launch_bounds__(256) k_cone_restore(const uint4* __restrict__ cache, const uint32_t* __restrict__ rows, uint32_t nk,
                                                      uint32_t B, const uint32_t* __restrict__ entry_of, uint4* __restrict__ V29, uint32_t stride16);
__global__ void __launch_bounds__(64) k_stage_in(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t n16);
__global__ void __launch_bounds__(64) k_wipe_cols(Fr* __restrict__ V, const uint32_t* __restrict__ rows, uint32_t nrows,
                                                  uint32_t B, uint32_t n);
// several contiguous ranges in ONE launch (a small batch's wipes are a dozen tiny buffers: a dozen launches on the calling
// thread before collect returns); block b belongs to the range r with first[r] <= b < first[r + 1], 256 words per block
struct WipeRanges {
  uint4* p[16];
  uint32_t n16[16];
  uint32_t first[17];
  uint32_t count;
};
__global__ void __launch_bounds__(64) k_wipe_ranges(WipeRanges R);
__global__ void __launch_bounds__(64) k_wipe_bytes(uint4* __restrict__ dst, uint32_t n16);   // grid: div_up(n16, 256) workgroups of 64 lanes
__global__ void __launch_bounds__(64) k_wipe_rows16(uint4* __restrict__ base, uint32_t nrows, uint32_t stride16, uint32_t n16);
__global__ void __launch_bounds__(256) k_count_nonzero16(const uint4* __restrict__ src, size_t n16, unsigned long long* __restrict__ out);
__global__ void __launch_bounds__(64) k_wipe_v29(uint4* __restrict__ V29, uint32_t nrows, uint32_t B, uint32_t n);

}  // namespace rlnamd
