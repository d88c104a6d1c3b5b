// prover_plan.h -- the host planning of the batched prover: everything Prover::Prover derives from the parsed zkey and
// graph before it uploads anything (the k_witness29 program, the hint cut nodes, the point lists and the table-walk plans),
// the hint hashing with its chain cache, and the shape decision of Prover::enqueue.  Pure host code, no HIP call: it is
// compiled into the library and, by a plain C++ compiler, into the CPU tests (tests/host/proverplan.cpp).
#pragma once
#include <stdint.h>

#include <mutex>
#include <vector>

#include "prover.h"
#include "prover_desc.h"
#include "zkey.h"

namespace rlnamd {

constexpr uint32_t HINT_PROOFS = 64;   // most proofs of a batch that is interpreted as segments (ProverTuning::hint_max <= this)
constexpr uint32_t TINY_STRIDE = 8;    // partial sums of a tiny batch: [chunk][8]

// c-bit windows, the first `wide` of them one bit wider; W = the fewest windows that cover the 127 bits of a GLV half
// (< 2^126, plus the carry of the signed recoding)
WinSched make_sched(int c, int wide);

// ---- named input slots (single message-id circuits; witness.rs:832-881): the proof-values kernel and the hints need them
struct NamedInputs {
  InputSlots slots{};
  bool have_values_kernel = false;   // single message id, six instance variables, every shipped name
  bool have_hint_slots = false;      // the names the hints read, with one message id per message slot (max_out of them)
  uint32_t hint_msg_off = 0, hint_msgs = 1;
  // the Merkle path by itself (Prover::submit_members writes it on the device): both names, tree_depth elements each
  bool have_path_slots = false;
  uint32_t path_off = 0, path_idx_off = 0;
  // what a batch with drawn message ids reads and writes (Prover::submit_members_drawn): slots.limit and slots.ext of
  // each input row, and ONE messageId slot -- the multi-message-id circuit, which has max_out of them, is refused
  bool have_drawn_slots = false;
  uint32_t drawn_msg_off = 0;
  // ... and a batch with drawn BLOCKS of ids (Prover::submit_members_drawn_counts): slots.limit, slots.ext, messageId[max_out]
  // and selectorUsed[max_out], max_out >= 1.  A single message-id graph names no selectors and needs none (drawn_sel false):
  // its one slot is always used.
  bool have_drawn_multi_slots = false, drawn_sel = false;
  uint32_t drawn_multi_msg_off = 0, drawn_multi_sel_off = 0, drawn_multi_slots = 1;
};
NamedInputs find_named_inputs(const Graph& graph, uint32_t ni);

// ---- hints: the values between the circuit's chained hashes, hashed on the host (depth + 2 Poseidon hashes, ~0.3 ms).
// The chain part of a member's hints -- rate commitment and the running hash after every level -- is a function of PUBLIC
// values only: the identity commitment (hint 0, hashed from the secret on every call) and the tree's nodes along the
// member's path.  A node that proves message after message with one identity while the root stands asks for the same
// chain again and again: the last few are remembered under a fingerprint of (identity commitment, limit, path
// elements, path bits) -- no secret in it, none in what is stored -- and a call that finds its chain hashes twice
// (identity commitment, a1) instead of depth + 2 times.  Nothing is trusted for it: k_hint_check compares every hint
// with the device's own value, a fingerprint collision or a stale entry costs one run over the whole graph.
class HintChains {
 public:
  // the first step of a proof's hints by itself: identity commitment, the chain's fingerprint, and whether that chain is
  // remembered -- what a batch above hint_max needs to know before it decides for the segments (Prover::enqueue)
  struct Probe {
    Fr idc;
    uint64_t fp[2];
    bool found;
  };
  void configure(const NamedInputs& in, uint32_t entries) { in_ = in; entries_ = entries; }
  uint32_t count() const { return in_.slots.depth + 1 + in_.hint_msgs; }   // hints per proof
  void probe(const uint8_t* in_le, Probe* pr) const;
  // idc, rate commitment, the running hash after levels 1 .. depth - 1, a1 of every message slot (pr: probe()'s result for
  // these inputs, or null)
  void hints(const uint8_t* in_le, Fr* out, const Probe* pr = nullptr) const;
  uint64_t hits() const;

 private:
  struct Entry {
    uint64_t fp[2] = {0, 0};
    uint64_t stamp = 0;
    std::vector<Fr> chain;   // hints 1 .. depth
  };
  NamedInputs in_;
  uint32_t entries_ = 0;     // ProverTuning::hint_chains
  mutable std::mutex mu_;
  mutable std::vector<Entry> cache_;
  mutable uint64_t clock_ = 0, hits_ = 0;
};

// Where the graph can be cut (segments behind hints): the nodes that hold the values between the chained hashes, found on
// two probe witnesses -- every computed node whose value equals one of HintChains::hints' under both -- so that nothing
// about the circuit's node numbering is assumed.  cuts[j] = the nodes that carry hint j; empty when a hint matches no node
// (such a circuit keeps the whole-graph interpreter).
std::vector<std::vector<uint32_t>> find_hint_cuts(const Graph& graph, const NamedInputs& in, const HintChains& chains);

// ---- the program of k_witness29 (prover_front.hip)
struct Wit29Program {
  std::vector<GNode29> prog;          // padded: the kernel prefetches two chunks past the end
  uint32_t nprog = 0;                 // program nodes (after fusion)
  std::vector<uint32_t> slot2node;    // stored values: slot -> graph node
  std::vector<uint32_t> store_slot;   // graph node -> slot, 0xFFFFFFFF: not stored
};
Wit29Program compile_witness29(const Graph& graph, const std::vector<uint8_t>& is_cut);

// ---- table walks.  Scalar ids: [0, NS) witness, [NS, NS + n) h, then r, s, -(r s).
// A walk = a list of (table row, scalar id, output segment) entries cut into chunks.  `dig_sid` = the id the digits
// of an entry live under (G2: the ids above the h block move down), `is_h` = the scalar is a coefficient of h.
struct VRow {
  uint32_t k, sid, dig_sid, seg;
  bool is_h;
};
struct G1Rows {
  std::vector<G1Affine> pts;         // finite points, pair members first
  std::vector<uint32_t> sids;        // scalar id of every point
  uint32_t npaired = 0;              // points [0, npaired) are pair members (ROW_PAIRED)
  std::vector<VRow> rows, fused;     // the plain rows; the rows of the fused small-batch plan
  // The throughput plan's rows.  For a wire i >= 1 with a_query[i] and b_g1_query[i] finite and a_query[i] = +- b_g1_query[i]
  // (a constraint that squares a linear combination has the same combination on both sides: a third of the A rows of the
  // shipped keys) the walk of the B1 row would repeat, under the same scalar, the partial sum the A row makes.  `shared` is
  // `rows` without those B1 rows and with their A rows moved to SEG_SHARED_EQ / SEG_SHARED_OPP; with S+ and S- the sums of
  // those two segments, A = seg 0 + S+ + S- and B1 = seg 1 + S+ - S- (k_shared_join).  Rows of scalar id 0 and the blinding
  // rows are never shared.  The points, their order and the tables do not depend on any of this: the dropped B1 rows stay
  // resident for the other plans.
  std::vector<VRow> shared;
  std::vector<uint32_t> shared_eq, shared_opp;   // the wires, ascending
};
struct G2Rows {
  std::vector<G2Affine> pts;
  std::vector<uint32_t> dsid;        // digit id of every point
  std::vector<VRow> rows;
};
G1Rows g1_walk_rows(const Zkey& zk, uint32_t NS, uint32_t n, uint32_t ni);   // n: size of the evaluation domain
G2Rows g2_walk_rows(const Zkey& zk, uint32_t NS, uint32_t n);

// chunks of one segment -> groups of <= 16 chunks -> the segment
void make_reduce_ranges(const std::vector<uint32_t>& segfirst, std::vector<ChunkDesc>& groups, std::vector<ChunkDesc>& segs);

// One walk: the rows a mode takes (full: all; partial: rows whose scalar is a known witness signal, incl. w_0 = 1, which
// carries alpha / beta / query[0]; finish: the rest), cut into chunks of chunk_pts, with the reduction ranges over them.
struct WalkPlan {
  std::vector<uint32_t> rows, rsid;                       // row words and the scalar id of every entry
  std::vector<ChunkDesc> chunks, groups, segs, segchunks; // segchunks: the chunk range of every segment (k_sum_tree)
  std::vector<uint32_t> early_ids, late_ids;              // chunk indices without / with rows that depend on the quotient h
  uint32_t nseg = 0;                                      // reduction segments: outputs x GLV halves
  // pair chunks (throughput plan only; walk29.h PairPlan): rows of the even members, their scalar ids, the chunk ranges
  // over them and the two output chunk slots of every pair chunk
  std::vector<uint32_t> prows, prsid, pout;
  std::vector<ChunkDesc> pchunks;
  // two-stage sum of the tiny plans: segblocks[seg] = the range of block_pts-chunk blocks of a segment, maxblk = the most
  // blocks any segment has
  std::vector<ChunkDesc> segblocks;
  uint32_t nblocks = 0, maxblk = 0;
};
constexpr uint32_t GLV_HALVES = 2;   // halves per scalar: the GLV split k1 + lambda k2 (glv.h)
// npaired: points [0, npaired) are pair members (their row words carry ROW_PAIRED in every plan).  pair_chunks: walk them
// as pair chunks (lane pairs, one 128-byte line per two additions) instead of as single rows; every pair chunk owns a chunk
// slot in each of its two members' segments.  A pair member whose partner the family does not hold (G1Rows::shared) is
// walked as a single row of its interleaved table.
WalkPlan make_walk_plan(const std::vector<VRow>& vrows, uint32_t nseg, uint32_t chunk_pts, int mode,
                        const std::vector<uint8_t>& known, uint32_t npaired = 0, bool pair_chunks = false,
                        uint32_t block_pts = SUM_TREE_LANES);

// ---- the shape of one batch (Prover::enqueue): decided here, before the first launch
enum WalkPlanKind { PLAN_BIG = 0, PLAN_SMALL, PLAN_FUSED, PLAN_TINY };   // plan1 / plan1s / plan1f / plan1tf; plan2 / plan2s / - / plan2t
struct BatchQuery {
  size_t n = 0;
  int mode = PROVE_FULL;
  bool inputs = false, partial_points = false, handles = false, pre_hints = false;   // which host pointers the caller brought
  bool idle = true;            // nothing of this prover in flight (asked only where the answer matters: enqueue)
  bool shared = false;         // another prover on the device
  bool no_hints_now = false;   // the re-run of a batch whose hints did not check
  // capabilities of the prover
  bool witlanes_ok = false, segs_ok = false, cone_ok = false, have_values_kernel = false;
  uint32_t ni = 0;
  int logn = 0;
  size_t capacity = 0;         // Prover::capacity()
  uint32_t small_stride = 64;
  bool compact = false;        // the prover's big batches take the compact stream shape (stream_plan below)
};
struct BatchShape {
  bool lone, small, wl_used, cone, hinted, early, fused, tiny_partial, tiny, walk_lp, g2_on_front, values_w, ntt_lds;
  bool probe_chains;           // hinted holds only if few enough of the proofs' chains have to be hashed (enqueue asks)
  // big batches in the compact stream shape: the public values are the circuit's outputs, read behind k_v29_to_fr on the
  // interpreter's own stream (values_w says the same for the small shapes and the lanes = nodes interpreter, on the
  // values' stream).  Full and finish; a partial batch returns no values and keeps k_proof_values.
  bool values_front;
  WalkPlanKind plan1, plan2;
  uint32_t PB, dB;             // strides of the partial-sum arrays and of the digit rows
};
BatchShape batch_shape(const BatchQuery& q, const ProverTuning& T);

// ---- the transforms of the quotient with lanes = proofs (prover_front.hip: k_ntt_pass, k_ntt_turn): iNTT as DIF levels
// 0 .. logn - 1 (level t pairs points n >> (t + 1) apart), the coset scaling, NTT as DIT levels 0 .. logn - 1 (level t
// pairs points 1 << t apart).  A launch holds a block of 2^k points per lane, k <= NTT_MAX_K (a 16-point block spills).
// The lowest kt DIF levels, the scaling and the lowest kt DIT levels close over the same 2^kt contiguous points: one
// launch, the turn.  kt = ((logn - 1) mod 3) + 1, so that the levels on either side of it split into threes (and a
// transform of at most three levels is the turn alone): 13 levels are 3, 3, 3, 3 | turn(1) | 3, 3, 3, 3.
enum NttPassKind : uint8_t { NTT_DIF = 0, NTT_TURN, NTT_DIT };
struct NttPass {
  uint8_t kind;   // NttPassKind
  uint8_t k;      // levels: points per block = 1 << k
  uint8_t s0;     // first level (NTT_TURN: its first DIF level, logn - k; its DIT levels start at 0)
};
// The tables of a 2^logn-point domain: tw_f[k] = w^k and tw_i[k] = w^-k for k < n / 2 (w = W^(2^(28 - logn))), and
// coset[pos] = g^bitrev(pos) / n, g the root of the doubled domain -- the scaling between the transforms acts on
// bit-reversed order.  Throws unless tw_f[0] and tw_i[0] are the Montgomery one: the kernels leave those products out.
// tw_f29 / tw_i29 / coset29: the same entries for the passes of the big batches, which work on 9 x 29-bit limbs
// (prover_front.hip): t 2^261 mod r, canonical, nine words an entry; entry 0 of both twiddle tables is checked against
// Fr29C::ONE.
struct NttTables {
  std::vector<Fr> tw_f, tw_i, coset;
  std::vector<uint32_t> tw_f29, tw_i29, coset29;
};
NttTables ntt_tables(int logn);
int ntt_turn_width(int logn);                  // kt; 0 for logn < 1
std::vector<NttPass> ntt_pass_list(int logn);  // in launch order; empty for logn < 1

// ---- which stream every role of a BIG batch (!BatchShape::small) takes: Prover::enqueue, wipe_slot.  ROCclr maps streams
// onto GPU_MAX_HW_QUEUES hardware queues; streams that share a queue run their kernels in submission order, and a wait at
// the head of one holds up what the other submitted behind it.  So a big batch keeps no more streams busy than the process
// has queues: `wide` (8 queues and more) is the map of eight streams, `compact` the same launches on four.
// The prover's streams by index, in the order they are created (the first stream of a process runs every kernel ~70 us
// slower: the wipes' own stream, which only the small shapes and the wide map use).
enum StreamId : uint8_t { ST_W = 0, ST_A, ST_A2, ST_AB, ST_V, ST_B, ST_C, ST_B2, ST_COUNT };
enum StreamRole : uint8_t {
  ROLE_INTERP = 0,   // stage-in, graph interpreter, k_v29_to_fr
  ROLE_VALUES,       // public values
  ROLE_QUOTIENT,     // mat-vec, NTTs, quotient, recode
  ROLE_WALK1,        // G1 table walk
  ROLE_WALK2,        // G2 table walk
  ROLE_SUMS1,        // G1 group / segment sums
  ROLE_SUMS2,        // G2 sums, fold, finalize, output kernels, results home, evC
  ROLE_WIPE,         // the wipe of the slot the batch used (collect)
  ROLE_COUNT
};
enum StreamShape { SHAPE_AUTO = 0, SHAPE_WIDE = 1, SHAPE_COMPACT = 2 };
struct StreamEdge {   // `to` reads what `from` wrote: in stream order behind it where they share a stream, else behind an event
  uint8_t from, to;
};
// What Prover::enqueue takes from the plan is the stream table `at`, `shape` and `values_front`; its event records and
// waits are written out in enqueue.  `order`, `edges`, `needs_event` and `busy_streams` DESCRIBE those launches for the
// host test (tests/host/streamplan.cpp), which therefore covers the table -- who shares a stream with whom, whether the
// table admits an acyclic submission -- and not the presence of each hipStreamWaitEvent (the GPU tests cover those).
struct StreamPlan {
  int shape = SHAPE_WIDE;                 // resolved: SHAPE_WIDE or SHAPE_COMPACT
  uint8_t at[2][ROLE_COUNT] = {};         // [parity of the batch's sequence number][role] -> StreamId
  uint8_t order[ROLE_COUNT] = {};         // the roles in the order enqueue submits them (ROLE_WIPE last: at collect)
  bool values_front = false;              // ROLE_VALUES is k_values_from_witness behind the interpreter (BatchShape::values_front)
  static constexpr int NEDGE = 9;
  static const StreamEdge edges[NEDGE];   // producer -> consumer inside one batch
  // the next batch on the slot (nslot batches later) waits for the wipe: always through the slot's event (evZ), and in
  // stream order as well where the wipe went to that batch's interpreter stream
  bool needs_event(int parity, const StreamEdge& e) const { return at[parity][e.from] != at[parity][e.to]; }
  int busy_streams() const;               // distinct streams of the roles other than ROLE_WIPE, both parities
};
// queues: GPU_MAX_HW_QUEUES as the process got it (hw_queues_from_env).  SHAPE_AUTO never keeps more streams busy than
// the process has queues: wide at 8 queues and more, compact at COMPACT_MIN_QUEUES .. 7, and wide -- the map every
// queue count had before there were two -- below that, where no four-stream map fits either.  SHAPE_COMPACT asked for
// by name is the four-stream map whatever `queues` is.  No HIP call.
constexpr int COMPACT_MIN_QUEUES = 4;
StreamPlan stream_plan(int queues, int nslot, int shape = SHAPE_AUTO);
int hw_queues_from_env(const char* value);   // the variable's text (or null): 4, HIP's default, when absent or unparsable
int stream_shape_from_name(const char* name);   // "auto" / "wide" / "compact" -> StreamShape; -1: none of them
const char* stream_shape_name(int shape);

}  // namespace rlnamd
