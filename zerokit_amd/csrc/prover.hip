// prover.hip -- host side of the batched prover: uploads of the tables and plans, workspace slots, the stream pipeline
// (Prover::enqueue), streamed submit / collect, wipes and the parity taps.  What is uploaded and which shape a batch takes
// is decided in prover_plan.cpp (host only, no HIP call: the k_witness29 program, hint cuts and hint hashing, point lists,
// walk plans, batch_shape); the kernels live in prover_front.hip, prover_walks.hip and prover_back.hip (declarations:
// prover_kernels.h).
#include "prover.h"

#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <mutex>
#include <thread>

#include "prover_kernels.h"
#include "prover_plan.h"
#include "fq29.h"
#include "glv.h"
#include "pairing.h"
#include "poseidon.h"
#include "witness_ops.h"
#include "witness_lanes.h"
#include "witness_sched.h"
#include "fin29.h"
#include "merkle.h"
#include "quota_ledger.h"
#include "ffi_wire.h"   // secure_zero

namespace rlnamd {

const char* const kProverStageNames[PROVER_STAGES] = {"witness", "matvec", "ntt",      "recode",
                                                      "msm_g1",  "msm_g2", "finalize", "values"};

// =====================================================================================================
// host side
// =====================================================================================================
// Everything one in-flight batch owns.  Two slots let batch k+1 run its latency-bound front end (witness
// interpreter, NTT) and batch k-1 its back end (reduction, finalize) on their own streams while batch k
// keeps the chip busy with the MSM.
//
// What wipe_slot overwrites and Prover::residue_slot counts (field), and what neither touches (why):
//   digits / digits2                      counted [0] / [1]
//   abc                                   counted [2]
//   part1 grp1 sums1 prod tbl affA affB1  counted [3]
//   part2 grp2 sums2 affB2                counted [4]
//   inputs rs idx h_idx                   counted [5]  (with Impl::wgiven, the witness of upload_witness)
//   h_in: inputs | (r, s)                 counted [6]
//   h_hints                               counted [7]  (a1 = Poseidon(secret, external nullifier, message id) is a hint:
//                                                       with the proof's public (x, y), y - x a1 is the identity secret)
//   V29                                   counted [8]
//   V                                     wiped; tapped column by column through fetch_witness
//   err coords values comp h_comp h_values h_err   exempt: the results the caller receives
//   pp_in pp_out h_pp pp_pow, h_in: points         exempt: partial points (and powers of them), handed to the caller like a proof
//   h_cone                                exempt: entry numbers of the partial-proof cache
struct Slot {
  DevBuf<uint32_t> err, coords, values;
  DevBuf<uint8_t> comp;
  DevBuf<Fr> V, abc;
  DevBuf<uint4> V29;              // Fr29 interpreter: stored node values, [slot][proof][12 words]
  DevBuf<int16_t> digits, digits2;  // signed window digits under the G1 / G2 schedule
  DevBuf<G1XYZZ> part1, grp1, sums1, prod, tbl;
  DevBuf<G2XYZZ> part2, grp2, sums2;
  DevBuf<G1Affine> affA, affB1;
  DevBuf<G2Affine> affB2;
  DevBuf<uint32_t> pp_out;       // partial mode output, 320 B per proof
  uint32_t* h_pp = nullptr;
  int mode = 0;
  // streamed batches (Prover::submit): every slot owns its inputs, (r, s) and partial points plus the pinned staging
  // buffer they are copied from, so a caller with a stream of distinct batches never drains the pipeline
  DevBuf<uint32_t> inputs, rs, pp_in;
  uint8_t* h_in = nullptr;      // pinned staging: inputs | rs | partial points
  uint32_t* h_cone = nullptr;   // pinned: partial-cache entry of every proof of the batch (read by k_cone_save / _restore)
  uint32_t* h_hints = nullptr;  // pinned: the hints of a batch interpreted as segments (HINT_PROOFS x n_hints x 8 words)
  bool hinted = false;          // ... and this batch was; cleared once its hints have checked (Prover::collect)
  bool hints_staged = false;    // h_hints holds a batch's hints: until wipe_slot clears them
  hipEvent_t evU = nullptr;     // H2D of this slot's inputs done
  hipEvent_t evE = nullptr;     // small batches: the walk of the h-independent G1 rows done
  uint64_t ticket = 0;          // submit() ticket of the batch the slot holds (0: resident-input run)
  uint8_t* h_comp = nullptr;    // pinned: every run ends with the proofs + values copied to the host
  uint32_t* h_values = nullptr;
  uint32_t* h_err = nullptr;
  hipEvent_t evA = nullptr, evB = nullptr, evB2 = nullptr, evR = nullptr, evC = nullptr, evW = nullptr, evV = nullptr;
  hipEvent_t evX = nullptr;     // the witness is in V (before the small-batch recodes that follow it on the same stream)
  hipEvent_t evP = nullptr;     // fused finish: s pi_a + r rho is in `prod` (k_pp_smul)
  DevBuf<uint4> pp_pow;         // ... from the powers of pi_a, rho made at finish time when no cache entry holds them (<= 96 proofs)
  hipEvent_t t[15] = {};  // timing marks
  bool used = false;
  bool marked = false;          // the timing marks t[] of the slot's batch were recorded
  bool wiped = false;           // the batch's inputs and witness values have been overwritten (Prover::wipe)
  hipEvent_t evZ = nullptr;     // ... and that wipe has finished.  Kept apart from evC: "is the device idle" (lone) asks evC
  hipEvent_t free_event() const { return wiped ? evZ : evC; }   // what the slot's next user waits for
  size_t n = 0;
  // what the batch's walks used (wipe_slot): proof stride of the digit rows, stride and row counts of the partial sums
  uint32_t dB = 0, PB = 0, nch1 = 0, nch2 = 0;
  // a batch submitted by member (Prover::submit_members): the leaf indices, pinned and on the device -- who proves is a
  // secret as the inputs are -- and the event behind the gather that fills the path slots of `inputs`
  DevBuf<uint64_t> idx;
  uint64_t* h_idx = nullptr;
  hipEvent_t evT = nullptr, evG = nullptr;   // the tree's stream up to the gather; the gather done
  hipEvent_t evQ = nullptr;                  // a quota ledger's stream up to the write of the batch's drawn message ids
  bool members = false;
  bool drawn = false;           // ... with message ids drawn from a quota ledger: collect hands out no proof bytes for a refused row
  uint32_t seq = 0;             // the batch's sequence number (Impl::seq) and whether it took the big-batch streams
  bool big = false;             // (prover_plan.h: stream_plan): which stream its wipe goes to
};

// Provers alive per device, in this process.  `lone` (nothing of THIS prover in flight) lets a batch trade instructions for
// latency; the wide form of that trade -- a wave and a CU's LDS per proof for up to 1 024 proofs -- is only taken when no
// other prover shares the device: two provers proving alternating 1 024-proof batches each saw the other's batch as
// "lone" and lost a quarter of their common rate to it (14.6 k -> 10.7 k proofs/s, measured).
static std::atomic<int> g_provers_on_device[64];

// ... and in OTHER processes (round 6, VERDICT r5: "a second process on the device is not seen").  Every process that holds
// a prover on a device holds a READ record lock (fcntl, byte 0) on /dev/shm/rlnamd_<PCI bus id>.lock for as long as it
// does; F_GETLK for a write lock then names a conflicting holder only when ANOTHER process has one (a process's own record
// locks never conflict with it, and they vanish with the process: no stale counts).  Probed at most every 50 ms.
struct DeviceNeighbours {
  int fd = -1;
  void open_for(int dev) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    for (char* c = bus; *c; c++)
      if (*c == ':' || *c == '.') *c = '_';
    const std::string path = std::string("/dev/shm/rlnamd_") + bus + ".lock";
    fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
    if (fd < 0) return;
    (void)fchmod(fd, 0666);
    struct flock fl {};
    fl.l_type = F_RDLCK;
    fl.l_whence = SEEK_SET;
    fl.l_start = 0;
    fl.l_len = 1;
    if (fcntl(fd, F_SETLK, &fl) != 0) {
      ::close(fd);
      fd = -1;
    }
  }
  bool other_process() const {
    if (fd < 0) return false;
    struct flock fl {};
    fl.l_type = F_WRLCK;
    fl.l_whence = SEEK_SET;
    fl.l_start = 0;
    fl.l_len = 1;
    return fcntl(fd, F_GETLK, &fl) == 0 && fl.l_type != F_UNLCK;
  }
};
static std::mutex g_neigh_mu;
static DeviceNeighbours g_neigh[64];       // one descriptor per device and process (closing ANY descriptor of the file would
static int g_neigh_users[64];              // drop the process's record locks: the descriptor is shared by its provers)

struct DeviceCount {   // (a member of Impl: a constructor that throws half-way still gives its count back)
  int dev = -1;
  mutable std::chrono::steady_clock::time_point probed{};
  mutable bool other = false;
  DeviceCount() = default;
  DeviceCount(const DeviceCount&) = delete;
  DeviceCount& operator=(const DeviceCount&) = delete;
  void take() {
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) {
      dev = d;
      g_provers_on_device[d]++;
      std::lock_guard<std::mutex> lk(g_neigh_mu);
      if (g_neigh_users[d]++ == 0) g_neigh[d].open_for(d);
    }
  }
  bool other_process() const {
    if (dev < 0) return false;
    const auto now = std::chrono::steady_clock::now();
    if (now - probed > std::chrono::milliseconds(50)) {
      probed = now;
      std::lock_guard<std::mutex> lk(g_neigh_mu);
      other = g_neigh[dev].other_process();
    }
    return other;
  }
  bool shared() const { return dev >= 0 && (g_provers_on_device[dev] > 1 || other_process()); }
  ~DeviceCount() {
    if (dev < 0) return;
    g_provers_on_device[dev]--;
    std::lock_guard<std::mutex> lk(g_neigh_mu);
    if (--g_neigh_users[dev] == 0 && g_neigh[dev].fd >= 0) {
      ::close(g_neigh[dev].fd);
      g_neigh[dev].fd = -1;
    }
  }
};

struct Prover::Impl {
  hipStream_t sA = nullptr, sAb = nullptr, sA2 = nullptr, sB = nullptr, sB2 = nullptr, sC = nullptr;
  // EIGHT streams in all: ROCclr maps streams onto GPU_MAX_HW_QUEUES hardware queues (see common.cpp) and two streams
  // that share a queue serialise -- a ninth stream was measured as a 0.12 ms hole in the single-proof timeline.  A big
  // batch keeps all eight busy only where the process has eight queues; at four to seven, four (st / splan further down)
  hipStream_t sV = nullptr;   // proof values (24 chained Poseidon hashes per proof, latency-bound: ~17 ms of a 46 ms step)
  hipStream_t sW = nullptr;   // wipes: a stream of their own -- on sC a wipe would queue behind the back ends of every later
                              // batch, and the slot's next user would wait for all of them (measured: the pipeline drained)
  uint32_t seq = 0;  // batches enqueued: consecutive front ends alternate between sA and sAb
  // Big batches take their streams from the plan (prover_plan.h: stream_plan, by StreamId): eight of them busy with 8
  // hardware queues or more (wide), four at 4 .. 7 queues (compact).  Small batches take the streams named in enqueue either way.
  hipStream_t st[ST_COUNT] = {};
  StreamPlan splan;
  float ms[PROVER_STAGES] = {0};
  DevBuf<unsigned long long> walk_clk;  // clock tap of the two walks: G1 cycles, G1 ticks, G2 cycles, G2 ticks
  ProverTuning tune;             // every switch, read once (prover.h)
  DeviceCount device;            // counted in g_provers_on_device while the object lives
  DevBuf<GNode29> nodes29;
  DevBuf<uint32_t> consts29, slot2node;
  WitLanes witlanes;             // lanes = independent nodes: the interpreter of batches walked with lanes = chunks
  uint32_t nstore29 = 0, nprog29 = 0;   // stored values, program nodes (after fusion)

  uint32_t N = 0, NS = 0, NI = 0, nc = 0, ni = 0, n = 0;
  int logn = 0;
  DevBuf<uint32_t> sig2node;     // witness signal -> its row of V (the node's row; a row behind them for a later signal of an aliased node)
  DevBuf<uint32_t> alias_src, alias_dst;
  uint32_t n_alias = 0;
  DevBuf<uint32_t> a_ptr, a_col, b_ptr, b_col;
  DevBuf<uint32_t> mv_long;       // rows with more than MV_LONG entries in A or B
  uint32_t n_mv_long = 0;
  DevBuf<Fr> a_coef, b_coef;
  DevBuf<Fr> tw_f, tw_i, coset;
  DevBuf<uint32_t> tw_f29, tw_i29, coset29;   // the same tables for the passes of the big batches (NttTables)
  std::vector<NttPass> ntt_passes;   // the launches of the transforms with lanes = proofs (prover_plan.h)
  // MSM: the comb tables in the packed 9 x 29-bit form (one 64-byte line per G1 entry)
  DevBuf<G1Affine29> t1_29;
  DevBuf<G2Affine29> t2_29;
  DevBuf<uint32_t> sid1, sid2;
  // a walk = a list of table rows cut into chunks, plus the two-level reduction ranges; one per mode
  struct Plan {   // a WalkPlan (prover_plan.h) on the device, field by field
    DevBuf<uint32_t> rows, rsid, early_ids, late_ids, prows, prsid, pout;
    DevBuf<ChunkDesc> chunks, groups, segs, segchunks, segblocks, pchunks;
    uint32_t nchunks = 0, ngroups = 0, nseg = 0, n_early = 0, n_late = 0, npchunks = 0, nblocks = 0, maxblk = 0;
    void upload(const WalkPlan& W, hipStream_t s) {   // (waits for the copies: W may be a temporary)
      nchunks = (uint32_t)W.chunks.size();
      ngroups = (uint32_t)W.groups.size();
      nseg = W.nseg;
      n_early = (uint32_t)W.early_ids.size();
      n_late = (uint32_t)W.late_ids.size();
      npchunks = (uint32_t)W.pchunks.size();
      nblocks = W.nblocks;
      maxblk = W.maxblk;
      rows.assign(W.rows, s);
      rsid.assign(W.rsid, s);
      chunks.assign(W.chunks, s);
      groups.assign(W.groups, s);
      segs.assign(W.segs, s);
      segchunks.assign(W.segchunks, s);
      segblocks.assign(W.segblocks, s);
      early_ids.assign(W.early_ids, s);
      late_ids.assign(W.late_ids, s);
      if (npchunks) {
        prows.assign(W.prows, s);
        prsid.assign(W.prsid, s);
        pout.assign(W.pout, s);
        pchunks.assign(W.pchunks, s);
      }
      RLN_HIP(hipStreamSynchronize(s));
    }
  };
  // [WalkPlanKind][PROVE_FULL, PROVE_PARTIAL, PROVE_FINISH] (prover_plan.h).  PLAN_BIG: the throughput plans.  PLAN_SMALL:
  // the same walks cut into shorter chunks for batches walked with lanes = chunks: a walk lasts as long as its longest
  // chunk (a lane's serial chain of additions), and a handful of proofs cannot fill the chip anyway.  PLAN_FUSED (G1,
  // full and finish): s A and r B1 as rows of the C segment.  PLAN_TINY (<= tune.tiny_max proofs, alone on the device):
  // ONE (row, half) per lane -- a lane's chain is 9 (G1) or 8 (G2) additions instead of 36 / 16 -- and the partial sums,
  // four times as many, meet in a two-stage tree; its G1 plan is the fused one except for a partial proof.
  Plan plan1[4][3], plan2[4][3];
  uint32_t max_chunks1t = 0, max_chunks2t = 0, max_blocks1t = 0, max_blocks2t = 0;
  uint32_t max_chunks1s = 0, max_chunks2s = 0, small_stride = 64;   // partial sums of a small batch: [chunk][64]
  uint32_t max_chunks1 = 0, max_chunks2 = 0, max_groups1 = 0, max_groups2 = 0;
  uint32_t npts1 = 0, npts2 = 0, npaired1 = 0;   // npaired1: G1 points [0, npaired1) are pair members
  uint32_t nseg1_big = G1_SEGS, nwalked1 = 0;    // PLAN_BIG of the G1 walk: output segments; table rows a full proof walks (tune.shared_rows)
  std::vector<uint8_t> known;  // per witness signal: computable from the partial witness (evaluate_partial)
  // ---- the graph as independent segments behind hints (witness_sched.h: wl_segments; Prover::enqueue): the values between
  //      the circuit's chained hashes are computed on a host core (HintChains: depth + 2 Poseidon hashes, ~0.3 ms), every
  //      segment of the graph is interpreted at once on the device with them as extra inputs, and every cut node's own value
  //      is compared with its hint afterwards (k_hint_check -> WERR_HINT -> the batch is run again over the whole graph)
  WitSegs segs;
  DevBuf<uint32_t> cut_node, cut_hint;
  uint32_t n_cut = 0, n_hints = 0;
  uint64_t hinted_batches = 0, hint_fallbacks = 0;
  bool no_hints_now = false;     // set around the re-run of a batch whose hints did not check
  int rerun_slot = -1;           // ... with the slot the batch has: the re-run takes it again, not the next of the ring
  HintChains hints;              // their hashing on the host, with the cache of remembered chains (prover_plan.h)
  // ---- the partial-proof cache and the cone program (prover.h: collect_partial_cached / submit_finish)
  WitLanes cone;                 // the unknown cone of evaluate_partial, scheduled like the full graph (witness_sched.h: wl_cone)
  uint32_t cone_nodes = 0;
  DevBuf<uint32_t> cone_rows;    // stored slots of the KNOWN nodes: what an entry keeps
  uint32_t cone_nk = 0, cone_cap = 0;
  uint32_t cone_stride = 0;      // uint4 units per entry: cone_nk * 3 of stored values, then PP_POWERS16 of powers (fin29.h)
  DevBuf<uint4> cone_cache;      // [entry][cone_stride]
  DevBuf<uint32_t> iota96;       // 0 .. 95: "entry p of proof p" for the per-slot powers of a finish without cache entries
  std::vector<uint32_t> cone_gen, cone_free;   // generation per entry (a stale handle is refused); free list
  std::vector<uint8_t> cone_live;
  hipEvent_t evConeSaved = nullptr;   // sW: the last save / wipe of entries
  hipEvent_t evConeRead = nullptr, evConeRead2 = nullptr;   // the last read of entries: k_cone_restore (front-end stream), k_pp_smul (sC)
  uint64_t cone_batches = 0;
  // handle = prover tag (20 bits, unique per Prover of the process: another prover's handle must not alias an entry here)
  //          | generation of the entry (20 bits) | entry index + 1 (24 bits)
  uint32_t cone_tag = 0;
  uint64_t cone_handle(uint32_t e) const {
    return ((uint64_t)cone_tag << 44) | ((uint64_t)(cone_gen[e] & 0xFFFFFu) << 24) | (uint64_t)(e + 1);
  }
  uint32_t cone_entry(uint64_t h) const {   // NONE when the handle is not a live entry of THIS prover
    const uint32_t idx = (uint32_t)(h & 0xFFFFFFu), gen = (uint32_t)((h >> 24) & 0xFFFFFu), tag = (uint32_t)(h >> 44);
    if (tag != cone_tag || idx == 0 || idx > cone_cap || !cone_live[idx - 1] || (cone_gen[idx - 1] & 0xFFFFFu) != gen) return 0xFFFFFFFFu;
    return idx - 1;
  }
  DevBuf<uint32_t> pp_in;      // resident partial-proof points for finish mode, 320 B per proof
  DevBuf<uint32_t> wgiven;     // externally calculated witnesses for the next run (upload_witness), else empty
  size_t wgiven_n = 0;
  InputSlots slots{};
  bool have_path_slots = false;           // the graph names pathElements and identityPathIndex (submit_members)
  uint32_t path_off = 0, path_idx_off = 0;
  bool have_drawn_slots = false;          // ... and userMessageLimit, externalNullifier and ONE messageId (submit_members_drawn)
  uint32_t drawn_msg_off = 0;
  // ... or messageId[max_out] and selectorUsed[max_out] (submit_members_drawn_counts; no selectors on a single message-id graph)
  bool have_drawn_multi_slots = false, drawn_sel = false;
  uint32_t drawn_multi_msg_off = 0, drawn_multi_sel_off = 0, drawn_multi_slots = 1;
  bool have_values_kernel = false;
  // resident inputs (shared by both slots; upload() drains the pipeline first)
  DevBuf<uint32_t> inputs, rs;
  static constexpr int NSLOT = 6;
  Slot slot[NSLOT];
  int nslot = 5;                // Tuning::slots
  WinSched ws{}, ws2{};         // window schedules of the G1 and G2 comb tables
  static constexpr uint32_t nh = GLV_HALVES;  // halves per scalar: the GLV split k1 + lambda k2 (glv.h)
  int cur = 0;
  Slot* last = nullptr;
  uint64_t tickets = 0;         // submit() tickets handed out

  // Overwrites what batch `S` knew about its witnesses (see k_wipe_cols): the slot's staged inputs (pinned host + device),
  // its (r, s) and the witness values, on the back-end stream behind the batch's last reader; evC is recorded again, so
  // whoever reuses the slot -- or reads the resident inputs next -- waits for the wipe as well.
  size_t batch_cap = 0;   // = Prover::B_
  void mark_drawn(uint64_t ticket) {   // the batch behind `ticket` carries message ids drawn from a quota ledger
    for (int k = 0; k < nslot; k++)
      if (slot[k].used && slot[k].ticket == ticket && ticket != 0) slot[k].drawn = true;
  }
  void wipe_slot(Slot& S, bool resident) {
    const size_t n = S.n ? S.n : batch_cap;
    const size_t B = batch_cap;
    if (!n) return;
    // compact: the wipe of a big batch's slot goes to the front-end stream of the slot's next batch -- wipe and reuse in
    // stream order (the slot's evZ is recorded all the same: a small batch, or a caller that collects out of order, may
    // be the next user)
    hipStream_t sW = (S.big && splan.shape == SHAPE_COMPACT) ? st[splan.at[S.seq & 1][ROLE_WIPE]] : this->sW;
    RLN_HIP(hipStreamWaitEvent(sW, S.evC, 0));
    // (away from the wipes' own stream: behind the save of the batch's cache entries, which reads the witness there)
    if (sW != this->sW && evConeSaved) RLN_HIP(hipStreamWaitEvent(sW, evConeSaved, 0));
    // contiguous ranges are gathered and go out sixteen to a launch (k_wipe_ranges): a lone proof's collect used to make a
    // dozen launches for as many tiny buffers before it returned
    WipeRanges WR{};
    auto flush = [&]() {
      if (!WR.count) return;
      hipLaunchKernelGGL(k_wipe_ranges, dim3(WR.first[WR.count]), dim3(64), 0, sW, WR);
      WR.count = 0;
    };
    auto zero = [&](void* dst, size_t bytes) {   // multiples of 32 bytes (a kernel: no copy-engine / blit path in the pipeline)
      if (!bytes) return;
      if (WR.count == 16) flush();
      if (WR.count == 0) WR.first[0] = 0;
      WR.p[WR.count] = (uint4*)dst;
      WR.n16[WR.count] = (uint32_t)(bytes / 16);
      WR.first[WR.count + 1] = WR.first[WR.count] + (uint32_t)div_up(bytes / 16, 256);
      WR.count++;
    };
    if (resident) {
      zero(inputs.p, std::min(inputs.bytes(), n * (size_t)NI * 32));
      zero(rs.p, std::min(rs.bytes(), n * 64));
      if (wgiven.p) zero(wgiven.p, wgiven.bytes());
      wgiven_n = 0;
    } else {
      // pinned staging: plain stores followed by a compiler barrier that keeps them (explicit_bzero semantics)
      memset(S.h_in, 0, n * (size_t)NI * 32);
      memset(S.h_in + B * (size_t)NI * 32, 0, n * 64);
      __asm__ __volatile__("" : : "r"(S.h_in) : "memory");
      if (S.hints_staged) {   // the values between the chained hashes: the first of them gives the secret away (see Slot)
        memset(S.h_hints, 0, (size_t)HINT_PROOFS * 64 * 32);
        __asm__ __volatile__("" : : "r"(S.h_hints) : "memory");
        S.hints_staged = false;
      }
      zero(S.inputs.p, n * (size_t)NI * 32);
      zero(S.rs.p, n * 64);
      if (S.members) {   // the leaf indices of a batch submitted by member
        memset(S.h_idx, 0, B * 8);
        __asm__ __volatile__("" : : "r"(S.h_idx) : "memory");
        zero(S.idx.p, S.idx.bytes());
        S.members = false;
      }
    }
    const uint32_t pg = div_up(n, 64);
    const size_t np = std::min<size_t>(B, (n + 63) / 64 * 64);   // the padding lanes of the last wave wrote their columns too
    hipLaunchKernelGGL(k_wipe_cols, dim3(pg, nstore29), dim3(64), 0, sW, S.V.p, slot2node.p, nstore29, (uint32_t)B, (uint32_t)n);
    hipLaunchKernelGGL(k_wipe_v29, dim3(div_up(3 * np, 64), nstore29 + 1), dim3(64), 0, sW, S.V29.p, nstore29 + 1, (uint32_t)B,
                       (uint32_t)np);
    // an externally supplied witness (upload_witness) was stored at the signal rows
    hipLaunchKernelGGL(k_wipe_cols, dim3(pg, NS), dim3(64), 0, sW, S.V.p, sig2node.p, NS, (uint32_t)B, (uint32_t)n);
    // The signed window digits are a lossless re-encoding of every witness scalar (the identity secret among them) and
    // of r, s; A w, B w and the quotient are linear images of the witness; a walk's partial sum over a handful of rows is
    // w_i P_i for guessable w_i.  Columns [0, n) of all of them, by the strides the batch used.
    auto rows16 = [&](void* base, size_t nrows, size_t stride16, size_t n16) {
      if (!base || !nrows || !n16) return;
      hipLaunchKernelGGL(k_wipe_rows16, dim3(div_up(n16, 64), nrows), dim3(64), 0, sW, (uint4*)base, (uint32_t)nrows,
                         (uint32_t)stride16, (uint32_t)std::min(n16, stride16));
    };
    const size_t dB = S.dB ? S.dB : B;
    for (DevBuf<int16_t>* d : {&S.digits, &S.digits2}) {
      if (!d->p) continue;
      const size_t drows = d->n / B;
      if (dB == B) rows16(d->p, drows, B / 8, np / 8);                            // [row][B] int16
      else zero(d->p, std::min(d->bytes(), (drows * dB * 2 + 31) / 32 * 32));     // compact rows: contiguous
    }
    rows16(S.abc.p, S.abc.n / B, B * 2, np * 2);                                  // [3 n_constraints][B] x 32 bytes
    const size_t PB = S.PB ? S.PB : B;
    rows16(S.part1.p, S.PB ? S.nch1 : S.part1.n / PB, PB * (sizeof(G1XYZZ) / 16), std::min(np, PB) * (sizeof(G1XYZZ) / 16));
    rows16(S.part2.p, S.PB ? S.nch2 : S.part2.n / PB, PB * (sizeof(G2XYZZ) / 16), std::min(np, PB) * (sizeof(G2XYZZ) / 16));
    // what the sums leave behind: block sums of the same partials, the UNBLINDED A / B / C sums (with the
    // public proof they give r delta and s delta), the affine A / B1 / B2, the ladder's products and tables.  A few MB:
    // whole buffers, whatever shape the batch had.
    auto whole = [&](auto& buf) { if (buf.p) zero(buf.p, buf.bytes() / 32 * 32); };
    whole(S.grp1); whole(S.grp2); whole(S.sums1); whole(S.sums2); whole(S.prod); whole(S.tbl);
    whole(S.affA); whole(S.affB1); whole(S.affB2);
    flush();
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(S.evZ, sW));
    S.wiped = true;
  }

  // what batch_shape asks about a batch of n proofs in `mode` (the caller adds what it brings: points, handles, hints)
  BatchQuery query(size_t n, int mode, bool streamed) {
    BatchQuery q;
    q.n = n;
    q.mode = mode;
    q.inputs = streamed;
    q.partial_points = false;
    q.handles = false;
    q.pre_hints = false;
    // nothing of this prover in flight?  (asked only where the answer decides `lone`)
    q.idle = tune.lone >= 0 || n <= tune.lone_small_max || !last || hipEventQuery(last->evC) == hipSuccess;
    (void)hipGetLastError();   // hipErrorNotReady is not an error here
    q.shared = device.shared();
    q.no_hints_now = no_hints_now;
    q.witlanes_ok = witlanes.ok;
    q.segs_ok = segs.ok;
    q.cone_ok = cone.ok;
    q.have_values_kernel = have_values_kernel;
    q.ni = ni;
    q.logn = logn;
    q.capacity = batch_cap;
    q.small_stride = small_stride;
    q.compact = splan.shape == SHAPE_COMPACT;
    return q;
  }

  void sync_all() {
    RLN_HIP(hipStreamSynchronize(sA));
    RLN_HIP(hipStreamSynchronize(sAb));
    RLN_HIP(hipStreamSynchronize(sV));
    RLN_HIP(hipStreamSynchronize(sA2));
    RLN_HIP(hipStreamSynchronize(sB));
    if (sB2) RLN_HIP(hipStreamSynchronize(sB2));
    RLN_HIP(hipStreamSynchronize(sC));
    RLN_HIP(hipStreamSynchronize(sW));
  }
};

// waits for `ev` with the calling thread asleep between polls (50 us: 0.1 % of a 45 ms batch)
static void wait_yielding(hipEvent_t ev) {
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return;
    (void)hipGetLastError();   // hipErrorNotReady is not an error here
    if (e != hipErrorNotReady) RLN_HIP(e);
    struct timespec ts = {0, 50000};
    nanosleep(&ts, nullptr);
  }
}

static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

// The environment is read HERE and nowhere else in the prover, once per Prover (getenv is not safe against a concurrent
// setenv, and a switch that flips between two reads inside one enqueue would give a batch with inconsistent shapes).
ProverTuning ProverTuning::from_env() {
  ProverTuning t;
  t.window_bits = env_int("RLNAMD_WINDOW_BITS", t.window_bits);
  t.slots = env_int("RLNAMD_SLOTS", t.slots);
  t.lanechunk_max = (uint32_t)std::max(0, env_int("RLNAMD_LANECHUNK", (int)t.lanechunk_max));
  t.lanechunk_walk_max = (uint32_t)std::max(0, env_int("RLNAMD_LANECHUNK_WALK", (int)t.lanechunk_walk_max));
  t.witlanes_max = (uint32_t)std::max(0, env_int("RLNAMD_WITLANES_MAX", (int)t.witlanes_max));
  t.lone = env_int("RLNAMD_LONE", -1);
  t.lone_small_max = (uint32_t)std::max(0, env_int("RLNAMD_LONE_SMALL", (int)t.lone_small_max));
  t.tiny_max = (uint32_t)std::max(0, env_int("RLNAMD_TINY", (int)t.tiny_max));
  t.ntt_lg_max = (uint32_t)std::max(0, env_int("RLNAMD_NTT_LG_MAX", (int)t.ntt_lg_max));
  t.partial_cache = (uint32_t)std::max(0, env_int("RLNAMD_PARTIAL_CACHE", (int)t.partial_cache));
  t.hint_max = (uint32_t)std::min<int>(std::max(0, env_int("RLNAMD_HINTS", (int)t.hint_max)), (int)HINT_PROOFS);
  t.hint_fault = env_int("RLNAMD_HINT_FAULT", 0);
  {
    const int shape = stream_shape_from_name(getenv("RLNAMD_STREAM_SHAPE"));
    t.stream_shape = shape >= 0 ? shape : SHAPE_AUTO;
    t.hw_queues = hw_queues_from_env(getenv("GPU_MAX_HW_QUEUES"));   // read, never set: the host program's to choose
  }
  t.shared_rows = env_int("RLNAMD_SHARED_ROWS", t.shared_rows) != 0;
  t.verify_lanes = env_int("RLNAMD_VERIFY_LANES", 0);
  if (t.verify_lanes != 1 && t.verify_lanes != 8) t.verify_lanes = 0;
  {   // (at most half of the host's hardware threads unless the switch says otherwise)
    const unsigned hw = std::thread::hardware_concurrency();
    const int dflt = hw ? (int)std::min<unsigned>(t.hint_threads, std::max(1u, hw / 2)) : (int)t.hint_threads;
    t.hint_threads = (uint32_t)std::min(std::max(1, env_int("RLNAMD_HINT_THREADS", dflt)), 64);
  }
  t.hint_max_warm = (uint32_t)std::min<int>(std::max(0, env_int("RLNAMD_HINTS_WARM", (int)t.hint_max_warm)), (int)HINT_PROOFS);
  t.hint_chains = (uint32_t)std::min(std::max(0, env_int("RLNAMD_HINT_CHAINS", (int)t.hint_chains)), 1024);
  return t;
}
std::string ProverTuning::describe() const {
  char b[768];
  snprintf(b, sizeof b,
           "window_bits=%d slots=%d lanechunk=%u lanechunk_walk=%u witlanes_max=%u tiny=%u ntt_lg_max=%u partial_cache=%u lone=%d "
           "lone_small=%u hints=%u hints_warm=%u hint_threads=%u hint_chains=%u verify_lanes=%d stream_shape=%s hw_queues=%d "
           "shared_rows=%d",
           window_bits, slots, lanechunk_max, lanechunk_walk_max, witlanes_max, tiny_max, ntt_lg_max, partial_cache, lone,
           lone_small_max, hint_max, hint_max_warm, hint_threads, hint_chains, verify_lanes, stream_shape_name(stream_shape), hw_queues,
           shared_rows);
  return b;
}
const ProverTuning& Prover::tuning() const { return d_->tune; }
int Prover::device_shared() const { return (d_->device.dev >= 0 && g_provers_on_device[d_->device.dev] > 1 ? 1 : 0) | (d_->device.other_process() ? 2 : 0); }

// G1 table in the 9 x 29 form: slabs are built in the 8 x 32 form (k_table_build reads its own rows back) and
// converted into place
// where the constructor's time goes (Prover::init_ms): [0] parsing the arkzkey / graph + the verifier's precomputation,
// [1] hipMalloc of the comb tables, [2] building them (k_table_build / k_table_to29 + the wait), [3] everything else
// (plans, constants, the workspaces of every slot, pinned staging)
static thread_local float g_init_ms[4];
static float ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
template <class F, class Entry>
static void build_table29(const std::vector<Affine<F>>& pts, const WinSched& ws, DevBuf<Entry>& table, hipStream_t s,
                          uint32_t npaired = 0) {
  size_t npts = pts.size();
  const size_t stride = ws.stride;
  auto t_alloc = std::chrono::steady_clock::now();
  table.alloc(npts * stride);
  g_init_ms[1] += ms_since(t_alloc);
  auto t_build = std::chrono::steady_clock::now();
  DevBuf<Affine<F>> d_pts(npts);
  d_pts.upload(pts.data(), npts, s);
  size_t per_pt = stride / 2 * sizeof(F);
  size_t slab = std::max<size_t>(2, (((size_t)4 << 30) / per_pt) & ~(size_t)1);   // even: a pair never straddles two slabs
  slab = std::min(slab, (npts + 1) & ~(size_t)1);
  DevBuf<F> scratch(slab * stride / 2);
  DevBuf<Affine<F>> tmp(slab * stride);
  for (size_t k0 = 0; k0 < npts; k0 += slab) {
    size_t cnt = std::min(slab, npts - k0);
    const size_t nrows = cnt * ws.W;   // a wave per (point, window) row
    hipLaunchKernelGGL(k_table_build<F>, dim3((unsigned)nrows), dim3(64), 0, s, d_pts.p + k0, (uint32_t)cnt, ws, tmp.p,
                       scratch.p);
    hipLaunchKernelGGL((k_table_to29<Affine<F>, Entry>), dim3(div_up(cnt * stride, 256)), dim3(256), 0, s, tmp.p,
                       table.p + k0 * stride, cnt * stride, (uint32_t)stride, (uint32_t)k0, npaired);
    RLN_HIP(hipGetLastError());
  }
  RLN_HIP(hipStreamSynchronize(s));
  g_init_ms[2] += ms_since(t_build);
}

Prover::Prover(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len, ProverConfig cfg)
    : d_(new Impl) {
  require_gpu();
  d_->device.take();
  const auto t_ctor = std::chrono::steady_clock::now();
  for (float& v : g_init_ms) v = 0;
  zk_ = parse_arkzkey(zkey, zkey_len);
  graph_ = parse_graph(graph, graph_len);
  (void)prepared(zk_);  // verifier precomputation now, so concurrent verify calls only read it
  g_init_ms[0] = ms_since(t_ctor);
  Impl& D = *d_;
  // window_bits = g1 + 10000 * g2, each spec = c + 100 * wide: c-bit windows, the first `wide` of them (c + 1)-bit
  // (see WinSched); g2 = 0: the G2 table takes the G1 schedule.  The windows cover the 127-bit halves of the GLV split:
  // spec 114 = 15 + 8 x 14 bits, 9 windows, 18 additions per G1 point; spec 715 = 7 x 16 + 15 bits, 8 windows, 16
  // additions per G2 point.
  D.tune = ProverTuning::from_env();
  if (cfg.stream_shape >= SHAPE_AUTO && cfg.stream_shape <= SHAPE_COMPACT) D.tune.stream_shape = cfg.stream_shape;
  if (cfg.shared_rows >= 0) D.tune.shared_rows = cfg.shared_rows != 0;
  const int wb = cfg.window_bits > 0 ? cfg.window_bits : D.tune.window_bits;
  D.tune.window_bits = wb;
  const int spec1 = wb % 10000, spec2 = wb / 10000 ? wb / 10000 : spec1;
  c_ = spec1 % 100;
  const int wide = spec1 / 100;
  D.ws = make_sched(c_, wide);
  D.ws2 = make_sched(spec2 % 100, spec2 >= 100 ? spec2 / 100 : (wb / 10000 ? 0 : wide));
  W_ = D.ws.W * D.nh;
  c2_ = spec2 % 100;
  W2_ = D.ws2.W * D.nh;
  B_ = ((cfg.max_batch ? cfg.max_batch : 1) + 63) / 64 * 64;
  D.batch_cap = B_;

  // ---- consistency between zkey and graph (what arkworks asserts inside the prover)
  D.N = (uint32_t)graph_.nodes.size();
  D.NS = (uint32_t)graph_.signals.size();
  D.NI = graph_.inputs_size;
  D.nc = (uint32_t)zk_.num_constraints;
  D.ni = (uint32_t)zk_.num_instance_variables;
  if (zk_.a_query.size() != D.NS || zk_.b_g1_query.size() != D.NS || zk_.b_g2_query.size() != D.NS)
    throw Error("zkey/graph mismatch: query length != number of witness signals");
  if (zk_.gamma_abc_g1.size() != D.ni || zk_.l_query.size() + D.ni != D.NS)
    throw Error("MalformedVerifyingKey: instance/aux split does not match the witness length");
  uint32_t dom = 1;
  D.logn = 0;
  while (dom < D.nc + D.ni) {
    dom <<= 1;
    D.logn++;
  }
  D.n = dom;
  if (D.logn < 1 || D.logn > 27) throw Error("PolynomialDegreeTooLarge");
  if (zk_.h_query.size() < D.n) throw Error("zkey h_query shorter than the evaluation domain");

  {
    // the short latency-bound stages get the high-priority queues so their few waves are dispatched ahead
    // of the MSM's thousands of workgroups
    int lo = 0, hi = 0;
    RLN_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    // sW FIRST: kernels on the first stream a process creates run ~70 us slower each on this stack (kernel trace of single
    // proofs: 0.085 against 0.006 ms for k_v29_to_fr, every NTT pass 0.08 against 0.016 ms -- every second proof, the ones
    // whose front end landed there, took 3.3 instead of 2.8 ms); the wipes do not care
    RLN_HIP(hipStreamCreateWithPriority(&D.sW, hipStreamNonBlocking, hi));
    RLN_HIP(hipStreamCreateWithPriority(&D.sA, hipStreamNonBlocking, hi));
    RLN_HIP(hipStreamCreateWithPriority(&D.sA2, hipStreamNonBlocking, hi));
    RLN_HIP(hipStreamCreateWithPriority(&D.sAb, hipStreamNonBlocking, hi));
    RLN_HIP(hipStreamCreateWithPriority(&D.sV, hipStreamNonBlocking, hi));
    RLN_HIP(hipStreamCreateWithPriority(&D.sB, hipStreamNonBlocking, lo));
    RLN_HIP(hipStreamCreateWithPriority(&D.sC, hipStreamNonBlocking, hi));
    D.nslot = std::min(std::max(D.tune.slots, 2), (int)Impl::NSLOT);
    D.splan = stream_plan(D.tune.hw_queues, D.nslot, D.tune.stream_shape);
    D.tune.stream_shape = D.splan.shape;
    D.walk_clk.alloc(4);
    RLN_HIP(hipMemset(D.walk_clk.p, 0, 4 * sizeof(unsigned long long)));
    // the G1 walk is ~12 rounds of 2.8 ms workgroups: on one stream its last round leaves SIMDs idle until the G2
    // walk may start; on two streams the walks of neighbouring batches fill each other's tails (+3.3 - 3.7 % measured)
    RLN_HIP(hipStreamCreateWithPriority(&D.sB2, hipStreamNonBlocking, lo));
    D.st[ST_W] = D.sW; D.st[ST_A] = D.sA; D.st[ST_A2] = D.sA2; D.st[ST_AB] = D.sAb;
    D.st[ST_V] = D.sV; D.st[ST_B] = D.sB; D.st[ST_C] = D.sC; D.st[ST_B2] = D.sB2;
  }
  hipStream_t s = D.sB;

  RLN_HIP(hipFuncSetAttribute((const void*)(k_sum_tree<Fq2, G2Acc29>), hipFuncAttributeMaxDynamicSharedMemorySize, SUM_TREE_LDS_G2));
  RLN_HIP(hipFuncSetAttribute((const void*)(k_sum_blocks<Fq2, G2Acc29>), hipFuncAttributeMaxDynamicSharedMemorySize, SUM_TREE_LDS_G2));
  // k_witness29 takes 152 KiB of dynamic LDS; gfx950, the only target, gives a workgroup 160 KiB
  RLN_HIP(hipFuncSetAttribute((const void*)k_witness29<false>, hipFuncAttributeMaxDynamicSharedMemorySize, WIT29_LDS_BYTES));
  // Largest batch that takes the small-batch shapes (lanes = chunks walks, a wave per proof in the interpreter, early walks
  // and back end).  tools/lanechunk_sweep.py / tools/midstream.py: one batch alone is faster that way up to ~450 proofs
  // (64: 12.4 vs 23.2 ms, 128: 17.8 vs 27.4, 256: 28.4 vs 36.8), a STREAM of such batches up to ~150 (chunks of 64: 9.4 k
  // vs 8.1 k proofs/s, 128: equal, 256: 10.1 k vs 12.1 k) -- 128 wins or ties on both.
  // partial sums of a small batch: [chunk][stride]
  D.small_stride = std::max<uint32_t>(64, (std::min<uint32_t>(D.tune.lanechunk_max, (uint32_t)B_) + 63) / 64 * 64);
  // ---- named input slots: the proof-values kernel and the hints need them
  const NamedInputs named = find_named_inputs(graph_, D.ni);
  D.slots = named.slots;
  D.have_values_kernel = named.have_values_kernel;
  D.have_path_slots = named.have_path_slots;
  D.path_off = named.path_off;
  D.path_idx_off = named.path_idx_off;
  D.have_drawn_slots = named.have_drawn_slots;
  D.drawn_msg_off = named.drawn_msg_off;
  D.have_drawn_multi_slots = named.have_drawn_multi_slots;
  D.drawn_sel = named.drawn_sel;
  D.drawn_multi_msg_off = named.drawn_multi_msg_off;
  D.drawn_multi_sel_off = named.drawn_multi_sel_off;
  D.drawn_multi_slots = named.drawn_multi_slots;
  D.hints.configure(named, D.tune.hint_chains);
  // ---- where the graph can be cut (segments behind hints; find_hint_cuts): a circuit on which a hint matches no node
  //      keeps the whole-graph interpreter
  std::vector<std::vector<uint32_t>> hint_cuts;
  std::vector<uint8_t> is_cut(D.N, 0);
  if (named.have_hint_slots && D.tune.hint_max > 0 && D.hints.count() <= 64) {
    hint_cuts = find_hint_cuts(graph_, named, D.hints);
    if (!hint_cuts.empty()) D.n_hints = D.hints.count();
    for (const auto& nodes : hint_cuts)
      for (uint32_t n : nodes) is_cut[n] = 1;
  }
  // ---- the program of k_witness29 and the compact array of stored values (compile_witness29)
  const Wit29Program W29 = compile_witness29(graph_, is_cut);
  D.nprog29 = W29.nprog;
  D.nstore29 = (uint32_t)W29.slot2node.size();
  D.nodes29.assign(W29.prog, s);
  D.slot2node.assign(W29.slot2node, s);
  D.consts29.alloc(std::max<size_t>(graph_.constants.size(), 1) * 9);
  {
    DevBuf<Fr> consts;   // the constants in Fr form, for the conversion only
    if (!graph_.constants.empty()) {
      consts.assign(graph_.constants, s);
      hipLaunchKernelGGL(k_consts_to29, dim3(div_up(graph_.constants.size(), 256)), dim3(256), 0, s, consts.p,
                         D.consts29.p, (uint32_t)graph_.constants.size());
    }
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipStreamSynchronize(s));
  }
  // the same stored values, produced by a wave per proof (witness_lanes.h) when a batch is below a wave of proofs
  D.witlanes.build(graph_, W29.store_slot, D.nstore29, s);   // V29 has one row more than stored values
  if (D.witlanes.ok && !hint_cuts.empty()) {
    const WlSegments SG = wl_segments(graph_, hint_cuts);
    D.segs.build(SG, W29.store_slot, D.nstore29, s);
    // worth it only where the cuts really shorten the program (the shipped circuits: 381 of 4 813 steps)
    if (D.segs.ok && (D.segs.max_steps * 4 > D.witlanes.nsteps || D.segs.nseg > 256)) D.segs.ok = false;
    if (D.segs.ok) {
      D.n_cut = (uint32_t)SG.cut_nodes.size();
      D.cut_node.assign(SG.cut_nodes, s);
      D.cut_hint.assign(SG.cut_hint, s);
      RLN_HIP(hipStreamSynchronize(s));
    }
  }
  // One row of V per witness SIGNAL.  Signals that alias one graph node (the multi-message-id circuit: six nodes under
  // four signals each) hold one value in a calculated witness, but a supplied one (upload_witness) may give each its own,
  // and the reference reads the assignment by signal: the later signals of such a node get rows of their own behind the
  // nodes' rows, filled from the node's row behind the interpreter (k_alias_rows) and overwritten by a supplied witness.
  std::vector<uint32_t> sig_row = graph_.signals;
  {
    std::vector<uint8_t> taken(D.N, 0);
    std::vector<uint32_t> src, dst;
    for (uint32_t j = 0; j < D.NS; j++) {
      const uint32_t node = graph_.signals[j];
      if (taken[node]) {
        sig_row[j] = D.N + (uint32_t)dst.size();
        src.push_back(node);
        dst.push_back(sig_row[j]);
      }
      taken[node] = 1;
    }
    D.n_alias = (uint32_t)dst.size();
    if (D.n_alias) {
      D.alias_src.assign(src, s);
      D.alias_dst.assign(dst, s);
    }
  }
  D.sig2node.assign(sig_row, s);

  // ---- matrices as CSR over graph node ids
  auto csr = [&](const std::vector<SparseRow>& m, DevBuf<uint32_t>& ptr, DevBuf<uint32_t>& col, DevBuf<Fr>& coef) {
    std::vector<uint32_t> hp(D.nc + 1, 0), hc;
    std::vector<Fr> hv;
    for (uint32_t r = 0; r < D.nc; r++) {
      for (size_t k = 0; k < m[r].col.size(); k++) {
        hc.push_back(sig_row[m[r].col[k]]);
        hv.push_back(m[r].coeff[k]);
      }
      hp[r + 1] = (uint32_t)hc.size();
    }
    ptr.assign(hp, s);
    col.assign(hc, s);
    coef.assign(hv, s);
    RLN_HIP(hipStreamSynchronize(s));
  };
  csr(zk_.a, D.a_ptr, D.a_col, D.a_coef);
  csr(zk_.b, D.b_ptr, D.b_col, D.b_coef);
  {   // rows the small-batch mat-vec gives a wave each (k_matvec)
    std::vector<uint32_t> lr;
    for (uint32_t r = 0; r < D.nc; r++)
      if (zk_.a[r].col.size() > MV_LONG || zk_.b[r].col.size() > MV_LONG) lr.push_back(r);
    D.n_mv_long = (uint32_t)lr.size();
    D.mv_long.assign(lr, s);
    RLN_HIP(hipStreamSynchronize(s));
  }

  // ---- NTT tables and the launches of the big batches' transforms (prover_plan.h)
  {
    const NttTables T = ntt_tables(D.logn);
    D.ntt_passes = ntt_pass_list(D.logn);
    D.tw_f.assign(T.tw_f, s);
    D.tw_i.assign(T.tw_i, s);
    D.coset.assign(T.coset, s);
    D.tw_f29.assign(T.tw_f29, s);
    D.tw_i29.assign(T.tw_i29, s);
    D.coset29.assign(T.coset29, s);
    RLN_HIP(hipStreamSynchronize(s));
  }

  // ---- which witness signals are fixed by the partial witness (evaluate_partial, graph.rs:274-312; wl_known_nodes)
  {
    std::vector<uint8_t> node_known = wl_known_nodes(graph_);
    D.known.resize(D.NS);
    for (uint32_t i = 0; i < D.NS; i++) D.known[i] = node_known[graph_.signals[i]];
    {
      std::vector<uint32_t> io(96);
      for (uint32_t i = 0; i < 96; i++) io[i] = i;
      D.iota96.assign(io, s);
      RLN_HIP(hipStreamSynchronize(s));
    }
    // ---- the cone program and the cache of known stored values (prover.h: collect_partial_cached / submit_finish)
    const long want = cfg.partial_cache >= 0 ? cfg.partial_cache : (long)D.tune.partial_cache;
    D.tune.partial_cache = (uint32_t)std::max(0l, want);
    if (D.witlanes.ok && want > 0) {
      const WlCone C = wl_cone(graph_, std::move(node_known));
      std::vector<uint32_t> rows;   // stored slots of the known nodes
      for (uint32_t i = 0; i < W29.slot2node.size(); i++)
        if (C.node_known[W29.slot2node[i]]) rows.push_back(i);
      D.cone.build(C.graph, wl_cone_store_slots(C, W29.store_slot), D.nstore29, s);
      D.cone_nodes = (uint32_t)C.node_of.size();
      if (D.cone.ok && !rows.empty()) {
        D.cone_nk = (uint32_t)rows.size();
        D.cone_rows.assign(rows, s);
        RLN_HIP(hipStreamSynchronize(s));
        D.cone_cap = (uint32_t)std::min<long>(want, (1l << 24) - 2);
        static std::atomic<uint32_t> next_tag{1};
        D.cone_tag = next_tag++ & 0xFFFFFu;
        D.cone_stride = D.cone_nk * 3 + PP_POWERS16;
        D.cone_cache.alloc((size_t)D.cone_cap * D.cone_stride);
        RLN_HIP(hipMemset(D.cone_cache.p, 0, D.cone_cache.bytes()));
        D.cone_gen.assign(D.cone_cap, 1);
        D.cone_live.assign(D.cone_cap, 0);
        for (uint32_t e = D.cone_cap; e-- > 0;) D.cone_free.push_back(e);
        RLN_HIP(hipEventCreateWithFlags(&D.evConeSaved, hipEventDisableTiming));
        RLN_HIP(hipEventCreateWithFlags(&D.evConeRead, hipEventDisableTiming));
        RLN_HIP(hipEventCreateWithFlags(&D.evConeRead2, hipEventDisableTiming));
      } else {
        D.cone.ok = false;
      }
    }
  }

  // ---- MSM segments (prover_plan.h: g1_walk_rows / g2_walk_rows / make_walk_plan).  Every table row belongs to one output
  //      segment; the three walks are subsets of the rows: full = all, partial = rows whose scalar is a known witness
  //      signal, finish = the rest (unknown signals, h, blinding terms).
  auto plan = [&](Impl::Plan& P, const std::vector<VRow>& rows, uint32_t nseg, uint32_t chunk_pts, int mode, uint32_t* max_chunks,
                  uint32_t npaired = 0, bool pair_chunks = false, uint32_t block_pts = SUM_TREE_LANES) {
    P.upload(make_walk_plan(rows, nseg, chunk_pts, mode, D.known, npaired, pair_chunks, block_pts), s);
    *max_chunks = std::max(*max_chunks, P.nchunks);
  };
  const int modes[3] = {PROVE_FULL, PROVE_PARTIAL, PROVE_FINISH};
  {
    const G1Rows R = g1_walk_rows(zk_, D.NS, D.n, D.ni);
    D.npaired1 = R.npaired;
    D.npts1 = (uint32_t)R.pts.size();
    D.sid1.assign(R.sids, s);
    // the throughput plan: five segments, the rows A and B1 share walked once (prover_plan.h: G1Rows::shared)
    const std::vector<VRow>& big = D.tune.shared_rows ? R.shared : R.rows;
    D.nseg1_big = D.tune.shared_rows ? G1_SHARED_SEGS : G1_SEGS;
    D.nwalked1 = (uint32_t)big.size();
    for (int m : modes) {
      plan(D.plan1[PLAN_BIG][m], big, D.nseg1_big, 16u, m, &D.max_chunks1, R.npaired, true);   // rows (x halves) per single-wave workgroup
      D.max_groups1 = std::max(D.max_groups1, D.plan1[PLAN_BIG][m].ngroups);
    }
    for (int m : modes) plan(D.plan1[PLAN_SMALL][m], R.rows, 3, 4u, m, &D.max_chunks1s, R.npaired);
    // a lone tiny partial proof: the plain rows; full and finish: the fused rows (finish: the rows of the unknown signals
    // only -- alpha, beta, the known w_i are in pi_a, rho).  The tiny plans are summed by lane pairs.
    plan(D.plan1[PLAN_TINY][PROVE_PARTIAL], R.rows, 3, 1u, PROVE_PARTIAL, &D.max_chunks1t, R.npaired, false, SUM_TREE_LANES / 2);
    for (int m : {(int)PROVE_FULL, (int)PROVE_FINISH}) {
      plan(D.plan1[PLAN_FUSED][m], R.fused, 3, 4u, m, &D.max_chunks1s, R.npaired);
      plan(D.plan1[PLAN_TINY][m], R.fused, 3, 1u, m, &D.max_chunks1t, R.npaired, false, SUM_TREE_LANES / 2);
    }
    for (int m : modes) D.max_blocks1t = std::max(D.max_blocks1t, D.plan1[PLAN_TINY][m].nblocks);
    build_table29<Fq, G1Affine29>(R.pts, D.ws, D.t1_29, s, R.npaired);
  }
  {
    const G2Rows R = g2_walk_rows(zk_, D.NS, D.n);
    D.npts2 = (uint32_t)R.pts.size();
    D.sid2.assign(R.dsid, s);
    for (int m : modes) {
      plan(D.plan2[PLAN_BIG][m], R.rows, 1, 8u, m, &D.max_chunks2);
      D.max_groups2 = std::max(D.max_groups2, D.plan2[PLAN_BIG][m].ngroups);
    }
    for (int m : modes) plan(D.plan2[PLAN_SMALL][m], R.rows, 1, 2u, m, &D.max_chunks2s);
    for (int m : modes) {   // walked and summed by lane pairs
      plan(D.plan2[PLAN_TINY][m], R.rows, 1, 1u, m, &D.max_chunks2t, 0, false, SUM_TREE_LANES / 2);
      D.max_blocks2t = std::max(D.max_blocks2t, D.plan2[PLAN_TINY][m].nblocks);
    }
    build_table29<Fq2, G2Affine29>(R.pts, D.ws2, D.t2_29, s);
  }

  poseidon_dev();

  // ---- workspace
  const size_t B = B_;
  D.inputs.alloc(B * D.NI * 8);
  D.rs.alloc(B * 16);
  D.pp_in.alloc(B * 80);
  RLN_HIP(hipMemsetAsync(D.pp_in.p, 0, D.pp_in.bytes(), s));
  RLN_HIP(hipMemsetAsync(D.inputs.p, 0, D.inputs.bytes(), s));
  RLN_HIP(hipMemsetAsync(D.rs.p, 0, D.rs.bytes(), s));
  for (int si = 0; si < D.nslot; si++) {
    Slot& S = D.slot[si];
    S.err.alloc(B);
    S.coords.alloc(B * 64);
    S.values.alloc(B * 40);
    S.comp.alloc(B * 128);
    S.V.alloc((size_t)(D.N + D.n_alias) * B);
    S.V29.alloc(((size_t)D.nstore29 + 1) * 3 * B);   // + the trash row of k_witness_lanes
    S.abc.alloc(3 * (size_t)D.n * B);
    S.digits.alloc((size_t)(3 * D.NS + D.n + 4) * D.nh * D.ws.W * B);   // + s w_i, r w_i, r s of the fused small-batch plan
    S.digits2.alloc((size_t)(D.NS + 3) * D.nh * D.ws2.W * B);
    S.part1.alloc(std::max({(size_t)D.max_chunks1 * B, (size_t)D.max_chunks1s * D.small_stride,
                            (size_t)D.max_chunks1t * TINY_STRIDE}));
    S.grp1.alloc(std::max((size_t)D.max_groups1 * B, (size_t)D.max_blocks1t * TINY_STRIDE));
    S.sums1.alloc(D.nseg1_big * D.nh * B);   // (no plan has more segments than the throughput plan)
    S.part2.alloc(std::max({(size_t)D.max_chunks2 * B, (size_t)D.max_chunks2s * D.small_stride,
                            (size_t)D.max_chunks2t * TINY_STRIDE}));
    S.grp2.alloc(std::max((size_t)D.max_groups2 * B, (size_t)D.max_blocks2t * TINY_STRIDE));
    S.sums2.alloc(D.nh * B);
    S.prod.alloc(2 * B);
    S.tbl.alloc(2 * 16 * B);
    S.affA.alloc(B);
    S.affB1.alloc(B);
    S.affB2.alloc(B);
    S.pp_out.alloc(B * 80);
    S.inputs.alloc(B * D.NI * 8);
    S.rs.alloc(B * 16);
    S.pp_in.alloc(B * 80);
    RLN_HIP(hipMemsetAsync(S.inputs.p, 0, S.inputs.bytes(), s));
    RLN_HIP(hipMemsetAsync(S.rs.p, 0, S.rs.bytes(), s));
    RLN_HIP(hipMemsetAsync(S.pp_in.p, 0, S.pp_in.bytes(), s));
    RLN_HIP(hipHostMalloc((void**)&S.h_in, B * ((size_t)D.NI * 32 + 64 + 320), hipHostMallocDefault));
    memset(S.h_in, 0, B * ((size_t)D.NI * 32 + 64 + 320));   // (residue_slot reads whole buffers)
    RLN_HIP(hipHostMalloc((void**)&S.h_cone, B * 4, hipHostMallocDefault));
    static_assert(sizeof(uint64_t) == 8, "two leaf indices per 16-byte word");
    if (B % 2) throw Error("internal: the workspace capacity is a multiple of 64");   // idx / h_idx are staged and counted in 16-byte words
    S.idx.alloc(B);
    RLN_HIP(hipMemsetAsync(S.idx.p, 0, S.idx.bytes(), s));
    RLN_HIP(hipHostMalloc((void**)&S.h_idx, B * 8, hipHostMallocDefault));
    memset(S.h_idx, 0, B * 8);
    RLN_HIP(hipEventCreateWithFlags(&S.evT, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evG, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evQ, hipEventDisableTiming));
    RLN_HIP(hipHostMalloc((void**)&S.h_hints, (size_t)HINT_PROOFS * 64 * 32, hipHostMallocDefault));
    memset(S.h_hints, 0, (size_t)HINT_PROOFS * 64 * 32);
    RLN_HIP(hipEventCreateWithFlags(&S.evU, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evE, hipEventDisableTiming));
    RLN_HIP(hipHostMalloc((void**)&S.h_pp, B * 320, hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&S.h_comp, B * 128, hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&S.h_values, B * 160, hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&S.h_err, B * 4, hipHostMallocDefault));
    RLN_HIP(hipEventCreateWithFlags(&S.evA, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evB, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evB2, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evR, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evW, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evX, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evP, hipEventDisableTiming));
    S.pp_pow.alloc((size_t)std::min<size_t>(B, 96) * PP_POWERS16);
    RLN_HIP(hipEventCreateWithFlags(&S.evV, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evC, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&S.evZ, hipEventDisableTiming));
    for (auto& e : S.t) RLN_HIP(hipEventCreate(&e));
    RLN_HIP(hipMemsetAsync(S.digits.p, 0, S.digits.bytes(), s));
    RLN_HIP(hipMemsetAsync(S.digits2.p, 0, S.digits2.bytes(), s));
    // residue_slot counts whole buffers, and hipMalloc may hand out memory that an earlier prover of the process freed:
    // whatever it counts starts at zero
    auto clear = [&](auto& buf) { if (buf.p) RLN_HIP(hipMemsetAsync(buf.p, 0, buf.bytes(), s)); };
    clear(S.V29); clear(S.abc); clear(S.part1); clear(S.part2); clear(S.grp1); clear(S.grp2); clear(S.sums1); clear(S.sums2);
    clear(S.prod); clear(S.tbl); clear(S.affA); clear(S.affB1); clear(S.affB2);
  }
  RLN_HIP(hipStreamSynchronize(s));
  g_init_ms[3] = ms_since(t_ctor) - g_init_ms[0] - g_init_ms[1] - g_init_ms[2];
  for (int k = 0; k < 4; k++) init_ms_[k] = g_init_ms[k];
}

Prover::~Prover() {
  if (!d_) return;
  Impl& D = *d_;
  for (hipStream_t st : {D.sA, D.sAb, D.sA2, D.sB, D.sB2, D.sC, D.sV, D.sW})
    if (st) (void)hipStreamSynchronize(st);
  // freed device memory is not cleared by the runtime: nothing secret-dependent goes back to the allocator
  try {
    if (D.sW) {
      for (int k = 0; k < D.nslot; k++)
        if (D.slot[k].used && !D.slot[k].wiped && D.slot[k].evC) D.wipe_slot(D.slot[k], D.slot[k].ticket == 0);
      if (D.cone_cache.p)   // entries a caller never released hold witness values too
        hipLaunchKernelGGL(k_wipe_bytes, dim3(div_up(D.cone_cache.bytes() / 16, 256)), dim3(64), 0, D.sW, D.cone_cache.p,
                           (uint32_t)(D.cone_cache.bytes() / 16));
      for (hipStream_t st : D.st)   // (compact: a big batch's wipe went to a front-end stream)
        if (st) (void)hipStreamSynchronize(st);
    }
  } catch (...) {
  }
  for (Slot& S : D.slot) {
    if (S.h_pp) (void)hipHostFree(S.h_pp);
    if (S.h_in) (void)hipHostFree(S.h_in);
    if (S.h_cone) (void)hipHostFree(S.h_cone);
    if (S.h_idx) (void)hipHostFree(S.h_idx);
    if (S.evT) (void)hipEventDestroy(S.evT);
    if (S.evG) (void)hipEventDestroy(S.evG);
    if (S.evQ) (void)hipEventDestroy(S.evQ);
    if (S.h_hints) {   // (a slot whose batch was never collected, or whose wipe threw above)
      secure_zero(S.h_hints, (size_t)HINT_PROOFS * 64 * 32);
      (void)hipHostFree(S.h_hints);
    }
    if (S.evU) (void)hipEventDestroy(S.evU);
    if (S.evE) (void)hipEventDestroy(S.evE);
    if (S.h_comp) (void)hipHostFree(S.h_comp);
    if (S.h_values) (void)hipHostFree(S.h_values);
    if (S.h_err) (void)hipHostFree(S.h_err);
    for (hipEvent_t e : {S.evA, S.evB, S.evB2, S.evR, S.evC, S.evW, S.evV, S.evX, S.evZ, S.evP})
      if (e) (void)hipEventDestroy(e);
    for (auto& e : S.t)
      if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : {D.evConeSaved, D.evConeRead, D.evConeRead2})
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t st : {D.sA, D.sAb, D.sA2, D.sB, D.sB2, D.sC, D.sV, D.sW})
    if (st) (void)hipStreamDestroy(st);
}

size_t Prover::table_bytes() const { return d_->t1_29.bytes() + d_->t2_29.bytes(); }
size_t Prover::g1_rows() const { return d_->nwalked1; }
size_t Prover::g2_rows() const { return d_->npts2; }

void Prover::upload(size_t n, const uint8_t* inputs, const uint8_t* rs) {
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  Impl& D = *d_;
  D.sync_all();  // in-flight batches still read the resident inputs
  RLN_HIP(hipMemcpyAsync(D.inputs.p, inputs, n * D.NI * 32, hipMemcpyHostToDevice, D.sA));
  RLN_HIP(hipMemcpyAsync(D.rs.p, rs, n * 64, hipMemcpyHostToDevice, D.sA));
  RLN_HIP(hipStreamSynchronize(D.sA));
}

void Prover::upload_witness(size_t n, const uint8_t* w_le) {
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  Impl& D = *d_;
  D.sync_all();
  size_t words = n * (size_t)D.NS * 8;
  if (D.wgiven.n < words) D.wgiven.alloc(words);
  RLN_HIP(hipMemcpyAsync(D.wgiven.p, w_le, words * 4, hipMemcpyHostToDevice, D.sA));
  RLN_HIP(hipStreamSynchronize(D.sA));
  D.wgiven_n = n;
}

// iNTT (DIF) + g^i / n + NTT (DIT) over `vectors` vectors with lanes = proofs, by the pass list of prover_plan.h
// (the passes work on 29-bit limbs and leave loose representatives in the buffer between launches; the launch that ends
// the transform stores the canonical values: prover_front.hip)
static void launch_ntt(const std::vector<NttPass>& passes, Fr* data, const uint32_t* tw_i, const uint32_t* tw_f, int logn,
                       const uint32_t* scale, uint32_t B, uint32_t nb, uint32_t vectors, hipStream_t s) {
  for (const NttPass& ps : passes) {
    const bool last = &ps == &passes.back();
    // one wave per workgroup: a 4-wave workgroup needs four free wave slots on one CU at the same moment, which the
    // single-wave MSM workgroups streaming through the chip never leave (measured: mat-vec 0.6 -> 32 ms, NTT 5 -> 19 ms)
    const dim3 block(64, 1), grid(div_up(nb, 64), (1u << logn) >> ps.k, vectors);
    if (ps.kind == NTT_TURN) {
      switch (ps.k * 2 + (last ? 1 : 0)) {
        case 2: hipLaunchKernelGGL((k_ntt_turn<1, false>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        case 3: hipLaunchKernelGGL((k_ntt_turn<1, true>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        case 4: hipLaunchKernelGGL((k_ntt_turn<2, false>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        case 5: hipLaunchKernelGGL((k_ntt_turn<2, true>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        case 6: hipLaunchKernelGGL((k_ntt_turn<3, false>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        case 7: hipLaunchKernelGGL((k_ntt_turn<3, true>), grid, block, 0, s, data, tw_i, tw_f, logn, scale, B, nb); break;
        default: throw Error("NTT pass list: the turn has one to three levels");
      }
    } else if (ps.k != NTT_MAX_K) {
      throw Error("NTT pass list: a pass that is not the turn has NTT_MAX_K levels");
    } else if (ps.kind == NTT_DIF) {
      if (last) throw Error("NTT pass list: a transform ends with a forward pass or with the turn");
      hipLaunchKernelGGL((k_ntt_pass<NTT_MAX_K, true, false>), grid, block, 0, s, data, tw_i, logn, (int)ps.s0, B, nb);
    } else if (last) {
      hipLaunchKernelGGL((k_ntt_pass<NTT_MAX_K, false, true>), grid, block, 0, s, data, tw_f, logn, (int)ps.s0, B, nb);
    } else {
      hipLaunchKernelGGL((k_ntt_pass<NTT_MAX_K, false, false>), grid, block, 0, s, data, tw_f, logn, (int)ps.s0, B, nb);
    }
    RLN_HIP(hipGetLastError());
  }
}

// The transforms of the quotient, either way the prover launches them (prover_kernels.h): Prover::enqueue and the probe
// of arith_probe.hip (rlnamd_probe_quotient_transform) both come through here.
void launch_quotient_transform(bool lds, const std::vector<NttPass>& passes, Fr* data, const NttDeviceTables& T, int logn,
                               uint32_t B, uint32_t nb, uint32_t vectors, hipStream_t s) {
  if (!lds) {
    launch_ntt(passes, data, T.tw_i29, T.tw_f29, logn, T.coset29, B, nb, vectors, s);
    return;
  }
  const Fr *tw_i = T.tw_i, *tw_f = T.tw_f, *coset = T.coset;
  if (logn < 9 || logn > 18) throw Error("the LDS transforms take domains of 2^9 .. 2^18 points");
  // iNTT, coset scaling and NTT as edge / mid / edge: one butterfly per lane per level (prover_front.hip: k_ntt_mid)
  const dim3 grid(nb, (1u << logn) >> 9, vectors);
  if (logn > 9) hipLaunchKernelGGL(k_ntt_edge<true>, grid, dim3(256), 0, s, data, tw_i, logn, B, nb);
  hipLaunchKernelGGL(k_ntt_mid, grid, dim3(256), 0, s, data, tw_i, tw_f, logn, coset, B, nb);
  if (logn > 9) hipLaunchKernelGGL(k_ntt_edge<false>, grid, dim3(256), 0, s, data, tw_f, logn, B, nb);
  RLN_HIP(hipGetLastError());
}

// Enqueue one batch; returns as soon as the work is queued.  Stage A (stream sA): proof values, witness,
// matvec, NTTs.  Stage B (sB): digit recoding and the two MSMs.  Stage C (sC): two-level reduction, the
// three finalize kernels, D2H of proofs + values into pinned memory.  Consecutive batches alternate slots.
void Prover::run_async(size_t n, int mode) { enqueue(n, mode, nullptr, nullptr, nullptr); }

// Streamed batch ("H2D of witness inputs -> D2H of proofs"; the reference takes a fresh witness per call,
// protocol/proof.rs:753-777): the inputs go through the slot's pinned staging buffer to the slot's own device buffers on
// the front-end stream of this batch, so consecutive submits of DIFFERENT batches overlap like run_async's do.  Blocks
// only when every workspace slot is in flight (then until the oldest batch has finished).
uint64_t Prover::submit(size_t n, const uint8_t* inputs, const uint8_t* rs, int mode, const uint8_t* partial320) {
  if (n == 0) throw Error("empty batch");
  if (!inputs || !rs) throw Error("submit: inputs and rs are required");
  if (mode == PROVE_FINISH && !partial320) throw Error("submit: finish mode needs the partial points");
  return enqueue(n, mode, inputs, rs, partial320);
}

uint64_t Prover::submit_finish(size_t n, const uint8_t* inputs, const uint8_t* rs, const uint8_t* partial320,
                               const uint64_t* handles) {
  if (n == 0) throw Error("empty batch");
  if (!inputs || !rs || !partial320) throw Error("submit_finish: inputs, rs and the partial points are required");
  return enqueue(n, PROVE_FINISH, inputs, rs, partial320, handles);
}

// Submit by member: the Merkle paths are read on the device, where the tree already holds them (k_proofs_at into the
// slot's staged inputs, ordered against the tree's stream by two events: enqueue).  A batch that would be interpreted as
// segments behind hints needs the paths on the host -- the hints are hashed from them -- and so does a sparse tree: those
// fetch the paths with one proofs_at call, fill the path slots of a copy of the inputs and go through enqueue as any
// submit does.  The path slots of `inputs` are ignored on both routes and the staged bytes are the same.
void Prover::check_members(const MemberTree& t, size_t n, const uint64_t* leaf) const {
  const Impl& D = *d_;
  if (!D.have_path_slots) throw Error("submit_members: the witness graph names no pathElements / identityPathIndex inputs");
  if (t.depth != (int)graph_.tree_depth)
    throw Error("submit_members: the tree's depth (" + std::to_string(t.depth) + ") is not the circuit's (" +
                std::to_string(graph_.tree_depth) + ")");
  if (t.dense && t.dense->device != D.device.dev) throw Error("submit_members: the tree and the prover are on different devices");
  if (!t.dense && !t.proofs_at) throw Error("submit_members: no tree");
  for (size_t i = 0; i < n; i++)
    if (leaf[i] >> t.depth)
      throw Error("submit_members: leaf index " + std::to_string(leaf[i]) + " is outside a tree of depth " + std::to_string(t.depth));
}

// a held draw of a quota ledger (QuotaLedgerDev::draw_hold) and where the ids of the batch at hand start in it
struct DrawnIds {
  QuotaLedgerDev* quota;
  QuotaLedgerDev::Held held;
  const uint8_t* status;   // the draw's statuses on the host (the caller's array), from request 0
  size_t first;
  const uint8_t* counts = nullptr;   // a draw by count: the requests' counts on the host, from request 0; the ids are firsts
};

uint64_t Prover::submit_members(const MemberTree& t, size_t n, const uint64_t* leaf, const uint8_t* inputs, const uint8_t* rs,
                                int mode) {
  return submit_members_by(t, n, leaf, inputs, rs, mode, nullptr);
}

// Message ids drawn from a quota ledger.  The draw runs first, on the ledger's stream, and only its statuses come back;
// the ids stay in the draw's block on the device until the batch's kernel has copied them into the staged rows (enqueue)
// -- or, on the host route, until one copy has brought them back -- and the block is overwritten before the call returns.
void Prover::check_drawn(const MemberTree& t, const QuotaLedgerDev& q, size_t n, const uint8_t* inputs, std::vector<uint32_t>* limits,
                         std::vector<uint8_t>* ext_le) const {
  const Impl& D = *d_;
  if (!D.have_drawn_slots)
    throw Error("submit_members_drawn: the witness graph names no single messageId input beside userMessageLimit and "
                "externalNullifier (the multi-message-id circuit takes several ids a proof)");
  if (q.depth() != t.depth)
    throw Error("submit_members_drawn: the ledger's depth (" + std::to_string(q.depth()) + ") is not the tree's (" +
                std::to_string(t.depth) + ")");
  if (q.device() != D.device.dev) throw Error("submit_members_drawn: the ledger and the prover are on different devices");
  const size_t NIB = (size_t)D.NI * 32;
  limits->resize(n);
  ext_le->resize(32 * n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* limit = inputs + i * NIB + (size_t)D.slots.limit * 32;
    uint8_t high = 0;
    for (int b = 4; b < 32; b++) high |= limit[b];
    if (high) throw Error("submit_members_drawn: the message limit of proof " + std::to_string(i) + " is 2^32 or more");
    memcpy(&(*limits)[i], limit, 4);
    memcpy(ext_le->data() + 32 * i, inputs + i * NIB + (size_t)D.slots.ext * 32, 32);
  }
}

namespace {
struct ReleaseDraw {   // success or error: the draw's block is overwritten when the call returns
  QuotaLedgerDev& q;
  ~ReleaseDraw() {
    try {
      q.release();
    } catch (...) {
    }
  }
};
}  // namespace

uint64_t Prover::submit_members_drawn(const MemberTree& t, QuotaLedgerDev& q, size_t n, const uint64_t* leaf, const uint8_t* inputs,
                                      const uint8_t* rs, uint8_t* status) {
  if (n == 0) throw Error("empty batch");
  if (!leaf || !inputs || !rs || !status) throw Error("submit_members_drawn: leaf indices, inputs, rs and status are required");
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  check_members(t, n, leaf);
  std::vector<uint32_t> limits;
  std::vector<uint8_t> ext;
  check_drawn(t, q, n, inputs, &limits, &ext);
  ReleaseDraw release{q};
  const DrawnIds drawn{&q, q.draw_hold(n, leaf, ext.data(), limits.data(), status), status, 0};
  return submit_members_by(t, n, leaf, inputs, rs, PROVE_FULL, &drawn);
}

void Prover::prove_stream_members_drawn(const MemberTree& t, QuotaLedgerDev& q, size_t n, const uint64_t* leaf, const uint8_t* inputs,
                                        const uint8_t* rs, uint8_t* status, uint8_t* proofs, uint8_t* values, uint32_t* errors) {
  if (n && (!leaf || !inputs || !rs || !status))
    throw Error("prove_stream_members_drawn: leaf indices, inputs, rs and status are required");
  check_members(t, n, leaf);   // all of it before anything is drawn or enqueued
  std::vector<uint32_t> limits;
  std::vector<uint8_t> ext;
  check_drawn(t, q, n, inputs, &limits, &ext);
  if (n == 0) return;
  ReleaseDraw release{q};
  const DrawnIds drawn{&q, q.draw_hold(n, leaf, ext.data(), limits.data(), status), status, 0};   // ONE draw: the chunks read their slices
  size_t at = 0;
  prove_stream_from([&](size_t* off, size_t* cnt) {
    if (at >= n) return false;
    *off = at;
    *cnt = std::min(B_, n - at);
    at += *cnt;
    return true;
  }, inputs, rs, proofs, values, errors, 0, &t, leaf, &drawn);
}

// Blocks of ids for the multi-message-id circuit: the same call with a count a proof, the number of message slots it uses.
void Prover::check_drawn_counts(const MemberTree& t, const QuotaLedgerDev& q, size_t n, const uint8_t* inputs, const uint8_t* counts,
                                std::vector<uint32_t>* limits, std::vector<uint8_t>* ext_le) const {
  const Impl& D = *d_;
  if (!D.have_drawn_multi_slots)
    throw Error("submit_members_drawn_counts: the witness graph does not name userMessageLimit, externalNullifier, messageId and "
                "selectorUsed with one message id and one selector per message slot");
  if (q.depth() != t.depth)
    throw Error("submit_members_drawn_counts: the ledger's depth (" + std::to_string(q.depth()) + ") is not the tree's (" +
                std::to_string(t.depth) + ")");
  if (q.device() != D.device.dev) throw Error("submit_members_drawn_counts: the ledger and the prover are on different devices");
  const size_t NIB = (size_t)D.NI * 32;
  limits->resize(n);
  ext_le->resize(32 * n);
  for (size_t i = 0; i < n; i++) {
    const std::string bad = quota::count_refusal(i, counts[i]);   // (a count of 0: the ledger's own text, before the draw)
    if (!bad.empty()) throw Error(bad);
    if (counts[i] > D.drawn_multi_slots)
      throw Error("submit_members_drawn_counts: proof " + std::to_string(i) + " asks for " + std::to_string(counts[i]) +
                  " message ids, the circuit has " + std::to_string(D.drawn_multi_slots) + " message slots (max_out)");
    const uint8_t* limit = inputs + i * NIB + (size_t)D.slots.limit * 32;
    uint8_t high = 0;
    for (int b = 4; b < 32; b++) high |= limit[b];
    if (high) throw Error("submit_members_drawn_counts: the message limit of proof " + std::to_string(i) + " is 2^32 or more");
    memcpy(&(*limits)[i], limit, 4);
    memcpy(ext_le->data() + 32 * i, inputs + i * NIB + (size_t)D.slots.ext * 32, 32);
  }
}

uint64_t Prover::submit_members_drawn_counts(const MemberTree& t, QuotaLedgerDev& q, size_t n, const uint64_t* leaf, const uint8_t* inputs,
                                             const uint8_t* rs, const uint8_t* counts, uint8_t* status) {
  if (n == 0) throw Error("empty batch");
  if (!leaf || !inputs || !rs || !counts || !status)
    throw Error("submit_members_drawn_counts: leaf indices, inputs, rs, counts and status are required");
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  check_members(t, n, leaf);
  std::vector<uint32_t> limits;
  std::vector<uint8_t> ext;
  check_drawn_counts(t, q, n, inputs, counts, &limits, &ext);
  ReleaseDraw release{q};
  const DrawnIds drawn{&q, q.draw_hold_counts(n, leaf, ext.data(), limits.data(), counts, status), status, 0, counts};
  return submit_members_by(t, n, leaf, inputs, rs, PROVE_FULL, &drawn);
}

void Prover::prove_stream_members_drawn_counts(const MemberTree& t, QuotaLedgerDev& q, size_t n, const uint64_t* leaf,
                                               const uint8_t* inputs, const uint8_t* rs, const uint8_t* counts, uint8_t* status,
                                               uint8_t* proofs, uint8_t* values_public, uint32_t* errors) {
  if (n && (!leaf || !inputs || !rs || !counts || !status))
    throw Error("prove_stream_members_drawn_counts: leaf indices, inputs, rs, counts and status are required");
  check_members(t, n, leaf);   // all of it before anything is drawn or enqueued
  std::vector<uint32_t> limits;
  std::vector<uint8_t> ext;
  check_drawn_counts(t, q, n, inputs, counts, &limits, &ext);
  if (n == 0) return;
  ReleaseDraw release{q};
  // ONE draw: the chunks read their slices
  const DrawnIds drawn{&q, q.draw_hold_counts(n, leaf, ext.data(), limits.data(), counts, status), status, 0, counts};
  size_t at = 0;
  prove_stream_from([&](size_t* off, size_t* cnt) {
    if (at >= n) return false;
    *off = at;
    *cnt = std::min(B_, n - at);
    at += *cnt;
    return true;
  }, inputs, rs, proofs, values_public, errors, 0, &t, leaf, &drawn, true);
}

void Prover::prove_stream_members_public(const MemberTree& tree, size_t n, const uint64_t* leaf, const uint8_t* inputs,
                                         const uint8_t* rs, uint8_t* proofs, uint8_t* values_public, uint32_t* errors) {
  if (n && (!leaf || !inputs || !rs)) throw Error("prove_stream_members: leaf indices, inputs and rs are required");
  check_members(tree, n, leaf);   // all of it before the first chunk is enqueued
  size_t at = 0;
  prove_stream_from([&](size_t* off, size_t* cnt) {
    if (at >= n) return false;
    *off = at;
    *cnt = std::min(B_, n - at);
    at += *cnt;
    return true;
  }, inputs, rs, proofs, values_public, errors, 0, &tree, leaf, nullptr, true);
}

uint64_t Prover::submit_members_by(const MemberTree& t, size_t n, const uint64_t* leaf, const uint8_t* inputs, const uint8_t* rs,
                                   int mode, const DrawnIds* drawn) {
  if (n == 0) throw Error("empty batch");
  if (!leaf || !inputs || !rs) throw Error("submit_members: leaf indices, inputs and rs are required");
  if (mode != PROVE_FULL && mode != PROVE_PARTIAL)
    throw Error("submit_members: full and partial proofs only (a finish brings its path with its inputs: submit)");
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  check_members(t, n, leaf);
  Impl& D = *d_;
  bool host = !t.dense;
  if (!host && n <= D.tune.hint_max) host = batch_shape(D.query(n, mode, true), D.tune).hinted;
  if (!host) {
    MemberGather g{t.dense, leaf};
    if (drawn) {
      g.ids = drawn->held.ids + drawn->first;
      g.ids_status = drawn->held.status + drawn->first;
      g.ids_stream = drawn->held.stream;
      if (drawn->counts) g.ids_counts = drawn->held.counts + drawn->first;
    }
    const uint64_t ticket = enqueue(n, mode, inputs, rs, nullptr, nullptr, nullptr, &g);
    if (drawn) D.mark_drawn(ticket);
    return ticket;
  }
  const size_t d = (size_t)t.depth, NIB = (size_t)D.NI * 32;
  std::vector<uint8_t> elems(n * d * 32), bits(n * d), in(inputs, inputs + n * NIB), ids(drawn ? n * 4 : 0);
  auto scrub = [&]() {   // the copy holds what the caller's inputs hold: the identity secret among it
    for (std::vector<uint8_t>* v : {&in, &elems, &bits, &ids}) {   // (the path bits are the member's leaf index)
      memset(v->data(), 0, v->size());
      __asm__ __volatile__("" : : "r"(v->data()) : "memory");
    }
  };
  try {
    if (t.proofs_at) t.proofs_at(leaf, n, elems.data(), bits.data());
    else t.dense->proofs_at_host(leaf, n, elems.data(), bits.data());
    if (drawn) drawn->quota->held_ids(drawn->first, n, (uint32_t*)ids.data());   // the one copy back of this route
    for (size_t i = 0; i < n; i++) {
      uint8_t* row = in.data() + i * NIB;
      memcpy(row + (size_t)D.path_off * 32, elems.data() + i * d * 32, d * 32);
      memset(row + (size_t)D.path_idx_off * 32, 0, d * 32);
      for (size_t l = 0; l < d; l++) row[((size_t)D.path_idx_off + l) * 32] = bits[i * d + l];
      if (drawn && drawn->counts) {   // the bytes k_quota_fill_counts writes on the device route
        uint32_t first = 0;
        memcpy(&first, ids.data() + 4 * i, 4);
        std::vector<uint32_t> words(NIB / 4);   // (a row of bytes is not aligned for words)
        memcpy(words.data(), row, NIB);
        QuotaLedgerDev::fill_row_counts(words.data(), drawn->status[drawn->first + i] == quota::OK, first, drawn->counts[drawn->first + i],
                                        D.drawn_multi_msg_off, D.drawn_multi_sel_off, D.drawn_sel, D.drawn_multi_slots);
        memcpy(row, words.data(), NIB);
        memset(words.data(), 0, NIB);
        __asm__ __volatile__("" : : "r"(words.data()) : "memory");
      } else if (drawn) {   // the bytes k_quota_fill writes on the device route
        const bool granted = drawn->status[drawn->first + i] == quota::OK;
        memset(row + (size_t)D.drawn_msg_off * 32, granted ? 0 : 0xFF, 32);
        if (granted) memcpy(row + (size_t)D.drawn_msg_off * 32, ids.data() + 4 * i, 4);
      }
    }
    const uint64_t ticket = enqueue(n, mode, in.data(), rs, nullptr);
    if (drawn) D.mark_drawn(ticket);
    scrub();
    return ticket;
  } catch (...) {
    scrub();
    throw;
  }
}

uint32_t Prover::hint_words() const {
  const Impl& D = *d_;
  return D.segs.ok && D.tune.hint_max > 0 ? D.n_hints * 8 : 0;
}

void Prover::hints_for(const uint8_t* inputs, uint32_t* hints) const {
  const Impl& D = *d_;
  if (!D.segs.ok) throw Error("hints_for: this prover interprets no segments (hint_words() is 0)");
  Fr hv[64];
  D.hints.hints(inputs, hv);
  for (uint32_t j = 0; j < D.n_hints; j++) hv[j].to_canonical(hints + (size_t)j * 8);
  secure_zero(hv, sizeof hv);
}

uint64_t Prover::submit_hinted(size_t n, const uint8_t* inputs, const uint8_t* rs, const uint32_t* hints) {
  if (n == 0) throw Error("empty batch");
  if (!inputs || !rs) throw Error("submit: inputs and rs are required");
  return enqueue(n, PROVE_FULL, inputs, rs, nullptr, nullptr, hint_words() && n <= HINT_PROOFS ? hints : nullptr);
}

void Prover::collect_partial_cached(uint64_t ticket, size_t n, uint8_t* partial320, uint64_t* handles, uint32_t* errors) {
  Impl& D = *d_;
  ticket = settle_hints(ticket);
  Slot* Sp = nullptr;
  for (int k = 0; k < D.nslot; k++)
    if (D.slot[k].used && D.slot[k].ticket == ticket && ticket != 0) Sp = &D.slot[k];
  if (!Sp) throw Error("collect: unknown or expired ticket (its workspace slot has been reused)");
  Slot& S = *Sp;
  if (S.mode != PROVE_PARTIAL) throw Error("collect_partial_cached: not a partial-proof batch");
  if (n > S.n) throw Error("collect: more proofs requested than the batch holds");
  if (S.wiped) throw Error("collect_partial_cached: the batch has been wiped");
  RLN_HIP(hipEventSynchronize(S.evC));
  // entries for as many proofs as the cache has room for (in order); the rest get handle 0.  A proof whose graph
  // evaluation failed gets none either (its rows are not a witness).
  size_t cached = 0;
  for (size_t i = 0; i < n; i++) {
    if (handles) handles[i] = 0;
    if (!handles || !D.cone.ok || D.cone_free.empty() || S.h_err[i] != 0 || cached != i) continue;   // (a prefix: the save kernel's grid is [0, cached))
    const uint32_t e = D.cone_free.back();
    D.cone_free.pop_back();
    D.cone_live[e] = 1;
    S.h_cone[i] = e;
    handles[i] = D.cone_handle(e);
    cached++;
  }
  if (cached) {
    RLN_HIP(hipStreamWaitEvent(D.sW, S.evC, 0));
    hipLaunchKernelGGL(k_cone_save, dim3(div_up(D.cone_nk * 3, 256), (uint32_t)cached), dim3(256), 0, D.sW, S.V29.p, D.cone_rows.p,
                       D.cone_nk, (uint32_t)B_, S.h_cone, D.cone_cache.p, D.cone_stride);
    // the powers of pi_a and rho behind them (fin29.hip: what lets a finish drop the ladder of s A and r B1); the caller
    // does not wait for this -- the first finish that uses the entry does (evConeSaved)
    launch_pp_powers(D.sW, S.pp_out.p, S.h_cone, D.cone_cache.p, D.cone_stride, D.cone_nk * 3, (uint32_t)cached);
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(D.evConeSaved, D.sW));
  }
  collect(ticket, n, nullptr, nullptr, errors, nullptr, partial320, true);   // copy-out, then the wipe -- behind the save on sW
}

void Prover::release_partial(const uint64_t* handles, size_t n) {
  Impl& D = *d_;
  if (!D.cone_cap || !handles) return;
  bool any = false;
  for (size_t i = 0; i < n; i++) {
    const uint32_t e = D.cone_entry(handles[i]);
    if (e == 0xFFFFFFFFu) continue;
    if (!any) {   // a finish in flight may still read its entries
      RLN_HIP(hipStreamWaitEvent(D.sW, D.evConeRead, 0));
      RLN_HIP(hipStreamWaitEvent(D.sW, D.evConeRead2, 0));
    }
    any = true;
    uint4* at = D.cone_cache.p + (size_t)e * D.cone_stride;
    hipLaunchKernelGGL(k_wipe_bytes, dim3(div_up(D.cone_stride, 256)), dim3(64), 0, D.sW, at, D.cone_stride);
    D.cone_live[e] = 0;
    D.cone_gen[e]++;
    D.cone_free.push_back(e);
  }
  if (any) {
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(D.evConeSaved, D.sW));   // a later save / restore of a reused entry orders behind the wipe
  }
}

void Prover::hint_stats(uint64_t out[HINT_STATS_FIELDS]) const {
  const Impl& D = *d_;
  out[0] = D.segs.ok ? D.segs.nseg : 0;
  out[1] = D.segs.ok ? D.n_hints : 0;
  out[2] = D.segs.ok ? D.segs.max_steps : 0;
  out[3] = D.witlanes.ok ? D.witlanes.nsteps : 0;
  out[4] = D.hinted_batches;
  out[5] = D.hint_fallbacks;
  out[6] = D.hints.hits();
}

void Prover::partial_cache_info(uint64_t out[PARTIAL_CACHE_FIELDS]) {
  Impl& D = *d_;
  for (int k = 0; k < PARTIAL_CACHE_FIELDS; k++) out[k] = 0;
  out[0] = D.cone_cap;
  out[1] = D.cone_cap - D.cone_free.size();
  out[2] = (uint64_t)D.cone_stride * 16;
  out[4] = D.cone_batches;
  out[5] = D.cone_nodes;
  out[6] = D.cone.ok ? D.cone.nsteps : 0;
  out[7] = D.witlanes.ok ? D.witlanes.nsteps : 0;
  if (!D.cone_cap) return;
  sync();
  RLN_HIP(hipStreamSynchronize(D.sW));
  DevBuf<unsigned long long> cnt(1);
  RLN_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes(), D.sC));
  for (uint32_t e = 0; e < D.cone_cap; e++)
    if (!D.cone_live[e])
      hipLaunchKernelGGL(k_count_nonzero16, dim3(64), dim3(256), 0, D.sC, (const uint4*)(D.cone_cache.p + (size_t)e * D.cone_stride),
                         (size_t)D.cone_stride, cnt.p);
  RLN_HIP(hipGetLastError());
  unsigned long long h = 0;
  RLN_HIP(hipMemcpyAsync(&h, cnt.p, sizeof h, hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
  out[3] = h;
}

// A batch that was interpreted as segments behind hints is only as good as its hints: a cut node whose own value differs
// from the hint raised WERR_HINT (k_hint_check).  The library computes the hints itself, so this is not expected -- but it is
// checked, and such a batch is run again here over the whole graph before anyone sees a byte of it.  Returns the ticket
// that holds the batch's results from now on.
uint64_t Prover::settle_hints(uint64_t ticket) {
  Impl& D = *d_;
  Slot* Sp = nullptr;
  for (int k = 0; k < D.nslot; k++)
    if (D.slot[k].used && D.slot[k].ticket == ticket && ticket != 0) Sp = &D.slot[k];
  if (!Sp || !Sp->hinted) return ticket;
  Slot& S = *Sp;
  RLN_HIP(hipEventSynchronize(S.evC));
  S.hinted = false;
  bool bad = false;
  for (size_t i = 0; i < S.n; i++) bad = bad || (S.h_err[i] & WERR_HINT) != 0;
  if (!bad) return ticket;
  D.hint_fallbacks++;
  // The re-run takes the batch's OWN slot: the next slot of the ring may hold another ticket's results (with slots() batches
  // pending it always does).  Its inputs, (r, s) and points leave the slot's staging buffer for a host copy first, so that
  // the failed run can be wiped as any other batch -- staging, hints and, by the strides IT used, everything on the device
  // -- before the re-run stages them again; enqueue waits for that wipe (free_event) as a slot's next user does.  What the
  // re-run leaves is wiped by its own collect.  The ticket stays the caller's.
  const size_t n = S.n, in_bytes = n * (size_t)D.NI * 32;
  const int mode = S.mode;
  const bool finish = mode == PROVE_FINISH;
  std::vector<uint8_t> keep(in_bytes + n * 64 + (finish ? n * 320 : 0));
  struct ZeroOnExit wipe_keep{keep};
  memcpy(keep.data(), S.h_in, in_bytes);
  memcpy(keep.data() + in_bytes, S.h_in + B_ * (size_t)D.NI * 32, n * 64);
  if (finish) memcpy(keep.data() + in_bytes + n * 64, S.h_in + B_ * ((size_t)D.NI * 32 + 64), n * 320);
  if (!S.wiped) D.wipe_slot(S, false);
  D.no_hints_now = true;
  D.rerun_slot = (int)(Sp - D.slot);
  uint64_t again = 0;
  try {
    again = enqueue(n, mode, keep.data(), keep.data() + in_bytes, finish ? keep.data() + in_bytes + n * 64 : nullptr, nullptr);
  } catch (...) {
    D.no_hints_now = false;
    D.rerun_slot = -1;
    throw;
  }
  D.no_hints_now = false;
  D.rerun_slot = -1;
  return again;
}

void Prover::collect(uint64_t ticket, size_t n, uint8_t* proofs, uint8_t* values, uint32_t* errors, uint8_t* coords,
                     uint8_t* partial320, bool wipe_after) {
  Impl& D = *d_;
  ticket = settle_hints(ticket);
  Slot* Sp = nullptr;
  for (int k = 0; k < D.nslot; k++)
    if (D.slot[k].used && D.slot[k].ticket == ticket && ticket != 0) Sp = &D.slot[k];
  if (!Sp) throw Error("collect: unknown or expired ticket (its workspace slot has been reused)");
  Slot& S = *Sp;
  if (n > S.n) throw Error("collect: more proofs requested than the batch holds");
  // a big batch is tens of milliseconds away: poll and sleep instead of hipEventSynchronize, whose wait spins in the runtime
  // (a host core per GPU as measured, hipEventBlockingSync or not) -- eight replicas must not need eight cores to wait.
  // Small batches keep the spinning wait: their latency is the product.
  if (S.n > D.tune.lanechunk_max) wait_yielding(S.evC); else RLN_HIP(hipEventSynchronize(S.evC));
  if (S.mode == PROVE_PARTIAL) {
    if (partial320) memcpy(partial320, S.h_pp, n * 320);
  } else {
    if (proofs) memcpy(proofs, S.h_comp, n * 128);
    // a batch with drawn message ids: a refused row yields no proof bytes -- at once, and once more with the value bytes
    // and the coordinates behind the copies below, which write over whatever is cleared here
    for (size_t i = 0; i < n && S.drawn; i++)
      if (S.h_err[i]) {
        if (proofs) memset(proofs + 128 * i, 0, 128);
        if (values) memset(values + 160 * i, 0, 160);
      }
    if (values) {
      if (D.have_values_kernel)
        memcpy(values, S.h_values, n * 160);
      else if (D.ni == 6) {
        std::vector<uint8_t> pub;
        fetch_public_slot(&S, n, &pub);
        memcpy(values, pub.data(), n * 160);
      } else
        memset(values, 0, n * 160);
    }
    if (coords) RLN_HIP(hipMemcpy(coords, S.coords.p, n * 256, hipMemcpyDeviceToHost));
    // A batch with drawn message ids: a row the interpreter refused -- a request past its quota among them -- yields
    // nothing, behind every copy above.  The kernels do run for such a row, and every refused row reads the same
    // messageId (the reduction of its 0xFF bytes): the y values of two refused requests of one member under one external
    // nullifier would be two shares on one line, which is what the ledger exists to prevent.
    for (size_t i = 0; i < n && S.drawn; i++)
      if (S.h_err[i]) {
        if (proofs) memset(proofs + 128 * i, 0, 128);
        if (values) memset(values + 160 * i, 0, 160);
        if (coords) memset(coords + 256 * i, 0, 256);
      }
  }
  if (errors) memcpy(errors, S.h_err, n * 4);
  if (wipe_after && !S.wiped) D.wipe_slot(S, false);
}

// ticket 0: the resident-input run (upload / run / download): the shared input buffers and the last batch's witness.
void Prover::wipe(uint64_t ticket) {
  Impl& D = *d_;
  if (ticket == 0) {
    D.sync_all();
    if (D.last) D.wipe_slot(*D.last, true);
    D.sync_all();   // (the wipe's stream is the plan's: sW, or a front-end stream)
    return;
  }
  for (int k = 0; k < D.nslot; k++)
    if (D.slot[k].used && D.slot[k].ticket == ticket) {
      RLN_HIP(hipEventSynchronize(D.slot[k].evC));
      if (!D.slot[k].wiped) D.wipe_slot(D.slot[k], false);
      return;
    }
}

void Prover::collect_public(uint64_t ticket, size_t n, std::vector<uint8_t>* out_le) {
  Impl& D = *d_;
  ticket = settle_hints(ticket);
  for (int k = 0; k < D.nslot; k++)
    if (D.slot[k].used && D.slot[k].ticket == ticket && ticket != 0) {
      if (n > D.slot[k].n) throw Error("collect: more proofs requested than the batch holds");
      if (D.slot[k].wiped) throw Error("collect_public: the batch has been wiped (collect it with wipe_after = false first)");
      RLN_HIP(hipEventSynchronize(D.slot[k].evC));
      fetch_public_slot(&D.slot[k], n, out_le);
      const size_t row = num_public() * 32;   // (a refused row of a drawn batch yields nothing: collect)
      for (size_t i = 0; i < n && D.slot[k].drawn && out_le->size() >= n * row; i++)
        if (D.slot[k].h_err[i]) memset(out_le->data() + i * row, 0, row);
      return;
    }
  throw Error("collect: unknown or expired ticket (its workspace slot has been reused)");
}

int Prover::slots() const { return d_->nslot; }

// Any number of proofs through the streamed path: chunks of at most capacity() proofs, as many in flight as there are
// workspace slots, results written in index order.  This is what a caller with more proofs than one workspace holds
// gets instead of an upload / run / download loop that drains the pipeline after every chunk.
void Prover::prove_stream(size_t n, const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs, uint8_t* values,
                          uint32_t* errors) {
  size_t at = 0;
  prove_stream_from([&](size_t* off, size_t* cnt) {
    if (at >= n) return false;
    *off = at;
    *cnt = std::min(B_, n - at);
    at += *cnt;
    return true;
  }, inputs, rs, proofs, values, errors);
}

void Prover::prove_stream_members(const MemberTree& tree, size_t n, const uint64_t* leaf, const uint8_t* inputs,
                                  const uint8_t* rs, uint8_t* proofs, uint8_t* values, uint32_t* errors) {
  if (n && (!leaf || !inputs || !rs)) throw Error("prove_stream_members: leaf indices, inputs and rs are required");
  check_members(tree, n, leaf);   // all of it before the first chunk is enqueued
  size_t at = 0;
  prove_stream_from([&](size_t* off, size_t* cnt) {
    if (at >= n) return false;
    *off = at;
    *cnt = std::min(B_, n - at);
    at += *cnt;
    return true;
  }, inputs, rs, proofs, values, errors, 0, &tree, leaf);
}

void Prover::prove_stream_from(const ChunkSource& next, const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs,
                               uint8_t* values, uint32_t* errors, int max_in_flight, const MemberTree* tree,
                               const uint64_t* leaf, const DrawnIds* drawn, bool public_values) {
  Impl& D = *d_;
  struct Pending { uint64_t ticket; size_t off, cnt; };
  std::deque<Pending> q;
  const size_t NIB = (size_t)D.NI * 32;
  const int depth = max_in_flight > 0 ? std::min(max_in_flight, D.nslot) : D.nslot;
  auto take = [&]() {
    Pending f = q.front();
    q.pop_front();
    if (public_values) {   // every public signal, read before the collect that ends the batch; a refused row of a drawn batch: zero
      const size_t row = num_public() * 32;
      if (values) {
        std::vector<uint8_t> pub;
        collect_public(f.ticket, f.cnt, &pub);
        memcpy(values + f.off * row, pub.data(), f.cnt * row);
      }
      collect(f.ticket, f.cnt, proofs ? proofs + f.off * 128 : nullptr, nullptr, errors ? errors + f.off : nullptr);
      return;
    }
    collect(f.ticket, f.cnt, proofs ? proofs + f.off * 128 : nullptr, values ? values + f.off * 160 : nullptr,
            errors ? errors + f.off : nullptr);
  };
  try {
    size_t off = 0, cnt = 0;
    for (;;) {
      if ((int)q.size() == depth) take();   // the slot the next submit reuses
      if (!next(&off, &cnt)) break;         // (asked only when a slot is free: a shared cursor hands out no chunk early)
      if (cnt == 0) continue;
      if (cnt > B_) throw Error("prove_stream: a chunk larger than the prover workspace (max_batch)");
      DrawnIds slice{};
      if (drawn) slice = DrawnIds{drawn->quota, drawn->held, drawn->status, drawn->first + off, drawn->counts};
      q.push_back({tree ? submit_members_by(*tree, cnt, leaf + off, inputs + off * NIB, rs + off * 64, PROVE_FULL, drawn ? &slice : nullptr)
                        : submit(cnt, inputs + off * NIB, rs + off * 64),
                   off, cnt});
    }
    while (!q.empty()) take();
  } catch (...) {
    D.sync_all();
    for (int k = 0; k < D.nslot; k++)   // the error path leaves no witness behind either
      if (D.slot[k].used && !D.slot[k].wiped) D.wipe_slot(D.slot[k], false);
    D.sync_all();
    throw;
  }
}

// per_proof(i) for the n proofs of a batch: proofs i = k, k + nth, ... on thread k; the caller is thread 0
template <class F>
static void on_hint_threads(size_t n, size_t nth, F&& per_proof) {
  std::vector<std::thread> helpers;
  std::atomic<bool> failed{false};     // (an exception must not leave a helper thread: it would end the process)
  auto strand = [&](size_t k) {
    try {
      for (size_t i = k; i < n; i += nth) per_proof(i);
    } catch (...) {
      failed = true;
    }
  };
  try {
    for (size_t k = 1; k < nth; k++) helpers.emplace_back(strand, k);
  } catch (...) {   // no more threads to be had: the caller's thread takes what the missing ones would have
    const size_t started = helpers.size() + 1;
    for (size_t k = started; k < nth; k++) strand(k);
  }
  strand(0);
  for (std::thread& th : helpers) th.join();
  if (failed) throw Error("out of memory while hashing the hints of a batch");
}

uint64_t Prover::enqueue(size_t n, int mode, const uint8_t* h_inputs, const uint8_t* h_rs, const uint8_t* h_pp320,
                         const uint64_t* cone_handles, const uint32_t* pre_hints, const MemberGather* members) {
  if (n == 0) return 0;
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  if (mode < PROVE_FULL || mode > PROVE_FINISH) throw Error("unknown prover mode");
  Impl& D = *d_;
  const ProverTuning& T = D.tune;
  // ---- the shape of the batch (prover_plan.h: batch_shape), decided before anything is launched
  BatchQuery q = D.query(n, mode, h_inputs != nullptr);
  q.partial_points = h_pp320 != nullptr;
  q.handles = cone_handles != nullptr;
  q.pre_hints = pre_hints != nullptr;
  // a batch whose paths are gathered on the device has no path on the host to hash hints from
  q.no_hints_now = D.no_hints_now || members != nullptr;
  BatchShape sh = batch_shape(q, T);
  // the cone needs a live cache entry for every proof: a dead handle walks the whole graph
  std::vector<uint32_t> cone_entries;
  for (size_t i = 0; i < n && sh.cone; i++) {
    const uint32_t e = D.cone_entry(cone_handles[i]);
    if (e != 0xFFFFFFFFu) {
      cone_entries.push_back(e);
    } else {
      q.handles = false;
      sh = batch_shape(q, T);
    }
  }
  // above hint_max proofs the segments pay only when few enough of the proofs' chains have to be hashed (the others are
  // remembered: HintChains) that the host threads are done in ~0.5 ms
  std::vector<HintChains::Probe> probes;
  const size_t hint_nth = std::min<size_t>(std::max<size_t>(n, 1), std::max<uint32_t>(1u, T.hint_threads));
  if (sh.probe_chains) {
    probes.resize(n);
    // the first two proofs on this thread (15 us): a batch of members never seen ends here, before a helper thread is started
    for (size_t i = 0; i < 2 && sh.hinted; i++) {
      D.hints.probe(h_inputs + i * (size_t)D.NI * 32, &probes[i]);
      sh.hinted = probes[i].found;
    }
  }
  if (sh.probe_chains && sh.hinted) {
    on_hint_threads(n, hint_nth, [&](size_t i) {
      if (i >= 2) D.hints.probe(h_inputs + i * (size_t)D.NI * 32, &probes[i]);
    });
    size_t to_hash = 0;
    for (const HintChains::Probe& pr : probes) to_hash += pr.found ? 0 : 1;
    // a chain is ~0.2 ms on a host core against ~1.3 ms the segments save: at most 2.5 chains per thread
    sh.hinted = 2 * to_hash <= 5 * hint_nth;
  }
  if (!sh.hinted) probes.clear();
  const bool lone = sh.lone, small = sh.small, wl_used = sh.wl_used, cone = sh.cone, hinted = sh.hinted, early = sh.early,
             fused = sh.fused, tiny = sh.tiny, tiny_partial = sh.tiny_partial, walk_lp = sh.walk_lp;
  const Impl::Plan &P1 = D.plan1[sh.plan1][mode], &P2 = D.plan2[sh.plan2][mode];
  const uint32_t PB = sh.PB, dB = sh.dB;
  // the next slot of the ring -- or, for the re-run of a batch whose hints did not check, the slot the batch has (settle_hints)
  const bool in_place = D.rerun_slot >= 0;
  Slot& S = D.slot[in_place ? D.rerun_slot : D.cur];
  S.dB = dB;
  S.PB = PB;
  S.nch1 = P1.nchunks;
  S.nch2 = P2.nchunks;
  const bool streamed = h_inputs != nullptr;
  if (streamed) {
    if (D.wgiven_n) throw Error("upload_witness applies to the resident-input run that follows it, not to submit");
    // the slot's previous batch must be finished before its staging buffer (and its result buffers) are reused
    if (S.used) RLN_HIP(hipEventSynchronize(S.free_event()));
    memcpy(S.h_in, h_inputs, n * (size_t)D.NI * 32);
    memcpy(S.h_in + B_ * (size_t)D.NI * 32, h_rs, n * 64);
    if (h_pp320) memcpy(S.h_in + B_ * ((size_t)D.NI * 32 + 64), h_pp320, n * 320);
    if (members) {
      memcpy(S.h_idx, members->leaf, n * 8);
      S.members = true;
    }
  }
  const uint32_t* in_p = streamed ? S.inputs.p : D.inputs.p;
  const uint32_t* rs_p = streamed ? S.rs.p : D.rs.p;
  const uint32_t* pp_p = (streamed && h_pp320) ? S.pp_in.p : D.pp_in.p;
  S.mode = mode;
  if (!in_place) S.ticket = streamed ? ++D.tickets : 0;   // (a re-run answers to the ticket its caller holds)
  if (!in_place) S.drawn = false;                          // (submit_members_by marks the batch behind this call)
  if (!in_place) D.cur = (D.cur + 1) % D.nslot;
  // Front end in two pipeline stages on their own streams: A1 = graph interpreter (16 latency-bound waves per 1024
  // proofs, ~28 ms), A2 = mat-vec + NTTs + quotient (throughput kernels squeezed in beside the MSM, ~25 ms contended).
  // Chained on one stream they were the critical path (54 ms against 49 ms of MSM).
  const uint32_t sq = D.seq++;
  // With nothing of this prover in flight there is no second interpreter to overlap with, and the batch takes sA: on two
  // hardware queues sAb shares one with sC and sW, and a lone call on it measured 1.31 against 0.89 ms on sA.
  const bool idle = !D.last || hipEventQuery(D.last->evC) == hipSuccess;
  (void)hipGetLastError();   // hipErrorNotReady is not an error here
  // Big batches take their streams from the plan (prover_plan.h: stream_plan).  compact: the interpreter's stream by the
  // parity of the sequence number alone, so that a slot's wipe knows the stream of the slot's next batch.
  const bool big = !small, compact = big && D.splan.shape == SHAPE_COMPACT;
  const uint8_t* role = D.splan.at[(compact || !idle) ? (sq & 1) : 0];
  hipStream_t sA = big ? D.st[role[ROLE_INTERP]] : (!idle && (sq & 1)) ? D.sAb : D.sA;   // two graph interpreters in flight: 16 latency-bound waves each
  hipStream_t sB1 = big ? D.st[role[ROLE_WALK1]] : D.sB;   // the G1 walk's stream
  S.seq = sq;
  S.big = big;
  const uint32_t B = (uint32_t)B_, nb = (uint32_t)n;
  // Lone small batches: the G2 chain (recode, walk, sums, inversion, B's bytes -- the longest thing behind the interpreter)
  // stays on the interpreter's own stream, so nothing but kernel boundaries separates its links; the quotient chain
  // (mat-vec, NTTs, h rows, C sums, A's and C's bytes), which has ~0.2 ms of slack since the NTTs run in LDS, takes the
  // cross-stream hop (50 - 100 us each) instead.  In a stream of batches the front-end stream must be free for the
  // batch after next: there the walks keep their own streams.
  hipStream_t sA2 = big ? D.st[role[ROLE_QUOTIENT]] : !early ? D.sA2 : sh.g2_on_front ? D.sB2 : sA;
  const uint32_t pg = div_up(nb, 64);
  const uint32_t nbp = pg * 64;  // padded lanes compute on stale / zero inputs; results ignored
  // Results home.  Big batches: by a single-wave kernel writing the pinned pages (as the inputs come in: k_stage_in) -- the
  // runtime's copy kernel behind hipMemcpyAsync is a multi-wave workgroup that waits for wave slots beside the walks
  // (profiles/r6_kernel_stats.csv: __amd_rocclr_copyBuffer 0.45 ms on average, 17 ms at worst, for 0.3 MB).  Small batches
  // keep the copy engine path (5 us each, nothing beside them).
  auto d2h = [&](void* host, const void* dev, size_t bytes, hipStream_t st) {
    if (!small && bytes % 16 == 0)
      hipLaunchKernelGGL(k_stage_in, dim3(div_up(bytes / 16, 64)), dim3(64), 0, st, (const uint4*)dev, (uint4*)host, (uint32_t)(bytes / 16));
    else
      RLN_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
  };
  // The G1 walk of `cnt` chunks of the plan on stream `st` (ids: their chunk indices; null: the whole plan, chunks [0, cnt)).
  // Small batches: lanes = proofs over the short chunks (walk_lp) or lanes = chunks.  Big batches: the throughput form --
  // single chunks first, pair chunks (32 proofs x 2 members per wave: twice the proof groups) behind them.
  auto walk1 = [&](hipStream_t st, const uint32_t* ids, uint32_t cnt) {
    if (!cnt) return;
    const uint32_t blocks = div_up(cnt, 8) * 8 * pg;
    if (!small) {
      const PairPlan pp{P1.prows.p, P1.prsid.p, P1.pchunks.p, P1.pout.p, P1.npchunks};
      const uint32_t pblocks = div_up(P1.npchunks, 8) * 8 * (2 * pg);
      hipLaunchKernelGGL((k_msm29<G1Acc29, G1Affine29, G1XYZZ, 4>), dim3(blocks + pblocks), dim3(64), 0, st, D.t1_29.p,
                         P1.rsid.p, P1.rows.p, P1.chunks.p, cnt, S.digits.p, S.part1.p, D.ws, dB, pg, D.nh, D.walk_clk.p, ids,
                         0u, pp);
    } else if (walk_lp) {
      hipLaunchKernelGGL((k_msm29<G1Acc29, G1Affine29, G1XYZZ, 4>), dim3(blocks), dim3(64), 0, st, D.t1_29.p, P1.rsid.p,
                         P1.rows.p, P1.chunks.p, cnt, S.digits.p, S.part1.p, D.ws, dB, pg, D.nh, nullptr, ids, PB);
    } else {
      hipLaunchKernelGGL((k_msm29<G1Acc29, G1Affine29, G1XYZZ, 2, true>), dim3(div_up(cnt, 64), nb), dim3(64), 0, st,
                         D.t1_29.p, P1.rsid.p, P1.rows.p, P1.chunks.p, cnt, S.digits.p, S.part1.p, D.ws, dB, PB, D.nh,
                         nullptr, ids);
    }
  };
  // ---------------- stage A
  if (S.used) RLN_HIP(hipStreamWaitEvent(sA, S.free_event(), 0));  // slot free again
  if (streamed) {
    // by a kernel reading the pinned pages, not by hipMemcpyAsync: with the copy path in the pipeline every batch lost 8 ms
    // under the HIP runtime the torch wheel bundles (cross-queue signalling; profiles/r3_rocprof_summary.md section 1)
    auto h2d = [&](void* dst, const uint8_t* src, size_t bytes) {   // sizes are multiples of 32
      hipLaunchKernelGGL(k_stage_in, dim3(div_up(bytes / 16, 64)), dim3(64), 0, sA, (const uint4*)src, (uint4*)dst,
                         (uint32_t)(bytes / 16));
    };
    h2d(S.inputs.p, S.h_in, n * (size_t)D.NI * 32);
    h2d(S.rs.p, S.h_in + B_ * (size_t)D.NI * 32, n * 64);
    if (h_pp320) h2d(S.pp_in.p, S.h_in + B_ * ((size_t)D.NI * 32 + 64), n * 320);
    if (members) {
      // The paths, read where the tree holds them, land in the path slots of the inputs just staged -- behind that staging
      // on this stream, before evU and so before every reader.  Events only: the gather waits for whatever the tree's
      // stream holds so far (a scatter that set_few left behind included), and the tree's stream waits for the gather, so a
      // write made after this call finds the batch's paths read.  The caller holds the tree's lock across both.
      MerkleTreeDev& tree = *members->tree;
      h2d(S.idx.p, (const uint8_t*)S.h_idx, (n * 8 + 15) / 16 * 16);
      RLN_HIP(hipEventRecord(S.evT, tree.stream));
      RLN_HIP(hipStreamWaitEvent(sA, S.evT, 0));
      uint8_t* in8 = reinterpret_cast<uint8_t*>(S.inputs.p);
      const uint64_t NIB = (uint64_t)D.NI * 32;
      const PathDest dest{in8 + (size_t)D.path_off * 32, in8 + (size_t)D.path_idx_off * 32, NIB, 32, NIB, 32, 1};
      tree.proofs_at_device(S.idx.p, n, dest, sA);
      if (members->ids) {
        // Drawn message ids, beside the paths and by the same rule: the write waits for whatever the ledger's stream holds
        // so far (the draw), and the ledger's stream waits for the write (evG below), so the wipe of the draw's block that
        // follows this call finds the ids read.  The caller holds the ledger's lock across both.
        hipStream_t sQ = (hipStream_t)members->ids_stream;
        RLN_HIP(hipEventRecord(S.evQ, sQ));
        RLN_HIP(hipStreamWaitEvent(sA, S.evQ, 0));
        if (members->ids_counts)
          QuotaLedgerDev::fill_rows_counts(members->ids, members->ids_status, members->ids_counts, n, S.inputs.p, (size_t)D.NI * 8,
                                           D.drawn_multi_msg_off, D.drawn_multi_sel_off, D.drawn_sel, D.drawn_multi_slots, (void*)sA);
        else
          QuotaLedgerDev::fill_rows(members->ids, members->ids_status, n, S.inputs.p, (size_t)D.NI * 8, D.drawn_msg_off, (void*)sA);
      }
      RLN_HIP(hipEventRecord(S.evG, sA));
      RLN_HIP(hipStreamWaitEvent(tree.stream, S.evG, 0));
      if (members->ids) RLN_HIP(hipStreamWaitEvent((hipStream_t)members->ids_stream, S.evG, 0));
    }
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(S.evU, sA));
  }
  // Timing marks (stage_ms): a timed event record is a barrier packet and a timestamp write on its stream -- three of
  // them sit between the interpreter and the mat-vec of a single proof (~0.1 ms of its 5 ms).  Small batches record
  // none: their stage_ms reads 0.
  const bool marks = !small;
  S.marked = marks;
#define MARK(i, stream)                                   \
  do {                                                    \
    if (marks) RLN_HIP(hipEventRecord(S.t[i], stream));   \
  } while (0)
  if (cone) memcpy(S.h_cone, cone_entries.data(), n * sizeof(uint32_t));   // (the slot's previous batch has finished: see `streamed` above)
  S.hinted = hinted;
  if (hinted) {
    S.hints_staged = true;
    // a proof's hints: one dependent chain of depth + 2 hashes; the chains of the batch's proofs are independent of each
    // other: the calling thread and up to hint_threads - 1 helpers take them in turn
    if (pre_hints)
      memcpy(S.h_hints, pre_hints, n * (size_t)D.n_hints * 32);
    else
      on_hint_threads(n, hint_nth, [&](size_t i) {
        Fr hv[64];
        D.hints.hints(h_inputs + i * (size_t)D.NI * 32, hv, probes.empty() ? nullptr : &probes[i]);
        for (uint32_t j = 0; j < D.n_hints; j++) hv[j].to_canonical(S.h_hints + (i * D.n_hints + j) * 8);
        secure_zero(hv, sizeof hv);
      });
    if (T.hint_fault > 0 && (uint32_t)T.hint_fault <= D.n_hints) S.h_hints[(size_t)(T.hint_fault - 1) * 8] ^= 1u;   // test hook
    D.hinted_batches++;
  }
  if (fused && mode == PROVE_FINISH) {   // s pi_a + r rho beside everything else: needs (r, s) and the entries' powers only
    if (S.used) RLN_HIP(hipStreamWaitEvent(D.sC, S.free_event(), 0));
    RLN_HIP(hipStreamWaitEvent(D.sC, S.evU, 0));
    if (cone) {
      RLN_HIP(hipStreamWaitEvent(D.sC, D.evConeSaved, 0));
      launch_pp_smul(D.sC, D.cone_cache.p, S.h_cone, D.cone_stride, D.cone_nk * 3, rs_p, S.prod.p, nb);
      RLN_HIP(hipEventRecord(D.evConeRead2, D.sC));
    } else {   // no cache entries: the powers are made here, beside the interpreter of the whole graph (0.55 ms of its 1.5)
      launch_pp_powers(D.sC, pp_p, D.iota96.p, S.pp_pow.p, PP_POWERS16, 0, nb);
      launch_pp_smul(D.sC, S.pp_pow.p, D.iota96.p, PP_POWERS16, 0, rs_p, S.prod.p, nb);
    }
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(S.evP, D.sC));
  }
  MARK(1, sA);
  if (cone) {
    RLN_HIP(hipStreamWaitEvent(sA, D.evConeSaved, 0));   // sW: the entries are written by the partial batch's collect
    hipLaunchKernelGGL(k_cone_restore, dim3(div_up(D.cone_nk * 3, 256), nb), dim3(256), 0, sA, D.cone_cache.p, D.cone_rows.p,
                       D.cone_nk, B, S.h_cone, S.V29.p, D.cone_stride);
    RLN_HIP(hipEventRecord(D.evConeRead, sA));
    D.cone.launch(sA, in_p, D.NI, S.V29.p, S.err.p, B, nb);
    D.cone_batches++;
  } else if (hinted) {
    hipLaunchKernelGGL(k_wipe_bytes, dim3(1), dim3(64), 0, sA, (uint4*)S.err.p, (uint32_t)div_up(nb * 4, 16));   // the segments OR into it
    D.segs.launch(sA, in_p, D.NI, S.h_hints, S.V29.p, S.err.p, B, nb);
  } else if (wl_used) {
    D.witlanes.launch(sA, in_p, D.NI, S.V29.p, S.err.p, B, nb);
  } else {
    hipLaunchKernelGGL(k_witness29<false>, dim3(pg), dim3(64), WIT29_LDS_BYTES, sA, D.nodes29.p, D.nprog29,
                       D.consts29.p, (uint32_t)graph_.constants.size(), in_p, D.NI, S.V29.p, S.err.p, B, nbp, nullptr);
  }
  if (small)
    hipLaunchKernelGGL(k_v29_to_fr, dim3(div_up(D.nstore29, 64), nb), dim3(64, 1), 0, sA, S.V29.p, D.slot2node.p,
                       D.nstore29, S.V.p, B, nb, 1u);
  else
    hipLaunchKernelGGL(k_v29_to_fr, dim3(pg, D.nstore29), dim3(64, 1), 0, sA, S.V29.p, D.slot2node.p, D.nstore29, S.V.p,
                       B, nbp);
  if (D.n_alias)   // (the lanes k_v29_to_fr filled: the padded lanes of a big batch hold valid values too, their digits are read)
    hipLaunchKernelGGL(k_alias_rows, dim3(pg, D.n_alias), dim3(64), 0, sA, S.V.p, D.alias_src.p, D.alias_dst.p, D.n_alias, B,
                       small ? nb : nbp);
  if (hinted)
    hipLaunchKernelGGL(k_hint_check, dim3(div_up(D.n_cut, 64), nb), dim3(64), 0, sA, S.V.p, D.cut_node.p, D.cut_hint.p, D.n_cut,
                       S.h_hints, D.n_hints, B, S.err.p);
  if (D.wgiven_n) {
    if (D.wgiven_n != n || mode != PROVE_FULL) throw Error("upload_witness: the next run must be a full proof of the same batch");
    hipLaunchKernelGGL(k_scatter_witness, dim3(pg, div_up(D.NS, 4)), dim3(64, 4), 0, sA, D.wgiven.p, D.sig2node.p,
                       D.NS, S.V.p, S.err.p, B, nb);
    D.wgiven_n = 0;
  }
  // Small batches (latency): the digits of the witness scalars and of r, s are recoded right behind the interpreter,
  // so the G2 walk -- the longer of the two, and independent of the quotient h -- starts beside mat-vec / NTT instead
  // of behind them; only h's digits wait for the NTTs.
  RLN_HIP(hipEventRecord(S.evX, sA));   // mat-vec / NTT (sA2) need the witness, not the recodes below
  if (early) {
    // The witness digits right behind the interpreter, on its stream.  A lone batch keeps its whole G2 chain there
    // (g2_on_front above); the early G1 walk (sB) and the quotient chain (sA2) take one cross-stream hop each.  In a stream
    // of batches the recodes stay on the front-end stream too, where they do not queue behind the previous batch's walks,
    // and both walks wait for them on their own streams.
    hipStream_t sR1 = sA, sR3 = lone ? D.sB : sA;
    hipLaunchKernelGGL(k_recode, dim3(div_up(D.NS + 3, 64), nb), dim3(64, 1), 0, sR1, S.V.p, D.sig2node.p, D.NS,
                       S.abc.p, D.n, rs_p, D.ws, D.ws2, S.digits.p, S.digits2.p, B, nb, 1u, 1u, 0u, dB);
    if (lone) {
      RLN_HIP(hipEventRecord(S.evW, sA));
      RLN_HIP(hipStreamWaitEvent(D.sB, S.evW, 0));
    }
    if (fused)
      hipLaunchKernelGGL(k_recode, dim3(div_up(2 * D.NS + 1, 64), nb), dim3(64, 1), 0, sR3, S.V.p, D.sig2node.p, D.NS,
                         S.abc.p, D.n, rs_p, D.ws, D.ws2, S.digits.p, S.digits2.p, B, nb, 3u, 1u, 0u, dB);
    if (!lone) {
      RLN_HIP(hipEventRecord(S.evW, sA));
      RLN_HIP(hipStreamWaitEvent(D.sB, S.evW, 0));
      RLN_HIP(hipStreamWaitEvent(D.sB2, S.evW, 0));
    }
    MARK(14, D.sB);
    walk1(D.sB, P1.early_ids.p, P1.n_early);
    RLN_HIP(hipEventRecord(S.evE, D.sB));
  }
  MARK(2, sA);
  // compact: the public values are the circuit's own outputs w[1..5], read right here behind the interpreter -- no stream
  // and no queue for the 24 chained hashes of k_proof_values (17 ms of a step's span for 0.04 G of its 22.6 G
  // instructions).  A partial run returns no values and keeps k_proof_values, behind its G2 walk.
  const bool values_front = sh.values_front;   // (prover_plan.cpp: batch_shape)
  if (values_front) {
    MARK(0, sA);
    hipLaunchKernelGGL(k_values_from_witness, dim3(pg, 5), dim3(64), 0, sA, S.V.p, D.sig2node.p, B, nbp, S.values.p);
    MARK(13, sA);
    RLN_HIP(hipEventRecord(S.evV, sA));
  }
  if (sA2 != sA) RLN_HIP(hipStreamWaitEvent(sA2, S.evX, 0));
  MARK(12, sA2);
  if (mode != PROVE_PARTIAL) {  // the quotient h depends on the whole witness: not part of a partial proof
    CsrView A{D.a_ptr.p, D.a_col.p, D.a_coef.p}, Bm{D.b_ptr.p, D.b_col.p, D.b_coef.p};
    if (small)
      hipLaunchKernelGGL(k_matvec<true>, dim3(div_up(D.n, 64) + D.n_mv_long, nb), dim3(64, 1), 0, sA2, A, Bm, S.V.p,
                         D.sig2node.p, D.nc, D.ni, D.n, S.abc.p, B, nb, D.mv_long.p, div_up(D.n, 64));
    else
      hipLaunchKernelGGL(k_matvec<false>, dim3(pg, D.n), dim3(64, 1), 0, sA2, A, Bm, S.V.p, D.sig2node.p, D.nc,
                         D.ni, D.n, S.abc.p, B, nbp);
  }
  MARK(3, sA2);
  if (mode != PROVE_PARTIAL) {
    // small batches: lanes = groups
    // (above ~100 proofs the walks beside the quotient chain leave the 4-wave workgroups of the LDS kernels waiting for
    // four free wave slots on one CU: the single-wave passes then finish earlier -- 128 proofs 13.3 -> 12.6 ms, 96 and
    // below no better or worse; RLNAMD_NTT_LG_MAX)
    // (the LDS kernels have one lane per butterfly and take the batch's size; the passes, lanes = proofs, its padded size)
    launch_quotient_transform(sh.ntt_lds, D.ntt_passes, S.abc.p,
                              {D.tw_i.p, D.tw_f.p, D.coset.p, D.tw_i29.p, D.tw_f29.p, D.coset29.p}, D.logn, B,
                              sh.ntt_lds ? nb : nbp, 3, sA2);
    // (the recode below forms h = a o b - c itself)
  }
  MARK(4, sA2);
  // digit recoding closes the front end: the MSM streams carry nothing but the two table walks
  hipStream_t sR = sA2;
  MARK(5, sR);
  if (early)
    hipLaunchKernelGGL(k_recode, dim3(div_up(D.n, 64), nb), dim3(64, 1), 0, sR, S.V.p, D.sig2node.p, D.NS, S.abc.p, D.n,
                       rs_p, D.ws, D.ws2, S.digits.p, S.digits2.p, B, nb, 2u, 1u, 1u, dB);
  else
    hipLaunchKernelGGL(k_recode, dim3(pg, D.NS + D.n + 3), dim3(64, 1), 0, sR, S.V.p, D.sig2node.p, D.NS,
                       S.abc.p, D.n, rs_p, D.ws, D.ws2, S.digits.p, S.digits2.p, B, nbp, 0u, 0u,
                       mode != PROVE_PARTIAL ? 1u : 0u, dB);
  MARK(6, sR);
  // ---------------- stage B
  if (!early) {
    RLN_HIP(hipEventRecord(S.evA, sA2));
    RLN_HIP(hipStreamWaitEvent(sB1, S.evA, 0));
    MARK(14, sB1);
  }
  hipStream_t s2 = big ? D.st[role[ROLE_WALK2]] : sh.g2_on_front ? sA : D.sB2;   // the G2 walk on its own stream: its workgroups fill the G1 kernel's tail
  if (compact) {   // the G1 stream carries the previous batch's sums: the G2 walk waits for the digits, not for them
    RLN_HIP(hipStreamWaitEvent(s2, S.evA, 0));
  } else if (!early) {   // (early: the G2 walk's stream already has the witness + part-1 digits, all it reads)
    RLN_HIP(hipEventRecord(S.evR, sB1));
    RLN_HIP(hipStreamWaitEvent(s2, S.evR, 0));
  }
  if (early) {   // the h rows, on the front-end stream itself (no event hop); everything else is already walking
    walk1(sA2, P1.late_ids.p, P1.n_late);
    RLN_HIP(hipEventRecord(S.evR, sA2));
    RLN_HIP(hipStreamWaitEvent(D.sB, S.evR, 0));   // evB below then covers both launches
  } else {
    walk1(sB1, nullptr, P1.nchunks);
  }
  MARK(7, sB1);
  MARK(11, s2);
  if (P2.nchunks) {
    uint32_t blocks = div_up(P2.nchunks, 8) * 8 * pg;
    if (walk_lp)
      hipLaunchKernelGGL((k_msm29<G2Acc29, G2Affine29, G2XYZZ, 2>), dim3(blocks), dim3(64), 0, s2, D.t2_29.p, P2.rsid.p,
                         P2.rows.p, P2.chunks.p, P2.nchunks, S.digits2.p, S.part2.p, D.ws2, dB, pg, D.nh, nullptr, nullptr, PB);
    else if (tiny)   // a lane pair per (row, half): see Fq2PairOps
      hipLaunchKernelGGL((k_msm29<G2AccPair29, G2Affine29, G2XYZZ, 1, true>), dim3(div_up(2 * P2.nchunks, 64), nb), dim3(64), 0, s2,
                         D.t2_29.p, P2.rsid.p, P2.rows.p, P2.chunks.p, P2.nchunks, S.digits2.p, S.part2.p, D.ws2, dB, PB, D.nh,
                         nullptr);
    else if (small)
      hipLaunchKernelGGL((k_msm29<G2Acc29, G2Affine29, G2XYZZ, 1, true>), dim3(div_up(P2.nchunks, 64), nb), dim3(64), 0, s2,
                         D.t2_29.p, P2.rsid.p, P2.rows.p, P2.chunks.p, P2.nchunks, S.digits2.p, S.part2.p, D.ws2, dB, PB, D.nh,
                         nullptr);
    else
      hipLaunchKernelGGL((k_msm29<G2Acc29, G2Affine29, G2XYZZ, 2>), dim3(blocks), dim3(64), 0, s2, D.t2_29.p, P2.rsid.p,
                         P2.rows.p, P2.chunks.p, P2.nchunks, S.digits2.p, S.part2.p, D.ws2, dB, pg, D.nh,
                         D.walk_clk.p ? D.walk_clk.p + 2 : nullptr);
  }
  MARK(8, s2);
  if (!compact) RLN_HIP(hipEventRecord(S.evB, sB1));   // (compact: behind the G1 sums, below)
  RLN_HIP(hipEventRecord(S.evB2, s2));
  // ---------------- stage C
  // proof values (Poseidon chain, latency-bound, depends on the inputs only): the back-end stream has slack
  // (compact: the whole back end behind the G2 walk, on its stream -- in stream order behind the front end's events)
  hipStream_t sV = compact ? s2 : D.sV;
  hipStream_t sC = big ? D.st[role[ROLE_SUMS2]] : D.sC;
  if (S.used && !compact) {
    RLN_HIP(hipStreamWaitEvent(sC, S.free_event(), 0));
    RLN_HIP(hipStreamWaitEvent(sV, S.free_event(), 0));
  }
  if (!values_front) {
    if (streamed && !compact) RLN_HIP(hipStreamWaitEvent(sV, S.evU, 0));
    MARK(0, sV);
    // (whenever the batch is small enough for the lanes = nodes interpreter: the Poseidon chain alone is 5.3 ms)
    if (sh.values_w) {   // small batches: the circuit's own outputs (see k_values_from_witness)
      RLN_HIP(hipStreamWaitEvent(sV, S.evX, 0));   // sA: witness stored
      hipLaunchKernelGGL(k_values_from_witness, dim3(pg, 5), dim3(64), 0, sV, S.V.p, D.sig2node.p, B, nbp, S.values.p);
    } else if (D.have_values_kernel)
      hipLaunchKernelGGL(k_proof_values, dim3(pg), dim3(64), 0, sV, in_p, D.NI, D.slots, poseidon_view(2),
                         poseidon_view(3), poseidon_view(4), S.values.p, nbp);
    MARK(13, sV);
  }
  // Small full proofs: A and B1 are sums over h-independent rows only, so their reduction, the two inversions and the two
  // variable-base products s A, r B1 (the longest kernel of the back end) run on the idle D.sA2 as soon as the early G1
  // walk is done -- beside the NTTs and the walk of the h rows, not behind them.  sums1 segments: h * 3 + {A, B1, C}.
  // (round 6: PROVE_FINISH as well -- the partial points join their sums where each sum is complete, k_add_partial per
  // task; until then a lone finish took the serial back end of the big batches and was SLOWER than a lone full proof)
  const bool fin_pp = mode == PROVE_FINISH;
  const TaskSel all4 = task_sel({0, 1, 2, 3}), all3 = task_sel({0, 1, 2});
  hipStream_t sF = sC;   // the stream of k_fin_out and of the copies to the host
  // segment sums of a small batch: one 512-lane tree per (proof, segment); tiny batches (four times the partial sums) in
  // two stages -- every 512-chunk block of a segment to one point, then the blocks of the segment -- so that the depth
  // stays log2(partial sums) + 1 instead of growing with the serial share of a lane
  auto sum1 = [&](hipStream_t st, std::initializer_list<uint32_t> segs) {
    const TaskSel sel = task_sel(segs);
    const uint32_t ns = (uint32_t)segs.size();
    if (tiny) {   // a lane pair per point (fq29.h: G1AccPair29): the plan's blocks are SUM_TREE_LANES / 2 partial sums
      hipLaunchKernelGGL((k_sum_blocks<Fq, G1AccPair29>), dim3(nb, ns, std::max(P1.maxblk, 1u)), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G1 / 2, st, S.part1.p, P1.segchunks.p,
                         P1.segblocks.p, S.grp1.p, PB, sel);
      hipLaunchKernelGGL((k_sum_tree<Fq, G1AccPair29>), dim3(nb, ns), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G1 / 2, st, S.grp1.p, P1.segblocks.p, S.sums1.p, B, PB, sel);
    } else {
      hipLaunchKernelGGL((k_sum_tree<Fq, G1Acc29>), dim3(nb, ns), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G1, st, S.part1.p, P1.segchunks.p, S.sums1.p, B, PB, sel);
    }
  };
  auto sum2 = [&](hipStream_t st) {
    const TaskSel sel = task_sel({0, 1, 2, 3, 4, 5});
    if (tiny) {   // a lane pair per point (fq29.h: Fq2PairOps): the plan's blocks are SUM_TREE_LANES / 2 partial sums
      hipLaunchKernelGGL((k_sum_blocks<Fq2, G2AccPair29>), dim3(nb, P2.nseg, std::max(P2.maxblk, 1u)), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G2 / 2, st, S.part2.p,
                         P2.segchunks.p, P2.segblocks.p, S.grp2.p, PB, sel);
      hipLaunchKernelGGL((k_sum_tree<Fq2, G2AccPair29>), dim3(nb, P2.nseg), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G2 / 2, st, S.grp2.p, P2.segblocks.p, S.sums2.p, B, PB, sel);
    } else {
      hipLaunchKernelGGL((k_sum_tree<Fq2, G2Acc29>), dim3(nb, P2.nseg), dim3(SUM_TREE_LANES), SUM_TREE_LDS_G2, st, S.part2.p, P2.segchunks.p, S.sums2.p, B, PB, sel);
    }
  };
  if (early) {
    RLN_HIP(hipStreamWaitEvent(D.sA2, S.evE, 0));   // sB: the early G1 walk
    if (fused) {
      // fused plan: only A's segment sums are formed early; its fold and inversion ride in k_fin_out_ac_fused, and s A,
      // r B1 are inside the C segment (B1 is never formed)
      sum1(D.sA2, {0, 3});
      if (fin_pp) hipLaunchKernelGGL(k_add_partial, dim3(pg, 1), dim3(64), 0, D.sA2, S.sums1.p, S.sums2.p, pp_p, B, nbp, task_sel({0}), (const G1XYZZ*)nullptr);
    } else {
      sum1(D.sA2, {0, 1, 3, 4});
      if (fin_pp) hipLaunchKernelGGL(k_add_partial, dim3(pg, 2), dim3(64), 0, D.sA2, S.sums1.p, S.sums2.p, pp_p, B, nbp, task_sel({0, 1}), (const G1XYZZ*)nullptr);
      hipLaunchKernelGGL(k_glv_fold, dim3(pg, 2), dim3(64), 0, D.sA2, S.sums1.p, S.sums2.p, 3u, B, nbp, task_sel({0, 1}));
      hipLaunchKernelGGL(k_fin_affine, dim3(pg, 2), dim3(64), 0, D.sA2, S.sums1.p, S.sums2.p, S.affA.p, S.affB1.p,
                         S.affB2.p, B, nbp, task_sel({0, 1}));
      // small batches: s A / r B1 are a lone lane's chain, the NAF ladder in the 9 x 29 form (fin29.hip)
      launch_fin_smul29(D.sA2, S.affA.p, S.affB1.p, rs_p, S.prod.p, B, nb);
    }
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipEventRecord(S.evA, D.sA2));
    // The G2 sum and inversion (0.65 ms for one proof, behind the G2 walk only) beside the C segment (sC, behind the h
    // rows) instead of in front of it; k_fin_out waits for both, for s A, r B1 and the values.
    // (s2: the G2 walk's stream -- its back end follows it without a hop; in a stream of batches it goes to sC, where
    // it does not hold up the next batch's G2 walk)
    hipStream_t sG = lone ? s2 : D.sC;
    if (!lone) RLN_HIP(hipStreamWaitEvent(D.sC, S.evB2, 0));
    sum2(sG);
    if (fin_pp) hipLaunchKernelGGL(k_add_partial, dim3(pg, 1), dim3(64), 0, sG, S.sums1.p, S.sums2.p, pp_p, B, nbp, task_sel({3}), (const G1XYZZ*)nullptr);
    // B's side of the output right here (fold, inversion, bytes): see k_fin_out_b2
    hipLaunchKernelGGL(k_fin_out_b2, dim3(pg), dim3(64), 0, sG, S.sums2.p, S.coords.p, S.comp.p, B, nbp);
    if (lone) RLN_HIP(hipEventRecord(S.evB2, s2));
    RLN_HIP(hipEventRecord(S.evV, sV));
    // The C segment and A's / C's side of the output right behind the walk of the h rows, on that walk's stream: the
    // chain NTT -> h -> walk -> sum -> output crosses no stream (each hop is 50 - 100 us).  The copies home follow B's
    // bytes on the G2 chain's stream (lone: the front-end stream) and wait for this chain's event.
    // (Only for a lone batch: in a stream the front-end stream must be free for the batch after next -- there the C
    // segment stays on sC, behind evB, which covers both G1 walks.)
    hipStream_t sAC = lone ? sA2 : sF;
    if (lone) {
      sF = sA;
      MARK(9, sF);
      RLN_HIP(hipStreamWaitEvent(sAC, S.evE, 0));   // the early G1 walk: the C segment's h-independent rows
    } else {
      MARK(9, sF);
      RLN_HIP(hipStreamWaitEvent(sF, S.evB, 0));
    }
    sum1(sAC, {2, 5});
    if (fin_pp) hipLaunchKernelGGL(k_add_partial, dim3(pg, 1), dim3(64), 0, sAC, S.sums1.p, S.sums2.p, pp_p, B, nbp, task_sel({2}), (const G1XYZZ*)nullptr);
    if (fin_pp && fused) {   // + s pi_a + r rho (k_pp_smul, long done)
      RLN_HIP(hipStreamWaitEvent(sAC, S.evP, 0));
      hipLaunchKernelGGL(k_add_partial, dim3(pg, 1), dim3(64), 0, sAC, S.sums1.p, S.sums2.p, pp_p, B, nbp, task_sel({4}), (const G1XYZZ*)S.prod.p);
    }
    RLN_HIP(hipStreamWaitEvent(sAC, S.evA, 0));   // A affine, s A and r B1
    // A's and C's side of the output (fold of the C segment, inversion, bytes): see k_fin_out_ac
    if (fused)
      hipLaunchKernelGGL(k_fin_out_ac_fused, dim3(pg), dim3(64), 0, sAC, S.sums1.p, S.affA.p, S.coords.p, S.comp.p, B, nbp);
    else
      hipLaunchKernelGGL(k_fin_out_ac, dim3(pg), dim3(64), 0, sAC, S.sums1.p, S.prod.p, S.affA.p, S.coords.p, S.comp.p, B, nbp);
    if (lone) {   // (not lone: sG = sF = sC, in order)
      RLN_HIP(hipEventRecord(S.evA, sAC));        // (the wait above took the A sums' record; from here: "A's and C's bytes are there")
      RLN_HIP(hipStreamWaitEvent(sF, S.evA, 0));
    }
    RLN_HIP(hipStreamWaitEvent(sF, S.evV, 0));
  } else {
    if (tiny_partial) {   // the G2 sums right behind the G2 walk, on its stream, beside the G1 sums on sC
      sum2(s2);
      RLN_HIP(hipEventRecord(S.evB2, s2));
    }
    if (!values_front) RLN_HIP(hipEventRecord(S.evV, sV));
    if (compact) {
      // every walk's sums behind it on its own stream: the G1 sums run in the G1 stream's gap, with no G1 walk beside
      // them; fold, finalize and the results home follow the G2 sums and wait for the G1 sums and the values
      hipStream_t sS1 = D.st[role[ROLE_SUMS1]];
      if (P1.ngroups)
        hipLaunchKernelGGL(k_sum_ranges<Fq>, dim3(pg, P1.ngroups), dim3(64), 0, sS1, S.part1.p, P1.groups.p, P1.ngroups,
                           S.grp1.p, B, nbp);
      hipLaunchKernelGGL(k_sum_ranges<Fq>, dim3(pg, P1.nseg), dim3(64), 0, sS1, S.grp1.p, P1.segs.p, P1.nseg, S.sums1.p, B, nbp);
      RLN_HIP(hipEventRecord(S.evB, sS1));
      MARK(9, sC);   // (`finalize` here: from the end of the G2 walk; the G1 sums above are on the G1 stream, in no span)
      if (P2.ngroups)
        hipLaunchKernelGGL(k_sum_ranges<Fq2>, dim3(pg, P2.ngroups), dim3(64), 0, sC, S.part2.p, P2.groups.p, P2.ngroups,
                           S.grp2.p, B, nbp);
      hipLaunchKernelGGL(k_sum_ranges<Fq2>, dim3(pg, P2.nseg), dim3(64), 0, sC, S.grp2.p, P2.segs.p, P2.nseg, S.sums2.p, B, nbp);
      RLN_HIP(hipStreamWaitEvent(sC, S.evB, 0));
      RLN_HIP(hipStreamWaitEvent(sC, S.evV, 0));
    } else {
      RLN_HIP(hipStreamWaitEvent(sC, S.evV, 0));
      RLN_HIP(hipStreamWaitEvent(sC, S.evB, 0));
      if (tiny_partial) sum1(sC, {0, 1, 2, 3, 4, 5});
      RLN_HIP(hipStreamWaitEvent(sC, S.evB2, 0));
      MARK(9, sC);
    }
  }
  if (early || tiny_partial || compact) {
  } else if (small) {   // (here: a small partial batch) lanes = partial sums (k_sum_tree)
    sum1(sC, {0, 1, 2, 3, 4, 5});
    sum2(sC);
  } else {
    if (P1.ngroups)
      hipLaunchKernelGGL(k_sum_ranges<Fq>, dim3(pg, P1.ngroups), dim3(64), 0, sC, S.part1.p, P1.groups.p, P1.ngroups,
                         S.grp1.p, B, nbp);
    if (P2.ngroups)
      hipLaunchKernelGGL(k_sum_ranges<Fq2>, dim3(pg, P2.ngroups), dim3(64), 0, sC, S.part2.p, P2.groups.p, P2.ngroups,
                         S.grp2.p, B, nbp);
    hipLaunchKernelGGL(k_sum_ranges<Fq>, dim3(pg, P1.nseg), dim3(64), 0, sC, S.grp1.p, P1.segs.p, P1.nseg, S.sums1.p, B, nbp);
    hipLaunchKernelGGL(k_sum_ranges<Fq2>, dim3(pg, P2.nseg), dim3(64), 0, sC, S.grp2.p, P2.segs.p, P2.nseg, S.sums2.p, B, nbp);
  }
  if (!early) {   // sums of the second halves through phi, onto the first: afterwards sums1[0..3) / sums2[0]
    if (P1.nseg / D.nh == G1_SHARED_SEGS) {   // (a big batch that walked the shared rows once: their two sums join A and B1)
      hipLaunchKernelGGL(k_glv_fold, dim3(pg, 6), dim3(64), 0, sC, S.sums1.p, S.sums2.p, G1_SHARED_SEGS, B, nbp,
                         task_sel({0, 1, 2, SEG_SHARED_EQ, SEG_SHARED_OPP, G1_SHARED_SEGS}));   // (the last: the G2 sum)
      hipLaunchKernelGGL(k_shared_join, dim3(pg, 2), dim3(64), 0, sC, S.sums1.p, B, nbp);
    } else {
      hipLaunchKernelGGL(k_glv_fold, dim3(pg, 4), dim3(64), 0, sC, S.sums1.p, S.sums2.p, 3u, B, nbp, all4);
    }
  }
  if (mode == PROVE_PARTIAL) {
    hipLaunchKernelGGL(k_partial_out, dim3(pg, 4), dim3(64), 0, sC, S.sums1.p, S.sums2.p, S.pp_out.p, B, nbp);
    RLN_HIP(hipGetLastError());
    d2h(S.h_pp, S.pp_out.p, n * 320, sC);
  } else {
    if (!early) {   // (here: a big batch)
      if (mode == PROVE_FINISH)
        hipLaunchKernelGGL(k_add_partial, dim3(pg, 4), dim3(64), 0, sC, S.sums1.p, S.sums2.p, pp_p, B, nbp, all4, (const G1XYZZ*)nullptr);
      hipLaunchKernelGGL(k_fin_affine, dim3(pg, 3), dim3(64), 0, sC, S.sums1.p, S.sums2.p, S.affA.p, S.affB1.p,
                         S.affB2.p, B, nbp, all3);
      hipLaunchKernelGGL(k_fin_smul, dim3(pg, 2), dim3(64), 0, sC, S.affA.p, S.affB1.p, rs_p, S.tbl.p, S.prod.p, B,
                         nbp);
      hipLaunchKernelGGL(k_fin_out, dim3(pg), dim3(64), 0, sF, S.sums1.p, S.prod.p, S.affA.p, S.affB2.p, S.coords.p,
                         S.comp.p, B, nbp);
    }
    RLN_HIP(hipGetLastError());
    d2h(S.h_comp, S.comp.p, n * 128, sF);
    d2h(S.h_values, S.values.p, n * 160, sF);
  }
  d2h(S.h_err, S.err.p, n * 4, sF);
  MARK(10, sF);
  RLN_HIP(hipEventRecord(S.evC, sF));
  S.used = true;
  S.wiped = false;
  S.n = n;
  D.last = &S;
  return S.ticket;
}

void Prover::sync() { sync_measure(false); }

void Prover::sync_measure(bool last_only) {
  Impl& D = *d_;
  D.sync_all();
  if (D.last) {
    // stage spans, averaged over the batches still held in the workspace slots (the last <= nslot launches of the
    // same kind): in the pipeline a span includes whatever shared the chip with it
    const int pairs[PROVER_STAGES][2] = {{1, 2}, {12, 3}, {3, 4}, {5, 6}, {14, 7}, {11, 8}, {9, 10}, {0, 13}};
    float acc[PROVER_STAGES] = {0};
    int cnt = 0;
    for (int k = 0; k < D.nslot; k++) {
      Slot& S = D.slot[k];
      if (!S.used || !S.marked || S.mode != D.last->mode || S.n != D.last->n || (last_only && &S != D.last)) continue;
      for (int i = 0; i < PROVER_STAGES; i++) {
        float ms = 0;
        RLN_HIP(hipEventElapsedTime(&ms, S.t[pairs[i][0]], S.t[pairs[i][1]]));
        acc[i] += ms;
      }
      cnt++;
    }
    for (int i = 0; i < PROVER_STAGES; i++) D.ms[i] = cnt ? acc[i] / cnt : 0.f;
  }
}

void Prover::run(size_t n, int mode) {
  sync();  // nothing else in flight: the stage spans of this batch are those of the stages by themselves
  run_async(n, mode);
  sync_measure(true);
}

void Prover::upload_partial(size_t n, const uint8_t* coords320) {
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  Impl& D = *d_;
  D.sync_all();
  RLN_HIP(hipMemcpyAsync(D.pp_in.p, coords320, n * 320, hipMemcpyHostToDevice, D.sA));
  RLN_HIP(hipStreamSynchronize(D.sA));
}

void Prover::download_partial(size_t n, uint8_t* coords320) {
  Impl& D = *d_;
  sync();
  if (!D.last || D.last->mode != PROVE_PARTIAL || n > D.last->n) throw Error("the last run was not a partial-proof run");
  memcpy(coords320, D.last->h_pp, n * 320);
}

const std::vector<uint8_t>& Prover::known_mask() const { return d_->known; }

void Prover::stage_ms(float out[PROVER_STAGES]) const {
  for (int i = 0; i < PROVER_STAGES; i++) out[i] = d_->ms[i];
}

void Prover::walk_clock_mhz(double out[2]) {
  Impl& D = *d_;
  sync();
  unsigned long long h[4] = {0, 0, 0, 0};
  if (D.walk_clk.p) {
    RLN_HIP(hipMemcpy(h, D.walk_clk.p, sizeof(h), hipMemcpyDeviceToHost));
    RLN_HIP(hipMemset(D.walk_clk.p, 0, sizeof(h)));
  }
  for (int g = 0; g < 2; g++) out[g] = h[2 * g + 1] ? 100.0 * (double)h[2 * g] / (double)h[2 * g + 1] : 0.0;
}

void Prover::download(size_t n, ProofOut* out) {
  if (n > B_) throw Error("batch larger than the prover workspace (max_batch)");
  Impl& D = *d_;
  sync();
  if (!D.last) throw Error("no resident run to read from");
  Slot& S = *D.last;
  std::vector<uint32_t> coords(n * 64);
  RLN_HIP(hipMemcpyAsync(coords.data(), S.coords.p, n * 256, hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
  // Without the proof-values kernel (a single message-id circuit whose graph does not carry the shipped input
  // names) the five values are the circuit's own public outputs w[1..6] = y, root, nullifier, x, ext -- the same
  // numbers for every satisfying witness (witness.rs:759-804).  Other shapes (multi message-id) are read by the
  // caller through fetch_public; their `values` are zero here, never stale.
  std::vector<uint8_t> pub;
  const bool from_public = !D.have_values_kernel && D.ni == 6;
  if (from_public) fetch_public(n, &pub);
  for (size_t i = 0; i < n; i++) {
    memcpy(out[i].compressed, S.h_comp + i * 128, 128);
    memcpy(out[i].coords, coords.data() + i * 64, 256);
    if (D.have_values_kernel)
      memcpy(out[i].values, S.h_values + i * 40, 160);
    else if (from_public)
      memcpy(out[i].values, pub.data() + i * 160, 160);
    else
      memset(out[i].values, 0, 160);
    out[i].error = S.h_err[i];
  }
}

void Prover::fetch_public(size_t n, std::vector<uint8_t>* out_le) {
  Impl& D = *d_;
  sync();
  if (!D.last || n > B_) throw Error("no resident run to read from");
  fetch_public_slot(D.last, n, out_le);
}

// the slot's batch must have finished (its evC passed); sC is in stream order behind it
void Prover::fetch_public_slot(void* slot, size_t n, std::vector<uint8_t>* out_le) {
  Impl& D = *d_;
  Slot& S = *(Slot*)slot;
  const uint32_t npub = D.ni - 1;
  DevBuf<uint32_t> tmp(n * npub * 8);
  hipLaunchKernelGGL(k_public_signals, dim3(div_up(n, 64), div_up(npub, 4)), dim3(64, 4), 0, D.sC, S.V.p,
                     D.sig2node.p, npub, (uint32_t)B_, (uint32_t)n, tmp.p);
  out_le->resize(n * npub * 32);
  RLN_HIP(hipMemcpyAsync(out_le->data(), tmp.p, out_le->size(), hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
}

void Prover::fetch_witness(size_t p, std::vector<uint8_t>* w_le) {
  Impl& D = *d_;
  sync();
  if (!D.last || p >= B_) throw Error("no resident run to read from");
  DevBuf<uint32_t> tmp((size_t)D.NS * 8);
  hipLaunchKernelGGL(k_gather_col, dim3(div_up(D.NS, 256)), dim3(256), 0, D.sC, D.last->V.p, D.sig2node.p, D.NS,
                     (uint32_t)B_, (uint32_t)p, tmp.p);
  w_le->resize((size_t)D.NS * 32);
  RLN_HIP(hipMemcpyAsync(w_le->data(), tmp.p, w_le->size(), hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
}

void Prover::fetch_h(size_t p, std::vector<uint8_t>* h_le) {
  Impl& D = *d_;
  sync();
  if (!D.last || p >= B_) throw Error("no resident run to read from");
  DevBuf<uint32_t> tmp((size_t)D.n * 8);
  hipLaunchKernelGGL(k_gather_col, dim3(div_up(D.n, 256)), dim3(256), 0, D.sC, D.last->abc.p, (const uint32_t*)nullptr,
                     D.n, (uint32_t)B_, (uint32_t)p, tmp.p);
  h_le->resize((size_t)D.n * 32);
  RLN_HIP(hipMemcpyAsync(h_le->data(), tmp.p, h_le->size(), hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
}

void Prover::residue(uint64_t out[RESIDUE_FIELDS]) {
  Impl& D = *d_;
  sync();
  if (!D.last) throw Error("no run to read from");
  uint64_t all[RESIDUE_SLOT_FIELDS];
  residue_of(D.last, all);
  for (int k = 0; k < RESIDUE_FIELDS; k++) out[k] = all[k];
}

void Prover::residue_slot(int slot, uint64_t out[RESIDUE_SLOT_FIELDS]) {
  Impl& D = *d_;
  if (slot < 0 || slot >= D.nslot) throw Error("residue_slot: no such workspace slot");
  sync();
  residue_of(&D.slot[slot], out);
}

// the pipeline has been drained (sync): the wipes' stream too
void Prover::residue_of(void* slot, uint64_t out[RESIDUE_SLOT_FIELDS]) {
  Impl& D = *d_;
  Slot& S = *(Slot*)slot;
  constexpr int NDEV = RESIDUE_SLOT_FIELDS;
  DevBuf<unsigned long long> cnt(NDEV);
  RLN_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes(), D.sC));
  auto count = [&](int k, const void* p, size_t bytes) {
    if (p && bytes >= 16)
      hipLaunchKernelGGL(k_count_nonzero16, dim3(2048), dim3(256), 0, D.sC, (const uint4*)p, bytes / 16, cnt.p + k);
  };
  count(0, S.digits.p, S.digits.bytes());
  count(1, S.digits2.p, S.digits2.bytes());
  count(2, S.abc.p, S.abc.bytes());
  count(3, S.part1.p, S.part1.bytes());
  count(4, S.part2.p, S.part2.bytes());
  for (auto* b : {&S.grp1, &S.sums1, &S.prod, &S.tbl}) count(3, b->p, b->bytes());
  for (auto* b : {&S.grp2, &S.sums2}) count(4, b->p, b->bytes());
  count(3, S.affA.p, S.affA.bytes());
  count(3, S.affB1.p, S.affB1.bytes());
  count(4, S.affB2.p, S.affB2.bytes());
  count(5, S.inputs.p, S.inputs.bytes());
  count(5, S.rs.p, S.rs.bytes());
  count(5, D.wgiven.p, D.wgiven.bytes());   // a supplied witness (upload_witness): wiped with the resident inputs
  count(5, S.idx.p, S.idx.bytes());   // the leaf indices of a batch submitted by member, device and (below) pinned copy
  count(8, S.V29.p, S.V29.bytes());
  RLN_HIP(hipGetLastError());
  unsigned long long h[NDEV];
  RLN_HIP(hipMemcpyAsync(h, cnt.p, sizeof h, hipMemcpyDeviceToHost, D.sC));
  RLN_HIP(hipStreamSynchronize(D.sC));
  for (int k = 0; k < NDEV; k++) out[k] = h[k];
  for (size_t i = 0; i + 1 < B_; i += 2) out[5] += (S.h_idx[i] | S.h_idx[i + 1]) ? 1 : 0;
  // the pinned buffers, read by the host: the inputs | (r, s) regions of the staging (not the partial points behind them)
  // and the hints, whole
  auto host16 = [](const void* p, size_t bytes) {
    const uint64_t* w = (const uint64_t*)p;
    uint64_t nz = 0;
    for (size_t i = 0; i + 1 < bytes / 8; i += 2) nz += (w[i] | w[i + 1]) ? 1 : 0;
    return nz;
  };
  out[6] = host16(S.h_in, B_ * ((size_t)D.NI * 32 + 64));
  out[7] = host16(S.h_hints, (size_t)HINT_PROOFS * 64 * 32);
  out[9] = 0;
}

}  // namespace rlnamd
