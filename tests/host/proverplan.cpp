// The prover's host planning (zerokit_amd/csrc/prover_plan.cpp) without a GPU: the k_witness29 program run by a host
// emulator with the product's own field arithmetic, the invariants of every table-walk plan, the hints against a plain
// evaluation of the graph, and the shape decision of Prover::enqueue.  Driven by tests/test_prover_plan_host.py and,
// under ASan / UBSan, by tests/host/sanitize_main.cpp.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "field.h"
#include "prover_plan.h"
#include "witness_ops.h"
#include "witness_sched.h"
#include "zkey.h"

using namespace rlnamd;

static std::string g_err;

namespace {

struct Planning {   // what Prover::Prover derives before it uploads anything
  NamedInputs named;
  HintChains chains;
  std::vector<std::vector<uint32_t>> cuts;
  std::vector<uint8_t> is_cut;
};
void plan_hints(const Graph& g, uint32_t ni, Planning* P) {
  P->named = find_named_inputs(g, ni);
  P->chains.configure(P->named, ProverTuning().hint_chains);
  P->is_cut.assign(g.nodes.size(), 0);
  if (P->named.have_hint_slots && P->chains.count() <= 64) P->cuts = find_hint_cuts(g, P->named, P->chains);
  for (const auto& nodes : P->cuts)
    for (uint32_t n : nodes) P->is_cut[n] = 1;
}

// the k_witness29 program on the host: ring by program index, constants, far operands by slot
uint32_t run_program(const Graph& g, const Wit29Program& W, const uint8_t* inputs_le, std::vector<Fr>* stored) {
  std::vector<Fr> ring(W.nprog, Fr::zero());   // value of every program node; a ring reference must be younger than WIT29_RING
  stored->assign(W.slot2node.size(), Fr::zero());
  std::vector<uint8_t> written(W.slot2node.size(), 0);
  uint32_t err = 0;
  for (uint32_t i = 0; i < W.nprog; i++) {
    const GNode29& d = W.prog[i];
    const uint32_t op = d.w0 & 0xFF, slot = d.w0 >> 16;
    auto operand = [&](uint32_t x) -> Fr {
      const uint32_t kind = x & OPK_MASK, idx = x & ~OPK_MASK;
      if (kind == OPK_CONST) {
        if (idx >= g.constants.size()) throw std::runtime_error("constant index out of range");
        return g.constants[idx];
      }
      if (kind == OPK_RING) {
        if (idx >= i || i - idx >= WIT29_RING) throw std::runtime_error("ring reference reaches back WIT29_RING or more");
        return ring[idx];
      }
      if (kind != OPK_FAR) throw std::runtime_error("unknown operand kind");
      if (idx >= stored->size() || !written[idx]) throw std::runtime_error("far operand reads a slot not yet stored");
      return (*stored)[idx];
    };
    Fr v = Fr::zero();
    switch (op) {
      case G_INPUT: {
        if (d.a >= g.inputs_size) throw std::runtime_error("input index out of range");
        uint32_t c[8];
        memcpy(c, inputs_le + (size_t)d.a * 32, 32);
        if (limbs_geq(c, FrParams::MOD)) err = WERR_INPUT_RANGE;
        v = Fr::from_canonical(c);
        break;
      }
      case G_CONST:
        if (d.a >= g.constants.size()) throw std::runtime_error("constant index out of range");
        v = g.constants[d.a];
        break;
      case G_MUL: v = operand(d.a) * operand(d.b); break;
      case W29_FMA: v = operand(d.a) * operand(d.b) + operand(d.c); break;
      case G_ADD: v = operand(d.a) + operand(d.b); break;
      case G_SUB: v = operand(d.a) - operand(d.b); break;
      case G_NEG: v = operand(d.a).neg(); break;
      case G_TERN: v = operand(d.a).is_zero() ? operand(d.c) : operand(d.b); break;
      default: v = witness_slow_op(op, operand(d.a), op == G_ID ? Fr::zero() : operand(d.b), &err); break;
    }
    ring[i] = v;
    if (d.w0 & W29_STORE) {
      if (slot >= stored->size()) throw std::runtime_error("store slot out of range");
      (*stored)[slot] = v;
      written[slot] = 1;
    }
  }
  for (size_t k = (size_t)W.nprog; k < W.prog.size(); k++)
    if (W.prog[k].w0 | W.prog[k].a | W.prog[k].b | W.prog[k].c) throw std::runtime_error("program padding is not zero");
  if (W.prog.size() < ((size_t)W.nprog / WIT29_CH + 3) * WIT29_CH || W.prog.size() % WIT29_CH)
    throw std::runtime_error("program not padded by two chunks");
  return err;
}

// ---- walk plans
typedef std::tuple<uint32_t, uint32_t, uint32_t> Entry;   // (table row, digit id, GLV half)
struct PlanCheck {
  const char* family;
  int mode;
  std::string* log;
  int failures = 0;
  void fail(const std::string& what) {
    failures++;
    if (log->size() < 4000) *log += std::string(family) + " mode " + std::to_string(mode) + ": " + what + "\n";
  }
};

std::vector<Entry> expected_entries(const std::vector<VRow>& vrows, int mode, const std::vector<uint8_t>& known) {
  std::vector<Entry> e;
  for (const VRow& v : vrows) {
    const bool is_known = v.sid < known.size() && known[v.sid];
    const bool walked = mode == PROVE_FULL || (mode == PROVE_PARTIAL ? is_known : !is_known);
    for (uint32_t h = 0; walked && h < GLV_HALVES; h++) e.push_back(Entry(v.k, v.dig_sid, h));
  }
  std::sort(e.begin(), e.end());
  return e;
}

// every invariant of one plan; returns the (row, digit id, half) entries it walks, sorted
std::vector<Entry> check_plan(const WalkPlan& P, const std::vector<VRow>& vrows, uint32_t nseg, uint32_t chunk_pts, int mode,
                              const std::vector<uint8_t>& known, uint32_t npaired, bool pair_chunks, uint32_t block_pts,
                              uint32_t h_first, uint32_t h_end, PlanCheck& C) {
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seg_of;   // (row, digit id) -> output segment
  std::vector<uint32_t> seg_of_row(vrows.size() * 2 + 4, 0xFFFFFFFFu);
  for (const VRow& v : vrows) {
    seg_of[{v.k, v.dig_sid}] = v.seg;
    if (v.sid == v.dig_sid) seg_of_row[v.k] = v.seg;   // (a fused family walks a row a second time, into the C segment)
  }
  auto is_h = [&](uint32_t sid) { return sid >= h_first && sid < h_end; };
  const uint32_t nchunks = (uint32_t)P.chunks.size();
  if (P.rows.size() != P.rsid.size() || P.prows.size() != P.prsid.size()) C.fail("rows and scalar ids differ in length");
  if (P.nseg != nseg * GLV_HALVES || P.segchunks.size() != P.nseg || P.segs.size() != P.nseg || P.segblocks.size() != P.nseg)
    C.fail("segment count");
  // segchunks tile [0, nchunks); groups / segs and segblocks tile every segment
  uint32_t at = 0, gat = 0, bat = 0, maxblk = 0;
  std::vector<uint32_t> seg_of_chunk(nchunks, 0xFFFFFFFFu);
  for (uint32_t sg = 0; sg < P.segchunks.size(); sg++) {
    const ChunkDesc r = P.segchunks[sg];
    if (r.pt_begin != at || r.pt_end < r.pt_begin || r.pt_end > nchunks) { C.fail("segchunks do not tile the chunks"); return {}; }
    for (uint32_t c = r.pt_begin; c < r.pt_end; c++) seg_of_chunk[c] = sg;
    at = r.pt_end;
    if (sg < P.segs.size()) {
      const ChunkDesc gr = P.segs[sg];
      if (gr.pt_begin != gat || gr.pt_end > P.groups.size() || gr.pt_end < gr.pt_begin) { C.fail("segs do not tile the groups"); return {}; }
      uint32_t cat = r.pt_begin;
      for (uint32_t k = gr.pt_begin; k < gr.pt_end; k++) {
        if (P.groups[k].pt_begin != cat || P.groups[k].pt_end <= cat || P.groups[k].pt_end - cat > 16) C.fail("a group is not <= 16 consecutive chunks");
        cat = P.groups[k].pt_end;
      }
      if (cat != r.pt_end) C.fail("the groups of a segment do not cover its chunks");
      gat = gr.pt_end;
    }
    if (sg < P.segblocks.size()) {
      const ChunkDesc br = P.segblocks[sg];
      const uint32_t want = (r.pt_end - r.pt_begin + block_pts - 1) / block_pts;
      if (br.pt_begin != bat || br.pt_end - br.pt_begin != want) C.fail("segblocks do not cover the segment's chunks once");
      bat = br.pt_end;
      maxblk = std::max(maxblk, want);
    }
  }
  if (at != nchunks) C.fail("segchunks end before the last chunk");
  if (gat != P.groups.size()) C.fail("segs end before the last group");
  if (bat != P.nblocks || maxblk != P.maxblk) C.fail("nblocks / maxblk");
  // chunks: consecutive ranges of `rows`, none above chunk_pts, every row of a chunk in the chunk's segment; empty chunks
  // are the slots of the pair chunks
  std::vector<Entry> got;
  std::vector<uint8_t> is_slot(nchunks, 0), in_ids(nchunks, 0);
  uint32_t rat = 0;
  for (uint32_t c = 0; c < nchunks; c++) {
    const ChunkDesc r = P.chunks[c];
    if (r.pt_end == r.pt_begin) {
      if (r.pt_begin != 0) C.fail("an empty chunk that is not {0, 0}");
      is_slot[c] = 1;
      continue;
    }
    if (r.pt_begin != rat || r.pt_end > P.rows.size()) { C.fail("chunks do not tile the rows"); return {}; }
    if (r.pt_end - r.pt_begin > chunk_pts) C.fail("a chunk exceeds chunk_pts");
    rat = r.pt_end;
    for (uint32_t e = r.pt_begin; e < r.pt_end; e++) {
      const uint32_t w = P.rows[e], k = w & ROW_INDEX, h = w >> 31;
      if (((w & ROW_PAIRED) != 0) != (k < npaired)) C.fail("ROW_PAIRED flag");
      auto it = seg_of.find({k, P.rsid[e]});
      if (it == seg_of.end()) { C.fail("a row the family does not hold"); continue; }
      if (seg_of_chunk[c] != h * nseg + it->second) C.fail("a row outside its chunk's segment");
      got.push_back(Entry(k, P.rsid[e], h));
    }
  }
  if (rat != P.rows.size()) C.fail("rows beyond the last chunk");
  if (!pair_chunks && !P.pchunks.empty()) C.fail("pair chunks in a plan without them");
  // early and late ids partition the non-pair chunks; late chunks hold only h rows, early chunks none
  for (int late = 0; late < 2; late++)
    for (uint32_t c : (late ? P.late_ids : P.early_ids)) {
      if (c >= nchunks || is_slot[c] || in_ids[c]) { C.fail("early / late ids are not a partition"); continue; }
      in_ids[c] = 1;
      for (uint32_t e = P.chunks[c].pt_begin; e < P.chunks[c].pt_end; e++)
        if (is_h(P.rsid[e]) != (late != 0)) C.fail(late ? "a late chunk holds a row that does not depend on h" : "an early chunk holds an h row");
    }
  for (uint32_t c = 0; c < nchunks; c++)
    if (!is_slot[c] && !in_ids[c]) C.fail("a chunk in neither the early nor the late ids");
  // pair chunks: ranges of prows, none above chunk_pts; two distinct empty slots inside the members' segments
  if (P.pout.size() != 2 * P.pchunks.size()) C.fail("pout length");
  std::vector<uint8_t> slot_taken(nchunks, 0);
  uint32_t pat = 0;
  for (size_t c = 0; c < P.pchunks.size() && P.pout.size() == 2 * P.pchunks.size(); c++) {
    const ChunkDesc r = P.pchunks[c];
    if (r.pt_begin != pat || r.pt_end <= r.pt_begin || r.pt_end > P.prows.size()) { C.fail("pair chunks do not tile prows"); return {}; }
    if (r.pt_end - r.pt_begin > chunk_pts) C.fail("a pair chunk exceeds chunk_pts");
    pat = r.pt_end;
    const uint32_t o0 = P.pout[2 * c], o1 = P.pout[2 * c + 1];
    if (o0 >= nchunks || o1 >= nchunks || o0 == o1 || !is_slot[o0] || !is_slot[o1] || slot_taken[o0] || slot_taken[o1]) {
      C.fail("a pair chunk's slots are not two distinct empty chunks of its own");
      continue;
    }
    slot_taken[o0] = slot_taken[o1] = 1;
    for (uint32_t e = r.pt_begin; e < r.pt_end; e++) {
      const uint32_t w = P.prows[e], q = w & ROW_INDEX, h = w >> 31;
      if (!(w & ROW_PAIRED) || (q & 1) || q + 1 >= npaired) { C.fail("a pair row that is not the even member of a pair"); continue; }
      if (seg_of_chunk[o0] != h * nseg + seg_of_row[q] || seg_of_chunk[o1] != h * nseg + seg_of_row[q + 1]) C.fail("a pair slot outside its member's segment");
      if (is_h(P.prsid[e])) C.fail("a pair under an h scalar");
      got.push_back(Entry(q, P.prsid[e], h));
      got.push_back(Entry(q + 1, P.prsid[e], h));
    }
  }
  if (pat != P.prows.size()) C.fail("prows beyond the last pair chunk");
  for (uint32_t c = 0; c < nchunks; c++)
    if (is_slot[c] && !slot_taken[c]) C.fail("an empty chunk no pair chunk fills");
  std::sort(got.begin(), got.end());
  if (got != expected_entries(vrows, mode, known)) C.fail("the chunks' rows are not the rows the mode walks, each (row, half) once");
  return got;
}

}  // namespace

extern "C" {
const char* proverplan_error() { return g_err.c_str(); }

// The k_witness29 program of `graph`, compiled as the prover compiles it (cut nodes of the hints included) and run over
// inputs_le.  witness_out_le: num_signals x 32 canonical LE.  stats: [0] program nodes, [1] stored values, [2] error flags,
// [3] non-empty cut sets, [4] W29_RED nodes, [5] W29_RARE nodes, [6] fused products
int proverplan_run_program(const uint8_t* graph, size_t len, uint32_t ni, const uint8_t* inputs_le, size_t inputs_size,
                           uint8_t* witness_out_le, uint32_t* stats) {
  try {
    const Graph g = parse_graph(graph, len);
    if (inputs_size != g.inputs_size) throw std::runtime_error("inputs size mismatch");
    Planning P;
    plan_hints(g, ni, &P);
    const Wit29Program W = compile_witness29(g, P.is_cut);
    if (W.slot2node.size() >= 65536) throw std::runtime_error("a stored slot does not fit 16 bits");
    for (uint32_t sl = 0; sl < W.slot2node.size(); sl++)
      if (W.store_slot[W.slot2node[sl]] != sl) throw std::runtime_error("store_slot is not the inverse of slot2node");
    std::vector<Fr> stored;
    stats[2] = run_program(g, W, inputs_le, &stored);
    for (size_t i = 0; i < g.signals.size(); i++) {
      const uint32_t sl = W.store_slot[g.signals[i]];
      if (sl == 0xFFFFFFFFu) throw std::runtime_error("a witness signal is not stored");
      uint32_t c[8];
      stored[sl].to_canonical(c);
      memcpy(witness_out_le + 32 * i, c, 32);
    }
    for (const auto& nodes : P.cuts)
      for (uint32_t n : nodes)
        if (W.store_slot[n] == 0xFFFFFFFFu) throw std::runtime_error("a cut node is not stored");
    stats[0] = W.nprog;
    stats[1] = (uint32_t)W.slot2node.size();
    stats[3] = 0;
    for (const auto& nodes : P.cuts) stats[3] += !nodes.empty();
    stats[4] = stats[5] = 0;
    for (uint32_t i = 0; i < W.nprog; i++) {
      stats[4] += (W.prog[i].w0 & W29_RED) != 0;
      stats[5] += (W.prog[i].w0 & W29_RARE) != 0;
    }
    stats[6] = (uint32_t)g.nodes.size() - W.nprog;
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}

// Every plan family of the prover in every mode it is built for, checked against the invariants above.  Returns the
// number of failures (-1: an exception); log: what failed; stats: [0] plans checked, [1] G1 points, [2] pair members,
// [3] G2 points, [4] pair chunks of the full throughput plan
int proverplan_check_plans(const uint8_t* zkey, size_t zlen, const uint8_t* graph, size_t glen, char* log, size_t log_len,
                           uint32_t* stats) {
  try {
    const Zkey zk = parse_arkzkey(zkey, zlen);
    const Graph g = parse_graph(graph, glen);
    const uint32_t NS = (uint32_t)g.signals.size(), nc = (uint32_t)zk.num_constraints, ni = (uint32_t)zk.num_instance_variables;
    uint32_t n = 1;
    while (n < nc + ni) n <<= 1;
    const std::vector<uint8_t> node_known = wl_known_nodes(g);
    std::vector<uint8_t> known(NS);
    for (uint32_t i = 0; i < NS; i++) known[i] = node_known[g.signals[i]];
    const G1Rows R1 = g1_walk_rows(zk, NS, n, ni);
    const G2Rows R2 = g2_walk_rows(zk, NS, n);
    if (R1.rows.size() != R1.pts.size() || R1.sids.size() != R1.pts.size() || R2.rows.size() != R2.pts.size() || (R1.npaired & 1))
      throw std::runtime_error("row lists and point lists differ in length");
    for (uint32_t q = 0; q + 1 < R1.npaired; q += 2)
      if (R1.sids[q] != R1.sids[q + 1] || R1.sids[q] >= NS) throw std::runtime_error("pair members do not share a witness scalar");
    std::string text;
    int failures = 0;
    uint32_t plans = 0;
    struct Family { const char* name; const std::vector<VRow>* rows; uint32_t nseg, chunk_pts; bool pairs; uint32_t block_pts; uint32_t npaired; bool fused, has_h; };
    const Family fam[] = {
        {"plan1", &R1.rows, 3, 16, true, SUM_TREE_LANES, R1.npaired, false, true},
        {"plan1s", &R1.rows, 3, 4, false, SUM_TREE_LANES, R1.npaired, false, true},
        {"plan1t (plain rows)", &R1.rows, 3, 1, false, SUM_TREE_LANES / 2, R1.npaired, false, true},
        {"plan1f", &R1.fused, 3, 4, false, SUM_TREE_LANES, R1.npaired, true, true},
        {"plan1tf", &R1.fused, 3, 1, false, SUM_TREE_LANES / 2, R1.npaired, true, true},
        {"plan2", &R2.rows, 1, 8, false, SUM_TREE_LANES, 0, false, false},
        {"plan2s", &R2.rows, 1, 2, false, SUM_TREE_LANES, 0, false, false},
        {"plan2t", &R2.rows, 1, 1, false, SUM_TREE_LANES / 2, 0, false, false},
    };
    for (const Family& F : fam) {
      std::vector<Entry> walked[3];
      for (int mode : {(int)PROVE_FULL, (int)PROVE_PARTIAL, (int)PROVE_FINISH}) {
        const WalkPlan P = make_walk_plan(*F.rows, F.nseg, F.chunk_pts, mode, known, F.npaired, F.pairs, F.block_pts);
        PlanCheck C{F.name, mode, &text};
        walked[mode] = check_plan(P, *F.rows, F.nseg, F.chunk_pts, mode, known, F.npaired, F.pairs, F.block_pts, F.has_h ? NS : 0, F.has_h ? NS + n : 0, C);
        failures += C.failures;
        plans++;
        if (F.pairs && mode == PROVE_FULL) stats[4] = (uint32_t)P.pchunks.size();
      }
      if (!F.fused) {   // partial and finish are disjoint and their union is the full walk
        std::vector<Entry> both;
        std::set_intersection(walked[1].begin(), walked[1].end(), walked[2].begin(), walked[2].end(), std::back_inserter(both));
        std::vector<Entry> all(walked[1]);
        all.insert(all.end(), walked[2].begin(), walked[2].end());
        std::sort(all.begin(), all.end());
        if (!both.empty() || all != walked[0]) {
          failures++;
          text += std::string(F.name) + ": partial and finish do not partition full\n";
        }
      }
    }
    stats[0] = plans;
    stats[1] = (uint32_t)R1.pts.size();
    stats[2] = R1.npaired;
    stats[3] = (uint32_t)R2.pts.size();
    snprintf(log, log_len, "%s", text.c_str());
    return failures;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Hints of one proof against a plain evaluation of the graph at the discovered cut nodes, twice (the second call must
// find its chain remembered).  stats: [0] non-empty cut sets, [1] hints per proof, [2] cut nodes whose value differs from
// their hint (first call), [3] the same for the second call, [4] chain hits after the first call, [5] after the second,
// [6] values that differ between the two calls
int proverplan_check_hints(const uint8_t* graph, size_t len, uint32_t ni, const uint8_t* inputs_le, size_t inputs_size, uint32_t* stats) {
  try {
    const Graph g = parse_graph(graph, len);
    if (inputs_size != g.inputs_size) throw std::runtime_error("inputs size mismatch");
    Planning P;
    plan_hints(g, ni, &P);
    stats[0] = 0;
    for (const auto& nodes : P.cuts) stats[0] += !nodes.empty();
    stats[1] = P.chains.count();
    if (P.cuts.size() != P.chains.count()) throw std::runtime_error("no cut set for some hint");
    uint32_t err = 0;
    const std::vector<Fr> val = wl_eval_host(g, inputs_le, &err);
    if (err) throw std::runtime_error("graph evaluation failed");
    std::vector<Fr> first(P.chains.count()), second(P.chains.count());
    const uint64_t before = P.chains.hits();
    P.chains.hints(inputs_le, first.data());
    stats[4] = (uint32_t)(P.chains.hits() - before);
    HintChains::Probe pr;
    P.chains.probe(inputs_le, &pr);
    if (!pr.found) throw std::runtime_error("the chain is not remembered after its first call");
    P.chains.hints(inputs_le, second.data(), &pr);
    stats[5] = (uint32_t)(P.chains.hits() - before);
    stats[2] = stats[3] = stats[6] = 0;
    for (uint32_t j = 0; j < P.cuts.size(); j++) {
      for (uint32_t n : P.cuts[j]) {
        stats[2] += !(val[n] == first[j]);
        stats[3] += !(val[n] == second[j]);
      }
      stats[6] += !(first[j] == second[j]);
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}

// batch_shape under the default tuning (lone_force: ProverTuning::lone).  in: n, mode, inputs, partial_points, handles,
// pre_hints, idle, shared, capacity.  The prover's capabilities are those of the shipped single-message circuits: every
// interpreter, the values kernel, six instance variables, a 2^13 domain.  out: lone, small, wl_used, cone, hinted,
// probe_chains, early, fused, tiny_partial, tiny, walk_lp, g2_on_front, values_w, ntt_lds, plan1, plan2, PB, dB
void proverplan_shape(const uint32_t* in, int lone_force, uint32_t* out) {
  ProverTuning T;
  T.lone = lone_force;
  BatchQuery q;
  q.n = in[0];
  q.mode = (int)in[1];
  q.inputs = in[2];
  q.partial_points = in[3];
  q.handles = in[4];
  q.pre_hints = in[5];
  q.idle = in[6];
  q.shared = in[7];
  q.capacity = in[8];
  q.witlanes_ok = q.segs_ok = q.cone_ok = q.have_values_kernel = true;
  q.ni = 6;
  q.logn = 13;
  q.small_stride = std::max<uint32_t>(64, (std::min<uint32_t>(T.lanechunk_max, in[8]) + 63) / 64 * 64);
  const BatchShape S = batch_shape(q, T);
  const uint32_t v[18] = {S.lone, S.small, S.wl_used, S.cone, S.hinted, S.probe_chains, S.early, S.fused, S.tiny_partial,
                          S.tiny, S.walk_lp, S.g2_on_front, S.values_w, S.ntt_lds, (uint32_t)S.plan1, (uint32_t)S.plan2, S.PB, S.dB};
  memcpy(out, v, sizeof v);
}
}
