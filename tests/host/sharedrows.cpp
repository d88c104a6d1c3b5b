// The shared rows of the throughput plan (zerokit_amd/csrc/prover_plan.h: G1Rows::shared) without a GPU: which wires the
// detector finds, the structure of the five-segment plans in the three modes, which rows they walk and into which
// segment, and -- in host curve arithmetic under small scalars -- that A = s0 + s3 + s4 and B1 = s1 + s3 - s4 are the
// sums of the legacy family's segments 0 and 1.  A checksum over the legacy families and the point list pins that those
// did not move.  Driven by tests/test_shared_rows_host.py and, under ASan / UBSan, by tests/host/sharedrows_main.cpp.
//
// -DSHAREDROWS_LEGACY_ONLY leaves only sharedrows_legacy_checksum, which needs nothing but G1Rows::pts / sids / npaired /
// rows / fused: built that way against an older tree it gives the value the test records.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iterator>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "curve.h"
#include "field.h"
#include "prover_plan.h"
#include "witness_sched.h"
#include "zkey.h"

using namespace rlnamd;

static std::string g_err;

namespace {

struct Setup {
  Zkey zk;
  Graph g;
  uint32_t NS = 0, n = 1, ni = 0;
  std::vector<uint8_t> known;
  G1Rows R;
};
void setup(const uint8_t* zkey, size_t zlen, const uint8_t* graph, size_t glen, Setup* S) {
  S->zk = parse_arkzkey(zkey, zlen);
  S->g = parse_graph(graph, glen);
  S->NS = (uint32_t)S->g.signals.size();
  S->ni = (uint32_t)S->zk.num_instance_variables;
  while (S->n < (uint32_t)S->zk.num_constraints + S->ni) S->n <<= 1;
  const std::vector<uint8_t> node_known = wl_known_nodes(S->g);
  S->known.resize(S->NS);
  for (uint32_t i = 0; i < S->NS; i++) S->known[i] = node_known[S->g.signals[i]];
  S->R = g1_walk_rows(S->zk, S->NS, S->n, S->ni);
}

struct Fnv {
  uint64_t h = 0xCBF29CE484222325ull;
  void bytes(const void* p, size_t len) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < len; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  }
  void u32(uint32_t v) { bytes(&v, 4); }
};

}  // namespace

extern "C" {
const char* sharedrows_error() { return g_err.c_str(); }

// FNV-1a over the point list (canonical coordinates), the scalar ids, npaired and every field of `rows` and `fused`
int sharedrows_legacy_checksum(const uint8_t* zkey, size_t zlen, const uint8_t* graph, size_t glen, uint64_t* out) {
  try {
    Setup S;
    setup(zkey, zlen, graph, glen, &S);
    Fnv f;
    f.u32((uint32_t)S.R.pts.size());
    for (const G1Affine& P : S.R.pts) {
      uint32_t c[8];
      P.x.to_canonical(c);
      f.bytes(c, 32);
      P.y.to_canonical(c);
      f.bytes(c, 32);
    }
    for (uint32_t v : S.R.sids) f.u32(v);
    f.u32(S.R.npaired);
    for (const std::vector<VRow>* fam : {&S.R.rows, &S.R.fused}) {
      f.u32((uint32_t)fam->size());
      for (const VRow& v : *fam) {
        f.u32(v.k);
        f.u32(v.sid);
        f.u32(v.dig_sid);
        f.u32(v.seg);
        f.u32(v.is_h ? 1 : 0);
      }
    }
    *out = f.h;
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}
}

#ifndef SHAREDROWS_LEGACY_ONLY
namespace {

typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Walked;   // (table row, digit id, GLV half, output segment)

struct Check {
  std::string text;
  int failures = 0;
  std::string where;
  void fail(const std::string& what) {
    failures++;
    if (text.size() < 4000) text += where + ": " + what + "\n";
  }
};

// The structural checks tests/host/proverplan.cpp makes for the legacy families, for a plan of `nseg` output segments with
// pair chunks: segchunks tile the chunks, groups / segs and segblocks tile every segment, chunks tile the rows, ROW_PAIRED
// exactly below npaired, every row in its chunk's segment, early / late ids, a pair chunk's two slots distinct empty
// chunks in its members' segments.  Returns what the plan walks, sorted.
std::vector<Walked> check_plan(const WalkPlan& P, const std::vector<VRow>& vrows, uint32_t nseg, uint32_t chunk_pts, uint32_t npaired,
                               uint32_t block_pts, uint32_t h_first, uint32_t h_end, Check& C) {
  std::vector<uint32_t> seg_of_row, sid_of_row;
  for (const VRow& v : vrows) {
    if (v.k >= seg_of_row.size()) {
      seg_of_row.resize(v.k + 1, 0xFFFFFFFFu);
      sid_of_row.resize(v.k + 1, 0xFFFFFFFFu);
    }
    if (seg_of_row[v.k] != 0xFFFFFFFFu) C.fail("the family holds a table row twice");
    seg_of_row[v.k] = v.seg;
    sid_of_row[v.k] = v.dig_sid;
  }
  auto held = [&](uint32_t k) { return k < seg_of_row.size() && seg_of_row[k] != 0xFFFFFFFFu; };
  auto is_h = [&](uint32_t sid) { return sid >= h_first && sid < h_end; };
  const uint32_t nchunks = (uint32_t)P.chunks.size();
  if (P.rows.size() != P.rsid.size() || P.prows.size() != P.prsid.size()) C.fail("rows and scalar ids differ in length");
  if (P.nseg != nseg * GLV_HALVES || P.segchunks.size() != P.nseg || P.segs.size() != P.nseg || P.segblocks.size() != P.nseg) {
    C.fail("segment count");
    return {};
  }
  uint32_t at = 0, gat = 0, bat = 0, maxblk = 0;
  std::vector<uint32_t> seg_of_chunk(nchunks, 0xFFFFFFFFu);
  for (uint32_t sg = 0; sg < P.nseg; sg++) {
    const ChunkDesc r = P.segchunks[sg];
    if (r.pt_begin != at || r.pt_end < r.pt_begin || r.pt_end > nchunks) { C.fail("segchunks do not tile the chunks"); return {}; }
    for (uint32_t c = r.pt_begin; c < r.pt_end; c++) seg_of_chunk[c] = sg;
    at = r.pt_end;
    const ChunkDesc gr = P.segs[sg];
    if (gr.pt_begin != gat || gr.pt_end > P.groups.size() || gr.pt_end < gr.pt_begin) { C.fail("segs do not tile the groups"); return {}; }
    uint32_t cat = r.pt_begin;
    for (uint32_t k = gr.pt_begin; k < gr.pt_end; k++) {
      if (P.groups[k].pt_begin != cat || P.groups[k].pt_end <= cat || P.groups[k].pt_end - cat > 16) C.fail("a group is not <= 16 consecutive chunks");
      cat = P.groups[k].pt_end;
    }
    if (cat != r.pt_end) C.fail("the groups of a segment do not cover its chunks");
    gat = gr.pt_end;
    const ChunkDesc br = P.segblocks[sg];
    const uint32_t want = (r.pt_end - r.pt_begin + block_pts - 1) / block_pts;
    if (br.pt_begin != bat || br.pt_end - br.pt_begin != want) C.fail("segblocks do not cover the segment's chunks once");
    bat = br.pt_end;
    maxblk = std::max(maxblk, want);
  }
  if (at != nchunks) C.fail("segchunks end before the last chunk");
  if (gat != P.groups.size()) C.fail("segs end before the last group");
  if (bat != P.nblocks || maxblk != P.maxblk) C.fail("nblocks / maxblk");
  std::vector<Walked> got;
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
      if (!held(k) || sid_of_row[k] != P.rsid[e]) { C.fail("a row the family does not hold"); continue; }
      if (seg_of_chunk[c] != h * nseg + seg_of_row[k]) C.fail("a row outside its chunk's segment");
      got.push_back(Walked(k, P.rsid[e], h, seg_of_chunk[c] - h * nseg));
    }
  }
  if (rat != P.rows.size()) C.fail("rows beyond the last chunk");
  for (int late = 0; late < 2; late++)
    for (uint32_t c : (late ? P.late_ids : P.early_ids)) {
      if (c >= nchunks || is_slot[c] || in_ids[c]) { C.fail("early / late ids are not a partition"); continue; }
      in_ids[c] = 1;
      for (uint32_t e = P.chunks[c].pt_begin; e < P.chunks[c].pt_end; e++)
        if (is_h(P.rsid[e]) != (late != 0)) C.fail(late ? "a late chunk holds a row that does not depend on h" : "an early chunk holds an h row");
    }
  for (uint32_t c = 0; c < nchunks; c++)
    if (!is_slot[c] && !in_ids[c]) C.fail("a chunk in neither the early nor the late ids");
  if (P.pout.size() != 2 * P.pchunks.size()) { C.fail("pout length"); return {}; }
  std::vector<uint8_t> slot_taken(nchunks, 0);
  uint32_t pat = 0;
  for (size_t c = 0; c < P.pchunks.size(); c++) {
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
      if (!held(q) || !held(q + 1)) { C.fail("a pair chunk walks a row the family does not hold"); continue; }
      if (seg_of_chunk[o0] != h * nseg + seg_of_row[q] || seg_of_chunk[o1] != h * nseg + seg_of_row[q + 1]) C.fail("a pair slot outside its member's segment");
      if (sid_of_row[q] != P.prsid[e] || sid_of_row[q + 1] != P.prsid[e]) C.fail("a pair whose members do not share the chunk's scalar");
      if (is_h(P.prsid[e])) C.fail("a pair under an h scalar");
      got.push_back(Walked(q, P.prsid[e], h, seg_of_chunk[o0] - h * nseg));
      got.push_back(Walked(q + 1, P.prsid[e], h, seg_of_chunk[o1] - h * nseg));
    }
  }
  if (pat != P.prows.size()) C.fail("prows beyond the last pair chunk");
  for (uint32_t c = 0; c < nchunks; c++)
    if (is_slot[c] && !slot_taken[c]) C.fail("an empty chunk no pair chunk fills");
  std::sort(got.begin(), got.end());
  return got;
}

// sum over the rows of segment `seg` of scalar[sid] x point, scalars below 2^16
G1XYZZ segment_sum(const G1Rows& R, const std::vector<VRow>& fam, uint32_t seg, const std::vector<uint16_t>& scalar) {
  G1XYZZ acc = G1XYZZ::inf();
  for (const VRow& v : fam) {
    if (v.seg != seg || !scalar[v.dig_sid]) continue;
    uint32_t k[8] = {scalar[v.dig_sid], 0, 0, 0, 0, 0, 0, 0};
    acc.add(scalar_mul(R.pts[v.k], k));
  }
  return acc;
}
bool same_point(const G1XYZZ& a, const G1XYZZ& b) {
  const G1Affine p = a.to_affine(), q = b.to_affine();
  return p.x == q.x && p.y == q.y;
}

}  // namespace

extern "C" {
// want_eq / want_opp: the wires with a_query[i] == b_g1_query[i] / == -b_g1_query[i], ascending, from an independent
// reading of the key.  Returns the number of failures (-1: an exception); log: what failed.  stats: [0] wires of E+,
// [1] wires of E-, [2] table rows, [3] rows of the shared family, [4] plans checked, [5] pair chunks of the full plan,
// [6] shared A rows walked as single rows of a paired table (full plan, per half), [7] arithmetic identities checked
int sharedrows_check(const uint8_t* zkey, size_t zlen, const uint8_t* graph, size_t glen, const uint32_t* want_eq, size_t n_eq,
                     const uint32_t* want_opp, size_t n_opp, uint64_t seed, char* log, size_t log_len, uint64_t* stats) {
  try {
    Setup S;
    setup(zkey, zlen, graph, glen, &S);
    const G1Rows& R = S.R;
    const uint32_t NS = S.NS, n = S.n;
    Check C;
    // ---- the detector
    C.where = "detector";
    if (R.shared_eq != std::vector<uint32_t>(want_eq, want_eq + n_eq)) C.fail("the wires with A_i == B1_i are not the expected ones");
    if (R.shared_opp != std::vector<uint32_t>(want_opp, want_opp + n_opp)) C.fail("the wires with A_i == -B1_i are not the expected ones");
    std::vector<uint8_t> kind(NS, 0);
    for (uint32_t i : R.shared_eq) kind.at(i) |= 1;
    for (uint32_t i : R.shared_opp) kind.at(i) |= 2;
    if (kind[0]) C.fail("scalar id 0 is shared");
    for (uint32_t i = 0; i < NS; i++)
      if (kind[i] == 3) C.fail("a wire in both E+ and E-");
    // ---- what the family must hold, from the legacy rows: without the B1 rows of the shared wires, their A rows in
    //      segment 3 / 4, every other row where it was
    C.where = "family";
    if (R.rows.size() != R.pts.size()) C.fail("the legacy family does not hold every table row once");
    std::vector<VRow> want;
    std::vector<uint8_t> dropped(R.pts.size(), 0), shared_a(R.pts.size(), 0);
    size_t n_a = 0, n_b = 0;
    for (const VRow& v : R.rows) {
      const uint32_t kd = v.sid < NS ? kind[v.sid] : 0;
      if (kd && v.seg == 1) { dropped[v.k] = 1; n_b++; continue; }
      VRow w = v;
      if (kd && v.seg == 0) { w.seg = kd == 1 ? SEG_SHARED_EQ : SEG_SHARED_OPP; shared_a[v.k] = 1; n_a++; }
      want.push_back(w);
    }
    if (n_a != n_eq + n_opp || n_b != n_eq + n_opp) C.fail("a shared wire without exactly one A row and one B1 row");
    auto same_rows = [](const std::vector<VRow>& a, const std::vector<VRow>& b) {
      if (a.size() != b.size()) return false;
      for (size_t i = 0; i < a.size(); i++)
        if (a[i].k != b[i].k || a[i].sid != b[i].sid || a[i].dig_sid != b[i].dig_sid || a[i].seg != b[i].seg || a[i].is_h != b[i].is_h) return false;
      return true;
    };
    if (!same_rows(R.shared, want)) C.fail("the shared family is not the legacy rows with the B1 rows dropped and the A rows moved");
    // (the points a dropped row and its A row name really are one point up to sign)
    {
      std::vector<uint32_t> a_of(NS, 0xFFFFFFFFu);
      for (const VRow& v : R.rows)
        if (shared_a[v.k]) a_of[v.sid] = v.k;
      for (const VRow& v : R.rows)
        if (dropped[v.k]) {
          const G1Affine &a = R.pts[a_of.at(v.sid)], &b = R.pts[v.k];
          const bool eq = a.x == b.x && a.y == b.y, opp = a.x == b.x && a.y == b.y.neg();
          if (!(kind[v.sid] == 1 ? eq : opp)) C.fail("a dropped B1 row is not +- the A row of its wire");
        }
    }
    // ---- the plans of the three modes
    std::vector<Walked> walked[3];
    uint64_t plans = 0;
    for (int mode : {(int)PROVE_FULL, (int)PROVE_PARTIAL, (int)PROVE_FINISH}) {
      C.where = "shared plan, mode " + std::to_string(mode);
      const WalkPlan P = make_walk_plan(R.shared, G1_SHARED_SEGS, 16, mode, S.known, R.npaired, true);
      walked[mode] = check_plan(P, R.shared, G1_SHARED_SEGS, 16, R.npaired, SUM_TREE_LANES, NS, NS + n, C);
      plans++;
      // what the mode walks: each row of the family whose scalar the mode takes, once per half, in the family's segment
      std::vector<Walked> expect;
      for (const VRow& v : want) {
        const bool is_known = v.sid < NS && S.known[v.sid];
        if (!(mode == PROVE_FULL || (mode == PROVE_PARTIAL) == is_known)) continue;
        for (uint32_t h = 0; h < GLV_HALVES; h++) expect.push_back(Walked(v.k, v.dig_sid, h, v.seg));
      }
      std::sort(expect.begin(), expect.end());
      if (walked[mode] != expect) C.fail("the plan does not walk the family's rows of this mode, each (row, half) once in its segment");
      uint64_t singles = 0;
      for (const Walked& w : walked[mode]) {
        const uint32_t k = std::get<0>(w), sg = std::get<3>(w);
        if (dropped[k]) C.fail("a dropped B1 row is walked");
        if (shared_a[k] != (sg == SEG_SHARED_EQ || sg == SEG_SHARED_OPP)) C.fail("segments 3 and 4 do not hold exactly the shared A rows");
      }
      if (mode == PROVE_FULL) {
        for (uint32_t w : P.rows) singles += (w >> 31) == 0 && shared_a[w & ROW_INDEX] && (w & ROW_INDEX) < R.npaired;
        stats[5] = P.pchunks.size();
        stats[6] = singles;
        size_t seen = 0;
        for (const Walked& w : walked[mode]) seen += shared_a[std::get<0>(w)];
        if (seen != GLV_HALVES * (n_eq + n_opp)) C.fail("a shared A row is not walked once per GLV half");
      }
    }
    {
      C.where = "shared plan";
      std::vector<Walked> both, all(walked[1]);
      std::set_intersection(walked[1].begin(), walked[1].end(), walked[2].begin(), walked[2].end(), std::back_inserter(both));
      all.insert(all.end(), walked[2].begin(), walked[2].end());
      std::sort(all.begin(), all.end());
      if (!both.empty() || all != walked[0]) C.fail("partial and finish do not partition full");
    }
    // the legacy throughput plan (RLNAMD_SHARED_ROWS=0) through the changed builder: every table row, both halves
    {
      C.where = "legacy plan";
      const WalkPlan P = make_walk_plan(R.rows, G1_SEGS, 16, PROVE_FULL, S.known, R.npaired, true);
      const std::vector<Walked> got = check_plan(P, R.rows, G1_SEGS, 16, R.npaired, SUM_TREE_LANES, NS, NS + n, C);
      plans++;
      if (got.size() != GLV_HALVES * R.rows.size()) C.fail("the legacy plan does not walk every (row, half)");
      for (uint32_t w : P.rows)
        if ((w & ROW_INDEX) < R.npaired) C.fail("the legacy plan walks a pair member as a single row");
    }
    // ---- arithmetic: A = s0 + s3 + s4 and B1 = s1 + s3 - s4 of the new family are segments 0 and 1 of the legacy one
    C.where = "arithmetic";
    const uint32_t nsid = NS + n + 3;
    uint64_t st = seed, identities = 0;
    auto rnd16 = [&]() {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      return (uint16_t)(st >> 40);
    };
    std::vector<std::vector<uint16_t>> cases;
    {
      std::vector<uint16_t> sc(nsid);
      for (uint16_t& v : sc) v = rnd16();
      sc[0] = 1;
      cases.push_back(sc);                                  // seeded scalars everywhere
      for (uint32_t i = 0; i < NS; i++)
        if (kind[i]) sc[i] = 0;
      cases.push_back(sc);                                  // every shared scalar 0: S+ and S- are the point at infinity
      for (const std::vector<uint32_t>* E : {&R.shared_eq, &R.shared_opp})
        if (!E->empty()) {
          std::vector<uint16_t> one(nsid, 0);
          one[(*E)[E->size() / 2]] = (uint16_t)(rnd16() | 1);
          cases.push_back(one);                             // one shared scalar, nothing else: A_rest and B1_rest are infinity
        }
    }
    for (size_t ci = 0; ci < cases.size(); ci++) {
      const std::vector<uint16_t>& sc = cases[ci];
      const G1XYZZ s3 = segment_sum(R, R.shared, SEG_SHARED_EQ, sc), s4 = segment_sum(R, R.shared, SEG_SHARED_OPP, sc);
      G1XYZZ a = segment_sum(R, R.shared, 0, sc), b = segment_sum(R, R.shared, 1, sc);
      a.add(s3);
      a.add(s4);
      b.add(s3);
      b.add(s4.neg());
      if (!same_point(a, segment_sum(R, R.rows, 0, sc))) C.fail("s0 + s3 + s4 is not the legacy A sum (case " + std::to_string(ci) + ")");
      if (!same_point(b, segment_sum(R, R.rows, 1, sc))) C.fail("s1 + s3 - s4 is not the legacy B1 sum (case " + std::to_string(ci) + ")");
      if (!same_point(segment_sum(R, R.shared, 2, sc), segment_sum(R, R.rows, 2, sc))) C.fail("the C segment moved");
      if (ci == 1 && (!s3.is_inf() || !s4.is_inf())) C.fail("shared sums under zero scalars are not the point at infinity");
      if (ci >= 2 && (s3.is_inf() && s4.is_inf())) C.fail("a lone shared scalar gives no shared sum");
      identities += 3;
    }
    stats[0] = R.shared_eq.size();
    stats[1] = R.shared_opp.size();
    stats[2] = R.pts.size();
    stats[3] = R.shared.size();
    stats[4] = plans;
    stats[7] = identities;
    snprintf(log, log_len, "%s", C.text.c_str());
    return C.failures;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
}
#endif
