// prover_plan.cpp -- the host planning of the batched prover (prover_plan.h).  No device code and no HIP call.
#include "prover_plan.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "fq29_constants.h"
#include "glv.h"
#include "poseidon.h"
#include "witness_sched.h"

namespace rlnamd {

WinSched make_sched(int c, int wide) {
  if (c < 2 || c > 16 || wide < 0 || c + (wide > 0 ? 1 : 0) > 16) throw Error("window bits must be in [2, 16]");
  WinSched ws{};
  int W = (GlvParams::HALF_BITS - wide + c - 1) / c;
  if (wide > W) throw Error("more wide windows than windows");
  if (W > 32) throw Error("window bits too small: more than 32 windows");
  ws.W = W;
  uint32_t bit = 0, off = 0;
  for (int j = 0; j < W; j++) {
    int cw = c + (j < wide ? 1 : 0);
    ws.cw[j] = (uint8_t)cw;
    ws.bo[j] = (uint16_t)bit;
    ws.ro[j] = off;
    bit += cw;
    off += 1u << (cw - 1);
  }
  ws.stride = off;
  return ws;
}

NamedInputs find_named_inputs(const Graph& graph, uint32_t ni) {
  NamedInputs R;
  auto find = [&](const char* name, uint32_t want_len, uint32_t* off) {
    auto it = graph.input_mapping.find(name);
    if (it == graph.input_mapping.end() || it->second.second != want_len) return false;
    *off = it->second.first;
    return true;
  };
  InputSlots& sl = R.slots;
  sl.depth = graph.tree_depth;
  R.have_path_slots = graph.tree_depth > 0 && find("pathElements", graph.tree_depth, &R.path_off) &&
                      find("identityPathIndex", graph.tree_depth, &R.path_idx_off);
  // the hints need one message id per message slot (the multi-message-id circuit: max_out of them)
  uint32_t unused = 0;
  R.hint_msgs = graph.max_out;
  R.have_hint_slots = find("identitySecret", 1, &sl.secret) && find("userMessageLimit", 1, &sl.limit) &&
                      find("messageId", graph.max_out, &R.hint_msg_off) && find("pathElements", graph.tree_depth, &sl.path) &&
                      find("identityPathIndex", graph.tree_depth, &sl.path_idx) && find("x", 1, &sl.x) &&
                      find("externalNullifier", 1, &sl.ext) &&
                      (graph.max_out == 1 || find("selectorUsed", graph.max_out, &unused));
  // the proof-values kernel: the same names on a single message-id circuit with six instance variables
  R.have_values_kernel = R.have_hint_slots && graph.max_out == 1 && ni == 6;
  if (R.have_values_kernel) sl.msg_id = R.hint_msg_off;
  R.have_drawn_slots = find("userMessageLimit", 1, &sl.limit) && find("externalNullifier", 1, &sl.ext) &&
                       find("messageId", 1, &R.drawn_msg_off);
  R.drawn_multi_slots = graph.max_out;
  R.drawn_sel = find("selectorUsed", graph.max_out, &R.drawn_multi_sel_off);
  R.have_drawn_multi_slots = graph.max_out >= 1 && find("userMessageLimit", 1, &sl.limit) && find("externalNullifier", 1, &sl.ext) &&
                             find("messageId", graph.max_out, &R.drawn_multi_msg_off) && (R.drawn_sel || graph.max_out == 1);
  return R;
}

// ------------------------------------------------------------------------------------------------- hints
static Fr read_input(const uint8_t* in_le, uint32_t slot) {
  uint32_t c[8];
  memcpy(c, in_le + 32 * (size_t)slot, 32);
  return Fr::from_canonical(c);
}

void HintChains::probe(const uint8_t* in_le, Probe* pr) const {
  const InputSlots& slots = in_.slots;
  const Fr secret = read_input(in_le, slots.secret);
  pr->idc = poseidon_hash_host(poseidon_host_params(2), &secret);
  // fingerprint of the public values the chain depends on (two multiply-xorshift lanes over the 32-bit words)
  uint64_t fp[2] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full};
  auto mix = [&](const uint32_t* w, int n) {
    for (int k = 0; k < n; k++) {
      fp[0] = (fp[0] ^ w[k]) * 0xFF51AFD7ED558CCDull;
      fp[0] ^= fp[0] >> 29;
      fp[1] = (fp[1] + w[k]) * 0xC4CEB9FE1A85EC53ull;
      fp[1] ^= fp[1] >> 31;
    }
  };
  auto mix_slots = [&](uint32_t first, uint32_t count) {
    for (uint32_t k = 0; k < count; k++) {
      uint32_t w[8];
      memcpy(w, in_le + 32 * (size_t)(first + k), 32);
      mix(w, 8);
    }
  };
  mix(pr->idc.v, 8);
  mix_slots(slots.limit, 1);
  mix_slots(slots.path, slots.depth);
  mix_slots(slots.path_idx, slots.depth);
  pr->fp[0] = fp[0];
  pr->fp[1] = fp[1];
  pr->found = false;
  if (entries_) {
    std::lock_guard<std::mutex> lk(mu_);
    for (const Entry& e : cache_)
      if (e.fp[0] == fp[0] && e.fp[1] == fp[1] && e.chain.size() == slots.depth) pr->found = true;
  }
}

void HintChains::hints(const uint8_t* in_le, Fr* out, const Probe* pr) const {
  const InputSlots& slots = in_.slots;
  const PoseidonParams &P3 = poseidon_host_params(3), &P4 = poseidon_host_params(4);
  Probe mine;
  if (!pr) {
    probe(in_le, &mine);
    pr = &mine;
  }
  const Fr secret = read_input(in_le, slots.secret), limit = read_input(in_le, slots.limit);
  const Fr idc = pr->idc;
  out[0] = idc;
  const uint64_t fp[2] = {pr->fp[0], pr->fp[1]};
  bool found = false;
  if (entries_) {
    std::lock_guard<std::mutex> lk(mu_);
    for (Entry& e : cache_)
      if (e.fp[0] == fp[0] && e.fp[1] == fp[1] && e.chain.size() == slots.depth) {
        for (uint32_t l = 0; l < slots.depth; l++) out[1 + l] = e.chain[l];
        e.stamp = ++clock_;
        hits_++;
        found = true;
        break;
      }
  }
  if (!found) {
    Fr in2[2] = {idc, limit};
    Fr node = poseidon_hash_host(P3, in2);
    out[1] = node;
    for (uint32_t l = 0; l < slots.depth; l++) {
      const Fr e = read_input(in_le, slots.path + l);
      const bool right = !read_input(in_le, slots.path_idx + l).is_zero();   // the node is the right child: hash(sibling, node)
      in2[0] = right ? e : node;
      in2[1] = right ? node : e;
      node = poseidon_hash_host(P3, in2);
      if (l + 1 < slots.depth) out[2 + l] = node;
    }
    if (entries_) {
      std::lock_guard<std::mutex> lk(mu_);
      Entry* slot = nullptr;
      if (cache_.size() < entries_) {
        cache_.emplace_back();
        slot = &cache_.back();
      } else {   // the least recently used
        slot = &cache_[0];
        for (Entry& e : cache_)
          if (e.stamp < slot->stamp) slot = &e;
      }
      slot->fp[0] = fp[0];
      slot->fp[1] = fp[1];
      slot->stamp = ++clock_;
      slot->chain.assign(out + 1, out + 1 + slots.depth);
    }
  }
  for (uint32_t k = 0; k < in_.hint_msgs; k++) {   // a1 of every message slot (one on the single-message circuits)
    const Fr in3[3] = {secret, read_input(in_le, slots.ext), read_input(in_le, in_.hint_msg_off + k)};
    out[slots.depth + 1 + k] = poseidon_hash_host(P4, in3);
  }
}

uint64_t HintChains::hits() const {
  std::lock_guard<std::mutex> lk(mu_);
  return hits_;
}

std::vector<std::vector<uint32_t>> find_hint_cuts(const Graph& graph, const NamedInputs& in, const HintChains& chains) {
  const uint32_t N = (uint32_t)graph.nodes.size(), n_hints = graph.tree_depth + 1 + graph.max_out;
  const InputSlots& slots = in.slots;
  // two probes with complementary path bits and unrelated values: a node that merely carries the running hash on one
  // side of a level's left / right selection equals the hint under one of them only
  std::vector<std::vector<uint32_t>> cuts(n_hints);
  std::vector<uint8_t> match(N, 1);
  std::vector<uint32_t> match_hint(N, 0xFFFFFFFFu);
  bool all = true;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  for (int round = 0; round < 2 && all; round++) {
    std::vector<uint8_t> probe((size_t)graph.inputs_size * 32, 0);
    probe[0] = 1;
    auto put = [&](uint32_t slot) {
      for (int k = 0; k < 31; k++) {   // 248 pseudo-random bits: below r
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        probe[32 * (size_t)slot + k] = (uint8_t)(st >> 56);
      }
    };
    put(slots.secret); put(slots.x); put(slots.ext);
    probe[32 * (size_t)slots.limit] = (uint8_t)(100 + round);
    for (uint32_t k = 0; k < in.hint_msgs; k++) probe[32 * (size_t)(in.hint_msg_off + k)] = (uint8_t)(7 + round + 3 * k);
    {
      auto it = graph.input_mapping.find("selectorUsed");   // every message slot in use
      if (it != graph.input_mapping.end())
        for (uint32_t k = 0; k < it->second.second; k++) probe[32 * (size_t)(it->second.first + k)] = 1;
    }
    for (uint32_t l = 0; l < slots.depth; l++) {
      put(slots.path + l);
      probe[32 * (size_t)(slots.path_idx + l)] = (uint8_t)((l + round) & 1);
    }
    uint32_t perr = 0;
    const std::vector<Fr> val = wl_eval_host(graph, probe.data(), &perr);
    std::vector<Fr> hv(n_hints);
    chains.hints(probe.data(), hv.data());
    all = perr == 0;
    for (uint32_t n = 0; n < N && all; n++) {
      if (!match[n]) continue;
      if (graph.nodes[n].op == G_INPUT || graph.nodes[n].op == G_CONST) { match[n] = 0; continue; }
      uint32_t j = round == 0 ? 0xFFFFFFFFu : match_hint[n];
      if (round == 0) {
        for (uint32_t q = 0; q < n_hints; q++)
          if (val[n] == hv[q]) j = q;
        match_hint[n] = j;
      }
      if (j == 0xFFFFFFFFu || !(val[n] == hv[j])) match[n] = 0;
    }
  }
  for (uint32_t n = 0; n < N && all; n++)
    if (match[n]) cuts[match_hint[n]].push_back(n);
  for (uint32_t j = 0; j < n_hints && all; j++) all = !cuts[j].empty();
  if (!all) cuts.clear();
  return cuts;
}

// ------------------------------------------------------------------------------------------------- the k_witness29 program
// (1) Fusion: an Add one of whose operands is a product used nowhere else (and is no witness signal) becomes ONE node,
// a * b + c (W29_FMA: the addend enters the product's final carry chain, Fr29::mul_add) -- in the shipped circuits every
// addition of a Poseidon round is of that kind, 23 414 nodes become ~15 000.  (2) Program order = node order without the
// fused products; the LDS ring is addressed by program index.  (3) Stored values (witness signals, inputs, operands
// further back than the ring) live in a compact array indexed by `slot`.  (4) W29_RED where the static bound of a value
// (in units of r) would pass WIT29_BMAX.
Wit29Program compile_witness29(const Graph& graph, const std::vector<uint8_t>& is_cut) {
  const uint32_t NONE = 0xFFFFFFFFu;
  const std::vector<GNode>& G = graph.nodes;
  const uint32_t N = (uint32_t)G.size();
  Wit29Program R;
  std::vector<uint32_t>& slot2node = R.slot2node;
  auto is_const = [&](uint32_t o) { return G[o].op == G_CONST; };
  auto nops = [&](const GNode& g) {
    return (g.op == G_INPUT || g.op == G_CONST) ? 0 : (g.op == G_NEG || g.op == G_ID) ? 1 : g.op == G_TERN ? 3 : 2;
  };
  std::vector<uint32_t> uses(N, 0);
  for (uint32_t n = 0; n < N; n++) {
    const uint32_t o[3] = {G[n].a, G[n].b, G[n].c};
    for (int k = 0; k < nops(G[n]); k++) {
      if (o[k] >= n) throw Error("Graph error: node operand refers forward");
      uses[o[k]]++;
    }
  }
  std::vector<uint8_t> is_signal(N, 0);
  for (uint32_t sgn : graph.signals) is_signal[sgn] = 1;
  std::vector<uint32_t> fused_mul(N, NONE);   // for an Add: the product folded into it
  std::vector<uint8_t> removed(N, 0);
  for (uint32_t n = 0; n < N; n++) {
    if (G[n].op != G_ADD) continue;
    for (uint32_t m : {G[n].b, G[n].a}) {
      if (G[m].op == G_MUL && uses[m] == 1 && !is_signal[m] && !is_cut[m] && !removed[m] && G[n].a != G[n].b) {
        fused_mul[n] = m;
        removed[m] = 1;
        break;
      }
    }
  }
  // program nodes: operands as ORIGINAL node ids
  struct PNode { uint32_t op, node, src[3]; };
  std::vector<PNode> P;
  std::vector<uint32_t> pidx(N, NONE);
  for (uint32_t n = 0; n < N; n++) {
    if (removed[n]) continue;
    PNode q{G[n].op, n, {G[n].a, G[n].b, G[n].c}};
    if (fused_mul[n] != NONE) {
      const uint32_t m = fused_mul[n];
      q.op = W29_FMA;
      q.src[0] = G[m].a;
      q.src[1] = G[m].b;
      q.src[2] = G[n].a == m ? G[n].b : G[n].a;
    }
    pidx[n] = (uint32_t)P.size();
    P.push_back(q);
  }
  auto pn_ops = [&](const PNode& q) { return q.op == W29_FMA ? 3 : nops(GNode{q.op, 0, 0, 0}); };
  std::vector<uint8_t> store(N, 0);
  for (uint32_t n = 0; n < N; n++) store[n] = is_signal[n] || G[n].op == G_INPUT || is_cut[n];   // (a cut node is compared with its hint)
  for (uint32_t i = 0; i < P.size(); i++)
    for (int k = 0; k < pn_ops(P[i]); k++) {
      const uint32_t o = P[i].src[k];
      if (!is_const(o) && i - pidx[o] >= WIT29_RING) store[o] = 1;
    }
  std::vector<uint32_t> slot_of(N, 0);
  R.store_slot.assign(N, NONE);
  for (uint32_t n = 0; n < N; n++)
    if (store[n] && !removed[n]) {
      slot_of[n] = R.store_slot[n] = (uint32_t)slot2node.size();
      slot2node.push_back(n);
    }
  // The descriptor holds the slot in 16 bits.  The shipped circuits have at most 29 254 graph nodes, stored values
  // being a subset of them, so only a much larger circuit can fail here.
  if (slot2node.size() >= 65536)
    throw Error("graph too large for the witness interpreter: " + std::to_string(slot2node.size()) +
                " stored values, the descriptor holds 16 bits");
  std::vector<GNode29>& prog = R.prog;
  prog.resize(P.size());
  std::vector<double> bnd(N, 1.01);
  for (uint32_t i = 0; i < P.size(); i++) {
    const PNode& q = P[i];
    GNode29 d{};
    uint32_t flags = store[q.node] ? W29_STORE : 0;
    d.a = q.src[0];   // G_INPUT: input index, G_CONST: constant index
    double b = 1.01;  // inputs, constants, slow operations: a fresh product with a constant
    // the fast path of the kernel: Mul / Add / a * b + c with every operand in LDS (ring or constant table)
    bool rare = q.op != G_MUL && q.op != G_ADD && q.op != W29_FMA;
    if (q.op != G_INPUT && q.op != G_CONST) {
      auto enc = [&](uint32_t o) -> uint32_t {
        if (is_const(o)) {
          if (G[o].a >= WIT29_LDS_CONSTS) rare = true;
          return OPK_CONST | G[o].a;
        }
        if (i - pidx[o] < WIT29_RING) return OPK_RING | pidx[o];
        rare = true;
        return OPK_FAR | slot_of[o];
      };
      auto bo = [&](uint32_t o) { return is_const(o) ? 1.01 : bnd[o]; };
      const int k = pn_ops(q);
      double bs[3] = {0, 0, 0};
      uint32_t e[3] = {0, 0, 0};
      for (int j = 0; j < k; j++) {
        e[j] = enc(q.src[j]);
        bs[j] = bo(q.src[j]);
      }
      d.a = e[0];
      d.b = e[1];
      d.c = e[2];
      if (q.op == G_MUL) b = 1.0 + 0.006 * bs[0] * bs[1];
      else if (q.op == W29_FMA) b = 1.0 + 0.006 * bs[0] * bs[1] + bs[2];
      else if (q.op == G_ADD) b = bs[0] + bs[1];
      else if (q.op == G_SUB) b = bs[0] + 8.0;
      else if (q.op == G_NEG) b = 8.0;
      else if (q.op == G_TERN) b = std::max(bs[1], bs[2]);
    }
    if (b > WIT29_BMAX) {
      flags |= W29_RED;
      rare = true;
      b = 1.0 + 0.006 * b;
    }
    if (rare) flags |= W29_RARE;
    bnd[q.node] = b;
    d.w0 = q.op | flags | (slot_of[q.node] << 16);
    prog[i] = d;
  }
  R.nprog = (uint32_t)prog.size();
  prog.resize(((size_t)R.nprog / WIT29_CH + 4) * WIT29_CH, GNode29{});   // the kernel prefetches two chunks past the end
  return R;
}

// ------------------------------------------------------------------------------------------------- point lists
G1Rows g1_walk_rows(const Zkey& zk, uint32_t NS, uint32_t n, uint32_t ni) {
  const uint32_t SID_R = NS + n, SID_S = SID_R + 1, SID_NRS = SID_R + 2;
  G1Rows R;
  std::vector<G1Affine>& pts = R.pts;
  std::vector<uint32_t>& sids = R.sids;
  std::vector<uint32_t> row_seg;
  auto push = [&](const G1Affine& P, uint32_t sid, uint32_t seg) {
    if (P.is_inf()) return;
    pts.push_back(P);
    sids.push_back(sid);
    row_seg.push_back(seg);
  };
  // seg 0: A = alpha + sum_i w_i A_i + r delta      (scalar id 0 carries a_query[0] and alpha: k_recode makes it ONE whatever w_0 is)
  for (uint32_t i = 0; i < NS; i++) push(zk.a_query[i], i, 0);
  push(zk.alpha_g1, 0, 0);
  push(zk.delta_g1, SID_R, 0);
  // seg 1: B1 = beta + sum_i w_i B_i + s delta
  for (uint32_t i = 0; i < NS; i++) push(zk.b_g1_query[i], i, 1);
  push(zk.beta_g1, 0, 1);
  push(zk.delta_g1, SID_S, 1);
  // seg 2: Cpart = sum_j w_(ni+j) L_j + sum_k h_k H_k - (r s) delta
  for (uint32_t j = 0; j < zk.l_query.size(); j++) push(zk.l_query[j], ni + j, 2);
  for (uint32_t k = 0; k < n; k++) push(zk.h_query[k], NS + k, 2);
  push(zk.delta_g1, SID_NRS, 2);
  // PAIRS: points walked under the same witness scalar (A_i, B1_i, L_i share w_i; a_query[0], alpha, b_g1_query[0],
  // beta share w_0 = 1) are put side by side, two by two, at the front of the point list; their tables are interleaved
  // (ROW_PAIRED) and the throughput plan walks them with lane pairs.  A third row of a scalar stays single.
  {
    std::vector<std::vector<uint32_t>> by_sid(NS);
    for (uint32_t k = 0; k < sids.size(); k++)
      if (sids[k] < NS) by_sid[sids[k]].push_back(k);
    std::vector<uint32_t> order;
    std::vector<uint8_t> taken(sids.size(), 0);
    for (const auto& v : by_sid)
      for (size_t t = 0; t + 1 < v.size(); t += 2) {
        order.push_back(v[t]);
        order.push_back(v[t + 1]);
        taken[v[t]] = taken[v[t + 1]] = 1;
      }
    R.npaired = (uint32_t)order.size();
    for (uint32_t k = 0; k < sids.size(); k++)
      if (!taken[k]) order.push_back(k);
    std::vector<G1Affine> p2(pts.size());
    std::vector<uint32_t> s2(sids.size()), g2(sids.size());
    for (size_t i = 0; i < order.size(); i++) {
      p2[i] = pts[order[i]];
      s2[i] = sids[order[i]];
      g2[i] = row_seg[order[i]];
    }
    pts.swap(p2);
    sids.swap(s2);
    row_seg.swap(g2);
  }
  for (uint32_t k = 0; k < sids.size(); k++)
    R.rows.push_back({k, sids[k], sids[k], row_seg[k], sids[k] >= NS && sids[k] < NS + n});
  // Throughput plan, shared rows: the wires whose A and B1 rows are one point up to sign (affine coordinates: x equal, y
  // equal or opposite).  Scalar id 0 never: its rows carry alpha and beta beside query[0].
  {
    std::vector<uint8_t> kind(NS, 0);   // 1: A_i == B1_i, 2: A_i == -B1_i
    for (uint32_t i = 1; i < NS; i++) {
      const G1Affine &a = zk.a_query[i], &b = zk.b_g1_query[i];
      if (a.is_inf() || b.is_inf() || a.x != b.x) continue;
      if (a.y == b.y) kind[i] = 1;
      else if (a.y == b.y.neg()) kind[i] = 2;
      if (kind[i]) (kind[i] == 1 ? R.shared_eq : R.shared_opp).push_back(i);
    }
    for (const VRow& v : R.rows) {
      const uint32_t kd = v.sid < NS ? kind[v.sid] : 0;
      if (kd && v.seg == 1) continue;   // the B1 row: the sum of the A row serves for it
      VRow w = v;
      if (kd && v.seg == 0) w.seg = kd == 1 ? SEG_SHARED_EQ : SEG_SHARED_OPP;
      R.shared.push_back(w);
    }
  }
  // Small full proofs, fused plan: s A + r B1 - r s delta = s alpha + r beta + r s delta + sum (s w_i) A_i + sum (r w_i) B1_i,
  // so the two variable-base products of the back end (k_fin_smul: a lone lane's ladder of 127 doublings, the longest
  // kernel behind the interpreter) become extra rows of the C segment -- the A and B1 rows walked a second time under
  // the scalar ids of s w_i and r w_i (k_recode part 3) -- and the B1 segment is not walked at all.  More additions
  // in total (+ 25 % G1 rows), which is why only batches below the small-batch threshold take this plan.
  std::vector<VRow>& f = R.fused;
  const uint32_t NX = NS + n + 3;   // first extra scalar id: s w_i at NX + i, r w_i at NX + NS + i, r s at NX + 2 NS
  for (uint32_t k = 0; k < sids.size(); k++) {
    const uint32_t sd = sids[k], sg = row_seg[k];
    const bool is_h = sd >= NS && sd < NS + n;
    if (sg == 0) {
      f.push_back({k, sd, sd, 0, false});                               // A itself is an output
      if (sd < NS) f.push_back({k, sd, NX + sd, 2, false});             // (s w_i) A_i   (alpha carries sid 0: s alpha)
      // delta with r (part of A) contributes s r delta to s A: counted once below
    } else if (sg == 1) {
      if (sd < NS) f.push_back({k, sd, NX + NS + sd, 2, false});        // (r w_i) B1_i  (beta carries sid 0: r beta)
    } else if (sd == SID_NRS) {
      f.push_back({k, sd, NX + 2 * NS, 2, false});                      // + r s delta instead of - r s delta
    } else {
      f.push_back({k, sd, sd, 2, is_h});                                // L and H rows
    }
  }
  return R;
}

G2Rows g2_walk_rows(const Zkey& zk, uint32_t NS, uint32_t n) {
  G2Rows R;
  std::vector<uint32_t> sids;
  auto push = [&](const G2Affine& P, uint32_t sid) {
    if (P.is_inf()) return;
    R.pts.push_back(P);
    sids.push_back(sid);
  };
  for (uint32_t i = 0; i < NS; i++) push(zk.b_g2_query[i], i);
  push(zk.beta_g2, 0);
  push(zk.delta_g2, NS + n + 1);   // s
  // the G2 digit array holds the witness scalars and r, s, -(r s) only (k_recode): ids above the h block move down
  R.dsid = sids;
  for (uint32_t& v : R.dsid)
    if (v >= NS) v -= n;
  for (uint32_t k = 0; k < sids.size(); k++) R.rows.push_back({k, sids[k], R.dsid[k], 0u, false});
  return R;
}

// ------------------------------------------------------------------------------------------------- walk plans
void make_reduce_ranges(const std::vector<uint32_t>& segfirst, std::vector<ChunkDesc>& groups, std::vector<ChunkDesc>& segs) {
  const uint32_t G = 16;
  for (size_t sgi = 0; sgi + 1 < segfirst.size(); sgi++) {
    uint32_t g0 = (uint32_t)groups.size();
    for (uint32_t c = segfirst[sgi]; c < segfirst[sgi + 1]; c += G)
      groups.push_back({c, std::min(c + G, segfirst[sgi + 1])});
    segs.push_back({g0, (uint32_t)groups.size()});
  }
}

WalkPlan make_walk_plan(const std::vector<VRow>& vrows, uint32_t nseg, uint32_t chunk_pts, int mode,
                        const std::vector<uint8_t>& known, uint32_t npaired, bool pair_chunks, uint32_t block_pts) {
  WalkPlan P;
  const uint32_t NS = (uint32_t)known.size();
  auto roww = [&](uint32_t k, uint32_t h) { return k | (k < npaired ? ROW_PAIRED : 0u) | (h << 31); };
  std::vector<uint32_t> segfirst;
  const bool pairs_here = pair_chunks && npaired > 0;
  // rows a mode walks: everything (full), the signals the partial witness fixes (partial), the others (finish)
  auto walked = [&](const VRow& v) {
    const bool is_known = v.sid < NS && known[v.sid];
    return mode == PROVE_FULL || (mode == PROVE_PARTIAL) == is_known;
  };
  // pair chunks first: entries grouped by (half, segment of member 0, segment of member 1)
  struct PairChunk { uint32_t h, sg0, sg1, begin, end; };
  std::vector<PairChunk> pcs;
  std::vector<const VRow*> byk;   // pair members the family holds, by table row
  if (pairs_here) {
    byk.assign(npaired, nullptr);
    for (const VRow& v : vrows)
      if (v.k < npaired) byk[v.k] = &v;
    for (uint32_t h = 0; h < GLV_HALVES; h++)
      for (uint32_t sg0 = 0; sg0 < nseg; sg0++)
        for (uint32_t sg1 = 0; sg1 < nseg; sg1++) {
          const uint32_t first = (uint32_t)P.prows.size();
          for (uint32_t q = 0; q + 1 < npaired; q += 2) {
            const VRow *a = byk[q], *b = byk[q + 1];
            if (!a || !b || a->seg != sg0 || b->seg != sg1) continue;
            if (a->dig_sid != b->dig_sid || a->is_h || b->is_h) throw Error("internal: pair members must share a witness scalar");
            if (!walked(*a)) continue;   // (the members share the scalar, so the mode takes both or neither)
            P.prows.push_back(roww(q, h));
            P.prsid.push_back(a->dig_sid);
          }
          for (uint32_t k = first; k < P.prows.size(); k += chunk_pts)
            pcs.push_back({h, sg0, sg1, k, (uint32_t)std::min<size_t>(k + chunk_pts, P.prows.size())});
        }
    P.pout.assign(2 * pcs.size(), 0);
    for (const PairChunk& c : pcs) P.pchunks.push_back({c.begin, c.end});
  }
  // reduction segment h * nseg + sg: the rows of output sg walked with GLV half h (bit 31 of the row entry)
  for (uint32_t h = 0; h < GLV_HALVES; h++)
    for (uint32_t sg = 0; sg < nseg; sg++) {
      segfirst.push_back((uint32_t)P.chunks.size());
      // rows whose scalar is a coefficient of h come last and start a chunk of their own, so that a small batch can
      // walk everything else while the NTTs still run (early_ids / late_ids)
      for (int late = 0; late < 2; late++) {
        uint32_t first = (uint32_t)P.rows.size();
        for (const VRow& v : vrows) {
          if (v.seg != sg || (int)v.is_h != late) continue;
          // walked by a pair chunk -- unless the family leaves its partner out: then it is a single row here
          if (pairs_here && v.k < npaired && byk[v.k ^ 1u]) continue;
          if (walked(v)) {
            P.rows.push_back(roww(v.k, h));
            P.rsid.push_back(v.dig_sid);
          }
        }
        for (uint32_t k = first; k < P.rows.size(); k += chunk_pts) {
          (late ? P.late_ids : P.early_ids).push_back((uint32_t)P.chunks.size());
          P.chunks.push_back({k, (uint32_t)std::min<size_t>(k + chunk_pts, P.rows.size())});
        }
      }
      // chunk slots of this segment that pair chunks fill: empty ranges in `chunks` (the single-chunk path skips them)
      for (size_t c = 0; c < pcs.size(); c++)
        for (uint32_t m = 0; m < 2; m++)
          if (pcs[c].h == h && (m ? pcs[c].sg1 : pcs[c].sg0) == sg) {
            P.pout[2 * c + m] = (uint32_t)P.chunks.size();
            P.chunks.push_back({0, 0});
          }
    }
  segfirst.push_back((uint32_t)P.chunks.size());
  make_reduce_ranges(segfirst, P.groups, P.segs);
  P.nseg = nseg * GLV_HALVES;
  for (size_t sgi = 0; sgi + 1 < segfirst.size(); sgi++) {
    P.segchunks.push_back({segfirst[sgi], segfirst[sgi + 1]});
    const uint32_t k = (segfirst[sgi + 1] - segfirst[sgi] + block_pts - 1) / block_pts;
    P.segblocks.push_back({P.nblocks, P.nblocks + k});
    P.nblocks += k;
    P.maxblk = std::max(P.maxblk, k);
  }
  return P;
}

// ------------------------------------------------------------------------------------------------- the shape of a batch
BatchShape batch_shape(const BatchQuery& q, const ProverTuning& T) {
  BatchShape S{};
  const size_t n = q.n;
  const int mode = q.mode;
  // lone: nothing else in flight -- the batch may trade throughput for latency (the fused plan's + 25 % G1 rows, the
  // single-stream chains, the wave-per-proof interpreter above the small-batch threshold).  T.lone: -1 detect; 0 / 1:
  // force (measurements, tests).  Up to lone_small_max proofs the lone shapes are taken behind a batch that is still in
  // flight as well -- a stream of such batches was measured 1.2 - 2 x slower in the throughput shapes: three batches of
  // 16 in flight 11.9 ms, 5.7 ms in the lone shapes; above 48 the two are the same.
  S.lone = T.lone >= 0 ? T.lone != 0 : (n <= T.lone_small_max || q.idle);
  // small batches (ProverTuning::lanechunk_max) take the latency shapes: walks with lanes = chunks (walk29.h), kernels with
  // the lanes on one proof's elements, the copy engine for the results.  (n <= capacity, so such a batch fits in small_stride.)
  S.small = n <= T.lanechunk_max;
  // The lanes = nodes interpreter (a wave and 157 KB of LDS per proof, ~25 x the instructions per proof of k_witness29,
  // 1.5 ms per 256 proofs against 11 ms): always below the small-batch threshold; up to witlanes_max only for a LONE batch
  // -- in a stream of such batches it costs throughput, and there the previous batch is still in flight.  The wide form of
  // that trade is only taken when no other prover shares the device.
  const uint32_t wl_lone_max = q.shared ? std::min(T.witlanes_max, 256u) : T.witlanes_max;
  S.wl_used = q.witlanes_ok && (S.small || (n <= wl_lone_max && S.lone));
  // Finish with the partial run's values at hand (prover.h: submit_finish): every proof of the batch has a live cache
  // entry and the batch is one the wave-per-proof interpreter takes -> the known rows come back from the cache and only
  // the cone evaluate_partial leaves unknown is interpreted.  Anything else -- a dead handle, a big batch -- walks the
  // whole graph: same bytes.
  S.cone = mode == PROVE_FINISH && q.handles && q.inputs && S.wl_used && q.cone_ok;
  // A lone batch of a few proofs: the graph as independent segments behind hints (HintChains): up to hint_max proofs
  // whatever their chains cost; above it, up to hint_max_warm, when few enough of the proofs' chains have to be hashed
  // (probe_chains); whatever the batch's size up to HINT_PROOFS when the caller brings the hints (submit_hinted).
  S.hinted = q.segs_ok && q.inputs && S.wl_used && !S.cone && S.lone && !q.no_hints_now &&
             n <= (q.pre_hints ? HINT_PROOFS : std::max(T.hint_max, T.hint_max_warm));
  S.probe_chains = S.hinted && !q.pre_hints && n > T.hint_max;
  // Small batches (latency, not throughput): the whole front end stays on ONE stream (every cross-stream event hop costs
  // 0.1 - 0.15 ms), the digits of the witness scalars are recoded right behind the interpreter, and both walks start on
  // everything that does not depend on the quotient h while mat-vec / NTTs still run; only the h rows of the G1 walk
  // wait for them.
  S.early = S.small && mode != PROVE_PARTIAL;
  // small full proofs: s A and r B1 are rows of the C segment (plan1f), no ladder (up to 96 proofs: above, the walks are
  // issue-bound even for a lone batch and the extra rows cost more than the ladder they replace -- 128 proofs 16.6 ->
  // 15.3 ms without them, 64 proofs 10.1 -> 10.3 ms).  A streamed finish takes it too -- the variable-base part that is
  // left, s pi_a + r rho, comes from powers of the two points (k_pp_smul).
  S.fused = S.lone && n <= 96 && S.early && (mode == PROVE_FULL || (mode == PROVE_FINISH && q.inputs && q.partial_points));
  // tiny: a lane per (row, half) and a two-stage sum (plan1tf / plan2t) -- only the fused proof of a lone batch, and only
  // when it walks with lanes = chunks; a lone tiny PARTIAL proof as well (the plain rows of the known signals)
  S.tiny_partial = S.lone && S.small && mode == PROVE_PARTIAL && n <= T.tiny_max && n <= TINY_STRIDE && n <= T.lanechunk_walk_max;
  S.tiny = (S.fused && n <= T.tiny_max && n <= TINY_STRIDE && n <= T.lanechunk_walk_max) || S.tiny_partial;
  S.plan1 = S.tiny ? PLAN_TINY : S.fused ? PLAN_FUSED : S.small ? PLAN_SMALL : PLAN_BIG;
  S.plan2 = S.tiny ? PLAN_TINY : S.small ? PLAN_SMALL : PLAN_BIG;
  S.PB = S.tiny ? TINY_STRIDE : S.small ? q.small_stride : (uint32_t)q.capacity;
  // mid-size small batches: the short-chunk plans walked with lanes = proofs (walk29.h).  A lone batch: above 48 proofs
  // (64: 11.3 -> 9.9 ms, 128: 18.1 -> 16.3 ms; 32: 6.9 ms against 8.4).  In a stream of batches the lanes = chunks form
  // pays its scattered gathers in throughput much earlier (streams of 64 / 128-proof batches: 9.5 -> 10.8 k, 10.7 -> 11.9 k
  // proofs/s), so there it stops at 16 proofs.
  S.walk_lp = S.early && (n > T.lanechunk_walk_max || (!S.lone && n >= 16));
  // proof stride of the digit arrays: compact where the walks run with lanes = chunks (k_recode); the batch capacity
  // otherwise (the lanes = proofs walks have padding lanes that read beside the batch: those must stay digits of the
  // same window)
  S.dB = (S.early && !S.walk_lp) ? (uint32_t)n : (uint32_t)q.capacity;
  // Lone small batches: the G2 chain stays on the interpreter's own stream (Prover::enqueue)
  S.g2_on_front = S.lone && S.early;
  // the circuit's own outputs instead of the Poseidon chain of k_proof_values (5.3 ms alone), whenever the batch is small
  // enough for the lanes = nodes interpreter
  S.values_w = (S.early || S.wl_used) && q.have_values_kernel && q.ni == 6;
  // NTTs as the three LDS kernels (above ~100 proofs the walks beside the quotient chain leave their 4-wave workgroups
  // waiting for four free wave slots on one CU: the single-wave passes then finish earlier)
  S.ntt_lds = S.small && n <= T.ntt_lg_max && q.logn >= 9 && q.logn <= 18;
  // compact stream shape, big batches: the same outputs behind the interpreter on its own stream -- every mode for a batch
  // that takes them anyway (values_w), otherwise full and finish
  S.values_front = q.compact && !S.small && q.have_values_kernel && q.ni == 6 && (S.values_w || mode != PROVE_PARTIAL);
  return S;
}

// ------------------------------------------------------------------------------------------------- the transforms of a big batch
static uint32_t bitrev(uint32_t x, int bits) {
  uint32_t r = 0;
  for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}

// t 2^256 (8 x 32 Montgomery) -> t 2^261 mod r, canonical, cut into nine 29-bit limbs: the Montgomery form of fq29.h
static std::vector<uint32_t> table29(const std::vector<Fr>& t) {
  const Fr k = Fr::from_u32(32);   // 2^261 / 2^256
  std::vector<uint32_t> out(t.size() * 9);
  for (size_t i = 0; i < t.size(); i++) {
    const Fr x = t[i] * k;   // the words of (32 t) 2^256 = t 2^261
    for (int j = 0; j < 9; j++) {
      const int bit = 29 * j, w = bit >> 5, s = bit & 31;
      const uint64_t two = (uint64_t)x.v[w] | (w + 1 < 8 ? (uint64_t)x.v[w + 1] << 32 : 0);
      out[i * 9 + j] = (uint32_t)(two >> s) & (j < 8 ? (1u << 29) - 1 : 0xFFFFFFFFu);
    }
  }
  return out;
}

NttTables ntt_tables(int logn) {
  if (logn < 1 || logn > 27) throw Error("NTT tables: domain size out of range");
  const uint32_t n = 1u << logn;
  Fr g = Fr::from_canonical(FR_ROOT_2_28);
  for (int i = 0; i < 28 - (logn + 1); i++) g = g.sqr();  // order 2n
  const Fr w = g.sqr();                                   // order n
  const Fr wi = w.inv();
  NttTables T;
  T.tw_f.resize(n / 2);
  T.tw_i.resize(n / 2);
  T.coset.resize(n);
  Fr a = Fr::one(), b = Fr::one();
  for (uint32_t k = 0; k < n / 2; k++) {
    T.tw_f[k] = a;
    T.tw_i[k] = b;
    a = a * w;
    b = b * wi;
  }
  if (T.tw_f[0] != Fr::one() || T.tw_i[0] != Fr::one()) throw Error("NTT tables: tw[0] is not one");
  std::vector<Fr> gp(n);
  Fr acc = Fr::from_u32(n).inv();
  for (uint32_t i = 0; i < n; i++) {
    gp[i] = acc;
    acc = acc * g;
  }
  for (uint32_t pos = 0; pos < n; pos++) T.coset[pos] = gp[bitrev(pos, logn)];
  T.tw_f29 = table29(T.tw_f);
  T.tw_i29 = table29(T.tw_i);
  T.coset29 = table29(T.coset);
  for (int j = 0; j < 9; j++)
    if (T.tw_f29[j] != Fr29C::ONE[j] || T.tw_i29[j] != Fr29C::ONE[j]) throw Error("NTT tables: tw29[0] is not one");
  return T;
}

int ntt_turn_width(int logn) { return logn < 1 ? 0 : (logn - 1) % NTT_MAX_K + 1; }

std::vector<NttPass> ntt_pass_list(int logn) {
  std::vector<NttPass> L;
  if (logn < 1) return L;
  const int kt = ntt_turn_width(logn);   // logn - kt is a multiple of NTT_MAX_K
  for (int s0 = 0; s0 < logn - kt; s0 += NTT_MAX_K) L.push_back({NTT_DIF, (uint8_t)NTT_MAX_K, (uint8_t)s0});
  L.push_back({NTT_TURN, (uint8_t)kt, (uint8_t)(logn - kt)});
  for (int s0 = kt; s0 < logn; s0 += NTT_MAX_K) L.push_back({NTT_DIT, (uint8_t)NTT_MAX_K, (uint8_t)s0});
  return L;
}

// ------------------------------------------------------------------------------------------------- the streams of a big batch
const StreamEdge StreamPlan::edges[StreamPlan::NEDGE] = {
    {ROLE_INTERP, ROLE_VALUES}, {ROLE_INTERP, ROLE_QUOTIENT}, {ROLE_QUOTIENT, ROLE_WALK1}, {ROLE_QUOTIENT, ROLE_WALK2},
    {ROLE_WALK1, ROLE_SUMS1},   {ROLE_WALK2, ROLE_SUMS2},     {ROLE_SUMS1, ROLE_SUMS2},    {ROLE_VALUES, ROLE_SUMS2},
    {ROLE_SUMS2, ROLE_WIPE}};

int StreamPlan::busy_streams() const {
  uint32_t seen = 0;
  int n = 0;
  for (int p = 0; p < 2; p++)
    for (int r = 0; r < ROLE_COUNT; r++)
      if (r != ROLE_WIPE && !(seen >> at[p][r] & 1u)) {
        seen |= 1u << at[p][r];
        n++;
      }
  return n;
}

int hw_queues_from_env(const char* value) {
  if (!value || !*value) return 4;
  char* end = nullptr;
  const long v = strtol(value, &end, 10);
  if (end == value || *end != 0 || v < 1 || v > 1024) return 4;
  return (int)v;
}

int stream_shape_from_name(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "auto")) return SHAPE_AUTO;
  if (!strcmp(name, "wide")) return SHAPE_WIDE;
  if (!strcmp(name, "compact")) return SHAPE_COMPACT;
  return -1;
}
const char* stream_shape_name(int shape) { return shape == SHAPE_WIDE ? "wide" : shape == SHAPE_COMPACT ? "compact" : "auto"; }

StreamPlan stream_plan(int queues, int nslot, int shape) {
  StreamPlan P;
  P.shape = shape == SHAPE_WIDE || shape == SHAPE_COMPACT ? shape
            : (queues >= 8 || queues < COMPACT_MIN_QUEUES)        ? SHAPE_WIDE
                                                                  : SHAPE_COMPACT;
  if (P.shape == SHAPE_WIDE) {
    // Eight streams: two interpreters in flight (consecutive batches alternate), the quotient chain beside them, a stream
    // per walk, one back end, the Poseidon chain of the values and the wipes on streams of their own.
    const uint8_t order[ROLE_COUNT] = {ROLE_INTERP, ROLE_QUOTIENT, ROLE_WALK1, ROLE_WALK2, ROLE_VALUES, ROLE_SUMS1, ROLE_SUMS2, ROLE_WIPE};
    for (int r = 0; r < ROLE_COUNT; r++) P.order[r] = order[r];
    for (int p = 0; p < 2; p++) {
      P.at[p][ROLE_INTERP] = p ? ST_AB : ST_A;
      P.at[p][ROLE_VALUES] = ST_V;
      P.at[p][ROLE_QUOTIENT] = ST_A2;
      P.at[p][ROLE_WALK1] = ST_B;
      P.at[p][ROLE_WALK2] = ST_B2;
      P.at[p][ROLE_SUMS1] = ST_C;
      P.at[p][ROLE_SUMS2] = ST_C;
      P.at[p][ROLE_WIPE] = ST_W;
    }
    return P;
  }
  // Four streams (auto takes this map only where the process has at least four queues).  The whole front end of a batch in stream
  // order on one of two alternating high-priority streams -- each has two steps for it and runs up to two batches ahead
  // of its walks -- with the values read off the witness behind the interpreter; every walk with its own sums behind it
  // on a low-priority stream, the rest of the back end behind the G2 sums.  A slot's wipe goes to the stream its next
  // batch's front end takes (nslot batches later), so wipe and reuse are in stream order.
  const uint8_t order[ROLE_COUNT] = {ROLE_INTERP, ROLE_VALUES, ROLE_QUOTIENT, ROLE_WALK1, ROLE_WALK2, ROLE_SUMS1, ROLE_SUMS2, ROLE_WIPE};
  for (int r = 0; r < ROLE_COUNT; r++) P.order[r] = order[r];
  P.values_front = true;
  const uint8_t front[2] = {ST_A, ST_AB};
  for (int p = 0; p < 2; p++) {
    P.at[p][ROLE_INTERP] = P.at[p][ROLE_VALUES] = P.at[p][ROLE_QUOTIENT] = front[p];
    P.at[p][ROLE_WALK1] = P.at[p][ROLE_SUMS1] = ST_B;
    P.at[p][ROLE_WALK2] = P.at[p][ROLE_SUMS2] = ST_B2;
    P.at[p][ROLE_WIPE] = front[(p + nslot) & 1];
  }
  return P;
}

}  // namespace rlnamd
