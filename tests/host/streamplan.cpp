// stream_plan (zerokit_amd/csrc/prover_plan.cpp) without a GPU: which stream every role of a big batch takes, for every
// queue count and slot count the prover can meet.  A program of its own (tests/test_stream_plan_host.py builds and runs it;
// it may be built with -fsanitize=address,undefined as well): prints one line per failed check and the number of checks,
// exit status 1 if any failed.  What is covered is the stream TABLE the prover takes from the plan -- who shares a stream
// with whom, and that the table admits a submission without a cyclic wait; the event records and waits themselves are
// written out in Prover::enqueue and are covered by the GPU tests (tests/test_gpu_stream_shapes.py), not here.
//   streamplan              all checks
//   streamplan dump Q N     the plan of Q queues and N slots, one "parity role stream" line each (the test reads wide's map)
//   streamplan shape N MODE IDLE COMPACT   batch_shape's values_w / values_front for a batch of N proofs
//   streamplan config JSON  the "stream_shape" a config_path object gives a ProverConfig, or the error's text
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "prover_plan.h"
#include "tree_config.h"

using namespace rlnamd;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)            \
  do {                              \
    g_checks++;                     \
    if (!(cond)) {                  \
      g_failed++;                   \
      printf("FAILED %s: ", #cond); \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

static const char* const kRole[ROLE_COUNT] = {"interp", "values", "quotient", "walk1", "walk2", "sums1", "sums2", "wipe"};
static const char* const kStream[ST_COUNT] = {"sW", "sA", "sA2", "sAb", "sV", "sB", "sC", "sB2"};

// The replay: `nb` batches submitted the way a stream of batches is (collect of batch b - nslot, with its wipe, right before
// batch b is submitted), as a graph on the host.  A node = one role of one batch; an edge = "must finish before": the
// previous node submitted to the same stream, the producer of every StreamPlan edge (through an event where the streams
// differ -- where they are the same the producer must have been submitted earlier), and the slot's wipe before its next
// batch's interpreter (the slot's event).  Returns false on a cycle or on a consumer submitted ahead of its producer.
static bool replay(const StreamPlan& P, int nslot, int nb, std::string* why) {
  struct Node { std::vector<int> before; };
  std::vector<Node> nodes;
  std::map<std::pair<int, int>, int> id;   // (batch, role) -> node
  int last_on[ST_COUNT];
  for (int& v : last_on) v = -1;
  auto submit = [&](int b, int r) {
    const int s = P.at[b & 1][r];
    const int me = (int)nodes.size();
    nodes.push_back({});
    id[{b, r}] = me;
    if (last_on[s] >= 0) nodes[me].before.push_back(last_on[s]);
    last_on[s] = me;
    for (const StreamEdge& e : StreamPlan::edges)
      if (e.to == r) {
        auto it = id.find({b, (int)e.from});
        if (it == id.end()) {
          *why = std::string(kRole[r]) + " submitted ahead of its producer " + kRole[e.from];
          return false;
        }
        nodes[me].before.push_back(it->second);   // (same stream: already implied by the stream's order)
      }
    if (r == ROLE_INTERP && b >= nslot) {
      auto it = id.find({b - nslot, (int)ROLE_WIPE});
      if (it == id.end()) {
        *why = "a batch submitted before the wipe of its slot";
        return false;
      }
      nodes[me].before.push_back(it->second);
    }
    return true;
  };
  for (int b = 0; b < nb; b++) {
    if (b >= nslot && !submit(b - nslot, ROLE_WIPE)) return false;
    for (int k = 0; k < ROLE_COUNT; k++)
      if (P.order[k] != ROLE_WIPE && !submit(b, P.order[k])) return false;
  }
  for (int b = nb > nslot ? nb - nslot : 0; b < nb; b++)
    if (!submit(b, ROLE_WIPE)) return false;
  // every edge points to an earlier node unless something is wrong: Kahn's algorithm all the same (the check is the
  // graph's, not the construction's)
  std::vector<int> indeg(nodes.size(), 0);
  std::vector<std::vector<int>> out(nodes.size());
  for (size_t v = 0; v < nodes.size(); v++)
    for (int u : nodes[v].before) {
      out[u].push_back((int)v);
      indeg[v]++;
    }
  std::vector<int> ready;
  for (size_t v = 0; v < nodes.size(); v++)
    if (!indeg[v]) ready.push_back((int)v);
  size_t done = 0;
  while (!ready.empty()) {
    const int u = ready.back();
    ready.pop_back();
    done++;
    for (int v : out[u])
      if (--indeg[v] == 0) ready.push_back(v);
  }
  if (done != nodes.size()) *why = "cyclic wait";
  return done == nodes.size();
}

static void check_plan(const StreamPlan& P, int queues, int nslot, int asked) {
  const char* name = stream_shape_name(P.shape);
  CHECK(P.shape == SHAPE_WIDE || P.shape == SHAPE_COMPACT, "q=%d nslot=%d: unresolved shape", queues, nslot);
  if (asked == SHAPE_AUTO) {
    // auto never keeps more streams busy than the process has queues: compact at 4 .. 7, wide at 8 and more, and wide --
    // what every queue count had before -- below four, where neither map fits
    CHECK(P.shape == ((queues >= 8 || queues < COMPACT_MIN_QUEUES) ? SHAPE_WIDE : SHAPE_COMPACT), "q=%d: auto gave %s", queues, name);
    if (queues >= COMPACT_MIN_QUEUES) CHECK(P.busy_streams() <= queues, "q=%d: auto (%s) keeps %d streams busy", queues, name, P.busy_streams());
  }
  else CHECK(P.shape == asked, "q=%d: asked %s, got %s", queues, stream_shape_name(asked), name);
  std::set<int> seen_roles;
  for (int k = 0; k < ROLE_COUNT; k++) seen_roles.insert(P.order[k]);
  CHECK(seen_roles.size() == ROLE_COUNT && P.order[ROLE_COUNT - 1] == ROLE_WIPE, "%s: order is not a permutation ending in the wipe", name);
  for (int p = 0; p < 2; p++) {
    for (int r = 0; r < ROLE_COUNT; r++) CHECK(P.at[p][r] < ST_COUNT, "%s: role %s has no stream", name, kRole[r]);
    // the two walks never share a stream with each other or with a front end (either parity's)
    CHECK(P.at[p][ROLE_WALK1] != P.at[p][ROLE_WALK2], "%s: the walks share %s", name, kStream[P.at[p][ROLE_WALK1]]);
    for (int q = 0; q < 2; q++)
      for (int w : {ROLE_WALK1, ROLE_WALK2})
        for (int f : {ROLE_INTERP, ROLE_QUOTIENT, ROLE_VALUES})
          if (!(f == ROLE_VALUES && !P.values_front))
            CHECK(P.at[p][w] != P.at[q][f], "%s: %s shares %s with %s", name, kRole[w], kStream[P.at[p][w]], kRole[f]);
    // every consumer behind its producer on one stream, or listed as needing an event
    int pos[ROLE_COUNT];
    for (int k = 0; k < ROLE_COUNT; k++) pos[P.order[k]] = k;
    for (const StreamEdge& e : StreamPlan::edges) {
      CHECK(pos[e.from] < pos[e.to], "%s: %s is submitted ahead of %s", name, kRole[e.to], kRole[e.from]);
    }
  }
  // the walks keep their streams from batch to batch (a walk's stream is what orders it behind the previous one)
  CHECK(P.at[0][ROLE_WALK1] == P.at[1][ROLE_WALK1] && P.at[0][ROLE_WALK2] == P.at[1][ROLE_WALK2], "%s: a walk changes streams", name);
  if (P.shape == SHAPE_COMPACT) {
    CHECK(P.busy_streams() <= 4, "compact keeps %d streams busy", P.busy_streams());
    CHECK(P.values_front, "compact without the values on the front end");
    for (int p = 0; p < 2; p++) {
      // the whole front end in stream order; each walk's sums behind it; the wipe on the stream of the slot's next batch
      CHECK(P.at[p][ROLE_INTERP] == P.at[p][ROLE_QUOTIENT] && P.at[p][ROLE_INTERP] == P.at[p][ROLE_VALUES], "compact: front end on two streams");
      CHECK(P.at[p][ROLE_SUMS1] == P.at[p][ROLE_WALK1] && P.at[p][ROLE_SUMS2] == P.at[p][ROLE_WALK2], "compact: sums away from their walk");
      CHECK(P.at[p][ROLE_WIPE] == P.at[(p + nslot) & 1][ROLE_INTERP], "compact nslot=%d: wipe of parity %d on %s, next batch on %s", nslot, p,
            kStream[P.at[p][ROLE_WIPE]], kStream[P.at[(p + nslot) & 1][ROLE_INTERP]]);
    }
    CHECK(P.at[0][ROLE_INTERP] != P.at[1][ROLE_INTERP], "compact: consecutive front ends share a stream");
    CHECK(P.at[0][ROLE_INTERP] != ST_W && P.at[1][ROLE_INTERP] != ST_W && P.at[0][ROLE_WALK1] != ST_W && P.at[0][ROLE_WALK2] != ST_W,
          "compact: a busy stream is the first stream the process creates");
  } else {
    // today's map of eight streams
    const uint8_t want[2][ROLE_COUNT] = {{ST_A, ST_V, ST_A2, ST_B, ST_B2, ST_C, ST_C, ST_W}, {ST_AB, ST_V, ST_A2, ST_B, ST_B2, ST_C, ST_C, ST_W}};
    for (int p = 0; p < 2; p++)
      for (int r = 0; r < ROLE_COUNT; r++)
        CHECK(P.at[p][r] == want[p][r], "wide: parity %d role %s on %s, expected %s", p, kRole[r], kStream[P.at[p][r]], kStream[want[p][r]]);
    CHECK(!P.values_front, "wide with the values on the front end");
    const uint8_t order[ROLE_COUNT] = {ROLE_INTERP, ROLE_QUOTIENT, ROLE_WALK1, ROLE_WALK2, ROLE_VALUES, ROLE_SUMS1, ROLE_SUMS2, ROLE_WIPE};
    CHECK(!memcmp(P.order, order, sizeof order), "wide: another submission order");
  }
  CHECK(P.busy_streams() <= (P.shape == SHAPE_COMPACT ? 4 : 8), "%s keeps %d streams busy", name, P.busy_streams());
  std::string why;
  CHECK(replay(P, nslot, nslot + 3, &why), "%s q=%d nslot=%d: %s", name, queues, nslot, why.c_str());
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "dump")) {
    const StreamPlan P = stream_plan(atoi(argv[2]), atoi(argv[3]));
    printf("shape %s busy %d values_front %d\n", stream_shape_name(P.shape), P.busy_streams(), (int)P.values_front);
    for (int p = 0; p < 2; p++)
      for (int r = 0; r < ROLE_COUNT; r++) printf("%d %s %s\n", p, kRole[r], kStream[P.at[p][r]]);
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "shape")) {
    BatchQuery q;
    q.n = (size_t)atoi(argv[2]);
    q.mode = atoi(argv[3]);
    q.idle = atoi(argv[4]) != 0;
    q.compact = atoi(argv[5]) != 0;
    q.inputs = true;
    q.witlanes_ok = q.segs_ok = q.cone_ok = q.have_values_kernel = true;
    q.ni = 6;
    q.logn = 13;
    q.capacity = 1024;
    q.small_stride = 128;
    const BatchShape S = batch_shape(q, ProverTuning());
    printf("small %d values_w %d values_front %d\n", (int)S.small, (int)S.values_w, (int)S.values_front);
    q.ni = 9;   // the multi-message circuit has no values kernel
    q.have_values_kernel = false;
    printf("multi values_front %d\n", (int)batch_shape(q, ProverTuning()).values_front);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "config")) {
    try {
      const TreeConfig c = parse_tree_config(argv[2]);
      printf("stream_shape %d\n", c.prover_config().stream_shape);
    } catch (const Error& e) {
      printf("error %s\n", e.what());
    }
    return 0;
  }
  for (int queues : {1, 2, 3, 4, 7, 8, 32})
    for (int nslot = 2; nslot <= 6; nslot++)
      for (int asked : {SHAPE_AUTO, SHAPE_WIDE, SHAPE_COMPACT}) check_plan(stream_plan(queues, nslot, asked), queues, nslot, asked);
  // the replay does find what it looks for: the wipe in FRONT of the back end it waits for, on one stream
  {
    StreamPlan P = stream_plan(4, 5, SHAPE_COMPACT);
    const uint8_t order[ROLE_COUNT] = {ROLE_INTERP, ROLE_VALUES, ROLE_QUOTIENT, ROLE_WALK1, ROLE_WALK2, ROLE_SUMS2, ROLE_SUMS1, ROLE_WIPE};
    memcpy(P.order, order, sizeof order);
    std::string why;
    CHECK(!replay(P, 5, 8, &why), "a consumer ahead of its producer went unnoticed");
  }
  // the queue count as the environment gives it
  CHECK(hw_queues_from_env(nullptr) == 4 && hw_queues_from_env("") == 4 && hw_queues_from_env("x") == 4 && hw_queues_from_env("8x") == 4, "default queues");
  CHECK(hw_queues_from_env("0") == 4 && hw_queues_from_env("-2") == 4, "non-positive queues");
  CHECK(hw_queues_from_env("8") == 8 && hw_queues_from_env("2") == 2 && hw_queues_from_env("32") == 32, "parsed queues");
  CHECK(stream_shape_from_name("auto") == SHAPE_AUTO && stream_shape_from_name("wide") == SHAPE_WIDE &&
            stream_shape_from_name("compact") == SHAPE_COMPACT && stream_shape_from_name("narrow") < 0 && stream_shape_from_name(nullptr) < 0,
        "shape names");
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
