// ntt_pass_list / ntt_tables (zerokit_amd/csrc/prover_plan.cpp) without a GPU: the launches that carry the quotient's three
// transforms in big batches.  A program of its own (tests/test_ntt_plan_host.py builds and runs it; it may be built with
// -fsanitize=address,undefined as well): prints one line per failed check and the number of checks, exit status 1 if any
// failed.
//   1. the list for logn = 1 .. 20: every DIF level and every DIT level exactly once, in order; no block above eight
//      points; one turn, of width ((logn - 1) mod 3) + 1, between the two directions; a transform of at most three
//      levels is the turn alone; nothing for logn < 1
//   2. the list replayed on the host for logn = 3, 4, 5, 12, 13 over a seeded vector: pass() and turn() below are
//      k_ntt_pass and k_ntt_turn (prover_front.hip) with the wave's group index as a loop -- the same base, stride and
//      twiddle-index formulas, the same products left out -- in the plain Fr arithmetic of field.h.  The result must
//      equal, limb for limb, the direct evaluation of the definition: c_i = 1/n sum_j a_j w^(-i j), d_i = g^i c_i,
//      h_k = sum_i d_i w^(i k).  A wrong base, stride or twiddle index shows here.
//   nttplan list LOGN   prints "kind k s0" per launch (kind: dif / turn / dit)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "prover_plan.h"

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

static const char* const kKind[3] = {"dif", "turn", "dit"};

static void check_list(int logn) {
  const std::vector<NttPass> L = ntt_pass_list(logn);
  const int kt = ntt_turn_width(logn);
  CHECK(kt == (logn - 1) % 3 + 1 && kt >= 1 && kt <= 3, "logn=%d: turn width %d", logn, kt);
  CHECK((logn - kt) % 3 == 0, "logn=%d: %d levels beside the turn do not split into threes", logn, logn - kt);
  std::vector<int> dif(logn, 0), dit(logn, 0);
  int turns = 0, phase = 0;   // phase: 0 before the turn, 1 after it
  int next_dif = 0, next_dit = 0;
  for (const NttPass& p : L) {
    CHECK(p.k >= 1 && p.k <= NTT_MAX_K && (1 << p.k) <= 8, "logn=%d: a block of %d points", logn, 1 << p.k);
    CHECK(p.kind <= NTT_DIT, "logn=%d: kind %d", logn, p.kind);
    if (p.kind == NTT_TURN) {
      turns++;
      CHECK(phase == 0, "logn=%d: a second turn", logn);
      phase = 1;
      CHECK(p.k == kt && p.s0 == logn - kt, "logn=%d: turn k=%d s0=%d", logn, p.k, p.s0);
      CHECK(next_dif == p.s0 && next_dit == 0, "logn=%d: the turn is not where the DIF passes stop", logn);
      for (int t = 0; t < p.k; t++) {
        if (p.s0 + t < logn) dif[p.s0 + t]++;
        if (t < logn) dit[t]++;
      }
      next_dif = p.s0 + p.k;
      next_dit = p.k;
    } else if (p.kind == NTT_DIF) {
      CHECK(phase == 0, "logn=%d: a DIF pass behind the turn", logn);
      CHECK(p.s0 == next_dif && p.k == NTT_MAX_K, "logn=%d: DIF pass s0=%d k=%d, expected s0=%d", logn, p.s0, p.k, next_dif);
      // its lowest stride is above the turn's points: the pass never meets stride 1 and never scales
      CHECK(p.s0 + p.k <= logn - kt, "logn=%d: DIF pass s0=%d reaches into the turn", logn, p.s0);
      for (int t = 0; t < p.k && p.s0 + t < logn; t++) dif[p.s0 + t]++;
      next_dif = p.s0 + p.k;
    } else {
      CHECK(phase == 1, "logn=%d: a DIT pass ahead of the turn", logn);
      CHECK(p.s0 == next_dit && p.k == NTT_MAX_K && p.s0 >= kt, "logn=%d: DIT pass s0=%d k=%d, expected s0=%d", logn, p.s0, p.k, next_dit);
      for (int t = 0; t < p.k && p.s0 + t < logn; t++) dit[p.s0 + t]++;
      next_dit = p.s0 + p.k;
    }
  }
  CHECK(turns == 1, "logn=%d: %d turns", logn, turns);
  CHECK(next_dif == logn && next_dit == logn, "logn=%d: levels end at %d / %d", logn, next_dif, next_dit);
  for (int t = 0; t < logn; t++) CHECK(dif[t] == 1 && dit[t] == 1, "logn=%d level %d: %d DIF, %d DIT", logn, t, dif[t], dit[t]);
  CHECK((int)L.size() == 2 * ((logn - kt) / 3) + 1, "logn=%d: %d launches", logn, (int)L.size());
  if (logn <= 3) CHECK(L.size() == 1 && L[0].kind == NTT_TURN && L[0].k == logn, "logn=%d: not the turn alone", logn);
}

// ---- the kernels' bodies on the host (prover_front.hip), one vector, one "lane"
template <bool DIF>
static void pass(std::vector<Fr>& x, const std::vector<Fr>& tw, int logn, int K, int s0) {
  const int R = 1 << K;
  const uint32_t n = 1u << logn;
  for (uint32_t g = 0; g < (n >> K); g++) {
    uint32_t stride, base;
    if (DIF) {
      stride = n >> (s0 + K);
      uint32_t blk = g / stride, lo = g % stride;
      base = blk * (n >> s0) + lo;
    } else {
      stride = 1u << s0;
      uint32_t blk = g / stride, lo = g % stride;
      base = blk * (stride << K) + lo;
    }
    const uint32_t lo = g % stride;
    Fr e[8];
    for (int m = 0; m < R; m++) e[m] = x.at(base + m * stride);
    for (int t = 0; t < K; t++) {
      const int half = DIF ? (R >> (t + 1)) : (1 << t);
      for (int m = 0; m < R; m++) {
        if (m & half) continue;
        const bool unit = (m & (half - 1)) == 0 && lo == 0;
        uint32_t j = (uint32_t)(m & (half - 1)) * stride + lo;
        uint32_t ti = DIF ? (j << (s0 + t)) : (j << (logn - 1 - (s0 + t)));
        if (DIF) {
          Fr u = e[m], v = e[m + half];
          e[m] = u + v;
          Fr d = u - v;
          if (!unit) d = d * tw.at(ti);
          e[m + half] = d;
        } else {
          Fr u = e[m], v = e[m + half];
          if (!unit) v = v * tw.at(ti);
          e[m] = u + v;
          e[m + half] = u - v;
        }
      }
    }
    for (int m = 0; m < R; m++) x.at(base + m * stride) = e[m];
  }
}

static void turn(std::vector<Fr>& x, const NttTables& T, int logn, int KT) {
  const int R = 1 << KT;
  const uint32_t n = 1u << logn;
  for (uint32_t g = 0; g < (n >> KT); g++) {
    const uint32_t base = g << KT;
    Fr e[8];
    for (int m = 0; m < R; m++) e[m] = x.at(base + m);
    for (int t = 0; t < KT; t++) {
      const int half = R >> (t + 1);
      for (int m = 0; m < R; m++) {
        if (m & half) continue;
        const uint32_t j = (uint32_t)(m & (half - 1));
        Fr u = e[m], v = e[m + half];
        e[m] = u + v;
        Fr d = u - v;
        if (j) d = d * T.tw_i.at((size_t)j << (logn - KT + t));
        e[m + half] = d;
      }
    }
    for (int m = 0; m < R; m++) e[m] = e[m] * T.coset.at(base + m);
    for (int t = 0; t < KT; t++) {
      const int half = 1 << t;
      for (int m = 0; m < R; m++) {
        if (m & half) continue;
        const uint32_t j = (uint32_t)(m & (half - 1));
        Fr u = e[m], v = e[m + half];
        if (j) v = v * T.tw_f.at((size_t)j << (logn - 1 - t));
        e[m] = u + v;
        e[m + half] = u - v;
      }
    }
    for (int m = 0; m < R; m++) x.at(base + m) = e[m];
  }
}

// out_k = sum_i in_i base^(i k), base of order n given by its powers pw[0 .. n): n^2 products, the rows dealt to a few threads
static std::vector<Fr> dft(const std::vector<Fr>& in, const std::vector<Fr>& pw) {
  const size_t n = in.size();
  std::vector<Fr> out(n);
  auto rows = [&](size_t k0, size_t step) {
    for (size_t k = k0; k < n; k += step) {
      Fr acc = Fr::zero();
      size_t e = 0;   // i k mod n
      for (size_t i = 0; i < n; i++) {
        acc = acc + in[i] * pw[e];
        e = (e + k) & (n - 1);
      }
      out[k] = acc;
    }
  };
  const size_t nt = n < 1024 ? 1 : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(rows, t, nt);
  rows(0, nt);
  for (std::thread& t : th) t.join();
  return out;
}

static void check_replay(int logn) {
  const uint32_t n = 1u << logn;
  const NttTables T = ntt_tables(logn);
  CHECK(T.tw_f.size() == n / 2 && T.tw_i.size() == n / 2 && T.coset.size() == n, "logn=%d: table sizes", logn);
  CHECK(T.tw_f[0] == Fr::one() && T.tw_i[0] == Fr::one(), "logn=%d: tw[0] is not the Montgomery one", logn);
  // x . one = x and a difference is reduced: what lets a butterfly with twiddle index 0 keep u - v as it is
  uint64_t st = 0x243F6A8885A308D3ull + (uint64_t)logn;
  std::vector<Fr> a(n);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t c[8];
    for (int k = 0; k < 8; k++) {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      c[k] = (uint32_t)(st >> 32);
    }
    c[7] &= 0x0FFFFFFFu;   // 252 bits: below r
    a[i] = Fr::from_canonical(c);
  }
  a[0] = Fr::zero();
  if (n > 2) a[2] = Fr::one().neg();
  {
    bool ok = true;
    for (uint32_t i = 0; i + 1 < n && i < 64; i++) {
      const Fr d = a[i] - a[i + 1];
      uint32_t c[8];
      d.to_canonical(c);
      ok = ok && Fr::from_canonical(c) == d && d * Fr::one() == d && !limbs_geq(d.v, FrParams::MOD);
    }
    CHECK(ok, "logn=%d: a difference that is not reduced, or changed by the product with one", logn);
  }
  // the launches
  std::vector<Fr> x = a;
  for (const NttPass& p : ntt_pass_list(logn)) {
    if (p.kind == NTT_TURN) turn(x, T, logn, p.k);
    else if (p.kind == NTT_DIF) pass<true>(x, T.tw_i, logn, p.k, p.s0);
    else pass<false>(x, T.tw_f, logn, p.k, p.s0);
  }
  // the definition: powers of w and of 1 / w from the tables' own generator (w^(n/2) = -1), g from coset[] at the
  // positions whose bit reversal is 0 and 1
  std::vector<Fr> pw(n), pwi(n);
  for (uint32_t k = 0; k < n / 2; k++) {
    pw[k] = T.tw_f[k];
    pw[k + n / 2] = T.tw_f[k].neg();
    pwi[k] = T.tw_i[k];
    pwi[k + n / 2] = T.tw_i[k].neg();
  }
  const Fr ninv = T.coset[0], g = T.coset[n / 2] * Fr::from_u32(n);   // coset[bitrev 1] = g / n
  CHECK(ninv * Fr::from_u32(n) == Fr::one(), "logn=%d: coset[0] is not 1 / n", logn);
  {
    Fr g2n = g;
    for (int i = 0; i < logn; i++) g2n = g2n.sqr();
    CHECK(g.sqr() == pw[1] && g2n == Fr::one().neg(), "logn=%d: g is not a root of the doubled domain", logn);
  }
  std::vector<Fr> c = dft(a, pwi);
  Fr gi = ninv;
  for (uint32_t i = 0; i < n; i++) {
    c[i] = c[i] * gi;
    gi = gi * g;
  }
  const std::vector<Fr> h = dft(c, pw);
  uint32_t bad = 0, first = 0;
  for (uint32_t i = n; i-- > 0;)
    if (x[i] != h[i]) {
      bad++;
      first = i;
    }
  CHECK(bad == 0, "logn=%d: %u of %u points differ from the definition, the first at %u", logn, bad, n, first);
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "list")) {
    for (const NttPass& p : ntt_pass_list(atoi(argv[2]))) printf("%s %d %d\n", kKind[p.kind], p.k, p.s0);
    return 0;
  }
  CHECK(ntt_pass_list(0).empty() && ntt_pass_list(-1).empty() && ntt_turn_width(0) == 0, "a list for no levels");
  for (int logn = 1; logn <= 20; logn++) check_list(logn);
  CHECK(ntt_pass_list(13).size() == 9 && ntt_turn_width(13) == 1, "13 levels: 3, 3, 3, 3 | turn(1) | 3, 3, 3, 3");
  CHECK(ntt_pass_list(12).size() == 7 && ntt_turn_width(12) == 3, "12 levels: 3, 3, 3 | turn(3) | 3, 3, 3");
  CHECK(ntt_turn_width(11) == 2 && ntt_pass_list(11).size() == 7, "11 levels: 3, 3, 3 | turn(2) | 3, 3, 3");
  try {
    for (int logn : {3, 4, 5, 12, 13}) check_replay(logn);
  } catch (const Error& e) {
    CHECK(false, "%s", e.what());
  }
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
