// The big batches' quotient transforms on 29-bit limbs (zerokit_amd/csrc/prover_front.hip: k_ntt_pass / k_ntt_turn) without
// a GPU.  A program of its own (tests/test_ntt29_host.py builds and runs it, also with -fsanitize=address,undefined): prints
// one line per failed check and the number of checks, exit status 1 if any failed.
//   pass29() and turn29() are the kernels with the wave's group index as a loop: the same base / stride / twiddle-index
//   formulas, the same choice of K, normalize() and reduction per level (ntt29_dif_level, ntt29_dit_level), in 29-bit limb
//   arithmetic on 64-bit integers, with the loose eight-word store and load between launches.  At every step they check what
//   tools/check_fq29_bounds.py proves for all inputs: no 32-bit limb reaches 2^32, no column of a product 2^64, every K
//   dominates its subtrahend limb by limb, the quotient estimate never exceeds x / r, every stored integer is below 2^256.
//   The canonical words the last launch stores must equal, word for word, the replay in the plain Fr arithmetic of field.h
//   (pass() and turn(): the 8 x 32 kernels these replaced, the bodies tests/host/nttplan.cpp checks against the
//   definition) for logn = 3, 4, 5, 12, 13 over inputs chosen for lazy growth.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fq29_constants.h"
#include "prover_plan.h"

using namespace rlnamd;
typedef unsigned __int128 u128;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)              \
  do {                                \
    g_checks++;                       \
    if (!(cond)) {                    \
      if (g_failed++ < 40) {          \
        printf("FAILED %s: ", #cond); \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

static const uint64_t M29 = (1u << 29) - 1;

struct L29 {
  uint64_t v[9];   // 64-bit so that an overflow of the device's 32-bit limb is seen, not wrapped
};

// ---- constants, derived here from r (the device's literals are compared with the bounds tool's)
static L29 KR[6];   // K2, K6, K12, K24, K12B2, K4B2
enum { NK_2, NK_6, NK_12, NK_24, NK_12B2, NK_4B2 };
static L29 NEGR;
static uint64_t MAGIC;

static L29 biased(uint32_t k, uint64_t lo) {
  int64_t d[9];
  uint64_t c = 0;
  for (int j = 0; j < 9; j++) {
    const uint64_t t = (uint64_t)k * Fr29C::P[j] + c;
    d[j] = (int64_t)(j < 8 ? t & M29 : t);
    c = t >> 29;
  }
  L29 out;
  for (int j = 0; j < 8; j++) {
    int64_t m = (d[j] - (int64_t)lo) % (int64_t)(M29 + 1);
    if (m < 0) m += (int64_t)(M29 + 1);
    const int64_t l = (int64_t)lo + m;
    out.v[j] = (uint64_t)l;
    d[j + 1] -= (l - d[j]) >> 29;
  }
  out.v[8] = (uint64_t)d[8];
  return out;
}
static void init_constants() {
  KR[NK_2] = biased(2, 1u << 29);
  KR[NK_6] = biased(6, 1u << 29);
  KR[NK_12] = biased(12, 1u << 29);
  KR[NK_24] = biased(24, 1u << 29);
  KR[NK_12B2] = biased(12, 2u << 29);
  KR[NK_4B2] = biased(4, 2u << 29);
  bool same = true;
  for (int j = 0; j < 9; j++) same = same && KR[NK_2].v[j] == Fr29C::K2[j] && KR[NK_6].v[j] == Fr29C::K6[j];
  CHECK(same, "K2 / K6 derived here differ from fq29_constants.h");
  int64_t borrow = 0;   // 2^261 - r
  for (int j = 0; j < 9; j++) {
    int64_t t = -(int64_t)Fr29C::P[j] + borrow;
    NEGR.v[j] = (uint64_t)t & M29;
    borrow = t >> 29;
  }
  MAGIC = ((uint64_t)1 << 53) / ((uint64_t)Fr29C::P[8] + 1);
}

// ---- the helpers of the kernels
static L29 slice(const Fr& a) {
  L29 u;
  for (int j = 0; j < 9; j++) {
    const int bit = 29 * j, w = bit >> 5, s = bit & 31;
    const uint64_t two = (uint64_t)a.v[w] | (w + 1 < 8 ? (uint64_t)a.v[w + 1] << 32 : 0);
    u.v[j] = (two >> s) & (j < 8 ? M29 : 0xFFFFFFFFull);
  }
  return u;
}
static void limbs_fit(const L29& a, const char* what) {
  bool ok = true;
  for (int j = 0; j < 9; j++) ok = ok && a.v[j] < ((uint64_t)1 << 32);
  CHECK(ok, "%s: a limb reaches 2^32", what);
}
static L29 add(const L29& a, const L29& b) {
  L29 r;
  for (int j = 0; j < 9; j++) r.v[j] = a.v[j] + b.v[j];
  limbs_fit(r, "sum");
  return r;
}
static L29 sub(const L29& u, int k, const L29& v) {
  L29 r;
  bool dom = true;
  for (int j = 0; j < 9; j++) {
    dom = dom && KR[k].v[j] >= v.v[j];
    r.v[j] = u.v[j] + KR[k].v[j] - v.v[j];
  }
  CHECK(dom, "K %d does not dominate its subtrahend", k);
  limbs_fit(r, "difference");
  return r;
}
static void normalize(L29& a) {
  for (int j = 0; j < 8; j++) {
    a.v[j + 1] += a.v[j] >> 29;
    a.v[j] &= M29;
  }
  CHECK(a.v[8] < ((uint64_t)1 << 32), "normalize: the top limb reaches 2^32");
}
static bool is_norm(const L29& a) {
  for (int j = 0; j < 8; j++)
    if (a.v[j] > M29) return false;
  return true;
}
// Fr29::mul (fq29.h): eight wide rounds and a masked one, then the carry chain; columns in 128 bits to see an overflow
static L29 mul(const L29& a, const uint32_t* b) {
  u128 t[10];
  for (int j = 0; j < 10; j++) t[j] = 0;
  bool fit = true;
  auto chk = [&]() {
    for (int j = 0; j < 10; j++) fit = fit && t[j] < ((u128)1 << 64);
  };
  for (int i = 0; i < 9; i++) {
    for (int j = 0; j < 9; j++) t[j] += (u128)a.v[j] * b[i];
    chk();
    if (i < 8) {
      const uint32_t m = (uint32_t)t[0] * Fr29C::INV32;
      for (int j = 0; j < 9; j++) t[j] += (u128)m * Fr29C::P[j];
      chk();
      CHECK(((uint64_t)t[0] & 0xFFFFFFFFull) == 0, "wide round: the retired column is not a multiple of 2^32");
      t[1] += (u128)(uint32_t)((uint64_t)t[0] >> 32) * 8;
      for (int j = 0; j < 9; j++) t[j] = t[j + 1];
    } else {
      const uint32_t m = ((uint32_t)t[0] * Fr29C::INV) & (uint32_t)M29;
      for (int j = 0; j < 9; j++) t[j] += (u128)m * Fr29C::P[j];
      chk();
      const u128 carry = t[0] >> 29;
      for (int j = 0; j < 9; j++) t[j] = t[j + 1];
      t[0] += carry;
    }
    t[9] = 0;
    chk();
  }
  L29 r;
  for (int j = 0; j < 8; j++) {
    r.v[j] = (uint64_t)t[j] & M29;
    t[j + 1] += t[j] >> 29;
    chk();
  }
  r.v[8] = (uint64_t)t[8];
  CHECK(fit, "a column of a product reaches 2^64");
  CHECK(r.v[8] < ((uint64_t)1 << 32), "product: the top limb reaches 2^32");
  return r;
}
// is the normalised a >= q r ?  (for the estimate's check)
static bool geq_multiple(const L29& a, uint64_t q) {
  uint64_t c = 0, w[9];
  for (int j = 0; j < 9; j++) {
    const uint64_t t = q * Fr29C::P[j] + c;
    w[j] = j < 8 ? t & M29 : t;
    c = t >> 29;
  }
  for (int j = 8; j >= 0; j--)
    if (a.v[j] != w[j]) return a.v[j] > w[j];
  return true;
}
static void reduce(L29& x) {   // ntt29_reduce
  CHECK(is_norm(x) && x.v[8] < ((uint64_t)1 << 29), "reduce: operand not normalised");
  const uint64_t q = (uint64_t)(((u128)(uint32_t)x.v[8] * MAGIC) >> 32) >> 21;
  CHECK(geq_multiple(x, q), "reduce: the estimate %llu exceeds x / r", (unsigned long long)q);
  uint64_t c = 0;
  for (int j = 0; j < 9; j++) {
    const uint64_t t = q * NEGR.v[j] + x.v[j] + c;
    x.v[j] = t & M29;
    c = t >> 29;
  }
  CHECK(!geq_multiple(x, 2), "reduce: 2 r or more is left");
}
static Fr pack(const L29& x, bool canonical) {   // ntt29_pack / pack_reduced
  L29 y = x;
  CHECK(is_norm(y) && y.v[8] < (1u << 24), "store: the integer reaches 2^256");
  if (canonical && geq_multiple(y, 1)) {
    int64_t borrow = 0;
    for (int j = 0; j < 9; j++) {
      const int64_t t = (int64_t)y.v[j] - (int64_t)Fr29C::P[j] + borrow;
      y.v[j] = (uint64_t)t & (j < 8 ? M29 : 0xFFFFFFFFull);
      borrow = t >> (j < 8 ? 29 : 63);
    }
    CHECK(borrow == 0, "canonical store: negative");
  }
  if (canonical) CHECK(!geq_multiple(y, 1), "canonical store: r or more is left");
  Fr o;
  for (int w = 0; w < 8; w++) {
    const int j0 = (32 * w) / 29, s = 32 * w - 29 * j0;
    uint64_t acc = y.v[j0] >> s;
    acc |= y.v[j0 + 1] << (29 - s);
    if (j0 + 2 < 9) acc |= y.v[j0 + 2] << (58 - s);
    o.v[w] = (uint32_t)acc;
  }
  return o;
}
static int dif_sums(int K, int m, int t) {
  int c = 0;
  for (int l = t - 1; l >= 0; l--) {
    if (m & ((1 << K) >> (l + 1))) break;
    c++;
  }
  return c;
}
// one level of a 2^K-point block; unit(jm) and twiddle(jm, t) as in the kernels
template <class UNIT, class TW>
static void dif_level(L29* e, int K, int t, UNIT unit, TW twiddle) {
  const int R = 1 << K, half = R >> (t + 1);
  for (int m = 0; m < R; m++) {
    if (m & half) continue;
    const int c = dif_sums(K, m + half, t);
    L29 u = e[m], v = e[m + half];
    if (c == 2) {
      normalize(u);
      normalize(v);
    }
    const int k = t == 0 ? NK_6 : c == 0 ? NK_2 : c == 1 ? (t == 1 ? NK_12B2 : NK_4B2) : NK_24;
    e[m] = add(u, v);
    L29 d = sub(u, k, v);
    if (unit(m & (half - 1))) normalize(d); else d = mul(d, twiddle(m & (half - 1), t));
    e[m + half] = d;
  }
}
template <class UNIT, class TW>
static void dit_level(L29* e, int K, bool from_loads, int t, UNIT unit, TW twiddle) {
  const int R = 1 << K, half = 1 << t;
  for (int m = 0; m < R; m++) {
    if (m & half) continue;
    L29 u = e[m], v = e[m + half];
    if (unit(m & (half - 1))) {
      if (t > 0) normalize(v);
      CHECK(is_norm(v), "DIT unit butterfly: subtrahend not normalised");
      const int k = from_loads ? (t == 0 ? NK_6 : t == 1 ? NK_12 : NK_24) : (t == 0 ? NK_2 : t == 1 ? NK_6 : NK_12);
      e[m] = add(u, v);
      e[m + half] = sub(u, k, v);
    } else {
      v = mul(v, twiddle(m & (half - 1), t));
      e[m] = add(u, v);
      e[m + half] = sub(u, NK_2, v);
    }
  }
}

template <bool DIF>
static void pass29(std::vector<Fr>& x, const std::vector<uint32_t>& tw29, int logn, int K, int s0, bool last) {
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
    const bool lo0 = lo == 0;
    L29 e[8];
    for (int m = 0; m < R; m++) e[m] = slice(x.at(base + m * stride));
    auto unit = [&](int jm) { return jm == 0 && lo0; };
    auto twiddle = [&](int jm, int t) -> const uint32_t* {
      const uint32_t j = (uint32_t)jm * stride + lo;
      const uint32_t ti = DIF ? (j << (s0 + t)) : (j << (logn - 1 - (s0 + t)));
      return &tw29.at((size_t)ti * 9 + 8) - 8;
    };
    for (int t = 0; t < K; t++) {
      if (DIF) dif_level(e, K, t, unit, twiddle); else dit_level(e, K, true, t, unit, twiddle);
    }
    for (int m = 0; m < R; m++) {
      L29 y = e[m];
      if (DIF) {
        if (dif_sums(K, m, K) > 0) normalize(y);
        if (m == 0 || lo0) reduce(y);
        x.at(base + m * stride) = pack(y, false);
      } else {
        normalize(y);
        reduce(y);
        x.at(base + m * stride) = pack(y, last);
      }
    }
  }
}

static void turn29(std::vector<Fr>& x, const NttTables& T, int logn, int KT, bool last) {
  const int R = 1 << KT;
  const uint32_t n = 1u << logn;
  for (uint32_t g = 0; g < (n >> KT); g++) {
    const uint32_t base = g << KT;
    L29 e[8];
    for (int m = 0; m < R; m++) e[m] = slice(x.at(base + m));
    auto unit = [](int jm) { return jm == 0; };
    auto tw_inv = [&](int jm, int t) -> const uint32_t* { return &T.tw_i29.at(((size_t)jm << (logn - KT + t)) * 9 + 8) - 8; };
    auto tw_fwd = [&](int jm, int t) -> const uint32_t* { return &T.tw_f29.at(((size_t)jm << (logn - 1 - t)) * 9 + 8) - 8; };
    for (int t = 0; t < KT; t++) dif_level(e, KT, t, unit, tw_inv);
    for (int m = 0; m < R; m++) e[m] = mul(e[m], &T.coset29.at((size_t)(base + m) * 9 + 8) - 8);
    for (int t = 0; t < KT; t++) dit_level(e, KT, false, t, unit, tw_fwd);
    for (int m = 0; m < R; m++) {
      L29 y = e[m];
      normalize(y);
      if (last || KT > 1) reduce(y);
      x.at(base + m) = pack(y, last);
    }
  }
}

// ---- the same launches in the plain Fr arithmetic of field.h: the 8 x 32 kernels' bodies (tests/host/nttplan.cpp checks
// these against the definition of the transforms)
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
        Fr u = e[m], v = e[m + half];
        if (DIF) {
          e[m] = u + v;
          Fr d = u - v;
          if (!unit) d = d * tw.at(ti);
          e[m + half] = d;
        } else {
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

static Fr words(const uint32_t (&w)[8]) {
  Fr f;
  for (int k = 0; k < 8; k++) f.v[k] = w[k];
  return f;
}

static void check_replay(int logn) {
  const uint32_t n = 1u << logn;
  const NttTables T = ntt_tables(logn);
  CHECK(T.tw_f29.size() == (size_t)n / 2 * 9 && T.tw_i29.size() == (size_t)n / 2 * 9 && T.coset29.size() == (size_t)n * 9,
        "logn=%d: table sizes", logn);
  {
    bool one = true, canon = true;
    for (int j = 0; j < 9; j++) one = one && T.tw_f29[j] == Fr29C::ONE[j] && T.tw_i29[j] == Fr29C::ONE[j];
    for (size_t i = 0; i < (size_t)n; i++) {
      L29 c;
      for (int j = 0; j < 9; j++) c.v[j] = T.coset29[i * 9 + j];
      canon = canon && is_norm(c) && !geq_multiple(c, 1);
    }
    CHECK(one, "logn=%d: entry 0 of a twiddle table is not the one of the 2^261 radix", logn);
    CHECK(canon, "logn=%d: a scale factor is not canonical", logn);
  }
  uint32_t rm1[8], one[8] = {1, 0, 0, 0, 0, 0, 0, 0}, zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 8; k++) rm1[k] = FrParams::MOD[k];
  rm1[0] -= 1;   // r is odd
  const std::vector<NttPass> L = ntt_pass_list(logn);
  uint64_t st = 0x13198A2E03707344ull + (uint64_t)logn;
  for (int kind = 0; kind < 8; kind++) {
    std::vector<Fr> a(n, words(zero));
    for (uint32_t i = 0; i < n; i++) {
      if (kind == 0) a[i] = words(rm1);
      else if (kind == 1) a[i] = words(one);
      else if (kind == 2) a[i] = words((i & 1) ? rm1 : zero);
      else if (kind >= 6) {
        uint32_t c[8];
        for (int k = 0; k < 8; k++) {
          st = st * 6364136223846793005ull + 1442695040888963407ull;
          c[k] = (uint32_t)(st >> 32);
        }
        c[7] &= 0x0FFFFFFFu;   // 252 bits: below r
        a[i] = words(c);
      }
    }
    if (kind == 3) a[0] = words(rm1);
    if (kind == 4) a[n / 2] = words(rm1);
    if (kind == 5) a[n - 1] = words(rm1);
    std::vector<Fr> x = a, y = a;
    for (const NttPass& p : L) {
      const bool last = &p == &L.back();
      if (p.kind == NTT_TURN) {
        turn(x, T, logn, p.k);
        turn29(y, T, logn, p.k, last);
      } else if (p.kind == NTT_DIF) {
        pass<true>(x, T.tw_i, logn, p.k, p.s0);
        pass29<true>(y, T.tw_i29, logn, p.k, p.s0, last);
      } else {
        pass<false>(x, T.tw_f, logn, p.k, p.s0);
        pass29<false>(y, T.tw_f29, logn, p.k, p.s0, last);
      }
    }
    uint32_t bad = 0, first = 0;
    for (uint32_t i = n; i-- > 0;)
      if (memcmp(x[i].v, y[i].v, 32) != 0) {
        bad++;
        first = i;
      }
    CHECK(bad == 0, "logn=%d input %d: %u of %u points differ from the Fr replay, the first at %u", logn, kind, bad, n, first);
  }
}

int main() {
  init_constants();
  try {
    for (int logn : {3, 4, 5, 12, 13}) check_replay(logn);
  } catch (const Error& e) {
    CHECK(false, "%s", e.what());
  }
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
