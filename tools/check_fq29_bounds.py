#!/usr/bin/env python3
"""Column-bound proof for zerokit_amd/csrc/fq29.h: replays the interleaved Montgomery product (redc_dot / sqr_add) of
every call site in fq29.h, walk29.h, poseidon.h and the NTT's mul_mont with ALL operand limbs at the maximum of their
representation class and the reduction digit at its maximum (2^32 - 1 in a wide round, 2^29 - 1 in a masked one), and
asserts that no 64-bit column accumulator reaches 2^64.  Every term of a column is non-negative and monotone in each
operand limb and in the digit, so the all-maximum replay bounds every real execution.  Run by tests/test_host_math.py.
The second half (NttReplay) does the same for the big batches' quotient transforms, which run whole passes on these limbs
with lazy sums: every level of every instantiated k_ntt_pass / k_ntt_turn and the reduction in front of their stores
(tests/test_ntt29_host.py).

Classes (limb vectors of 9 entries):
  N(B)      normalised value < B q: limbs 0..7 <= 2^29 - 1, limb 8 <= (B q) >> 232
  K - b     lazy difference, b normalised: limb j <= K[j]
  x + y     sums of the above, limb by limb
"""
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B29 = 29
M = (1 << B29) - 1
LIMIT = 1 << 64


def limbs(v):
    return [(v >> (B29 * j)) & M for j in range(8)] + [v >> (B29 * 8)]


def biased(v, lo):
    out, rem = [], v
    for _ in range(8):
        d = rem & M
        l = lo + ((d - lo) % (1 << B29))
        out.append(l)
        rem = (rem - l) >> B29
    out.append(rem)
    return out


class Field:
    def __init__(self, p):
        self.p = p
        self.P = limbs(p)
        self.K2, self.K4, self.K6, self.K8 = (biased(k * p, 1 << B29) for k in (2, 4, 6, 8))
        self.K4T = biased(4 * p, 3 << B29)

    def N(self, bq=10):
        return [M] * 8 + [(bq * self.p) >> 232]


def add(a, b):
    return [x + y for x, y in zip(a, b)]


def scale(a, k):
    return [k * x for x in a]


def replay(f, prods, wide, addend=None, square=False):
    """prods: list of (a, b) limb-maximum vectors; returns the maximum column value seen"""
    t = [0] * 10
    worst = 0

    def chk():
        nonlocal worst
        worst = max(worst, max(t))
        assert max(t) < LIMIT, "column overflow: %.3f x 2^60" % (max(t) / 2**60)

    for i in range(9):
        for a, b in prods:
            if square:   # row i of sqr_add: a_i^2 into t[i], (2 a_i) a_l into t[l]
                assert 2 * a[i] < 1 << 32
                t[i] += a[i] * a[i]
                for l in range(i + 1, 9):
                    t[l] += 2 * a[i] * a[l]
            else:
                for j in range(9):
                    assert a[j] < 1 << 32 and b[i] < 1 << 32
                    t[j] += a[j] * b[i]
            chk()
        w = wide and i < 8
        m = (1 << 32) - 1 if w else M
        for j in range(9):
            t[j] += m * f.P[j]
        chk()
        carry = t[0] >> 29
        t = t[1:] + [0]
        t[0] += carry
        chk()
    if addend:
        for j in range(9):
            assert addend[j] < 1 << 32
            t[j] += addend[j]
    for j in range(8):
        t[j + 1] += t[j] >> 29
        chk()
    assert t[8] < 1 << 32, "top limb does not fit"
    return worst


def call_sites(name, f):
    """The call-site table of one field ("Fq" or "Fr", f = Field(modulus)): rows (label, products, wide, addend, square).
    products: one (a, b) pair of limb-maximum vectors per product of the dot product (b is unused in a square row);
    wide: wide or masked reduction rounds; addend: limb maxima of the value added in finish(), or None; square: the row
    runs sqr_add's product scheme.  main() replays these rows; tests/test_gpu_field_ops.py drives the device with operands
    of the same classes, so what the replay proves and what the device is given cannot drift apart."""
    N = f.N()
    lazy2 = scale(N, 2)                       # sums of two normalised values, 2 x value
    sites = []
    if name == "Fq":
        D = add(N, f.K6)                      # Q + K6 - X3, un-normalised
        sites += [
            ("g1.U2  mul_add(px, ZZ, K6 - X)", [(N, N)], True, f.K6, False),
            ("g1.S2  mul_add(K2 - py, ZZZ, K4 - Y)", [(f.K2, N)], True, f.K4, False),
            ("g1.PP  sqr(P)", [(N, N)], True, None, True),
            ("g1.ZZ3/Q/PPP/ZZZ3  mul(N, N)", [(N, N)], True, None, False),
            ("g1.X3  sqr_add(R, K4T - PPP - 2Q)", [(N, N)], True, f.K4T, True),
            ("g1.Y3  dot2(R, Q + K6 - X3, K4 - Y, PPP)", [(N, D), (f.K4, N)], True, None, False),
            ("g1.dbl sqr(2 py)", [(lazy2, lazy2)], True, None, True),
            ("g1.dbl mul(2 py, V)", [(lazy2, N)], True, None, False),
            ("g1.dbl dot2(M, D, K4 - py, W)", [(N, N), (f.K4, N)], True, None, False),
            ("fq2.mul c0 dot2_add(a0, b0, K8 - a1, b1, K - x)", [(N, N), (f.K8, N)], True, f.K6, False),
            ("fq2.mul c1 dot2_add(a0, b1, a1, b0, K - x)", [(N, N), (N, N)], True, f.K6, False),
            ("fq2.sqr mul_add(a0 + a1, d, K4T - ..)", [(lazy2, N)], True, f.K4T, False),
            ("g2.Y3  dot4 (R0 D0, K8-R1 D1, K4-Y0 P0, Y1 P1)", [(N, N), (f.K8, N), (f.K4, N), (N, N)], True, None, False),
            ("g2.Y3  dot4 (R0 D1, R1 D0, K4-Y0 P1, K4-Y1 P0)", [(N, N), (N, N), (f.K4, N), (f.K4, N)], True, None, False),
            ("g2.dbl dot4 (M0 D0, K8-M1 D1, W0 K4-y0, W1 y1)", [(N, N), (f.K8, N), (N, f.K4), (N, N)], True, None, False),
            ("g2.dbl dot4 (M0 D1, M1 D0, W0 K4-y1, W1 K4-y0)", [(N, N), (N, N), (N, f.K4), (N, f.K4)], True, None, False),
        ]
    else:
        sites += [
            # partial-round lanes 1.. stay normalised but grow to < 72 r (poseidon.h): N(80); "+ ark" adds < r
            ("poseidon sqr(st + ark)", [(add(f.N(80), f.N(1)), None)], True, None, True),
            ("poseidon mul(x4, st + ark)", [(N, add(f.N(80), f.N(1)))], True, None, False),
            ("poseidon t=2 dot2(mds, st), st[1] lazy", [(N, N), (N, lazy2)], True, None, False),
            ("poseidon full round dot3(mds, st)", [(N, N)] * 3, True, None, False),
            ("poseidon full round dot4(mds, st)", [(N, N)] * 4, True, None, False),
            ("poseidon dense partial round dot3 masked, two lazy", [(N, N), (N, lazy2), (N, lazy2)], False, None, False),
            ("poseidon row (sparse partial round) dotn<4>", [(N, f.N(80))] * 4, True, None, False),
            ("poseidon dotn<5> masked", [(N, f.N(80))] * 5, False, None, False),
            ("poseidon mul_add(u_i, st[0], st[i])  (st[i] < 72 r)", [(N, N)], True, f.N(80), False),
            # four lanes per hash (poseidon_hash4_lanes): x = s_0 + k with s_0 < 4 r; p_i = row0[i] s_i < 1.5 r
            ("poseidon 4-lane mul(x, x | u_i | row0[0]), x = s_0 + k", [(add(N, f.N(1)), add(N, f.N(1)))], True, None, False),
            ("poseidon 4-lane mul(row0[i], s_i)  (s_i < 72 r)", [(N, f.N(80))], True, None, False),
            ("poseidon 4-lane s_0' = mul_add(b, x^4, p_1 + p_2)", [(N, N)], True, lazy2, False),
            ("witness interpreter a * b + c (mul_add, every value below 7.5 r)", [(N, N)], True, N, False),
        ]
    sites += [
        ("%s from_fq / to_fq / mul_mont  mul(N, const)" % name, [(N, limbs(f.p - 1))], True, None, False),
        ("%s mul(lazy, lazy)" % name, [(lazy2, lazy2)], True, None, False),
    ]
    return sites


FIELDS = (("Fq", Q), ("Fr", R))


# ====================================================================================================================
# The quotient transforms of a big batch on 29-bit limbs (prover_front.hip: k_ntt_pass / k_ntt_turn).  Every function
# below restates one helper of the kernels, on MAXIMA: a value is (limb maxima, maximum of the integer).  The replay
# walks every level of every instantiated pass and turn in both of a wave's modes (lo != 0: no butterfly is a unit one;
# lo == 0: every butterfly with a compile-time zero twiddle index is) and asserts
#   * no 32-bit limb sum and no normalisation carry reaches 2^32, no column of a product reaches 2^64,
#   * every K - v has K[j] >= v[j] in every limb (so no limb borrows),
#   * the quotient estimate of the pre-store reduction never exceeds x / r and leaves less than 2 r,
#   * every stored integer is below 2^256 (below 2 r where the canonical store's conditional subtraction follows).
# Kept apart from call_sites(): that table also drives the device's class-maximum operands (tests/field_ops_cases.py).
NTT_RHO = (R >> 232) + 1                  # ceil(r / 2^232)
NTT_MAGIC = (1 << 53) // NTT_RHO          # q = (v[8] * MAGIC) >> 53 = floor(v[8] / RHO), or one less on exact multiples
NTT_NEGR = limbs((1 << 261) - R)          # x - q r = x + q (2^261 - r) mod 2^261


def ntt_constants():
    """name -> (limbs, integer): the minuend biases of the transforms' differences"""
    lo1, lo2 = 1 << B29, 2 << B29
    return {"K2": (biased(2 * R, lo1), 2 * R), "K6": (biased(6 * R, lo1), 6 * R), "K12": (biased(12 * R, lo1), 12 * R),
            "K24": (biased(24 * R, lo1), 24 * R), "K12B2": (biased(12 * R, lo2), 12 * R), "K4B2": (biased(4 * R, lo2), 4 * R)}


class NttReplay:
    def __init__(self):
        self.f = Field(R)
        self.K = ntt_constants()
        self.tw = ([M] * 8 + [(R - 1) >> 232], R - 1)      # table entries: canonical t 2^261 mod r
        self.rows = {}                                     # label -> worst column
        self.stored = 0
        self.where = ""

    # ---- the helpers of the kernels
    def load(self):
        return ([M] * 8 + [(1 << 24) - 1], (1 << 256) - 1)           # any integer below 2^256, re-sliced

    def is_norm(self, a):
        return all(x <= M for x in a[0][:8])

    def add(self, a, b):
        l = [x + y for x, y in zip(a[0], b[0])]
        assert max(l) < 1 << 32, "%s: limb sum reaches 2^32" % self.where
        return (l, a[1] + b[1])

    def norm(self, a):
        c = 0
        for j in range(9):
            x = a[0][j] + c
            assert x < 1 << 32, "%s: normalisation carry reaches 2^32" % self.where
            c = x >> 29
        assert a[1] >> 232 < 1 << 29, "%s: value does not fit nine limbs" % self.where
        return ([M] * 8 + [a[1] >> 232], a[1])

    def sub(self, u, kname, v):
        K, kval = self.K[kname]
        assert all(K[j] >= v[0][j] for j in range(9)), "%s: %s does not dominate the subtrahend" % (self.where, kname)
        assert kval >= v[1]
        l = [x + y for x, y in zip(u[0], K)]
        assert max(l) < 1 << 32, "%s: limb sum reaches 2^32" % self.where
        return (l, u[1] + kval)

    def mul(self, d, label):                                           # Fr29::mul: wide rounds at every call site
        w = replay(self.f, [(d[0], self.tw[0])], True)
        key = (label, True)
        self.rows[key] = max(self.rows.get(key, 0), w)
        val = R + ((d[1] * self.tw[1]) >> 261) + (R >> 25)            # digits < 2^261 + 2^236
        return ([M] * 8 + [val >> 232], val)

    def reduce(self, a):
        assert self.is_norm(a)
        v8max = a[0][8]
        qmax = (v8max * NTT_MAGIC) >> 53
        assert NTT_MAGIC < 1 << 32 and v8max < 1 << 29 and qmax < 1 << 8
        worst = 0
        for k in range(qmax + 1):
            lo = -((-(k << 53)) // NTT_MAGIC)                          # smallest v[8] with estimate k
            hi = min(v8max, -((-((k + 1) << 53)) // NTT_MAGIC) - 1)    # largest
            assert (lo * NTT_MAGIC) >> 53 == k and (hi * NTT_MAGIC) >> 53 == k
            assert (lo << 232) >= k * R, "%s: estimate above x / r" % self.where
            worst = max(worst, min(((hi + 1) << 232) - 1, a[1]) - k * R)
        assert worst < 2 * R and worst < 1 << 256, "%s: reduction leaves %.3f r" % (self.where, worst / R)
        # columns of x + q NEGR: q NEGR[j] + v[j] + carry < 2^8 2^29 + 2^29 + 2^9
        return ([M] * 8 + [worst >> 232], worst)

    def store(self, a, canonical):
        assert self.is_norm(a) and a[1] < (2 * R if canonical else 1 << 256), \
            "%s: stored value reaches %.3f r" % (self.where, a[1] / R)
        assert a[0][8] < 1 << 24
        self.stored = max(self.stored, a[1])

    # ---- the levels, as the kernels run them
    @staticmethod
    def dif_sums(K, m, t):
        """how many of the DIF levels t - 1, t - 2, ... left element m on the sum side, consecutively"""
        c = 0
        for l in range(t - 1, -1, -1):
            if m & ((1 << K) >> (l + 1)):
                break
            c += 1
        return c

    def dif_levels(self, e, K, lo0, tag):
        for t in range(K):
            half = (1 << K) >> (t + 1)
            for m in range(1 << K):
                if m & half:
                    continue
                self.where = "%s DIF level %d m %d" % (tag, t, m)
                unit = lo0 and (m & (half - 1)) == 0
                c = self.dif_sums(K, m + half, t)
                assert c <= 2
                u, v = e[m], e[m + half]
                if c == 2:
                    u, v = self.norm(u), self.norm(v)
                kb = "K6" if t == 0 else "K2" if c == 0 else ("K12B2" if t == 1 else "K4B2") if c == 1 else "K24"
                e[m] = self.add(u, v)
                d = self.sub(u, kb, v)
                e[m + half] = self.norm(d) if unit else self.mul(d, "ntt29 DIF (u + %s - v) tw" % kb)

    def dit_levels(self, e, K, lo0, tag, unit_k=("K6", "K12", "K24")):
        for t in range(K):
            half = 1 << t
            for m in range(1 << K):
                if m & half:
                    continue
                self.where = "%s DIT level %d m %d" % (tag, t, m)
                unit = lo0 and (m & (half - 1)) == 0
                u, v = e[m], e[m + half]
                if not unit:
                    v = self.mul(v, "ntt29 DIT level %d v tw" % t)
                    kb = "K2"
                else:
                    if t > 0:
                        v = self.norm(v)
                    assert self.is_norm(v)
                    kb = unit_k[t]
                e[m] = self.add(u, v)
                e[m + half] = self.sub(u, kb, v)

    def pass_dif(self, K, lo0):
        tag = "k_ntt_pass<%d, DIF> lo %s 0" % (K, "==" if lo0 else "!=")
        e = [self.load() for _ in range(1 << K)]
        self.dif_levels(e, K, lo0, tag)
        for m in range(1 << K):
            self.where = "%s store m %d" % (tag, m)
            x = e[m]
            if self.dif_sums(K, m, K) > 0:
                x = self.norm(x)
            if m == 0 or lo0:
                x = self.reduce(x)
            self.store(x, False)

    def pass_dit(self, K, lo0, last):
        tag = "k_ntt_pass<%d, DIT%s> lo %s 0" % (K, ", last" if last else "", "==" if lo0 else "!=")
        e = [self.load() for _ in range(1 << K)]
        self.dit_levels(e, K, lo0, tag)
        for m in range(1 << K):
            self.where = "%s store m %d" % (tag, m)
            self.store(self.reduce(self.norm(e[m])), last)

    def turn(self, KT, last):
        tag = "k_ntt_turn<%d%s>" % (KT, ", last" if last else "")
        e = [self.load() for _ in range(1 << KT)]
        self.dif_levels(e, KT, True, tag)
        for m in range(1 << KT):
            self.where = "%s scale m %d" % (tag, m)
            e[m] = self.mul(e[m], "ntt29 turn scale")
        self.dit_levels(e, KT, True, tag, ("K2", "K6", "K12"))      # from products, not from loads
        for m in range(1 << KT):
            self.where = "%s store m %d" % (tag, m)
            x = self.norm(e[m])
            if last or KT > 1:
                x = self.reduce(x)
            self.store(x, last)


def ntt29_main(max_k=3):
    """replays every instantiation; returns rows like main()'s and the largest stored integer in units of r"""
    rp = NttReplay()
    for lo0 in (False, True):
        rp.pass_dif(max_k, lo0)
        for last in (False, True):
            rp.pass_dit(max_k, lo0, last)
    for kt in range(1, max_k + 1):
        for last in (False, True):
            rp.turn(kt, last)
    rows = [("Fr", label, "wide" if wide else "masked", w / 2**60) for (label, wide), w in sorted(rp.rows.items())]
    return rows, rp.stored / R


def ntt29_check_source(path):
    """the constants in prover_front.hip are the ones the replay used"""
    src = open(path).read()
    want = {k: v[0] for k, v in ntt_constants().items() if k not in ("K2", "K6")}
    want["NEGR"] = NTT_NEGR
    for name, l in want.items():
        assert ("%s[9] = {%s}" % (name, ", ".join("0x%08xu" % x for x in l))) in src, "prover_front.hip: %s differs" % name
    assert ("MAGIC = 0x%08xu" % NTT_MAGIC) in src, "prover_front.hip: MAGIC differs"
    f = Field(R)
    assert ntt_constants()["K2"][0] == f.K2 and ntt_constants()["K6"][0] == f.K6      # Fr29C's own


def main(verbose=True):
    rows = []
    for name, p in FIELDS:
        f = Field(p)
        for label, prods, wide, addend, square in call_sites(name, f):
            w = replay(f, prods, wide, addend, square)
            rows.append((name, label, "wide" if wide else "masked", w / 2**60))
    import os
    ntt_rows, stored = ntt29_main()
    rows += ntt_rows
    ntt29_check_source(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zerokit_amd", "csrc", "prover_front.hip"))
    if verbose:
        print("ntt29: largest integer stored between launches %.3f r (2^256 = %.3f r)" % (stored, (1 << 256) / R))
    if verbose:
        for r in rows:
            print("%-3s %-62s %-6s max column %6.3f x 2^60 (limit 16)" % r)
    return rows


if __name__ == "__main__":
    main()
