"""Operand sets, big-integer references and checkers for the arithmetic probes (include/rln_amd.h: rlnamd_probe_*).

Shared by tests/test_gpu_field_ops.py, which sends the operands to the device, and tests/test_field_ops_host.py, which
runs the same generators and checkers on a pure-Python model of fq29.h's redc_dot and on the host build of
witness_slow_op.  Every reference here is plain Python integer arithmetic; every comparison is exact.

Layouts: an 8 x 32 element is 8 little-endian words, a 9 x 29 element 9 raw limb words (value = sum v[j] 2^(29 j))."""
import importlib.util
import os
import random

import numpy as np

from oracle.pyref import wtns_graph
from oracle.pyref.bn254 import G1, G2, G1_GEN, G2_GEN, Q, R, f2_inv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("check_fq29_bounds", os.path.join(ROOT, "tools", "check_fq29_bounds.py"))
bounds = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bounds)

MODULUS = {0: R, 1: Q}          # probe field index -> modulus (0 = Fr / Fr29, 1 = Fq / Fq29)
FIELD_NAME = {0: "Fr", 1: "Fq"}
R256 = 1 << 256
R261 = 1 << 261
M29 = (1 << 29) - 1
_SH = [29 * j for j in range(9)]

# ---- operation numbers and words per tuple (include/rln_amd.h)
FP_OPS = ["add", "sub", "neg", "dbl", "mul", "sqr", "dot2", "dot3", "dot4", "dot2_sub", "from_canonical", "to_canonical",
          "inv", "fq2_mul", "fq2_sqr", "fq2_inv"]
FP_SHAPE = {"add": (2, 1), "sub": (2, 1), "neg": (1, 1), "dbl": (1, 1), "mul": (2, 1), "sqr": (1, 1), "dot2": (4, 1),
            "dot3": (6, 1), "dot4": (8, 1), "dot2_sub": (4, 1), "from_canonical": (1, 1), "to_canonical": (1, 1),
            "inv": (1, 1), "fq2_mul": (4, 2), "fq2_sqr": (2, 2), "fq2_inv": (2, 2)}   # elements in, elements out
F29_OPS = ["mul", "mul_add", "sqr", "sqr_add", "dot2", "dot2_add", "dot3", "dot3_wide", "dot4", "dot4_wide", "dotn5",
           "sub_k2", "sub_k4", "sub_k6", "sub_k8", "neg_k2", "neg_k4", "neg_k6", "neg_k8", "normalize", "is_zero",
           "slice", "pack_reduced", "from_fq", "to_fq", "mul_mont", "from_canonical", "unpack29", "pack29_reduced",
           "g1_walk", "g2_walk", "g1_add", "g2_add", "g1_table", "g2_table"]
F29_SHAPE = {"mul": (18, 9), "mul_add": (27, 9), "sqr": (9, 9), "sqr_add": (18, 9), "dot2": (36, 9), "dot2_add": (45, 9),
             "dot3": (54, 9), "dot3_wide": (54, 9), "dot4": (72, 9), "dot4_wide": (72, 9), "dotn5": (90, 9),
             "sub_k2": (18, 9), "sub_k4": (18, 9), "sub_k6": (18, 9), "sub_k8": (18, 9),
             "neg_k2": (9, 9), "neg_k4": (9, 9), "neg_k6": (9, 9), "neg_k8": (9, 9), "normalize": (9, 9), "is_zero": (9, 1),
             "slice": (8, 9), "pack_reduced": (9, 8), "from_fq": (8, 9), "to_fq": (9, 8), "mul_mont": (17, 8),
             "from_canonical": (8, 9), "unpack29": (8, 9), "pack29_reduced": (9, 8),
             "g1_add": (72, 36), "g2_add": (144, 72), "g1_table": (16, 16), "g2_table": (32, 32)}   # words in, words out
WALK_WORDS = {"g1_walk": (16, 36), "g2_walk": (32, 72)}   # entry words, accumulator words
WERR_SHIFT, WERR_BITOP, WERR_UNO_ID = 2, 3, 4
G_ID = 23


# ---- word <-> integer helpers
def words8(xs):
    """list of integers < 2^256 -> (n, 8) uint32"""
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u4").reshape(len(xs), 8).astype(np.uint32)


def ints8(arr):
    """(n, 8 k) uint32 -> n lists of k integers"""
    arr = np.ascontiguousarray(arr, dtype="<u4")
    k = arr.shape[1] // 8
    raw = arr.tobytes()
    return [[int.from_bytes(raw[32 * (i * k + e):32 * (i * k + e) + 32], "little") for e in range(k)]
            for i in range(arr.shape[0])]


def limbs9(v):
    return [(v >> s) & M29 for s in _SH[:8]] + [v >> 232]


def val9(limbs):
    return sum(x << s for x, s in zip(limbs, _SH))


def vals9(arr):
    """(n, 9 k) uint32 -> n lists of k integers (the values the limb vectors represent)"""
    rows = np.asarray(arr).tolist()
    return [[val9(r[9 * e:9 * e + 9]) for e in range(len(r) // 9)] for r in rows]


def tuples8(ts):
    """list of tuples of integers -> (n, 8 k) uint32"""
    k = len(ts[0])
    return words8([x for t in ts for x in t]).reshape(len(ts), 8 * k)


# ================================================================================================================
# 8 x 32 field
def edge_values(p):
    """The edge operand set S of one modulus (stored integers below p) -> (values, {category: members})"""
    rm = R256 % p
    top = p >> 224
    ones = sum(0xFFFFFFFF << (32 * i) for i in range(7)) | ((top - 1) << 224)   # a carry in every column
    cat = {
        "small": [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2],
        "montgomery": [rm, rm * rm % p, p - rm],
        "powers": [(1 << (32 * k)) + d for k in range(1, 8) for d in (-1, 0, 1)],
        "all_ones": [ones],
        "one_word_cleared": [ones & ~(0xFFFFFFFF << (32 * w)) for w in range(8)],
    }
    partners = []
    for s in (ones, rm, 1 << 128, (1 << 224) + 1, p - 2):
        partners += [p - s, p - s + 1, p - s - 1]        # s + partner = p, p + 1, p - 1
    cat["sum_partners"] = partners
    vals = []
    for vs in cat.values():
        for v in vs:
            assert 0 <= v < p
            if v not in vals:
                vals.append(v)
    return vals, cat


def fp_expected(op, p, t):
    """stored integers in (a R mod p) -> stored integers out, for one tuple"""
    ri = pow(R256, -1, p)
    if op == "add":
        return [(t[0] + t[1]) % p]
    if op == "sub":
        return [(t[0] - t[1]) % p]
    if op == "neg":
        return [(-t[0]) % p]
    if op == "dbl":
        return [2 * t[0] % p]
    if op == "mul":
        return [t[0] * t[1] * ri % p]
    if op == "sqr":
        return [t[0] * t[0] * ri % p]
    if op in ("dot2", "dot3", "dot4"):
        return [sum(t[2 * k] * t[2 * k + 1] for k in range(len(t) // 2)) * ri % p]
    if op == "dot2_sub":
        return [(t[0] * t[1] - t[2] * t[3]) * ri % p]
    if op == "from_canonical":      # any x < 2^256: x R^2 / 2^256 < p before the subtraction, so the result is x R mod p
        return [t[0] * R256 % p]
    if op == "to_canonical":
        return [t[0] * ri % p]
    if op == "inv":                 # a = x / R, a^-1 R = R^2 / x
        return [0 if t[0] == 0 else pow(t[0], -1, p) * R256 * R256 % p]
    if op == "fq2_mul":
        return [(t[0] * t[2] - t[1] * t[3]) * ri % p, (t[0] * t[3] + t[1] * t[2]) * ri % p]
    if op == "fq2_sqr":
        return [(t[0] * t[0] - t[1] * t[1]) * ri % p, 2 * t[0] * t[1] * ri % p]
    if op == "fq2_inv":
        if t[0] == 0 and t[1] == 0:
            return [0, 0]
        a = (t[0] * ri % p, t[1] * ri % p)
        i0, i1 = f2_inv(a)
        return [i0 * R256 % p, i1 * R256 % p]
    raise ValueError(op)


def fp_cases(op, p, n_random, seed):
    """operand tuples of one 8 x 32 operation -> (tuples, {category: count})"""
    rnd = random.Random(seed)
    S, cat = edge_values(p)
    arity = FP_SHAPE[op][0]
    counts = {}
    if op == "from_canonical":
        extra = [p, p + 1, 2 * p, 5 * p - 1, R256 - 1]
        ts = [(x,) for x in S + extra]
        counts["non_reduced"] = len(extra)
    elif arity == 1:
        ts = [(x,) for x in S]
    elif arity == 2:
        ts = [(x, y) for x in S for y in S]
        counts["sum_is_p"] = sum(1 for x, y in ts if x + y == p)
        counts["sum_is_p_plus_1"] = sum(1 for x, y in ts if x + y == p + 1)
        counts["sum_is_p_minus_1"] = sum(1 for x, y in ts if x + y == p - 1)
        counts["equal"] = sum(1 for x, y in ts if x == y)
    else:
        ts = [tuple([x] * arity) for x in S]                                    # all-equal tuples, all-(p - 1) among them
        ts += [tuple(rnd.choice(S) for _ in range(arity)) for _ in range(3000)]
        ts += [tuple(rnd.choice((p - 1, p - 2, cat["all_ones"][0])) for _ in range(arity)) for _ in range(64)]
        counts["all_p_minus_1"] = sum(1 for t in ts if all(x == p - 1 for x in t))
    counts["edge"] = len(ts)
    ts += [tuple(rnd.randrange(p) for _ in range(arity)) for _ in range(n_random)]
    counts["random"] = n_random
    counts["all_ones_operand"] = sum(1 for t in ts if cat["all_ones"][0] in t)
    return ts, counts


def fp_check(op, p, ts, out):
    """out: (n, 8 x results) uint32 from the probe"""
    got = ints8(out)
    bad = []
    for i, t in enumerate(ts):
        want = fp_expected(op, p, t)
        if got[i] != want:
            bad.append((i, t, got[i], want))
    assert not bad, "%s: %d of %d tuples differ, first: operands %s got %s want %s" % (
        op, len(bad), len(ts), [hex(x) for x in bad[0][1]], [hex(x) for x in bad[0][2]], [hex(x) for x in bad[0][3]])


# ================================================================================================================
# 9 x 29 products: the rows of tools/check_fq29_bounds.py
M_BOUND = (1 << 261) + (1 << 236)    # reduction digits < 2^32 in eight wide rounds, < 2^29 in the masked last one


def site_rows(field):
    """rows of the call-site table for one field plus the instantiations no call site uses today (masked dot4, the other
    field's dot3) at the classes fq29.h documents for them; each -> (label, op name, operand maxima in device order)"""
    name, p = FIELD_NAME[field], MODULUS[field]
    f = bounds.Field(p)
    N, lazy2 = f.N(), bounds.scale(f.N(), 2)
    rows = list(bounds.call_sites(name, f))
    rows += [
        ("extra: dot4 masked, two lazy operands (fq29.h)", [(N, lazy2), (N, lazy2), (N, N), (N, N)], False, None, False),
        ("extra: dot3 wide, all normalised", [(N, N)] * 3, True, None, False),
        ("extra: dot3 masked, two lazy", [(N, N), (N, lazy2), (N, lazy2)], False, None, False),
        ("extra: sqr(N)", [(N, None)], True, None, True),
        ("extra: dot2(N, N, N, N)", [(N, N), (N, N)], True, None, False),
        ("extra: sqr_add(N, K4T - ..)", [(N, N)], True, f.K4T, True),
        ("extra: dot2_add(N, N, K8 - x, N, K6 - y)", [(N, N), (f.K8, N)], True, f.K6, False),
    ]
    out = []
    for label, prods, wide, addend, square in rows:
        bounds.replay(f, prods, wide, addend, square)     # the extra rows pass the column proof too
        if square:
            assert len(prods) == 1 and wide
            op, maxes = ("sqr_add" if addend else "sqr"), [prods[0][0]]
        else:
            k = len(prods)
            if k <= 2:
                assert wide
                op = {1: "mul", 2: "dot2"}[k] + ("_add" if addend else "")
            else:
                assert addend is None and (k < 5 or (not wide and field == 0))   # poseidon_dotn29<5>: masked, Fr29
                op = {3: "dot3", 4: "dot4", 5: "dotn5"}[k] + ("_wide" if wide else "")
            maxes = [m for ab in prods for m in ab]
        if addend:
            maxes = maxes + [addend]
        out.append((label, op, [list(m) for m in maxes], bool(addend), square))
    return out


def product_operands(maxes, n_random, seed):
    """operand sets (i) - (iv) of one row -> ((n, 9 k) uint32, {category: count})"""
    k = len(maxes)
    flat = [m for op in maxes for m in op]
    rows = [flat, [0] * (9 * k)]
    for o in range(k):
        for j in range(9):
            r = [0] * (9 * k)
            r[9 * o + j] = maxes[o][j]
            rows.append(r)
    fixed = np.array(rows, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    rand = np.stack([rng.integers(0, m + 1, size=n_random, dtype=np.uint64) for m in flat], axis=1).astype(np.uint32)
    counts = {"class_maximum": 1, "zero": 1, "single_limb": 9 * k, "random": n_random}
    return np.concatenate([fixed, rand]), counts


def product_check(label, p, inp, out, has_add, square):
    """limbs normalised and (val(v) - val(add)) 2^261 = sum val(a_k) val(b_k) + M p with 0 <= M < 2^261 + 2^236;
    returns the largest M / 2^261 seen"""
    ops, res = vals9(inp), np.asarray(out).tolist()
    assert np.all(np.asarray(out)[:, :8] < (1 << 29)), "%s: a result limb 0 .. 7 reaches 2^29" % label
    worst = 0
    for i, (a, v) in enumerate(zip(ops, res)):
        add = a.pop() if has_add else 0
        s = a[0] * a[0] if square else sum(a[2 * k] * a[2 * k + 1] for k in range(len(a) // 2))
        m, rem = divmod((val9(v) - add) * R261 - s, p)
        assert rem == 0 and 0 <= m < M_BOUND, "%s: tuple %d: remainder %d, M / 2^261 = %.6f" % (label, i, rem, m / R261)
        worst = max(worst, m)
    return worst / R261


class Model29:
    """fq29.h's redc_dot / sqr_add / finish in Python, 64-bit columns wrapping as the device's do"""
    W64 = (1 << 64) - 1

    def __init__(self, p):
        self.p = p
        self.P = limbs9(p)
        self.inv32 = (-pow(self.P[0], -1, 1 << 32)) % (1 << 32)
        self.inv29 = self.inv32 & M29

    def _round(self, t, wide):
        W = self.W64
        if wide:
            m = (t[0] * self.inv32) & 0xFFFFFFFF
            for j in range(9):
                t[j] = (t[j] + m * self.P[j]) & W
            t[1] = (t[1] + ((t[0] >> 32) & 0xFFFFFFFF) * 8) & W
            t[:] = t[1:] + [0]
        else:
            m = ((t[0] & 0xFFFFFFFF) * self.inv29) & M29
            for j in range(9):
                t[j] = (t[j] + m * self.P[j]) & W
            carry = t[0] >> 29
            t[:] = t[1:] + [0]
            t[0] = (t[0] + carry) & W

    def _finish(self, t, add):
        W = self.W64
        if add is not None:
            for j in range(9):
                t[j] = (t[j] + add[j]) & W
        r = []
        for j in range(8):
            r.append(t[j] & M29)
            t[j + 1] = (t[j + 1] + (t[j] >> 29)) & W
        r.append(t[8] & 0xFFFFFFFF)
        return r

    def dot(self, pairs, wide, add=None):
        W, t = self.W64, [0] * 10
        for i in range(9):
            for a, b in pairs:
                for j in range(9):
                    t[j] = (t[j] + a[j] * b[i]) & W
            self._round(t, wide and i < 8)
        return self._finish(t, add)

    def sqr(self, a, add=None):
        W, t = self.W64, [0] * 10
        for i in range(9):
            t[i] = (t[i] + a[i] * a[i]) & W
            d = (2 * a[i]) & 0xFFFFFFFF
            for l in range(i + 1, 9):
                t[l] = (t[l] + d * a[l]) & W
            self._round(t, i < 8)
        return self._finish(t, add)

    def run(self, op, row):
        """one probe tuple (list of 9 k limbs) -> 9 result limbs"""
        e = [row[9 * k:9 * k + 9] for k in range(len(row) // 9)]
        add = e.pop() if op.endswith("_add") else None
        if op.startswith("sqr"):
            return self.sqr(e[0], add)
        wide = not (op in ("dot3", "dot4", "dotn5"))
        return self.dot([(e[2 * k], e[2 * k + 1]) for k in range(len(e) // 2)], wide, add)


# ================================================================================================================
# 9 x 29 exact-value primitives
def f29_consts(p):
    f = bounds.Field(p)
    return {"K2": f.K2, "K4": f.K4, "K6": f.K6, "K8": f.K8, "K4T": f.K4T, "P": f.P,
            "FROM_CANON": limbs9(pow(2, 522, p)), "FROM_FQ": limbs9(pow(2, 266, p)), "TO_FQ": limbs9(R256 % p),
            "QINV": pow(p, -1, 1 << 29)}


def slice_cases(p, n_random, seed):
    rnd = random.Random(seed)
    xs = [0, 1, R256 - 1, p, p - 1, 2 * p, M29, 1 << 29, (1 << 232) - 1, 1 << 232, 1 << 255]
    xs += [(1 << (29 * j)) - 1 for j in range(1, 9)] + [1 << (32 * k) for k in range(1, 8)]
    xs += [rnd.getrandbits(256) for _ in range(n_random)]
    return xs, {"all_ones_word": xs.count(R256 - 1), "random": n_random}


def _borrows_through(v, P):
    """does v - p borrow out of every one of the nine limbs (pack_reduced's chain)?"""
    l, b = limbs9(v), 0
    for j in range(9):
        x = l[j] - P[j] + b
        b = -1 if x < 0 else 0
        if b == 0:
            return False
    return True


def pack_cases(p, n_random, seed):
    """normalised values in [0, 2 p)"""
    rnd = random.Random(seed)
    P = limbs9(p)
    cat = {"named": [0, 1, p - 1, p, p + 1, 2 * p - 1],
           "p_pm_limb": [p + s * (1 << (29 * j)) for j in range(9) for s in (1, -1)],
           "full_borrow": [val9([rnd.randrange(P[0])] + [rnd.randint(0, P[j]) for j in range(1, 8)] + [P[8]]) for _ in range(32)]
           + [val9([P[0] - 1] + P[1:])],
           "random": [rnd.randrange(2 * p) for _ in range(n_random)]}
    vs = [v for c in cat.values() for v in c]
    assert all(0 <= v < 2 * p for v in vs)
    counts = {k: len(c) for k, c in cat.items()}
    counts["borrows_through_all_limbs"] = sum(1 for v in vs if _borrows_through(v, P))
    counts["at_least_p"] = sum(1 for v in vs if v >= p)
    return vs, counts


def is_zero_cases(p, n_random, seed):
    """normalised values below 8 p -> (values, expected flags, counts)"""
    rnd = random.Random(seed)
    qinv = pow(p, -1, 1 << 29)
    cat = {"multiples": [k * p for k in range(8)],
           "off_by_one": [k * p + d for k in range(8) for d in (1, -1) if k * p + d >= 0],
           "same_low_limb": [k * p + (1 << (29 * j)) for k in range(8) for j in range(1, 9)],
           "filter_passers": [], "random": [rnd.randrange(8 * p) for _ in range(n_random)]}
    while len(cat["filter_passers"]) < 256:
        k = rnd.randrange(8)
        v = (rnd.randrange(8 * p) >> 29 << 29) | ((k * p) & M29)
        if v < 8 * p and v % p:
            cat["filter_passers"].append(v)
    vs = [v for c in cat.values() for v in c]
    counts = {k: len(c) for k, c in cat.items()}
    counts["pass_the_filter_not_zero"] = sum(1 for v in vs if (((v & M29) * qinv) & M29) < 8 and v % p)
    return vs, [int(v % p == 0) for v in vs], counts


SUB_BOUND_TENTHS = {"K2": 19, "K4": 39, "K6": 59, "K8": 79}    # subtrahend below 1.9 / 3.9 / 5.9 / 7.9 p (fq29_constants.h)


def sub_cases(p, kname, n_random, seed):
    """(a, b) normalised: a below 10 p, b below the bound documented beside K; no limb of a + K - b or K - b wraps"""
    rnd = random.Random(seed)
    K = f29_consts(p)[kname]
    top = SUB_BOUND_TENTHS[kname] * p // 10
    bs = [0, 1, p - 1, p, top - 1, val9([M29] * 8 + [((top - 1) >> 232) - 1])]
    bs += [rnd.randrange(top) for _ in range(n_random)]
    as_ = [0, 10 * p - 1, val9([M29] * 8 + [0]), p, 1, p - 1] + [rnd.randrange(10 * p) for _ in range(n_random)]
    for b in bs:
        assert all(x <= k for x, k in zip(limbs9(b), K)), "a limb of K - b would borrow"
    return list(zip(as_, bs)), {"edge": 6, "random": n_random}


# ================================================================================================================
# group law
def fq2_to_mont261(c):
    return tuple(x * R261 % Q for x in c)


class Group:
    """G1 or G2 with the table-entry / accumulator layouts of the probe"""

    def __init__(self, g2):
        self.g2 = g2
        self.C = G2 if g2 else G1
        self.gen = G2_GEN if g2 else G1_GEN
        self.walk_op, self.add_op, self.table_op = ("g2_walk", "g2_add", "g2_table") if g2 else ("g1_walk", "g1_add", "g1_table")
        self.ew, self.aw = WALK_WORDS[self.walk_op]
        self.nc = 2 if g2 else 1    # Fq components per coordinate

    def coords(self, P):
        """affine point -> flat list of its Fq components (x, y | x.c0, x.c1, y.c0, y.c1)"""
        return list(P[0]) + list(P[1]) if self.g2 else [P[0], P[1]]

    def entry_words(self, P, radix=R261):
        return words8([c * radix % Q for c in self.coords(P)]).reshape(-1)

    def affine_of(self, comps_inv, acc_vals):
        """acc_vals: the 4 nc component integers X | Y | ZZ | ZZZ; comps_inv: (ZZ^-1, ZZZ^-1) as field elements"""
        nc = self.nc
        X, Y = acc_vals[0:nc], acc_vals[nc:2 * nc]
        izz, izzz = comps_inv
        if self.g2:
            F = self.C.F
            return (F.mul(tuple(X), izz), F.mul(tuple(Y), izzz))
        return (X[0] * izz % Q, Y[0] * izzz % Q)


def batch_inverse(xs):
    """Fq inverses of non-zero residues with one modular inversion"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % Q
    inv = pow(acc, -1, Q)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % Q
        inv = inv * xs[i] % Q
    return out


def table_points(grp, seed):
    """48 multiples of the generator: 16 random scalars, the 16 sums of neighbours (so that a running sum can meet its
    next table point), 16 small ones -> (scalars, affine points)"""
    rnd = random.Random(seed)
    ks = [rnd.randrange(1, R) for _ in range(16)]
    ks += [(ks[i] + ks[(i + 1) % 16]) % R for i in range(16)]
    ks += list(range(1, 17))
    return ks, [grp.C.mul(grp.gen, k) for k in ks]


def walk_scripts(lanes, steps, seed):
    """per lane a list of `steps` (entry index or None, negate) -- scripted prefixes, random tails; odd lanes mirror the
    lane before them with every sign flipped (their sums are the negatives: operands for the add mode)"""
    rnd = random.Random(seed)
    scripts = []
    for lane in range(lanes):
        if lane & 1:
            scripts.append([(k, not n) if k is not None else (k, n) for k, n in scripts[-1]])
            continue
        i = rnd.randrange(16)
        s1, s2 = rnd.random() < 0.5, rnd.random() < 0.5
        kind = (lane // 2) % 8
        if kind == 0:
            pre = [(i, s1), (i, s1)]                                             # a point twice in a row, from infinity
        elif kind == 1:
            pre = [(i, s1), (i, not s1), (rnd.randrange(48), s2)]                # cancellation, then on from infinity
        elif kind == 2:
            pre = [(i, s1), ((i + 1) % 16, s1), (16 + i, s1)]                    # the sum meets its next point: doubling, ZZ != 1
        elif kind == 3:
            pre = [(i, s1), ((i + 1) % 16, s1), (16 + i, not s1), (rnd.randrange(48), s2)]   # ... cancellation, ZZ != 1
        elif kind == 4:
            j = rnd.randrange(48)
            pre = [(i, s1), (j, s2), (j, not s2), (i, s1)]                       # back to the first point after several steps
        elif kind == 5:
            pre = [(None, False), (32 + rnd.randrange(16), s1), (None, False), (32 + rnd.randrange(16), s2)]   # empty steps, small multiples
        elif kind == 6:
            pre = [(32, False), (32, False), (33, True), (33, False), (34, True)]   # G, 2G, 0 ... small multiples colliding
        else:
            pre = []
        tail = [(rnd.randrange(48), rnd.random() < 0.5) for _ in range(steps - len(pre))]
        scripts.append((pre + tail)[:steps])
    return scripts


def walk_input(grp, pts, scripts):
    steps = len(scripts[0])
    ent = [grp.entry_words(P) for P in pts]
    arr = np.zeros((len(scripts), steps, 1 + grp.ew), dtype=np.uint32)
    for l, sc in enumerate(scripts):
        for s, (k, neg) in enumerate(sc):
            if k is None:
                arr[l, s, 0] = 2
            else:
                arr[l, s, 0] = 1 if neg else 0
                arr[l, s, 1:] = ent[k]
    return arr.reshape(len(scripts), -1)


def walk_reference(grp, pts, scripts):
    """-> (per lane per step: affine sum or None, {category: count})"""
    C = grp.C
    counts = {"doubling": 0, "doubling_zz_not_one": 0, "cancellation": 0, "cancellation_zz_not_one": 0, "from_infinity": 0,
              "continues_from_infinity": 0, "negated": 0, "empty_step": 0, "generic": 0}
    out = []
    for sc in scripts:
        acc, hist, adds, adds_since_inf = None, [], 0, 0
        for k, neg in sc:
            if k is None:
                counts["empty_step"] += 1
                hist.append(acc)
                continue
            P = C.neg(pts[k]) if neg else pts[k]
            counts["negated"] += int(neg)
            if acc is None:
                counts["from_infinity"] += 1
                counts["continues_from_infinity"] += int(adds > 0)
                adds_since_inf = 0
            elif acc == P:
                counts["doubling"] += 1
                counts["doubling_zz_not_one"] += int(adds_since_inf > 0)
            elif acc == C.neg(P):
                counts["cancellation"] += 1
                counts["cancellation_zz_not_one"] += int(adds_since_inf > 0)
            else:
                counts["generic"] += 1
            if acc is not None:
                adds_since_inf += 1
            acc = C.add(acc, P)
            adds += 1
            hist.append(acc)
        out.append(hist)
    return out, counts


ACC_BOUND_TENTHS = (52, 21, 17, 17)   # fq29.h: X < 5.2 q, Y < 2.1 q, ZZ, ZZZ < 1.7 q per Fq component


def acc_check(grp, accs, want, what):
    """accs: (n, aw) uint32 raw accumulators, want: n affine points or None.  Normalised limbs, the documented bounds,
    infinity <=> ZZ all-zero limbs, and the affine point (X / ZZ, Y / ZZZ mod q) equals the reference."""
    accs = np.asarray(accs)
    nc, n = grp.nc, accs.shape[0]
    lim = accs.reshape(n, 4 * nc, 9)
    assert np.all(lim[:, :, :8] < (1 << 29)), "%s: accumulator limbs are not normalised" % what
    vals = vals9(accs)
    zz_zero = ~np.any(lim[:, 2 * nc:3 * nc, :].reshape(n, -1) != 0, axis=1)
    finite = [i for i in range(n) if not zz_zero[i]]
    worst = [0.0] * 4
    for i in range(n):
        assert bool(zz_zero[i]) == (want[i] is None), "%s: item %d: infinity flag %s but the reference is %s" % (
            what, i, bool(zz_zero[i]), want[i])
    for i in finite:
        for c in range(4):
            for v in vals[i][c * nc:(c + 1) * nc]:
                worst[c] = max(worst[c], v / Q)
                assert 10 * v < ACC_BOUND_TENTHS[c] * Q, "%s: item %d: component %d is %.4f q" % (what, i, c, v / Q)
    # ZZ^-1, ZZZ^-1: one inversion for all (Fq2: conj / norm)
    if grp.g2:
        norms = [(vals[i][2 * c] ** 2 + vals[i][2 * c + 1] ** 2) % Q for i in finite for c in (2, 3)]
        assert all(norms), "%s: a finite accumulator has ZZ or ZZZ = 0 mod q" % what
        ni = batch_inverse(norms)
        invs = [((vals[i][2 * c] * ni[2 * a + c - 2]) % Q, (-vals[i][2 * c + 1] * ni[2 * a + c - 2]) % Q)
                for a, i in enumerate(finite) for c in (2, 3)]
    else:
        zs = [vals[i][c] % Q for i in finite for c in (2, 3)]
        assert all(zs), "%s: a finite accumulator has ZZ or ZZZ = 0 mod q" % what
        invs = batch_inverse(zs)
    for a, i in enumerate(finite):
        got = grp.affine_of((invs[2 * a], invs[2 * a + 1]), vals[i])
        assert got == want[i], "%s: item %d: affine point differs from the reference" % (what, i)
    return worst


# ================================================================================================================
# witness operations
def witness_cases(n_random, seed):
    """-> (in (n, 17) uint32, expected (n, 9) uint32, {category: count}); operands and values are Fr in the 8 x 32
    Montgomery form, the expected value and error word come from oracle.pyref.wtns_graph.eval_duo"""
    rnd = random.Random(seed)
    half = wtns_graph.HALF_M
    fixed = [0, 1, 2, 3, 7, 253, 254, 255, 256, (1 << 32) + 3, 1 << 252, 1 << 253, half - 1, half, half + 1, R - 2, R - 1]
    rand = [rnd.randrange(R) for _ in range(n_random)]
    pairs = [(a, b) for a in fixed for b in fixed]
    pairs += [(rnd.choice(rand), rnd.choice(rand)) for _ in range(n_random)]
    pairs += [(rnd.choice(fixed), rnd.choice(rand)) for _ in range(200)] + [(rnd.choice(rand), rnd.choice(fixed)) for _ in range(200)]
    pairs += [(x, x) for x in rand[:50]]
    rows, counts = [], {"shift_error": 0, "bitop_error": 0, "or_is_exactly_r": 0, "shift_counts": 0, "id": 0}
    for k, name in enumerate(wtns_graph.DUO):
        ps = list(pairs)
        if name in ("Shl", "Shr"):
            ps += [(a, c) for a in (1, R - 1, rand[0]) for c in range(1, 254)]
            counts["shift_counts"] += 3 * 253
        for a, b in ps:
            try:
                v, e = wtns_graph.eval_duo(name, a, b), 0
            except ValueError as ex:
                v, e = 0, (WERR_SHIFT if "shift" in str(ex) else WERR_BITOP)
                counts["shift_error" if e == WERR_SHIFT else "bitop_error"] += 1
            if name == "Bor" and (a | b) == R:
                counts["or_is_exactly_r"] += 1
                assert e == WERR_BITOP
            rows.append((2 + k, a, b, v, e))
    for a in fixed[:4]:
        rows.append((G_ID, a, 0, 0, WERR_UNO_ID))
        counts["id"] += 1
    counts["tuples"] = len(rows)
    mont = words8([x * R256 % R for r in rows for x in r[1:4]]).reshape(len(rows), 24)
    inp = np.concatenate([np.array([[r[0]] for r in rows], dtype=np.uint32), mont[:, :16]], axis=1)
    exp = np.concatenate([mont[:, 16:], np.array([[r[4]] for r in rows], dtype=np.uint32)], axis=1)
    return inp, exp, counts


def witness_check(inp, exp, out):
    out = np.asarray(out)
    bad = np.nonzero(np.any(out != exp, axis=1))[0]
    if len(bad):
        i = int(bad[0])
        ri = pow(R256, -1, R)
        a, b = ints8(inp[i:i + 1, 1:])[0]
        raise AssertionError("%d of %d witness operations differ; first: op %d a = %d b = %d: got %s err %d, want %s err %d" % (
            len(bad), len(exp), int(inp[i, 0]), a * ri % R, b * ri % R, ints8(out[i:i + 1, :8])[0], int(out[i, 8]),
            ints8(exp[i:i + 1, :8])[0], int(exp[i, 8])))
