"""The Python side of tests/test_gpu_field_ops.py on the CPU: its operand generators and checkers (tests/field_ops_cases.py)
run on a pure-Python model of fq29.h's redc_dot / sqr_add / finish, and its witness-operation table run on the host
build of witness_ops.h.  This verifies the reference and its input sets without a GPU, and separates a failure of the
device code alone from an error in the logic both builds share."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import field_ops_cases as fc

ROOT = fc.ROOT
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")


def limb_rows(vs):
    return np.array([fc.limbs9(v) for v in vs], dtype=np.uint32)


@pytest.mark.parametrize("field", [0, 1])
def test_edge_operand_set_of_the_8x32_field(field):
    """S holds about 40 values below p with every category the GPU test relies on; the references of the single
    operations agree with each other where they must"""
    p = fc.MODULUS[field]
    S, cat = fc.edge_values(p)
    assert 40 <= len(S) <= 60 and len(set(S)) == len(S)
    ones = cat["all_ones"][0]
    assert ones < p and all((ones >> (32 * w)) & 0xFFFFFFFF == 0xFFFFFFFF for w in range(7)) and (ones >> 224) == (p >> 224) - 1
    assert len(set(cat["one_word_cleared"])) == 8
    assert all((1 << (32 * k)) + d in S for k in range(1, 8) for d in (-1, 0, 1))
    ts, counts = fc.fp_cases("add", p, 10, 1)
    assert counts["sum_is_p"] >= 5 and counts["sum_is_p_plus_1"] >= 5 and counts["sum_is_p_minus_1"] >= 5
    ts, counts = fc.fp_cases("dot4", p, 10, 1)
    assert counts["all_p_minus_1"] >= 1
    # dot4 with every operand p - 1 is 4 (p - 1)^2 / 2^256 + (a multiple of p below 2^256 p) / 2^256 < 2 p before the subtraction
    assert 4 * (p - 1) ** 2 + (fc.R256 - 1) * p < 2 * p * fc.R256
    rnd = random.Random(2)
    for _ in range(50):
        a, b, c, d = (rnd.randrange(p) for _ in range(4))
        mul = lambda x, y: fc.fp_expected("mul", p, (x, y))[0]
        assert fc.fp_expected("dot2", p, (a, b, c, d))[0] == (mul(a, b) + mul(c, d)) % p
        assert fc.fp_expected("dot2_sub", p, (a, b, c, d))[0] == (mul(a, b) - mul(c, d)) % p
        assert mul(a, fc.fp_expected("inv", p, (a,))[0]) == fc.R256 % p                      # x inv(x) = 1 in Montgomery form
        assert fc.fp_expected("to_canonical", p, fc.fp_expected("from_canonical", p, (a,)))[0] == a
    for x in (p, p + 1, 2 * p, 5 * p - 1, fc.R256 - 1):      # x R^2 / 2^256 + m p / 2^256 < 2 p: one subtraction suffices
        assert x * (fc.R256 * fc.R256 % p) + (fc.R256 - 1) * p < 2 * p * fc.R256


@pytest.mark.parametrize("field", [0, 1])
def test_product_identity_on_a_python_model_of_redc_dot(field):
    """every row the GPU test sends (class maxima, zero, single limbs, random) through a Python model of the device
    algorithm with wrapping 64-bit columns: normalised limbs and (val(v) - val(add)) 2^261 = sum a b + M p, M below
    2^261 + 2^236"""
    p = fc.MODULUS[field]
    model = fc.Model29(p)
    worst = 0.0
    for k, (label, op, maxes, has_add, square) in enumerate(fc.site_rows(field)):
        inp, counts = fc.product_operands(maxes, 24, 1000 * field + k)
        assert counts["single_limb"] == 9 * len(maxes)
        out = np.array([model.run(op, row) for row in inp.tolist()], dtype=np.uint32)
        worst = max(worst, fc.product_check(label, p, inp, out, has_add, square))
    assert 0.9 < worst < 1 + 2.0 ** -25
    # the checker is not vacuous: one unit in one limb of one result fails it
    label, op, maxes, has_add, square = fc.site_rows(field)[0]
    inp, _ = fc.product_operands(maxes, 4, 5)
    out = np.array([model.run(op, row) for row in inp.tolist()], dtype=np.uint32)
    out[3, 2] ^= 1
    with pytest.raises(AssertionError):
        fc.product_check(label, p, inp, out, has_add, square)


@pytest.mark.parametrize("field", [0, 1])
def test_exact_value_input_sets(field):
    p = fc.MODULUS[field]
    c = fc.f29_consts(p)
    hdr = open(os.path.join(CSRC, "fq29_constants.h")).read()
    for name in ("K2", "K4", "K6", "K8", "K4T", "FROM_CANON", "FROM_FQ", "TO_FQ"):     # the reference's constants are the header's
        assert ("%s[9] = {" % name + ", ".join("0x%08xu" % l for l in c[name]) + "}") in hdr, name
    assert "QINV = 0x%08xu" % c["QINV"] in hdr
    vs, counts = fc.pack_cases(p, 64, 1)
    assert counts["borrows_through_all_limbs"] >= 33 and all(v < 2 * p for v in vs)
    vs, want, counts = fc.is_zero_cases(p, 64, 1)
    assert sum(want) == 8 and counts["pass_the_filter_not_zero"] >= 256 and all(v < 8 * p for v in vs)
    for kname in ("K2", "K4", "K6", "K8"):
        pairs, _ = fc.sub_cases(p, kname, 64, 3)
        assert fc.val9(c[kname]) == int(kname[1]) * p
        for a, b in pairs:
            d = [x + k - y for x, k, y in zip(fc.limbs9(a), c[kname], fc.limbs9(b))]
            assert min(d) >= 0 and max(d) < 1 << 32


@pytest.mark.parametrize("g2", [False, True])
def test_walk_scripts_hold_every_case(g2):
    grp = fc.Group(g2)
    ks, pts = fc.table_points(grp, 60 + g2)
    assert all(grp.C.on_curve(P) for P in pts) and len(set(pts)) == 48
    scripts = fc.walk_scripts(64 if g2 else 256, 16, 70 + g2)
    ref, counts = fc.walk_reference(grp, pts, scripts)
    assert all(len(s) == 16 for s in scripts)
    for cat in ("doubling", "doubling_zz_not_one", "cancellation", "cancellation_zz_not_one", "continues_from_infinity",
                "negated", "empty_step", "generic"):
        assert counts[cat] >= 2, cat
    # the running sums are what the scalars say
    l = 2
    total = 0
    for k, neg in scripts[l]:
        if k is not None:
            total += -ks[k] if neg else ks[k]
    assert ref[l][-1] == (grp.C.mul(grp.gen, total % fc.R) if total % fc.R else None)
    assert fc.walk_input(grp, pts, scripts).shape == (len(scripts), 16 * (1 + grp.ew))


class G1Model:
    """G1Acc29::madd / dbl_affine of fq29.h on limb lists, products by fc.Model29; None is infinity"""

    def __init__(self):
        self.m, self.c = fc.Model29(fc.Q), fc.f29_consts(fc.Q)
        self.one = fc.limbs9(fc.R261 % fc.Q)

    @staticmethod
    def norm(v):
        v = list(v)
        for j in range(8):
            v[j + 1] = (v[j + 1] + (v[j] >> 29)) & 0xFFFFFFFF
            v[j] &= fc.M29
        return v

    @staticmethod
    def lazy(f):
        v = [f(j) for j in range(9)]
        assert all(0 <= x < 1 << 32 for x in v), "a limb wraps"
        return v

    def zero_mod_q(self, v):
        return fc.val9(v) in [k * fc.Q for k in range(8)]

    def dbl(self, x, py):
        m, c = self.m, self.c
        U = self.lazy(lambda j: 2 * py[j])
        V = m.sqr(U)
        W, S, x2 = m.dot([(U, V)], True), m.dot([(x, V)], True), m.sqr(x)
        Mm = self.norm(self.lazy(lambda j: 3 * x2[j]))
        M2 = m.sqr(Mm)
        X3 = self.norm(self.lazy(lambda j: M2[j] + c["K4T"][j] - 2 * S[j]))
        D = self.norm(self.lazy(lambda j: S[j] + c["K6"][j] - X3[j]))
        nY = self.lazy(lambda j: c["K4"][j] - py[j])
        return [X3, m.dot([(Mm, D), (nY, W)], True), V, W]

    def madd(self, acc, x, y, negate):
        m, c = self.m, self.c
        px, py = fc.limbs9(x), fc.limbs9(y)
        if negate:
            py = self.lazy(lambda j: c["K2"][j] - py[j])
        if acc is None:
            return [px, self.norm(py), self.one, self.one]
        X, Y, ZZ, ZZZ = acc
        kX, nY = self.lazy(lambda j: c["K6"][j] - X[j]), self.lazy(lambda j: c["K4"][j] - Y[j])
        P, Rr = m.dot([(px, ZZ)], True, kX), m.dot([(py, ZZZ)], True, nY)
        if self.zero_mod_q(P):
            return self.dbl(px, self.norm(py)) if self.zero_mod_q(Rr) else None
        PP = m.sqr(P)
        ZZ3, Qv, PPP = m.dot([(ZZ, PP)], True), m.dot([(X, PP)], True), m.dot([(P, PP)], True)
        ZZZ3 = m.dot([(ZZZ, PPP)], True)
        kT = self.lazy(lambda j: c["K4T"][j] - (PPP[j] + 2 * Qv[j]))
        X3 = m.sqr(Rr, kT)
        D = self.lazy(lambda j: Qv[j] + c["K6"][j] - X3[j])
        return [X3, m.dot([(Rr, D), (nY, PPP)], True), ZZ3, ZZZ3]


def test_g1_walk_checker_on_a_python_model_of_madd():
    """the walk inputs, the reference sums and the accumulator checker (normalised limbs, X < 5.2 q, Y < 2.1 q, ZZ, ZZZ
    < 1.7 q, infinity <=> ZZ = 0, affine point) on a limb-exact Python model of G1Acc29::madd: doubling, cancellation and
    restarts included; a wrong bias constant in the model is caught"""
    grp = fc.Group(False)
    ks, pts = fc.table_points(grp, 60)
    scripts = fc.walk_scripts(32, 16, 70)
    ref, counts = fc.walk_reference(grp, pts, scripts)
    assert counts["doubling_zz_not_one"] >= 1 and counts["cancellation_zz_not_one"] >= 1
    ent = [[c * fc.R261 % fc.Q for c in grp.coords(P)] for P in pts]
    model = G1Model()

    def walk(mdl):
        accs = []
        for sc in scripts:
            acc = None
            for k, neg in sc:
                if k is not None:
                    acc = mdl.madd(acc, ent[k][0], ent[k][1], neg)
                accs.append([0] * 36 if acc is None else [l for comp in acc for l in comp])
        return np.array(accs, dtype=np.uint32)
    want = [P for lane in ref for P in lane]
    worst = fc.acc_check(grp, walk(model), want, "model walk")
    assert worst[0] < 5.2 and worst[1] < 2.1 and worst[2] < 1.7 and worst[3] < 1.7
    bad = G1Model()
    bad.c = dict(bad.c, K6=bad.c["K4"])     # K4 where madd needs K6: a limb wraps or the sum is wrong
    with pytest.raises(AssertionError):
        fc.acc_check(grp, walk(bad), want, "model walk, wrong bias")


@pytest.fixture(scope="module")
def WO():
    so = os.path.join(ROOT, "tests", "host", "libwitnessops.so")
    src = os.path.join(ROOT, "tests", "host", "witnessops.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("witness_ops.h", "field.h", "curve.h", "zkey.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    return ctypes.CDLL(so)


def test_witness_operations_of_the_host_build_against_eval_duo(WO):
    """witness_slow_op as the CPU compiles it, on the operand table of the GPU test"""
    inp, exp, counts = fc.witness_cases(2000, 90)
    assert counts["shift_error"] >= 100 and counts["bitop_error"] >= 1 and counts["or_is_exactly_r"] >= 1
    assert counts["shift_counts"] == 2 * 3 * 253 and counts["id"] >= 1 and counts["tuples"] > 20 * 2000
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    out = np.zeros(exp.shape, dtype=np.uint32)
    WO.wo_probe(ctypes.c_size_t(inp.shape[0]), ctypes.c_void_p(inp.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    fc.witness_check(inp, exp, out)
    out[5, 0] ^= 1
    with pytest.raises(AssertionError):
        fc.witness_check(inp, exp, out)
