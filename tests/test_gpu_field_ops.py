"""Device field arithmetic against Python integers at edge operands, through the arithmetic probes of
include/rln_amd.h (csrc/arith_probe.hip): the device branches of field.h (inline-asm carry chains, the generated
product-scanning multiply), every primitive of fq29.h with its lane-form group laws, poseidon.h's five-term dot
product and witness_ops.h's witness_slow_op.  One launch per primitive, a few thousand operand tuples each; every
comparison is exact.  Operand sets, references and checkers: tests/field_ops_cases.py (run on the CPU by
tests/test_field_ops_host.py).  Each test prints the count of every edge category it sent and asserts it."""
import random

import numpy as np
import pytest

import field_ops_cases as fc
from zerokit_amd._native import RLNError, check, lib

pytestmark = pytest.mark.gpu

FIELDS = [pytest.param(0, id="Fr"), pytest.param(1, id="Fq")]


def probe_fp(field, op, ts):
    na, no = fc.FP_SHAPE[op]
    inp = np.ascontiguousarray(fc.tuples8(ts), dtype=np.uint32)
    out = np.zeros((len(ts), 8 * no), dtype=np.uint32)
    check(lib().rlnamd_probe_field(field, fc.FP_OPS.index(op), 8 * na, 8 * no, len(ts), inp.ctypes.data, out.ctypes.data))
    return out


def probe_f29(field, op, inp, steps=None):
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    if steps is None:
        wi, wo = fc.F29_SHAPE[op]
    else:
        ew, aw = fc.WALK_WORDS[op]
        wi, wo = steps * (1 + ew), steps * aw
    assert inp.ndim == 2 and inp.shape[1] == wi
    out = np.zeros((inp.shape[0], wo), dtype=np.uint32)
    check(lib().rlnamd_probe_f29(field, fc.F29_OPS.index(op), wi, wo, inp.shape[0], inp.ctypes.data, out.ctypes.data))
    return out


def limb_rows(vs):
    return np.array([fc.limbs9(v) for v in vs], dtype=np.uint32)


# ---- 8 x 32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_field_8x32_operations_at_edge_and_random_operands(field):
    """+, -, neg, dbl, *, sqr, dot2, dot3, dot4, dot2_sub, from_canonical, to_canonical over S x S (tuples drawn from S for
    the wider ones) plus 20 000 random tuples: the canonical residue, word for word"""
    p = fc.MODULUS[field]
    for k, op in enumerate(fc.FP_OPS[:12]):
        ts, counts = fc.fp_cases(op, p, 20000, 100 + k)
        print(fc.FIELD_NAME[field], op, counts)
        assert counts["random"] == 20000 and counts["edge"] >= 40 and counts["all_ones_operand"] >= 1
        if fc.FP_SHAPE[op][0] == 2:
            assert counts["edge"] >= 40 * 40
            assert counts["sum_is_p"] >= 5 and counts["sum_is_p_plus_1"] >= 5 and counts["sum_is_p_minus_1"] >= 5
        if fc.FP_SHAPE[op][0] > 2:
            assert counts["all_p_minus_1"] >= 1
        if op == "from_canonical":
            assert counts["non_reduced"] == 5
        fc.fp_check(op, p, ts, probe_fp(field, op, ts))


@pytest.mark.parametrize("field", FIELDS)
def test_field_8x32_inverse(field):
    """inv over S and 2 000 random values: 0 -> 0, otherwise Python's pow converted to the Montgomery form"""
    p = fc.MODULUS[field]
    ts, counts = fc.fp_cases("inv", p, 2000, 7)
    print(fc.FIELD_NAME[field], "inv", counts)
    assert (0,) in ts and (p - 1,) in ts and counts["edge"] >= 40 and counts["random"] == 2000 and len(ts) == counts["edge"] + 2000
    assert counts["all_ones_operand"] >= 1
    fc.fp_check("inv", p, ts, probe_fp(field, "inv", ts))


def test_fq2_product_square_inverse():
    rnd = random.Random(5)
    S, _ = fc.edge_values(fc.Q)
    for op, nr in (("fq2_mul", 20000), ("fq2_sqr", 20000), ("fq2_inv", 2000)):
        ts, counts = fc.fp_cases(op, fc.Q, nr, 11)
        if op == "fq2_mul":
            ts += [(a, b, c, d) for (a, b) in ((0, 1), (1, 0), (fc.Q - 1, fc.Q - 1), (0, 0)) for c in rnd.sample(S, 6) for d in rnd.sample(S, 6)]
            ts += [(0, 1, 0, 1), (1, 0, 1, 0), (0, 1, 1, 0)]
        else:
            ts += [(0, 0), (0, 1), (1, 0), (fc.Q - 1, fc.Q - 1)]
        print(op, counts)
        q1 = fc.Q - 1
        assert counts["random"] == nr and counts["edge"] >= 40 and counts["all_ones_operand"] >= 1
        if op == "fq2_mul":
            assert counts["all_p_minus_1"] >= 1 and (q1, q1, q1, q1) in ts and (0, 0, 0, 0) in ts and (0, 1, 0, 1) in ts
        else:
            assert counts["edge"] >= 40 * 40 and all(t in ts for t in ((0, 0), (0, 1), (1, 0), (q1, q1)))
        fc.fp_check(op, fc.Q, ts, probe_fp(1, op, ts))


# ---- 9 x 29 products ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_f29_products_at_the_class_maxima_of_every_call_site(field):
    """every row of tools/check_fq29_bounds.py's call-site table: all limbs at the class maximum (the replay's vectors),
    all zero, one limb at its maximum, 4 096 uniform tuples; limbs normalised and
    (val(v) - val(add)) 2^261 = sum val(a) val(b) + M p with 0 <= M < 2^261 + 2^236"""
    p = fc.MODULUS[field]
    rows = fc.site_rows(field)
    assert len(rows) >= 20
    seen = set()
    for k, (label, op, maxes, has_add, square) in enumerate(rows):
        inp, counts = fc.product_operands(maxes, 4096, 1000 * field + k)
        assert counts["class_maximum"] == 1 and counts["zero"] == 1 and counts["single_limb"] == 9 * len(maxes)
        assert inp.shape[0] == 2 + 9 * len(maxes) + 4096 and list(inp[0]) == [m for o in maxes for m in o]
        out = probe_f29(field, op, inp)
        worst = fc.product_check(label, p, inp, out, has_add, square)
        print("%s %-70s %-9s worst M / 2^261 = %.5f" % (fc.FIELD_NAME[field], label, op, worst))
        seen.add(op)
    want = {"mul", "mul_add", "sqr", "sqr_add", "dot2", "dot2_add", "dot3", "dot3_wide", "dot4", "dot4_wide"}
    assert seen >= want | ({"dotn5"} if field == 0 else set())


# ---- 9 x 29 exact-value primitives ---------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_f29_slice_pack_and_conversions(field):
    p = fc.MODULUS[field]
    xs, counts = fc.slice_cases(p, 4096, 21)
    print("slice", counts)
    assert counts["all_ones_word"] == 1
    want = limb_rows(xs)
    for op in ("slice",) + (("unpack29",) if field == 1 else ()):
        assert np.array_equal(probe_f29(field, op, fc.words8(xs)), want), op

    vs, counts = fc.pack_cases(p, 4096, 22)
    print("pack_reduced", counts)
    assert counts["named"] == 6 and counts["p_pm_limb"] == 18 and counts["borrows_through_all_limbs"] >= 33
    assert counts["at_least_p"] >= 1000 and counts["random"] == 4096
    want = fc.words8([v % p for v in vs])
    for op in ("pack_reduced",) + (("pack29_reduced",) if field == 1 else ()):
        assert np.array_equal(probe_f29(field, op, limb_rows(vs)), want), op

    # from_fq: x 2^256 -> x 2^261 (a product with a constant: the identity of the product rows), and back exactly
    S, _ = fc.edge_values(p)
    rnd = random.Random(23)
    xs = S + [rnd.randrange(p) for _ in range(2000)]
    c = fc.f29_consts(p)
    f29 = probe_f29(field, "from_fq", fc.words8(xs))
    fc.product_check("from_fq", p, np.concatenate([limb_rows(xs), np.tile(np.array(c["FROM_FQ"], dtype=np.uint32), (len(xs), 1))], axis=1),
                     f29, False, False)
    assert np.array_equal(probe_f29(field, "to_fq", f29), fc.words8(xs)), "to_fq(from_fq(x)) != x"
    # to_fq of any normalised value below 10 p: val / 32 mod p
    vs = [0, 1, p, 10 * p - 1, fc.val9([fc.M29] * 8 + [(10 * p) >> 232])] + [rnd.randrange(10 * p) for _ in range(2000)]
    i32 = pow(32, -1, p)
    assert np.array_equal(probe_f29(field, "to_fq", limb_rows(vs)), fc.words8([v * i32 % p for v in vs]))
    # mul_mont(a, w29) = the 8 x 32 product a w
    pairs = [(a, w) for a in S for w in (0, 1, p - 1, (p + 1) // 2)] + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(4096)]
    inp = np.concatenate([fc.words8([a for a, _ in pairs]), limb_rows([w * fc.R261 % p for _, w in pairs])], axis=1)
    assert np.array_equal(probe_f29(field, "mul_mont", inp), fc.words8([a * w % p for a, w in pairs]))
    # the witness interpreters' input conversion: any 256-bit word x -> x 2^261 mod p
    xs = S + [p, 2 * p, fc.R256 - 1] + [rnd.getrandbits(256) for _ in range(2000)]
    out = probe_f29(field, "from_canonical", fc.words8(xs))
    fc.product_check("from_canonical", p, np.concatenate([limb_rows(xs), np.tile(np.array(c["FROM_CANON"], dtype=np.uint32), (len(xs), 1))], axis=1),
                     out, False, False)
    assert all((v[0] - x * fc.R261) % p == 0 for v, x in zip(fc.vals9(out), xs))


@pytest.mark.parametrize("field", FIELDS)
def test_f29_exact_zero_test(field):
    p = fc.MODULUS[field]
    vs, want, counts = fc.is_zero_cases(p, 4096, 31)
    print("is_zero_mod_q", counts)
    assert counts["multiples"] == 8 and counts["off_by_one"] == 15 and counts["same_low_limb"] == 64
    assert counts["pass_the_filter_not_zero"] >= 256 + 64 and counts["random"] == 4096
    got = probe_f29(field, "is_zero", limb_rows(vs))[:, 0].tolist()
    bad = [(hex(v), g, w) for v, g, w in zip(vs, got, want) if g != w]
    assert not bad, bad[:3]


@pytest.mark.parametrize("field", FIELDS)
def test_f29_borrow_free_differences_and_normalize(field):
    """sub(a, K, b), neg_lazy(K, b) for K2 .. K8 with b up to the bound documented beside K, and normalize: the plain
    integer a + K - b, no limb wrapping"""
    p = fc.MODULUS[field]
    c = fc.f29_consts(p)
    for kname in ("K2", "K4", "K6", "K8"):
        pairs, counts = fc.sub_cases(p, kname, 4096, 40 + int(kname[1]))
        K = c[kname]
        la, lb = limb_rows([a for a, _ in pairs]), limb_rows([b for _, b in pairs])
        out = probe_f29(field, "sub_" + kname.lower(), np.concatenate([la, lb], axis=1))
        assert np.all(out[:, :8] < (1 << 29)), kname
        assert [v[0] for v in fc.vals9(out)] == [a + fc.val9(K) - b for a, b in pairs], kname
        out = probe_f29(field, "neg_" + kname.lower(), lb)
        assert np.array_equal(out.astype(np.int64), np.array(K, dtype=np.int64)[None, :] - lb.astype(np.int64)), kname
    rng = np.random.default_rng(45)
    lazy = np.concatenate([np.array([c["K4T"], [(1 << 31) - 1] * 9, [0] * 9, [fc.M29] * 9, [1 << 29] * 9], dtype=np.uint32),
                           rng.integers(0, 1 << 31, size=(4096, 9), dtype=np.uint64).astype(np.uint32)])
    out = probe_f29(field, "normalize", lazy)
    assert np.all(out[:, :8] < (1 << 29)) and fc.vals9(out) == fc.vals9(lazy)


# ---- group law, lane forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("g2", [pytest.param(False, id="G1"), pytest.param(True, id="G2")])
def test_group_law_walks_and_additions_against_python(g2):
    """1 024 lanes x 16 madd steps from infinity over table entries built in Python (x 2^261 mod q of multiples of the
    generator): after every step normalised limbs, the accumulator bounds of fq29.h (X < 5.2 q, Y < 2.1 q, ZZ, ZZZ < 1.7 q),
    infinity <=> ZZ all-zero limbs, and the affine point equals the Python running sum; then add() over pairs of the
    recorded accumulators; to_table29 of the 8 x 32 points equals the Python entries"""
    grp = fc.Group(g2)
    ks, pts = fc.table_points(grp, 60 + g2)
    mont = np.stack([grp.entry_words(P, fc.R256) for P in pts])
    assert np.array_equal(probe_f29(1, grp.table_op, mont), np.stack([grp.entry_words(P) for P in pts])), "to_table29"

    lanes, steps = 1024, 16
    scripts = fc.walk_scripts(lanes, steps, 70 + g2)
    ref, counts = fc.walk_reference(grp, pts, scripts)
    print("walk", counts)
    for cat in ("doubling", "doubling_zz_not_one", "cancellation", "cancellation_zz_not_one", "continues_from_infinity",
                "negated", "empty_step", "generic"):
        assert counts[cat] >= 32, cat
    out = probe_f29(1, grp.walk_op, fc.walk_input(grp, pts, scripts), steps=steps).reshape(lanes, steps, grp.aw)
    worst = fc.acc_check(grp, out.reshape(-1, grp.aw), [P for lane in ref for P in lane], "madd walk")
    print("walk: largest X, Y, ZZ, ZZZ component / q:", ["%.3f" % w for w in worst])

    # add(): pairs of recorded accumulators
    rnd = random.Random(80 + g2)
    by_point = {}
    for l in range(lanes):
        for s in range(steps):
            by_point.setdefault(ref[l][s], []).append((l, s))
    pairs, cats = [], {"generic": 0, "same_accumulator": 0, "same_point_other_form": 0, "negative": 0, "left_infinity": 0,
                       "right_infinity": 0, "both_infinity": 0}

    def push(a, b, cat):
        pairs.append((a, b))
        cats[cat] += 1
    for _ in range(600):
        a, b = (rnd.randrange(lanes), rnd.randrange(steps)), (rnd.randrange(lanes), rnd.randrange(steps))
        Pa, Pb = ref[a[0]][a[1]], ref[b[0]][b[1]]
        if Pa is not None and Pb is not None and Pa[0] != Pb[0]:
            push(a, b, "generic")
    for l in range(0, lanes, 2):
        s = rnd.randrange(steps)
        if ref[l][s] is None:
            continue
        if l % 8 == 0:
            push((l, s), (l, s), "same_accumulator")
        else:
            push((l, s), (l + 1, s), "negative")       # the mirrored lane holds the negative of this sum
    infs = by_point.get(None, [])
    for P, where in by_point.items():
        if P is None:
            continue
        forms = {out[l, s].tobytes(): (l, s) for l, s in where}
        if len(forms) >= 2 and cats["same_point_other_form"] < 64:
            a, b = list(forms.values())[:2]
            push(a, b, "same_point_other_form")
    for k in range(32):
        fin = (rnd.randrange(lanes), steps - 1)
        if ref[fin[0]][fin[1]] is None:
            continue
        push(infs[k % len(infs)], fin, "left_infinity")
        push(fin, infs[(k + 1) % len(infs)], "right_infinity")
    push(infs[0], infs[-1], "both_infinity")
    print("add", cats)
    assert all(v >= 1 for v in cats.values()) and cats["generic"] >= 500 and cats["same_point_other_form"] >= 16
    inp = np.stack([np.concatenate([out[a], out[b]]) for a, b in pairs])
    want = [grp.C.add(ref[a[0]][a[1]], ref[b[0]][b[1]]) for a, b in pairs]
    worst = fc.acc_check(grp, probe_f29(1, grp.add_op, inp), want, "add")
    print("add: largest X, Y, ZZ, ZZZ component / q:", ["%.3f" % w for w in worst])


# ---- witness operations -------------------------------------------------------------------------------------------
def test_witness_operations_against_eval_duo():
    """all twenty binary graph operations and G_ID: value and error word of the device against
    oracle.pyref.wtns_graph.eval_duo (an error there: value 0 and WERR_SHIFT / WERR_BITOP)"""
    inp, exp, counts = fc.witness_cases(2000, 90)
    print("witness", counts)
    assert counts["shift_error"] >= 100 and counts["bitop_error"] >= 1 and counts["or_is_exactly_r"] >= 1
    assert counts["shift_counts"] == 2 * 3 * 253 and counts["id"] >= 1
    out = np.zeros(exp.shape, dtype=np.uint32)
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    check(lib().rlnamd_probe_witness_op(inp.shape[0], inp.ctypes.data, out.ctypes.data))
    fc.witness_check(inp, exp, out)


def test_probe_argument_checks():
    """n = 0 is OK without a launch; word counts that are not the operation's own, unknown operations and operations a
    field does not have are errors, not launches"""
    src, dst = np.zeros(33 * 72, dtype=np.uint32), np.zeros(33 * 72, dtype=np.uint32)   # room for the largest rejected shape
    L = lib()
    assert L.rlnamd_probe_field(0, 0, 16, 8, 0, None, None) == 0
    assert L.rlnamd_probe_f29(1, 0, 18, 9, 0, None, None) == 0
    assert L.rlnamd_probe_witness_op(0, None, None) == 0
    for rc in (L.rlnamd_probe_field(0, 0, 8, 8, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_field(0, fc.FP_OPS.index("fq2_mul"), 32, 16, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_field(2, 0, 16, 8, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_field(0, len(fc.FP_OPS), 16, 8, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_f29(1, 0, 18, 8, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_f29(0, fc.F29_OPS.index("g1_walk"), 17, 36, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_f29(1, fc.F29_OPS.index("g1_walk"), 33 * 17, 33 * 36, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_f29(1, fc.F29_OPS.index("dotn5"), 90, 9, 1, src.ctypes.data, dst.ctypes.data),
               L.rlnamd_probe_f29(1, len(fc.F29_OPS), 18, 9, 1, src.ctypes.data, dst.ctypes.data)):
        with pytest.raises(RLNError):
            check(rc)
