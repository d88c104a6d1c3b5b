"""tests/witness_edge_cases.py checked on the CPU: the scalars it builds from chosen halves split, in the CPU build of
glv_split (glv.h through tests/host/hostmath.cpp), into exactly those halves and signs; a plain restatement of emit_digits
re-sums every half with every digit in [-2^(c-1), 2^(c-1)]; the ties it promises occur; and the 129 witnesses of a circuit
hold every category.  The device runs the same witnesses in tests/test_gpu_adversarial_witness.py."""
import ctypes
import os
import re
import subprocess

import pytest

import witness_edge_cases as wec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = wec.R


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "tests", "host", "libhostmath.so")
    src = os.path.join(ROOT, "tests", "host", "hostmath.cpp")
    hdrs = [os.path.join(ROOT, "zerokit_amd", "csrc", h) for h in ("field.h", "curve.h", "pairing.h", "glv.h",
                                                                     "glv_constants.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "zerokit_amd", "csrc"), src, "-o", so])
    return ctypes.CDLL(so)


def _split(L, k):
    out = ctypes.create_string_buffer(34)
    L.hm_glv_split(k.to_bytes(32, "little"), out)
    return (int.from_bytes(out.raw[:16], "little"), out.raw[16], int.from_bytes(out.raw[17:33], "little"), out.raw[33])


def test_default_schedules_are_the_provers():
    txt = open(os.path.join(ROOT, "zerokit_amd", "csrc", "prover.h")).read()
    assert str(wec.DEFAULT_WINDOW_BITS) in re.findall(r"int window_bits = (\d+);", txt)      # ProverTuning's default
    cw1, cw2 = wec.schedules(wec.DEFAULT_WINDOW_BITS)
    assert cw1 == [10] * 13 and cw2 == [12] * 11
    assert wec.schedules(109) == ([10] + [9] * 13, [10] + [9] * 13)           # c = 9, the first window one bit wider
    assert wec.schedules(80108) == ([9] + [8] * 15, [8] * 16)
    assert all(sum(cw) >= wec.HALF_BITS for cw in (cw1, cw2))


@pytest.mark.parametrize("window_bits", [wec.DEFAULT_WINDOW_BITS, 80108, 160016])
def test_special_scalars_split_into_their_halves_and_recode(L, window_bits):
    """glv_split's CPU build returns the halves and signs each scalar was made from (also for the plain field values,
    against the model), and emit_digits re-sums to the half on both schedules with every digit in range"""
    cw1, cw2 = wec.schedules(window_bits)
    S = wec.special_scalars(cw1, cw2)
    assert len(S) == 2 + 8 + 10 + 2
    for name, k1, n1, k2, n2 in S:
        k = wec.scalar_of(k1, n1, k2, n2)
        assert 0 < k < R
        assert _split(L, k) == (k1, n1, k2, n2), name
    for _, v in wec.PLAIN + [("zero", 0), ("two", 2)]:
        got = _split(L, v)
        assert got == wec.glv_model(v) and wec.scalar_of(*got) == v
    assert _split(L, 0) == (0, 0, 0, 0) and _split(L, 1) == (1, 0, 0, 0) and _split(L, wec.LAMBDA) == (0, 0, 1, 0)
    assert _split(L, R - 1) == (1, 1, 0, 0)
    big = max(max(k1, k2) for n, k1, _, k2, _ in S if n == "max_halves")
    assert (1 << 125) < big < (1 << 126)
    assert all(wec._corner(a, b)[2] <= 1 << 100 for a in (0, 1) for b in (0, 1))   # within 2^-25 of the corner's halves
    ties = {}
    for cw, tag in ((cw1, "g1"), (cw2, "g2")):
        for name, k1, n1, k2, n2 in S:
            for half, neg in ((k1, n1), (k2, n2)):
                d, t = wec.emit_digits(half, neg, cw)
                assert wec.resum(d, cw) == (-half if neg else half), (name, tag)
                assert all(-(1 << (c - 1)) <= x <= (1 << (c - 1)) for x, c in zip(d, cw)), (name, tag)
                if c16 := [x for x, c in zip(d, cw) if c == 16]:
                    assert all(-32768 <= x <= 32767 for x in c16), (name, tag)      # the tie goes where an int16 holds it
                ties[(tag, name, neg)] = t
        # the tie witnesses tie in every window they fill, the ripple carries to the top
        full = sum(1 for j in range(len(cw)) if sum(cw[:j + 1]) <= 125)
        assert ties[(tag, "tie_pos_" + tag, 0)] >= full - 1 and ties[(tag, "tie_neg_" + tag, 1)] >= full - 1
        d, _ = wec.emit_digits((1 << 125) - 1, 0, cw)
        assert d[0] == -1 and all(x == 0 for x in d[1:-1]) and d[-1] > 0


def test_the_129_witnesses_hold_every_category():
    from oracle.c import binding as ob
    from zerokit_amd import workload
    c = ob.Circuit(10)
    named, rs = workload.circuit_range(2000, 8, 10, False)
    honest = [c.witness_packed(c.pack_named(w)) for w in named]
    W, RS, LB, counts = wec.build(c.n_signals, c.n_public, wec.DEFAULT_WINDOW_BITS, honest, rs)
    print(counts)
    wec.check_counts(counts)
    assert len(W) == len(RS) == len(LB) == 129 and all(len(w) == c.n_signals for w in W)
    assert all(0 <= v < 1 << 256 for w in W for v in w)
    assert W[0] == [0] * c.n_signals and RS[0] == (0, 0) and RS[1][0] and RS[1][1]
    assert sum(1 for w in W if any(v >= R for v in w)) == 2
    one = [w for w, lb in zip(W, LB) if lb.startswith("single_at")]
    assert [[i for i, v in enumerate(w) if v] for w in one] == [[1], [c.n_public], [c.n_public + 1], [c.n_signals - 1]]
    assert {w[0] for w, lb in zip(W, LB) if lb.startswith("w0_")} == {0, 2, R - 1}
    assert len(wec.edge_indices(LB)) == 129 - counts["honest"] - counts["mosaic"]
    assert len({tuple(w) for w in W}) == 129 - counts["honest"] + 8 - 1       # (the all-zero witness is there twice)
