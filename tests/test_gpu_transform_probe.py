"""The quotient's transforms on the device at EVERY domain size, on inputs no honest witness produces.

rlnamd_probe_quotient_transform runs inverse transform, coset scaling and forward transform through
launch_quotient_transform (prover.hip) -- the function Prover::enqueue launches them with -- over caller-supplied vectors:
  * the passes (k_ntt_pass / k_ntt_turn by ntt_pass_list) for logn 1 .. 14: every turn width with passes on both sides and
    alone (the shipped circuits reach two or three values of logn);
  * the LDS kernels (k_ntt_edge / k_ntt_mid) for logn 9 .. 14 and 18: E = logn - 9 = 0 (k_ntt_mid alone) .. 5 and the
    extreme E = 9, where a workgroup's 512 points are 512 apart (cl = 1).
The kernels leave out the products by tw[0] and rely on every intermediate being canonical: the inputs are all 0, all
r - 1, all 1, a single r - 1 (at 0, 1, n / 2 = bit-reversed 1, n - 1), alternating 0 / r - 1, the evaluations of
1 + X^(n-1), and random vectors; adjacent lanes hold different ones, so a lane mix-up shows.  nb = 1, 64, 65 of B = 128
lanes, three vectors.  Reference: oracle.pyref.groth16 in Python integers (ntt(inverse), x g^i, ntt), computed once per
logn; for logn 18 oracle/c's oracle_coset_transform (pinned to pyref for logn 1 .. 12 in tests/test_oracle_c.py), one
lane and one vector.  Exact equality."""
import ctypes as C
import random
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B = 128
NBS = (1, 64, 65)
VECTORS = 3


def _kinds(logn, rnd):
    from oracle.pyref import groth16
    n = 1 << logn
    w = groth16.root_of_unity(n)
    out = [[0] * n, [R - 1] * n, [1] * n]
    for pos in sorted({0, 1, n // 2, n - 1}):
        v = [0] * n
        v[pos] = R - 1
        out.append(v)
    out.append([0 if i % 2 == 0 else R - 1 for i in range(n)])
    wi, x, ev = pow(w, -1, R), 1, []
    for i in range(n):                     # 1 + X^(n-1) at w^i: X^(n-1) = X^-1 on the domain
        ev.append((1 + x) % R)
        x = x * wi % R
    out.append(ev)
    out += [[rnd.randrange(R) for _ in range(n)] for _ in range(2)]
    return out


def _coset_transform_pyref(v):
    from oracle.pyref import groth16
    n = len(v)
    g = groth16.root_of_unity(2 * n)
    t = groth16.ntt(v, inverse=True)
    p = 1
    for i in range(n):
        t[i] = t[i] * p % R
        p = p * g % R
    return groth16.ntt(t)


def _rows(v):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), dtype=np.uint8).reshape(len(v), 32)


_REF = {}
_REF_SECONDS = [0.0]


def _ref(logn):
    """(inputs, expected) per kind as (n, 32) byte rows, once per logn"""
    if logn not in _REF:
        t0 = time.perf_counter()
        kinds = _kinds(logn, random.Random(1000 + logn))
        _REF[logn] = ([_rows(v) for v in kinds], [_rows(_coset_transform_pyref(v)) for v in kinds])
        _REF_SECONDS[0] += time.perf_counter() - t0
    return _REF[logn]


def _lanes(rows, logn, nb):
    """[vector][index][lane]: lane p of vector v holds kind (p + 4 v + logn) mod K -- neighbours differ"""
    K = len(rows)
    a = np.empty((VECTORS, 1 << logn, nb, 32), dtype=np.uint8)
    for v in range(VECTORS):
        for p in range(nb):
            a[v, :, p, :] = rows[(p + 4 * v + logn) % K]
    return a


def _probe(logn, lds, b, nb, vectors, arr):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    src = np.ascontiguousarray(arr)
    out = np.empty_like(src)
    check(lib().rlnamd_probe_quotient_transform(logn, lds, b, nb, vectors, src.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p)))
    return out


def _where(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return "first differences at (vector, index, lane): %s of %d" % (bad[:6].tolist(), len(bad))


@pytest.mark.parametrize("logn", range(1, 15))
def test_passes_equal_python_integers(logn):
    ins, outs = _ref(logn)
    t0 = time.perf_counter()
    for nb in NBS:
        got = _probe(logn, 0, B, nb, VECTORS, _lanes(ins, logn, nb))
        want = _lanes(outs, logn, nb)
        assert np.array_equal(got, want), (logn, nb, _where(got, want))
    print("logn %d, turn width %d: passes, nb %s in %.2f s (reference so far %.1f s)" %
          (logn, (logn - 1) % 3 + 1, NBS, time.perf_counter() - t0, _REF_SECONDS[0]))


@pytest.mark.parametrize("logn", range(9, 15))
def test_lds_kernels_equal_python_integers_and_the_passes(logn):
    ins, outs = _ref(logn)
    t0 = time.perf_counter()
    for nb in NBS:
        src = _lanes(ins, logn, nb)
        got = _probe(logn, 1, B, nb, VECTORS, src)
        want = _lanes(outs, logn, nb)
        assert np.array_equal(got, want), (logn, nb, _where(got, want))
        if nb == NBS[-1]:
            other = _probe(logn, 0, B, nb, VECTORS, src)
            assert np.array_equal(got, other), (logn, nb, _where(got, other))
    print("logn %d, E = %d: edge / mid / edge, nb %s in %.2f s" % (logn, logn - 9, NBS, time.perf_counter() - t0))


@pytest.mark.parametrize("kind", ["random", "alternating", "single_at_n_minus_1"])
def test_lds_kernels_at_2_pow_18_equal_the_c_oracle(kind):
    """E = 9: cl = 1, a workgroup's points are 512 apart.  One lane of two, one vector."""
    from oracle.c import binding as ob
    logn, n = 18, 1 << 18
    rnd = random.Random(18)
    v = {"random": lambda: [rnd.randrange(R) for _ in range(n)],
         "alternating": lambda: [0 if i % 2 == 0 else R - 1 for i in range(n)],
         "single_at_n_minus_1": lambda: [0] * (n - 1) + [R - 1]}[kind]()
    t0 = time.perf_counter()
    want = _rows(ob.coset_transform(logn, v))
    t1 = time.perf_counter()
    got = _probe(logn, 1, 2, 1, 1, _rows(v).reshape(1, n, 1, 32))
    assert np.array_equal(got.reshape(n, 32), want), _where(got, want.reshape(1, n, 1, 32))
    print("logn 18 (%s): oracle %.2f s, device call %.2f s" % (kind, t1 - t0, time.perf_counter() - t1))


def test_bad_arguments_are_errors():
    from zerokit_amd._native import RLNError
    z = np.zeros((3, 1 << 9, 2, 32), dtype=np.uint8)
    for logn, lds, b, nb, vectors in ((0, 0, 2, 2, 3), (19, 0, 2, 2, 3), (19, 1, 2, 2, 3), (8, 1, 2, 2, 3), (9, 1, 2, 3, 3),
                                      (9, 0, 2, 0, 3), (9, 0, 2, 2, 0), (9, 0, 2, 2, 4)):
        with pytest.raises(RLNError):
            _probe(logn, lds, b, nb, vectors, z)
    assert not _probe(9, 1, 2, 2, 3, z).any()       # (the same buffer with good arguments: zeros stay zeros)
