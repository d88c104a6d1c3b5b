"""The big batches' quotient transforms on 29-bit limbs with loose values between launches (prover_front.hip: k_ntt_pass /
k_ntt_turn), on the device, at the smallest domains that reach every path of them:
  logn 3   the turn alone: canonical in and out in one launch (k_ntt_turn<3, last>)
  logn 4   one DIF pass, turn<1>, one DIT pass: the smallest size with a loose store on both sides of the turn
  logn 5   turn<2>
  logn 6   turn<3> between passes
  logn 7   two passes a side: the smallest with a loose load and a loose store in the same launch
through rlnamd_probe_quotient_transform, which launches them the way Prover::enqueue does.  Inputs chosen for lazy growth:
all r - 1, all 1, alternating 0 / r - 1, a single r - 1 at 0, n / 2 and n - 1, two random vectors; adjacent lanes hold
different ones.  nb = 1, 64, 65 of B = 128 lanes, three vectors.  Reference: oracle.pyref.groth16 in Python integers, once
per logn.  Exact equality.  One whole 129-proof batch against oracle/c closes the file."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B = 128
NBS = (1, 64, 65)
VECTORS = 3
LOGNS = (3, 4, 5, 6, 7)


def _kinds(logn, rnd):
    n = 1 << logn
    out = [[R - 1] * n, [1] * n, [0 if i % 2 == 0 else R - 1 for i in range(n)]]
    for pos in (0, n // 2, n - 1):
        v = [0] * n
        v[pos] = R - 1
        out.append(v)
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


def _ref(logn):
    """(inputs, expected) per kind as (n, 32) byte rows, once per logn"""
    if logn not in _REF:
        kinds = _kinds(logn, random.Random(2900 + logn))
        _REF[logn] = ([_rows(v) for v in kinds], [_rows(_coset_transform_pyref(v)) for v in kinds])
    return _REF[logn]


def _lanes(rows, logn, nb):
    """[vector][index][lane]: lane p of vector v holds kind (p + 3 v + logn) mod K -- neighbours differ"""
    K = len(rows)
    a = np.empty((VECTORS, 1 << logn, nb, 32), dtype=np.uint8)
    for v in range(VECTORS):
        for p in range(nb):
            a[v, :, p, :] = rows[(p + 3 * v + logn) % K]
    return a


def _probe(logn, nb, arr):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    src = np.ascontiguousarray(arr)
    out = np.empty_like(src)
    check(lib().rlnamd_probe_quotient_transform(logn, 0, B, nb, VECTORS, src.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p)))
    return out


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("logn", LOGNS)
def test_passes_on_29_bit_limbs_equal_python_integers(logn, nb):
    ins, outs = _ref(logn)
    got = _probe(logn, nb, _lanes(ins, logn, nb))
    want = _lanes(outs, logn, nb)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (logn, nb, "first differences at (vector, index, lane): %s of %d" % (bad[:6].tolist(), len(bad)))


def test_a_129_proof_batch_equals_the_c_oracle():
    """three lane groups, the last with one live lane: k_matvec, the nine launches of 2^13 points, the quotient in k_recode"""
    import conftest
    from zerokit_amd.batch import BatchProver
    n = 129
    key = (0, 1024) if (0, 1024) in conftest._CONFIG2_ORACLE else (0, n)
    ws, rs, proofs, pub = conftest.oracle_config2(*key)
    p = BatchProver(max_batch=192)
    try:
        out = p.prove(ws[:n], rs[:n])
        assert [o["error"] for o in out] == [0] * n
        assert [o["proof"] for o in out] == proofs[:n]
        assert [o["public_inputs"] for o in out] == pub[:n]
    finally:
        p.close()
