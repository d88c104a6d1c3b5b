"""The team form of the device verifier (zerokit_amd/csrc/verify_team_math.h: eight lanes per proof) compiled with g++,
its eight lanes run in a loop over an array in place of LDS, and checked on the CPU against the Python oracle
(oracle/pyref/bn254.py) and against the host verifier (zkey.cpp + pairing.h).  No GPU: the kernels of verify_team.hip
call exactly these functions."""
import ctypes
import os
import random
import subprocess

import pytest

import verify_cases as vc
from oracle.pyref import bn254 as o
from verify_cases import GT_ONE, Q, ROOT, le


def _build():
    so = os.path.join(ROOT, "tests", "host", "libverifyteam.so")
    src = os.path.join(ROOT, "tests", "host", "verifyteam.cpp")
    csrc = os.path.join(ROOT, "zerokit_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("field.h", "curve.h", "pairing.h", "zkey.cpp", "zkey.h", "common.h",
                                                    "verify_math.h", "verify_key.h", "verify_team_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", csrc, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.vth_n_values.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def VT():
    lib = _build()
    z = vc.zkey_bytes(20)
    assert lib.vth_load_zkey(z, len(z)) == 0
    return lib


def f12_bytes(f):
    return b"".join(le(c[0]) + le(c[1]) for c in f)


def f12_ints(bs):
    v = [int.from_bytes(bs[32 * i:32 * i + 32], "little") for i in range(12)]
    return [(v[2 * i], v[2 * i + 1]) for i in range(6)]


def op(VT, code, a, b=None, in_place=0):
    out = ctypes.create_string_buffer(384)
    assert VT.vth_f12_op(code, f12_bytes(a), f12_bytes(b) if b is not None else None, in_place, out) == 0
    return f12_ints(out.raw)


def both(VT, proof, vals):
    """(team verdict, its GT, host verdict, host GT) of one proof"""
    n = len(vals) // 32
    g1, g2 = ctypes.create_string_buffer(384), ctypes.create_string_buffer(384)
    v = VT.vth_verify(proof, vals, n, g1)
    h = VT.vth_host_verify(proof, vals, n, g2)
    assert v in (0, 1) and h in (0, 1)
    return v, g1.raw, h, g2.raw


def _operands():
    rnd = random.Random(1)

    def rand12():
        return [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(6)]
    one = o.f12_one()
    zero = [(0, 0)] * 6
    top = [(Q - 1, Q - 1)] * 6
    sparse = [(5, 0), (0, 0), (0, 0), (0, Q - 1), (0, 0), (0, 0)]
    return [rand12() for _ in range(4)] + [one, top, sparse], one, zero, top


def test_team_tower_arithmetic_against_the_oracle(VT):
    """every team operation, lane k forming coefficient k, on the operand set of the lane-per-proof test: product,
    square, inverse, both Frobenius maps, conjugation, cyclotomic square, a^u, the final exponentiation; out of place
    and with the destination on an operand"""
    vals, one, zero, top = _operands()
    for a in vals:
        for b in vals[:3] + [one, zero, top]:
            assert op(VT, 0, a, b) == o.f12_mul(a, b)
            assert op(VT, 0, a, b, in_place=1) == o.f12_mul(a, b)
        for ip in (0, 1):
            assert op(VT, 1, a, in_place=ip) == o.f12_mul(a, a)
            assert o.f12_mul(op(VT, 2, a, in_place=ip), a) == one
            assert op(VT, 3, a, in_place=ip) == o.f12_pow(a, Q)
            assert op(VT, 4, a, in_place=ip) == o.f12_pow(a, Q * Q)
            assert op(VT, 8, a, in_place=ip) == o.f12_pow(a, Q ** 6)
    assert op(VT, 0, zero, vals[0]) == zero and op(VT, 2, zero) == zero
    for a in vals[:3]:
        c = o.f12_pow(a, (Q ** 6 - 1) * (Q * Q + 1))   # into the cyclotomic subgroup
        assert op(VT, 5, c) == o.f12_mul(c, c)
        assert op(VT, 5, c, in_place=1) == o.f12_mul(c, c)
        assert op(VT, 7, c) == o.f12_pow(c, o.BN_U)
    a = vals[0]
    assert op(VT, 6, a) == o.final_exp(a)
    assert op(VT, 6, one) == one


def test_sparse_line_product_equals_the_dense_product(VT):
    """f (l0 + l1 w + l3 w^3) by the three-term row against the oracle's product with the line written out as an Fq12;
    lines with l0 in Fq2 (the variable pair), with l0 in Fq (gamma, delta), the identity line and all q - 1"""
    vals, one, zero, top = _operands()
    rnd = random.Random(5)

    def r2():
        return (rnd.randrange(Q), rnd.randrange(Q))
    lines = [(r2(), r2(), r2()), ((rnd.randrange(Q), 0), r2(), r2()), ((1, 0), (0, 0), (0, 0)),
             ((Q - 1, Q - 1),) * 3, ((0, 0), r2(), (0, 0))]
    for a in vals + [zero]:
        for l0, l1, l3 in lines:
            dense = [l0, l1, (0, 0), l3, (0, 0), (0, 0)]
            out = ctypes.create_string_buffer(384)
            line = b"".join(le(c[0]) + le(c[1]) for c in (l0, l1, l3))
            assert VT.vth_line_op(f12_bytes(a), line, out) == 0
            assert f12_ints(out.raw) == o.f12_mul(a, dense)


def test_reduction_bound_all_components_q_minus_1(VT):
    """a row of the product is a 6-term dot product taken as three 4-product sums with one reduction each; the largest
    operands (all twelve components q - 1, times xi on the wrapped terms) must still give the oracle's value"""
    top = [(Q - 1, Q - 1)] * 6
    assert op(VT, 0, top, top) == o.f12_mul(top, top)
    assert op(VT, 1, top) == o.f12_mul(top, top)
    assert op(VT, 0, top, top, in_place=1) == o.f12_mul(top, top)
    assert op(VT, 1, top, in_place=1) == o.f12_mul(top, top)


def _check_cases(VT, golden):
    for name, proof, pub in golden:
        v, gt, h, gh = both(VT, proof, b"".join(le(x) for x in pub))
        assert (v, h) == (1, 1) and gt == GT_ONE == gh, name
        seen = set()
        for rname, rproof, rpub in vc.rejects(name, proof, pub):
            vals = b"".join((x % (1 << 256)).to_bytes(32, "little") for x in rpub)
            v, gt, h, gh = both(VT, rproof, vals)
            assert v == h, rname
            assert gt == gh, rname
            seen.add((rname.split("/")[1].rstrip("0123456789"), v, gt == bytes(384)))
        # rejected by the pairing (a GT value that is not 1) and rejected before it (zeros) both occur
        assert ("input", 0, False) in seen and ("B_outside_subgroup", 0, True) in seen, seen
        assert ("A_infinity", 0, False) in seen and ("A_off_curve", 0, True) in seen, seen


def test_team_verification_equals_the_host_verifier_depth20(VT):
    """bytes in, verdict and GT value out: the golden proofs accept with GT = 1; every hand-made reject gets the host
    verifier's verdict and, where the pairing runs, its GT value"""
    _check_cases(VT, vc.golden_h20())


def test_team_verification_other_circuits():
    """the depth-10 circuit and the multi-message-id circuit (more than eight inputs: two rounds of eight lanes)"""
    lib = _build()
    counts = []
    for name, depth, multi, proof, pub in vc.golden_other():
        z = vc.zkey_bytes(depth, multi)
        assert lib.vth_load_zkey(z, len(z)) == 0
        assert lib.vth_n_values() == len(pub)
        counts.append(len(pub))
        _check_cases(lib, [(name, proof, pub)])
    assert max(counts) > 5
    z = vc.zkey_bytes(20)
    assert lib.vth_load_zkey(z, len(z)) == 0   # (the module fixture's key, for whichever test runs next)


def test_team_fuzz_single_byte_mutations_equal_the_host_verifier(VT):
    """300 seeded single-byte mutations of golden proofs and inputs: verdict and GT equal the host verifier's"""
    rejected = accepted = 0
    for name, proof, vals in vc.byte_mutations(vc.golden_h20(), 300, seed=2024):
        v, gt, h, gh = both(VT, proof, vals)
        assert v == h, name
        assert gt == gh, name
        rejected += v == 0
        accepted += v == 1
    assert rejected + accepted == 300 and rejected >= 250


@pytest.mark.parametrize("n", [3, 11])
def test_waves_of_eight_teams_write_rows_0_to_n_only(VT, n):
    """the driver the kernels share: n proofs as ceil(n / 8) waves of 8 teams; a team past the end redoes the last
    proof and stores nothing, so rows 0 .. n - 1 are written and a sentinel-filled output is untouched beyond them"""
    golden = vc.golden_h20()
    rows = []
    for i in range(n):
        name, proof, pub = golden[i % len(golden)]
        if i % 3 == 1:
            pub = list(pub)
            pub[0] = (pub[0] + 1) % vc.R      # rejected by the pairing
        if i % 5 == 4:
            proof = vc.off_curve_x() + proof[32:]   # rejected before it
        rows.append((proof, b"".join(le(x) for x in pub)))
    nv = len(rows[0][1]) // 32
    pad = 16
    ok = ctypes.create_string_buffer(b"\xa5" * (n + pad), n + pad)
    gt = ctypes.create_string_buffer(b"\xa5" * (384 * (n + pad)), 384 * (n + pad))
    assert VT.vth_verify_waves(n, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), nv, ok, gt) == 0
    assert ok.raw[n:] == b"\xa5" * pad and gt.raw[384 * n:] == b"\xa5" * (384 * pad)
    verdicts = set()
    for i, (proof, vals) in enumerate(rows):
        g = ctypes.create_string_buffer(384)
        h = VT.vth_host_verify(proof, vals, nv, g)
        assert ok.raw[i] == h, i
        assert gt.raw[384 * i:384 * i + 384] == g.raw, i
        verdicts.add(h)
    assert verdicts == {0, 1}
