"""The device verifier's mathematics (zerokit_amd/csrc/verify_math.h) compiled with g++ and checked on the CPU against
the Python oracle (oracle/pyref/bn254.py) and against the host verifier (zkey.cpp + pairing.h) it must agree with on
every input.  No GPU: the kernels of verify.hip call exactly these functions, one lane per proof."""
import ctypes
import os
import random
import subprocess

import pytest

import verify_cases as vc
from oracle.pyref import bn254 as o
from verify_cases import GT_ONE, Q, R, ROOT, le


def _build():
    so = os.path.join(ROOT, "tests", "host", "libverifymath.so")
    src = os.path.join(ROOT, "tests", "host", "verifymath.cpp")
    csrc = os.path.join(ROOT, "zerokit_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("field.h", "curve.h", "pairing.h", "zkey.cpp", "zkey.h", "common.h",
                                                    "verify_math.h", "verify_key.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", csrc, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.vmh_n_values.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def VM():
    lib = _build()
    z = vc.zkey_bytes(20)
    assert lib.vmh_load_zkey(z, len(z)) == 0
    return lib


def f12_bytes(f):
    return b"".join(le(c[0]) + le(c[1]) for c in f)


def f12_ints(bs):
    v = [int.from_bytes(bs[32 * i:32 * i + 32], "little") for i in range(12)]
    return [(v[2 * i], v[2 * i + 1]) for i in range(6)]


def op(VM, code, a, b=None):
    out = ctypes.create_string_buffer(384)
    assert VM.vmh_f12_op(code, f12_bytes(a), f12_bytes(b) if b is not None else None, out) == 0
    return f12_ints(out.raw)


def both(VM, proof, vals):
    """(device-math verdict, its GT, host verdict, host GT) of one proof"""
    n = len(vals) // 32
    g1, g2 = ctypes.create_string_buffer(384), ctypes.create_string_buffer(384)
    v = VM.vmh_verify(proof, vals, n, g1)
    h = VM.vmh_host_verify(proof, vals, n, g2)
    assert v in (0, 1) and h in (0, 1)
    return v, g1.raw, h, g2.raw


def test_tower_arithmetic_against_the_oracle(VM):
    """Fq12 product, square, inverse, both Frobenius maps and the cyclotomic square against f12_mul / f12_pow"""
    rnd = random.Random(1)

    def rand12():
        return [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(6)]
    one = o.f12_one()
    zero = [(0, 0)] * 6
    top = [(Q - 1, Q - 1)] * 6
    sparse = [(5, 0), (0, 0), (0, 0), (0, Q - 1), (0, 0), (0, 0)]
    vals = [rand12() for _ in range(4)] + [one, top, sparse]
    for a in vals:
        for b in vals[:3] + [one, zero, top]:
            assert op(VM, 0, a, b) == o.f12_mul(a, b)
        assert op(VM, 1, a) == o.f12_mul(a, a)
        assert o.f12_mul(op(VM, 2, a), a) == one
        assert op(VM, 3, a) == o.f12_pow(a, Q)
        assert op(VM, 4, a) == o.f12_pow(a, Q * Q)
    assert op(VM, 0, zero, vals[0]) == zero and op(VM, 2, zero) == zero
    for a in vals[:3]:
        c = o.f12_pow(a, (Q ** 6 - 1) * (Q * Q + 1))   # into the cyclotomic subgroup
        assert op(VM, 5, c) == o.f12_mul(c, c)
        assert op(VM, 7, c) == o.f12_pow(c, o.BN_U)
    a = vals[0]
    assert op(VM, 6, a) == o.final_exp(a)
    assert op(VM, 6, one) == one


def test_projective_miller_loop_gives_the_pairing(VM):
    """final_exp(miller(P, Q)) of the inversion-free loop == the oracle's pairing == pairing.h's, for the generators and
    random multiples; compared after the final exponentiation only (the Miller values differ by subfield factors)"""
    rnd = random.Random(2)
    pairs = [(o.G1_GEN, o.G2_GEN)]
    for _ in range(3):
        pairs.append((o.G1.mul(o.G1_GEN, rnd.randrange(1, R)), o.G2.mul(o.G2_GEN, rnd.randrange(1, R))))
    for P, Qp in pairs:
        g1 = le(P[0]) + le(P[1])
        g2 = le(Qp[0][0]) + le(Qp[0][1]) + le(Qp[1][0]) + le(Qp[1][1])
        a, h = ctypes.create_string_buffer(384), ctypes.create_string_buffer(384)
        assert VM.vmh_pairing(g1, g2, a) == 0 and VM.vmh_host_pairing(g1, g2, h) == 0
        assert a.raw == h.raw
        assert f12_ints(a.raw) == o.pairing(P, Qp)
        assert a.raw != GT_ONE


def _check_cases(VM, golden):
    for name, proof, pub in golden:
        v, gt, h, gh = both(VM, proof, b"".join(le(x) for x in pub))
        assert (v, h) == (1, 1) and gt == GT_ONE == gh, name
        seen = set()
        for rname, rproof, rpub in vc.rejects(name, proof, pub):
            vals = b"".join((x % (1 << 256)).to_bytes(32, "little") for x in rpub)
            v, gt, h, gh = both(VM, rproof, vals)
            assert v == h, rname
            assert gt == gh, rname
            seen.add((rname.split("/")[1].rstrip("0123456789"), v, gt == bytes(384)))
        # rejected by the pairing (a GT value that is not 1) and rejected before it (zeros) both occur
        assert ("input", 0, False) in seen and ("B_outside_subgroup", 0, True) in seen, seen
        assert ("A_infinity", 0, False) in seen and ("A_off_curve", 0, True) in seen, seen


def test_whole_verification_equals_the_host_verifier_depth20(VM):
    """bytes in, verdict and GT value out: the 6 golden proofs accept with GT = 1; every hand-made reject gets the host
    verifier's verdict and, where the pairing runs, its GT value"""
    _check_cases(VM, vc.golden_h20())


def test_whole_verification_other_circuits():
    """the depth-10 circuit (5 inputs) and the multi-message-id circuit (more): the input count comes from the key"""
    lib = _build()
    counts = []
    for name, depth, multi, proof, pub in vc.golden_other():
        z = vc.zkey_bytes(depth, multi)
        assert lib.vmh_load_zkey(z, len(z)) == 0
        assert lib.vmh_n_values() == len(pub)
        counts.append(len(pub))
        _check_cases(lib, [(name, proof, pub)])
    assert max(counts) > 5
    z = vc.zkey_bytes(20)
    assert lib.vmh_load_zkey(z, len(z)) == 0   # (the module fixture's key, for whichever test runs next)


def test_fuzz_single_byte_mutations_equal_the_host_verifier(VM):
    """300 seeded single-byte mutations of golden proofs and inputs: verdict and GT equal the host verifier's"""
    rejected = accepted = 0
    for name, proof, vals in vc.byte_mutations(vc.golden_h20(), 300, seed=2024):
        v, gt, h, gh = both(VM, proof, vals)
        assert v == h, name
        assert gt == gh, name
        rejected += v == 0
        accepted += v == 1
    assert rejected + accepted == 300 and rejected >= 250
