"""The optimistic verifier's mathematics (zerokit_amd/csrc/verify_agg_math.h) compiled with g++, its lanes run in a
loop, and checked on the CPU.  The chain of trust: the host twin rlnamd_verify_aggregate_with_zkey (pairing.h alone:
prod_i GT_i^(r_i)) against the Python oracle, which fixes the coefficient mapping; then the header's prepare_agg ->
single-pair Miller loop -> fold tree -> finish_host against the host twin.  No GPU: the kernels of verify_agg.hip call
exactly these functions."""
import ctypes
import os
import random
import subprocess

import pytest

import verify_cases as vc
from verify_cases import GT_ONE, R, ROOT, le

CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
SIZES = (1, 2, 3, 64, 65)
TOP = (1 << 128) - 1


def _build():
    so = os.path.join(ROOT, "tests", "host", "libverifyagg.so")
    src = os.path.join(ROOT, "tests", "host", "verifyagg.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("field.h", "curve.h", "pairing.h", "zkey.cpp", "zkey.h", "common.h",
                                                    "verify_math.h", "verify_key.h", "verify_agg_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", CSRC, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.vah_n_values.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def VA():
    lib = _build()
    z = vc.zkey_bytes(20)
    assert lib.vah_load_zkey(z, len(z)) == 0
    return lib


def raw(x):
    return (int(x) % (1 << 256)).to_bytes(32, "little")


def pack(rows, scalars):
    return (b"".join(r[0] for r in rows), b"".join(raw(v) for r in rows for v in r[1]),
            b"".join(int(s).to_bytes(16, "little") for s in scalars))


def header(VA, rows, scalars):
    n = len(rows)
    p, v, s = pack(rows, scalars)
    gt, rej = ctypes.create_string_buffer(384), ctypes.create_string_buffer(max(n, 1))
    assert VA.vah_aggregate(n, p, v, s, gt, rej) == 0
    return gt.raw, rej.raw[:n]


def twin(rows, scalars, zkey=None):
    """rlnamd_verify_aggregate_with_zkey: no GPU"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    z = zkey or vc.zkey_bytes(20)
    p, v, s = pack(rows, scalars)
    gt, rej = ctypes.create_string_buffer(384), ctypes.create_string_buffer(max(n, 1))
    check(lib().rlnamd_verify_aggregate_with_zkey(z, len(z), n, p, v, len(rows[0][1]) if rows else 5, s, gt, rej))
    return gt.raw, rej.raw[:n]


def tiled(n, golden=None):
    g = golden or vc.golden_h20()
    return [(g[i % len(g)][1], g[i % len(g)][2]) for i in range(n)]


def test_host_twin_against_the_oracle():
    """prod_i GT_i^(r_i) of two proofs whose pairing products are not 1 (one changed input; A and C swapped) under
    scalars 3 and 5, against oracle/pyref: pairing, f12_pow, f12_mul.  Fixes the coefficient mapping."""
    from oracle.pyref import arkzkey
    from oracle.pyref import bn254 as o
    g = vc.golden_h20()
    rej0 = dict((nm.split("/")[1], (pr, pu)) for nm, pr, pu in vc.rejects(*g[0]))
    rej1 = dict((nm.split("/")[1], (pr, pu)) for nm, pr, pu in vc.rejects(*g[1]))
    rows, scalars = [rej0["input0"], rej1["swapAC"]], [3, 5]
    zk = arkzkey.parse(vc.zkey_bytes(20))
    ab = o.pairing(o.G1.neg(zk.alpha_g1), zk.beta_g2)
    want = o.f12_one()
    for (proof, pub), r in zip(rows, scalars):
        A, B, Cp = arkzkey.proof_decompress(proof)
        ic = o.G1.to_jac(zk.gamma_abc_g1[0])
        for x, P in zip(pub, zk.gamma_abc_g1[1:]):
            ic = o.G1.jac_add_mixed(ic, o.G1.mul(P, x % R))
        ic = o.G1.to_affine(ic)
        gt = o.f12_mul(o.f12_mul(o.pairing(A, B), ab),
                       o.f12_mul(o.pairing(o.G1.neg(ic), zk.gamma_g2), o.pairing(o.G1.neg(Cp), zk.delta_g2)))
        assert gt != o.f12_one()
        want = o.f12_mul(want, o.f12_pow(gt, r))
    got, rej = twin(rows, scalars)
    assert rej == b"\x00\x00"
    assert got == b"".join(le(c[0]) + le(c[1]) for c in want)
    assert got != GT_ONE
    # and valid proofs give 1 whatever the scalars
    assert twin(tiled(3), [7, TOP, 1])[0] == GT_ONE


def partner(n):
    """the slot that slot 0 meets first in the fold of n partials"""
    return 32 if n > 32 else (1 << ((n - 1).bit_length() - 1))


def scalar_cases(n):
    """(label, rows, scalars) for one size: the cases the fold and the ladders can get wrong"""
    g = vc.golden_h20()
    rnd = random.Random(1000 + n)
    out = [("ones", tiled(n), [1] * n),
           ("top", tiled(n), [TOP] * n),
           ("random", tiled(n), [rnd.randrange(1, 1 << 128) for _ in range(n)]),
           ("equal scalars, identical proofs", [(g[0][1], g[0][2])] * n, [5] * n)]
    if n >= 2:
        # r C + r (-C) = infinity where slot 0 meets its partner: the second row is row 0 with C negated (the sign bit
        # of its compressed form), an invalid proof that passes every per-proof check
        rows = tiled(n)
        pr = bytearray(rows[0][0])
        pr[127] ^= 0x80
        rows[partner(n)] = (bytes(pr), rows[0][1])
        sc = [rnd.randrange(1, 1 << 128) for _ in range(n)]
        sc[partner(n)] = sc[0]
        out.append(("cancelling C", rows, sc))
    # rejected rows in between (and, at n = 1, alone)
    rows = tiled(n)
    rj = [(pr, pu) for nm, pr, pu in vc.rejects(*g[2])
          if nm.split("/")[1] in ("A_off_curve", "input_eq_r", "B_outside_subgroup", "C_off_curve", "A_noncanonical_x")]
    for k, i in enumerate(range(0, n, 3)):
        rows[i] = rj[k % len(rj)]
    out.append(("rejected rows", rows, [rnd.randrange(1, 1 << 128) for _ in range(n)]))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_header_against_the_host_twin(VA, n):
    """prepare_agg -> Miller -> fold tree -> finish_host == the host twin, bytes and reject flags, for every scalar
    case; all-valid cases give 1, the cancelling pair does not (its second row is invalid)"""
    for label, rows, scalars in scalar_cases(n):
        got, rej = header(VA, rows, scalars)
        want, wrej = twin(rows, scalars)
        assert rej == wrej, (n, label)
        assert got == want, (n, label)
        if label == "cancelling C":
            assert got != GT_ONE and not any(rej)
        elif label == "rejected rows":
            assert got == GT_ONE and sum(rej) == len(range(0, n, 3))
        else:
            assert got == GT_ONE and not any(rej), (n, label)


def test_invalid_proofs_and_infinite_points_change_the_value(VA):
    """rows the pairing rejects, among them A, B and C at infinity (the pair contributes 1, the sums still count): the
    header's value equals the twin's and is not 1"""
    g = vc.golden_h20()
    rj = dict((nm.split("/")[1], (pr, pu)) for nm, pr, pu in vc.rejects(*g[3]))
    rnd = random.Random(9)
    for name in ("input0", "swapAC", "A_infinity", "B_infinity", "C_infinity"):
        rows = tiled(5)
        rows[3] = rj[name]
        scalars = [rnd.randrange(1, 1 << 128) for _ in range(5)]
        got, rej = header(VA, rows, scalars)
        assert (got, rej) == twin(rows, scalars), name
        assert got != GT_ONE and not any(rej), name


def test_other_circuits(VA):
    """n_values comes from the key: the depth-10 and the multi-message-id golden proofs, with a changed input"""
    try:
        for name, depth, multi, proof, pub in vc.golden_other():
            z = vc.zkey_bytes(depth, multi)
            assert VA.vah_load_zkey(z, len(z)) == 0 and VA.vah_n_values() == len(pub)
            bad = list(pub)
            bad[-1] = (bad[-1] + 1) % R
            for rows, one in (([(proof, pub)] * 3, True), ([(proof, pub), (proof, bad), (proof, pub)], False)):
                got, rej = header(VA, rows, [TOP, 1, 12345])
                assert (got, rej) == twin(rows, [TOP, 1, 12345], zkey=z), name
                assert (got == GT_ONE) == one, name
    finally:
        z = vc.zkey_bytes(20)
        assert VA.vah_load_zkey(z, len(z)) == 0


def test_prepare_fills_the_same_prep_as_before_the_refactor(VA):
    """vm::prepare, whose reject rules now live in vm::checked_points, against its earlier text kept in the harness:
    the same Prep bytes for every golden proof and every case of rejects(); and the existing program
    (tests/host/verifymath.cpp) still gives the host verifier's verdict and GT value on them"""
    seen = 0
    for name, proof, pub in vc.golden_h20():
        for nm, pr, pu in [(name, proof, pub)] + vc.rejects(name, proof, pub):
            assert VA.vah_prep_same(pr, b"".join(raw(v) for v in pu)) == 1, nm
            seen += 1
    assert seen == 6 * 16
    import test_verify_math_host as tv
    lib = tv._build()
    z = vc.zkey_bytes(20)
    assert lib.vmh_load_zkey(z, len(z)) == 0
    tv._check_cases(lib, vc.golden_h20()[:2])


def test_seeded_byte_mutations_mix_both_verdicts():
    """the rows of the GPU suite's seeded mix (tests/test_gpu_verify_optimistic.py: mixed_rows) on host threads: at
    least 10 % rejected and at least 10 % accepted, so that a trivial verifier cannot pass there"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    proofs, vals = mixed_rows(1025, seed=31)
    z = vc.zkey_bytes(20)
    ok = ctypes.create_string_buffer(1025)
    check(lib().rlnamd_verify_many_with_zkey(z, len(z), 1025, proofs, vals, 5, 0, ok))
    acc = sum(ok.raw)
    assert acc >= 103 and 1025 - acc >= 103, acc


def mixed_rows(n, seed):
    """n rows tiled from the golden proofs; every fourth row, and the last, is one of byte_mutations' rows"""
    g = vc.golden_h20()
    muts = vc.byte_mutations(g, n, seed=seed)
    ps, vs = [], []
    for i in range(n):
        if i % 4 == 3 or i == n - 1:
            ps.append(muts[i][1])
            vs.append(muts[i][2])
        else:
            ps.append(g[i % len(g)][1])
            vs.append(b"".join(le(v) for v in g[i % len(g)][2]))
    return b"".join(ps), b"".join(vs)


def test_stand_alone_harness_under_asan_ubsan(tmp_path):
    """tests/host/verifyagg_main.cpp (its own main; never loaded into python) built with -fsanitize=address,undefined and
    run once: the header's path equals the plain product for n = 1, 2, 3, 64, 65 and the sanitizers stay silent"""
    exe = str(tmp_path / "verifyagg_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I", "/opt/rocm/include", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "verifyagg_main.cpp"), "-o", exe])
    g = vc.golden_h20()
    rows = [(c[1], c[2]) for c in g[:3]]
    rows.append([(pr, pu) for nm, pr, pu in vc.rejects(*g[3]) if nm.endswith("/A_off_curve")][0])
    rows.append([(pr, pu) for nm, pr, pu in vc.rejects(*g[4]) if nm.endswith("/input0")][0])
    blob = tmp_path / "rows.bin"
    blob.write_bytes(b"".join(pr + b"".join(raw(v) for v in pu) for pr, pu in rows))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "zerokit_amd", "resources", "tree_depth_20", "rln_final.arkzkey"),
                        str(blob)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
    assert "15 runs, 0 failures" in r.stdout
