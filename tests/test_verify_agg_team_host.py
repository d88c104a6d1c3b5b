"""The optimistic verifier's team form (zerokit_amd/csrc/verify_agg_team_math.h: eight lanes per proof) compiled with
g++, its lanes run one after the other over an array in place of LDS, and checked on the CPU: against the plain product
over pairing.h (vah_twin, byte for byte after finish_host) and against the lane form of verify_agg_math.h.  No GPU: the
kernels of verify_agg_team.hip call exactly these functions."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

import verify_cases as vc
from verify_cases import GT_ONE, R, ROOT

CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
SIZES = (1, 2, 7, 8, 9, 63, 64, 65)
TOP = (1 << 128) - 1
DAMAGED = ("input0", "swapAC", "A_infinity", "B_infinity", "C_infinity", "A_off_curve", "B_outside_subgroup")
HEADERS = ("field.h", "curve.h", "pairing.h", "zkey.cpp", "zkey.h", "common.h", "verify_math.h", "verify_key.h",
           "verify_agg_math.h", "verify_team_math.h", "verify_agg_team_math.h")


@functools.lru_cache(None)
def _lib():
    so = os.path.join(HOST, "libverifyaggteam.so")
    src = os.path.join(HOST, "verifyaggteam.cpp")
    deps = [src, os.path.join(HOST, "verifyagg.cpp")] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", CSRC, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.vah_n_values.restype = ctypes.c_size_t
    return lib


def load(depth=20, multi=False):
    z = vc.zkey_bytes(depth, multi)
    assert _lib().vah_load_zkey(z, len(z)) == 0
    return _lib().vah_n_values()


@pytest.fixture
def VT():
    load()
    return _lib()


def row(proof, pub):
    """(proof bytes, value bytes) from a golden case's integers"""
    return proof, b"".join((int(v) % (1 << 256)).to_bytes(32, "little") for v in pub)


def pack(rows, scalars):
    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(int(s).to_bytes(16, "little") for s in scalars)


def last(team, rows, scalars, nv=5):
    """(value after finish_host, reject flags, the G1 sum in affine form, the Fr sums) of the team or the lane form"""
    n = len(rows)
    p, v, s = pack(rows, scalars)
    gt, c, sums, rej = (ctypes.create_string_buffer(k) for k in (384, 65, 32 * (nv + 1), max(n, 1)))
    assert _lib().vat_last(team, n, p, v, s, gt, c, sums, rej) == 0
    return gt.raw, rej.raw[:n], c.raw, sums.raw


def twin(rows, scalars):
    n = len(rows)
    p, v, s = pack(rows, scalars)
    gt, rej = ctypes.create_string_buffer(384), ctypes.create_string_buffer(max(n, 1))
    assert _lib().vah_twin(n, p, v, s, gt, rej) == 0
    return gt.raw, rej.raw[:n]


def fold_rows(base, n):
    """rows 64 g .. 64 g + 63 alternate between two of `base`: every slot meets an identical row early in the fold"""
    return [base[(i // 64 + (i & 1)) % len(base)] for i in range(n)]


def fold_scalars(n, seed):
    """seeded scalars; the first is 1, the last 2^128 - 1, and rows 2 .. 9 (identical in pairs two apart) share one"""
    rnd = random.Random(seed)
    sc = [rnd.randrange(1, 1 << 128) for _ in range(n)]
    same = rnd.randrange(1, 1 << 128)
    for i in range(2, min(n - 1, 10)):
        sc[i] = same
    sc[0] = 1
    if n > 1:
        sc[-1] = TOP
    return sc


def depth20_cases(n):
    """(label, rows, scalars, all valid) for one size"""
    g = vc.golden_h20()
    base = [row(c[1], c[2]) for c in g]
    rj = dict((nm.split("/")[1], row(pr, pu)) for nm, pr, pu in vc.rejects(*g[2]))
    out = [("fold", fold_rows(base, n), fold_scalars(n, seed=n), True),
           ("ones", fold_rows(base, n), [1] * n, True),
           ("top, identical rows", [base[0]] * n, [TOP] * n, True)]
    rows = fold_rows(base, n)
    for k, i in enumerate(range(n // 2, n, 3)):
        rows[i] = rj[DAMAGED[(k + n) % len(DAMAGED)]]
    out.append(("damaged", rows, fold_scalars(n, seed=100 + n), False))
    return out


@functools.lru_cache(None)
def depth20_results(n):
    """every form's answer for every case of one size, computed once for the tests below"""
    load()
    return [(label, valid, last(1, rows, sc), last(0, rows, sc), twin(rows, sc))
            for label, rows, sc, valid in depth20_cases(n)]


def test_the_damaged_kinds_are_all_used():
    used = set()
    for n in SIZES:
        used |= {DAMAGED[(k + n) % len(DAMAGED)] for k, _ in enumerate(range(n // 2, n, 3))}
    assert used == set(DAMAGED)


@pytest.mark.parametrize("n", SIZES)
def test_teams_against_the_plain_product(n):
    """1. host_aggregate_teams + finish_host == vah_twin (pairing.h alone), value and reject flags; all-valid rows give
    1, with damaged rows in between the value is the twin's and not 1"""
    for label, valid, team, _, want in depth20_results(n):
        assert team[1] == want[1], (n, label)
        assert team[0] == want[0], (n, label)
        if valid:
            assert team[0] == GT_ONE and not any(team[1]), (n, label)
        else:
            assert team[0] != GT_ONE, (n, label)


@pytest.mark.parametrize("n", SIZES)
def test_teams_against_the_lane_form(n):
    """2. the same inputs: equal to verify_agg_math.h's lane form after finish_host, the G1 sum in affine form and the
    Fr sums exactly"""
    for label, _, team, lane, _ in depth20_results(n):
        assert team == lane, (n, label)


def test_other_circuits():
    """3. n_values comes from the key: the depth-10 and the multi-message-id circuit (more than 8 inputs: a second
    round of lanes), whole and with the last input changed, n = 1 and 9"""
    seen_multi = False
    for name, depth, multi, proof, pub in vc.golden_other():
        nv = load(depth, multi)
        assert nv == len(pub)
        if multi:
            assert nv > 8
            seen_multi = True
        bad = list(pub)
        bad[-1] = (bad[-1] + 1) % R
        for n in (1, 9):
            sc = fold_scalars(n, seed=7 * n)
            for rows, one in (([row(proof, pub)] * n, True),
                              ([row(proof, pub)] * (n // 2) + [row(proof, bad)] + [row(proof, pub)] * (n - n // 2 - 1), False)):
                team, lane = last(1, rows, sc, nv), last(0, rows, sc, nv)
                assert team[:2] == twin(rows, sc), (name, n)
                assert team == lane, (name, n)
                assert (team[0] == GT_ONE) == one, (name, n)
    assert seen_multi


def test_seeded_byte_mutations(VT):
    """4. 200 seeded single-byte mutations in one batch: value and flags are the twin's; the twin's flags show that at
    least 10 % of the rows are refused by the per-proof checks and at least 10 % are let through"""
    muts = vc.byte_mutations(vc.golden_h20(), 200, seed=47)
    rows = [(m[1], m[2]) for m in muts]
    sc = fold_scalars(200, seed=48)
    want = twin(rows, sc)
    assert 20 <= sum(want[1]) <= 180, sum(want[1])
    got = last(1, rows, sc)
    assert got[:2] == want


@pytest.mark.parametrize("n", (3, 11))
def test_waves_driver_writes_rows_0_to_n_and_nothing_else(VT, n):
    """5. the waves of eight teams over sentinel-filled arrays: the teams past the end redo the last proof and store
    nothing"""
    g = vc.golden_h20()
    rows = fold_rows([row(c[1], c[2]) for c in g], n)
    p, v, s = pack(rows, fold_scalars(n, seed=n))
    assert VT.vat_waves_bounds(n, 8, p, v, s) == 0


def test_refactored_t_prepare_keeps_the_exact_team_form(VT):
    """6. t_prepare, whose decompression and subgroup phases now live in t_checked_points: the exact team form still
    gives the host verifier's verdict and GT value on golden cases and every case of their rejects()"""
    seen = 0
    for name, proof, pub in vc.golden_h20():
        for nm, pr, pu in [(name, proof, pub)] + vc.rejects(name, proof, pub):
            a, b = ctypes.create_string_buffer(384), ctypes.create_string_buffer(384)
            vals = row(pr, pu)[1]
            va, vb = VT.vat_team_verify(pr, vals, a), VT.vat_host_verify(pr, vals, b)
            assert va == vb and va in (0, 1), nm
            assert a.raw == b.raw, nm
            seen += 1
    assert seen == 6 * 16


def test_stand_alone_harness_under_asan_ubsan(tmp_path):
    """7. tests/host/verifyaggteam_main.cpp (its own main; never loaded into python) built with
    -fsanitize=address,undefined and run as a program: depth 20 at n = 9 (valid rows; damaged rows in between) and the
    other two circuits at n = 1 equal the plain product, and the sanitizers stay silent"""
    exe = str(tmp_path / "verifyaggteam_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I", "/opt/rocm/include", "-I", CSRC, os.path.join(HOST, "verifyaggteam_main.cpp"), "-o", exe])
    g = vc.golden_h20()
    valid = [row(c[1], c[2]) for c in g]
    rj = dict((nm.split("/")[1], row(pr, pu)) for nm, pr, pu in vc.rejects(*g[3]))
    mixed = valid[:2] + [rj["A_off_curve"], valid[2], rj["input0"], rj["B_infinity"], valid[3], rj["B_outside_subgroup"],
                         rj["C_infinity"]]
    runs = [(20, False, valid, 9, 3), (20, False, mixed, 9, 0)]
    for name, depth, multi, proof, pub in vc.golden_other():
        runs.append((depth, multi, [row(proof, pub)], 1, 3))
        runs.append((depth, multi, [row(proof, pub[:-1] + [(pub[-1] + 1) % R])], 1, 0))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k, (depth, multi, rows, n, ones) in enumerate(runs):
        blob = tmp_path / ("rows%d.bin" % k)
        blob.write_bytes(b"".join(pr + va for pr, va in rows))
        d = "tree_depth_%d%s" % (depth, "_multi_max_out_4" if multi else "")
        r = subprocess.run([exe, os.path.join(ROOT, "zerokit_amd", "resources", d, "rln_final.arkzkey"), str(blob), str(n)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
        assert "3 runs, 0 failures, %d ones" % ones in r.stdout, (k, r.stdout)
