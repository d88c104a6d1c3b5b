"""The shared rows of the throughput plan (zerokit_amd/csrc/prover_plan.h: G1Rows::shared) without a GPU, on the three
shipped keys: tests/host/sharedrows.cpp, built with g++ and loaded with ctypes, is given the wires with
a_query[i] == +- b_g1_query[i] as tests/shared_rows_cases.py reads them from the key through oracle/pyref/arkzkey.py, and checks the
detector against them, the structure of the five-segment plans in full, partial and finish mode, which rows they walk
and where, and the two sums A = s0 + s3 + s4, B1 = s1 + s3 - s4 in host curve arithmetic.  The legacy families and the
point list are held to a checksum taken at the commit before the shared family existed.  The same checks run once more
in a stand-alone program built with ASan and UBSan."""
import ctypes
import os
import struct
import subprocess

import pytest

import shared_rows_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
SRCS = [os.path.join(CSRC, f) for f in ("prover_plan.cpp", "poseidon_host.cpp", "witness_sched.cpp", "zkey.cpp")]
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC]
SEED = 20261021

# circuit -> checksum of pts / sids / npaired / rows / fused: sharedrows_legacy_checksum built with
# -DSHAREDROWS_LEGACY_ONLY against the tree of the commit before the shared family existed
PARENT_SUM = {
    "tree_depth_20": 0xD56C3C629CD9AF41,
    "tree_depth_10": 0x12CEA0235B87CC5B,
    "tree_depth_20_multi_max_out_4": 0xB896C7231F4C94C3,
}
EXPECT = {sub: cases.COUNTS[sub] + (PARENT_SUM[sub],) for sub in cases.COUNTS}
_resource = cases.resource


def wires(sub):
    """(E+, E-, finite A rows, finite B1 rows) by tests/shared_rows_cases.py's own reading of the key"""
    k = cases.key_facts(sub)
    return k["eq"], k["opp"], k["finite_a"], k["finite_b1"]


@pytest.fixture(scope="module")
def SR():
    so = os.path.join(HOST, "libsharedrows.so")
    srcs = [os.path.join(HOST, "sharedrows.cpp")] + SRCS
    deps = srcs + [os.path.join(CSRC, h) for h in ("prover_plan.h", "prover_desc.h", "prover.h", "poseidon.h", "witness_sched.h",
                                                   "zkey.h", "field.h", "curve.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + srcs + ["-o", so])
    lib = ctypes.CDLL(so)
    lib.sharedrows_error.restype = ctypes.c_char_p
    lib.sharedrows_check.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    lib.sharedrows_legacy_checksum.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_uint64)]
    return lib


@pytest.mark.parametrize("sub", sorted(EXPECT))
def test_the_key_shares_the_rows_the_plan_counts_on(sub):
    """the counts this file reads from the key, which are the expectation the detector is held to below"""
    eq, opp, fin_a, fin_b = wires(sub)
    assert (len(eq), len(opp)) == EXPECT[sub][:2]
    assert 0 not in eq + opp and not set(eq) & set(opp)
    if sub == "tree_depth_20":
        assert (fin_a, fin_b) == (5797, 3845)


@pytest.mark.parametrize("sub", sorted(EXPECT))
def test_the_shared_family_and_its_plans(SR, sub):
    """detector == the wires above; the shared family is the legacy rows without the B1 rows of those wires and with
    their A rows in segments 3 / 4; the five-segment plans of the three modes pass the structural checks of the legacy
    plans (chunks tile rows, segments tile chunks, ROW_PAIRED exactly below npaired, pair slots in their members'
    segments, partial and finish partition full); no dropped row is walked, every shared A row once per GLV half;
    s0 + s3 + s4 and s1 + s3 - s4 equal the legacy sums under seeded 16-bit scalars, with every shared scalar zero, and
    with one shared scalar alone (one wire of E+, one of E-)"""
    eq, opp, _, _ = wires(sub)
    zb, gb = open(_resource(sub, "rln_final.arkzkey"), "rb").read(), open(_resource(sub, "graph.bin"), "rb").read()
    log = ctypes.create_string_buffer(8192)
    stats = (ctypes.c_uint64 * 8)()
    failures = SR.sharedrows_check(zb, len(zb), gb, len(gb), (ctypes.c_uint32 * len(eq))(*eq), len(eq),
                                   (ctypes.c_uint32 * len(opp))(*opp), len(opp), SEED, log, len(log), stats)
    assert failures == 0, (failures, SR.sharedrows_error().decode() if failures < 0 else log.value.decode())
    n_eq, n_opp, table_rows, family_rows, plans, pair_chunks, singles, identities = list(stats)
    assert (n_eq, n_opp) == EXPECT[sub][:2]
    assert family_rows == table_rows - n_eq - n_opp and plans == 4 and pair_chunks > 0 and identities == 12
    # A_i and B1_i of a wire are each other's pair partner: without the B1 row the A row is a single row of a paired table
    assert singles == n_eq + n_opp
    print("%s: %d + %d shared wires, %d of %d table rows walked" % (sub, n_eq, n_opp, family_rows, table_rows))


@pytest.mark.parametrize("sub", sorted(EXPECT))
def test_the_legacy_families_and_the_points_did_not_move(SR, sub):
    zb, gb = open(_resource(sub, "rln_final.arkzkey"), "rb").read(), open(_resource(sub, "graph.bin"), "rb").read()
    out = ctypes.c_uint64()
    assert SR.sharedrows_legacy_checksum(zb, len(zb), gb, len(gb), ctypes.byref(out)) == 0, SR.sharedrows_error().decode()
    assert out.value == EXPECT[sub][2], hex(out.value)


def test_the_same_checks_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (tests/host/sharedrows_main.cpp) built with the sanitizers and run as a child process, once
    per key"""
    exe = str(tmp_path / "sharedrows_asan")
    san = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    objs, jobs = [], []
    for src in [os.path.join(HOST, "sharedrows_main.cpp")] + SRCS:       # the units side by side: most of the test is this build
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        jobs.append(subprocess.Popen(san + FLAGS + ["-c", src, "-o", objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    subprocess.check_call(san + objs + ["-o", exe])
    runs = {}
    for sub in sorted(EXPECT):
        eq, opp, _, _ = wires(sub)
        path = str(tmp_path / (sub + ".wires"))
        with open(path, "wb") as f:
            f.write(struct.pack("<2I", len(eq), len(opp)) + struct.pack("<%dI" % (len(eq) + len(opp)), *(eq + opp)))
        runs[sub] = subprocess.Popen([exe, _resource(sub, "rln_final.arkzkey"), _resource(sub, "graph.bin"), path, str(SEED)],
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for sub, r in runs.items():
        out, err = r.communicate(timeout=600)
        want = "ok %d %d 4 12 %016x\n" % (EXPECT[sub][0], EXPECT[sub][1], EXPECT[sub][2])
        assert r.returncode == 0 and out == want, (sub, out[-2000:], err[-2000:])
