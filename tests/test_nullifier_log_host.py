"""The nullifier log's insert and judge passes (zerokit_amd/csrc/nullifier_log.h: what k_log_insert and k_log_judge
inline), built for the CPU and judged by the model of tests/nullifier_log_cases.py: on one thread over the sequential
policy, on 8 std::threads over the std::atomic policy, and in two stand-alone sanitizer programs.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

import nullifier_log_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
U64P = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libnullifierlog.so")
    src = os.path.join(HOST, "nullifierlog.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.nl_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.nl_new.restype = ctypes.c_void_p
    lib.nl_free.argtypes = [ctypes.c_void_p]
    lib.nl_free.restype = None
    lib.nl_observe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, U64P, ctypes.c_char_p, ctypes.c_char_p,
                               U64P, ctypes.c_int]
    lib.nl_observe.restype = ctypes.c_int
    lib.nl_home_slot.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.nl_home_slot.restype = ctypes.c_uint64
    lib.nl_info.argtypes = [ctypes.c_void_p, U64P]
    lib.nl_info.restype = None
    lib.nl_check_table.argtypes = [ctypes.c_void_p]
    lib.nl_check_table.restype = ctypes.c_int64
    return lib


def observe(L, log, shares, tags, threads):
    n = len(shares)
    status = ctypes.create_string_buffer(max(n, 1))
    secrets = ctypes.create_string_buffer(max(32 * n, 1))
    first = (ctypes.c_uint64 * max(n, 1))()
    tg = (ctypes.c_uint64 * max(n, 1))(*tags)
    rc = L.nl_observe(log, n, cases.pack(shares), tg, status, secrets, first, threads)
    return rc, (status.raw[:n], secrets.raw[:32 * n], list(first[:n]))


def run_stream(L, chunk, threads, seed, capacity=4096):
    shares, tags, _ = cases.stream()
    log = L.nl_new(capacity, seed)
    try:
        got = (b"", b"", [])
        for o in range(0, len(shares), chunk):
            rc, part = observe(L, log, shares[o:o + chunk], tags[o:o + chunk], threads)
            assert rc == 0
            got = tuple(a + b for a, b in zip(got, part))
        info = (ctypes.c_uint64 * 4)()
        L.nl_info(log, info)
        return got, L.nl_check_table(log), list(info)
    finally:
        L.nl_free(log)


@pytest.mark.parametrize("chunk", [4096, 1, 63, 1000])
def test_sequential_policy_matches_the_model(L, chunk):
    want = cases.expected()
    got, taken, info = run_stream(L, chunk, 0, seed=11)
    assert got == cases.flat(want)
    # one slot per key, every key reachable from its home slot without an empty slot on the way
    assert taken == sum(1 for w in want if w[0] == cases.NEW)
    assert info[:3] == [4096, 4096, 8192] and 1 <= info[3] <= 8192


def test_threads_insert_concurrently_and_agree_with_the_model_every_time(L):
    """8 std::threads over the std::atomic policy, share i in the hands of thread i mod 8, one call of 4 096 shares,
    50 times over (a fresh log and another seed each time: other collisions)"""
    want = cases.flat(cases.expected())
    distinct = sum(1 for w in cases.expected() if w[0] == cases.NEW)
    for rep in range(50):
        got, taken, _ = run_stream(L, 4096, 8, seed=100 + rep)
        assert got == want, rep
        assert taken == distinct, rep


def test_slots_home_slot_and_refusals(L):
    for capacity, slots in ((1, 16), (8, 16), (9, 32), (16, 32), (1000, 2048), (1024, 2048), (1025, 4096)):
        log = L.nl_new(capacity, 3)
        info = (ctypes.c_uint64 * 4)()
        L.nl_info(log, info)
        assert info[2] == slots
        L.nl_free(log)
    shares, tags, _ = cases.stream()
    a, b = L.nl_new(64, 1), L.nl_new(64, 2)
    try:
        keys = [s[0].to_bytes(32, "little") for s in shares[:200]]
        ha, hb = [L.nl_home_slot(a, k) for k in keys], [L.nl_home_slot(b, k) for k in keys]
        assert all(h < 128 for h in ha + hb) and ha != hb and len(set(ha)) > 64   # spread, and moved by the seed
        assert [L.nl_home_slot(a, k) for k in keys] == ha
        # a call that does not fit, and a field element >= r, leave the log as it was
        assert observe(L, a, shares[:65], tags[:65], 0)[0] == 1
        bad = list(shares[:3])
        bad[1] = (bad[1][0], cases.R, bad[1][2], bad[1][3])
        packed = b"".join(int(v).to_bytes(32, "little") for s in bad for v in s)
        st = ctypes.create_string_buffer(3)
        assert L.nl_observe(a, 3, packed, None, st, None, None, 0) == 2
        info = (ctypes.c_uint64 * 4)()
        L.nl_info(a, info)
        assert info[1] == 0 and L.nl_check_table(a) == 0
        rc, got = observe(L, a, shares[:64], tags[:64], 0)
        assert rc == 0 and got == cases.flat(cases.model(shares[:64], tags[:64]))
    finally:
        L.nl_free(a)
        L.nl_free(b)


def _sanitizer_program(tmp_path, name, sanitize, args):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "nullifierlog_main.cpp"), "-o", exe])
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])


def test_log_header_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/nullifierlog_main.cpp), built with the sanitizers and run once"""
    _sanitizer_program(tmp_path, "nullifierlog_asan", "address,undefined", [])


def test_threaded_insert_under_tsan(tmp_path):
    """the same program built with -fsanitize=thread, running its threaded case once"""
    _sanitizer_program(tmp_path, "nullifierlog_tsan", "thread", ["threads"])
