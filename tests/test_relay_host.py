"""The relay step's per-item logic (zerokit_amd/csrc/relay.h: what k_relay_gate, k_relay_emit and k_relay_fold inline),
built for the CPU and run in the device's order of passes (tests/host/relay.cpp), judged by the model of
tests/relay_cases.py; the same cases through a stand-alone sanitizer program; and the argument checks of
rlnamd_relay_step, which come before anything touches a device.  No GPU needed."""
import ctypes
import os
import struct
import subprocess

import pytest

import relay_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
U64P = ctypes.POINTER(ctypes.c_uint64)
CP = ctypes.c_char_p


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "librelayhost.so")
    src = os.path.join(HOST, "relay.cpp")
    deps = [src, os.path.join(HOST, "nullifierlog.cpp")] + \
        [os.path.join(CSRC, h) for h in ("relay.h", "nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.nl_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.nl_new.restype = ctypes.c_void_p
    lib.nl_free.argtypes = [ctypes.c_void_p]
    lib.nl_free.restype = None
    lib.nl_info.argtypes = [ctypes.c_void_p, U64P]
    lib.nl_info.restype = None
    lib.nl_check_table.argtypes = [ctypes.c_void_p]
    lib.nl_check_table.restype = ctypes.c_int64
    lib.rl_step.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t, CP, CP, CP, CP, ctypes.c_size_t,
                            U64P, CP, CP, CP, U64P]
    lib.rl_step.restype = ctypes.c_int
    lib.rl_get.argtypes = [ctypes.c_void_p, ctypes.c_uint64, CP, U64P]
    lib.rl_get.restype = None
    lib.rl_check.argtypes = [ctypes.c_size_t, CP, CP, CP, U64P, CP, CP, ctypes.c_size_t, CP, CP]
    lib.rl_check.restype = CP
    return lib


def step(L, log, k, rows, ok, xs, roots, tags):
    n = len(rows)
    verdict, status = ctypes.create_string_buffer(max(n, 1)), ctypes.create_string_buffer(max(n, 1))
    secrets = ctypes.create_string_buffer(max(32 * n, 1))
    first = (ctypes.c_uint64 * max(n, 1))()
    tg = None if tags is None else (ctypes.c_uint64 * max(n, 1))(*tags)
    rc = L.rl_step(log, k, cases.n_values(k), n, cases.pack_rows(rows), bytes(ok), cases.pack_frs(xs), cases.pack_frs(roots),
                   len(roots), tg, verdict, status, secrets, first)
    return rc, (list(verdict.raw[:n]), list(status.raw[:n]),
                [int.from_bytes(secrets.raw[32 * i:32 * i + 32], "little") for i in range(n)], list(first[:n]))


def records(L, log):
    info = (ctypes.c_uint64 * 4)()
    L.nl_info(log, info)
    out = []
    for row in range(info[1]):
        share, tag = ctypes.create_string_buffer(128), ctypes.c_uint64()
        L.rl_get(log, row, share, ctypes.byref(tag))
        out.append((tuple(int.from_bytes(share.raw[32 * j:32 * j + 32], "little") for j in range(4)), tag.value))
    return out


def run(L, k, chunk, n_roots, tagged=True, n=None):
    c = cases.messages(k)
    n = len(c["rows"]) if n is None else n
    rows, ok, xs, roots = c["rows"][:n], c["ok"][:n], c["xs"][:n], c["roots"][:n_roots]
    tags = c["tags"][:n] if tagged else None
    want = cases.model(rows, ok, xs, roots, tags, k, {}, 0)
    log = L.nl_new(4 * n, 17)
    try:
        got = ([], [], [], [])
        for o in range(0, n, chunk):
            rc, part = step(L, log, k, rows[o:o + chunk], ok[o:o + chunk], xs[o:o + chunk], roots,
                            None if tags is None else tags[o:o + chunk])
            assert rc == 0
            got = tuple(a + b for a, b in zip(got, part))
        assert got == tuple(want[:4])
        assert records(L, log) == list(zip(want[4], want[5]))
        assert L.nl_check_table(log) == len(set(s[0] for s in want[4]))
    finally:
        L.nl_free(log)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("chunk", [2000, 1, 63, 1000])
def test_step_matches_the_model_whatever_the_split(L, k, chunk):
    run(L, k, chunk, 64)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n_roots", [0, 1])
def test_no_root_accepts_any_and_one_root_only_itself(L, k, n_roots):
    run(L, k, 2000, n_roots)


@pytest.mark.parametrize("k", [1, 4])
def test_without_tags_a_share_is_tagged_with_its_sequence_number(L, k):
    run(L, k, 257, 64, tagged=False, n=600)


def test_hand_made_multi_rows(L):
    """max_out 4: a SPAM in slot 2 beside a NEW in slot 0 returns slot 2's secret; a proof with no used slot is accepted,
    SKIPPED and records nothing; a selector element of 2 is a bad proof whatever the other checks say"""
    R, k = cases.R, 4
    a0, a1 = 1234567, [11, 22, 33, 44, 55]
    nul = [101, 102, 103, 104, 105]
    ext, root = 77, 9

    def row(x, ids, sel, root=root):
        return cases.join([(a0 + x * a1[j]) % R for j in ids], root, [nul[j] for j in ids], x, ext, sel, k)

    rows = [row(5, [0, 1, 2, 3], [1, 0, 0, 0]),          # NEW: id 0
            row(6, [4, 1, 0, 3], [1, 0, 1, 0]),          # slot 0: id 4 NEW; slot 2: id 0 under another x: SPAM
            row(7, [0, 1, 2, 3], [0, 0, 0, 0]),          # no used slot
            row(8, [0, 1, 2, 3], [1, 2, 0, 0]),          # a selector of 2
            row(8, [0, 1, 2, 3], [1, 2, 0, 0], root=10),  # ... with a bad root and a bad signal as well
            row(5, [0, 1, 2, 3], [1, 1, 0, 0])]          # slot 0 a DUPLICATE, slot 1 NEW: DUPLICATE speaks first
    xs = [5, 6, 7, 8, 1, 5]
    tags = [10, 11, 12, 13, 14, 15]
    log = L.nl_new(64, 3)
    try:
        rc, got = step(L, log, k, rows, [1] * 6, xs, [root], tags)
        assert rc == 0
        assert got[0] == [cases.OK, cases.OK, cases.OK, cases.BAD_PROOF, cases.BAD_PROOF, cases.OK]
        assert got[1] == [cases.NEW, cases.SPAM, cases.SKIPPED, cases.SKIPPED, cases.SKIPPED, cases.DUPLICATE]
        assert got[2] == [0, a0, 0, 0, 0, 0]
        assert got[3] == [10, 10, 0, 0, 0, 10]
        assert [t for _s, t in records(L, log)] == [10, 11, 11, 15, 15]
        assert got == tuple(cases.model(rows, [1] * 6, xs, [root], tags, k, {}, 0)[:4])
    finally:
        L.nl_free(log)


def test_verdict_precedence_on_hand_made_single_rows(L):
    """proof before root before signal, every pair and all three"""
    good = [3, 9, 100, 5, 77]   # y, root, nullifier, x, ext
    bad_root = [3, 8, 100, 5, 77]
    rows = [good, good, bad_root, good, bad_root, bad_root, good, bad_root]
    ok = [1, 0, 1, 1, 0, 1, 0, 0]
    xs = [5, 5, 5, 6, 5, 6, 6, 6]
    log = L.nl_new(16, 3)
    try:
        rc, got = step(L, log, 1, rows, ok, xs, [9], None)
        assert rc == 0
        assert got[0] == [cases.OK, cases.BAD_PROOF, cases.BAD_ROOT, cases.BAD_SIGNAL, cases.BAD_PROOF, cases.BAD_ROOT,
                          cases.BAD_PROOF, cases.BAD_PROOF]
        assert got[1] == [cases.NEW] + [cases.SKIPPED] * 7
        assert len(records(L, log)) == 1
    finally:
        L.nl_free(log)


def test_refusals_of_the_host_step(L):
    c = cases.messages(4)
    log = L.nl_new(40, 3)
    try:
        # 11 messages of up to 4 shares do not fit 40 records, 10 do; neither 7 values nor 3 slots are a layout
        assert step(L, log, 4, c["rows"][:11], c["ok"][:11], c["xs"][:11], (), None)[0] == 1
        info = (ctypes.c_uint64 * 4)()
        L.nl_info(log, info)
        assert info[1] == 0 and L.nl_check_table(log) == 0
        assert step(L, log, 4, c["rows"][:10], c["ok"][:10], c["xs"][:10], (), None)[0] == 0
        one = ctypes.create_string_buffer(32 * 16)
        assert L.rl_step(log, 3, 15, 1, one, one, one, None, 0, None, one, one, None, None) == 2
        assert L.rl_step(log, 1, 7, 1, one, one, one, None, 0, None, one, one, None, None) == 2
    finally:
        L.nl_free(log)


CHECKS = [  # (proofs, values, signals, offsets, xs, roots, n_roots, verdict, status) present?, the text
    ((0, 1, 0, 0, 1, 0, 0, 1, 1), "relay step: null pointer for n > 0 messages"),
    ((1, 0, 0, 0, 1, 0, 0, 1, 1), "relay step: null pointer for n > 0 messages"),
    ((1, 1, 0, 0, 1, 0, 0, 0, 1), "relay step: null pointer for n > 0 messages"),
    ((1, 1, 0, 0, 1, 0, 0, 1, 0), "relay step: null pointer for n > 0 messages"),
    ((1, 1, 0, 0, 1, 1, 65, 1, 1), "relay step: at most 64 roots (RLNAMD_RELAY_ROOTS_MAX)"),
    ((1, 1, 0, 0, 1, 0, 3, 1, 1), "relay step: null roots for n_roots > 0"),
    ((1, 1, 1, 1, 1, 0, 0, 1, 1), "relay step: both signals and xs_le were given, a step takes one of them"),
    ((1, 1, 0, 1, 1, 0, 0, 1, 1), "relay step: both signals and xs_le were given, a step takes one of them"),
    ((1, 1, 0, 0, 0, 0, 0, 1, 1), "relay step: neither signals nor xs_le were given"),
    ((1, 1, 1, 1, 0, 1, 64, 1, 1), ""),
    ((1, 1, 0, 0, 1, 0, 0, 1, 1), ""),
]


def _check_args(have):
    buf = ctypes.create_string_buffer(32 * 65)
    off = (ctypes.c_uint64 * 2)(0, 0)
    p = lambda i: buf if have[i] else None
    return (p(0), p(1), p(2), off if have[3] else None, p(4), p(5), have[6], p(7), p(8))


def test_argument_checks_of_the_header(L):
    for have, text in CHECKS:
        a = _check_args(have)
        assert L.rl_check(1, *a).decode() == text, have
    assert L.rl_check(0, *([None] * 6), 99, None, None) == b""   # n = 0: nothing is looked at


def test_rlnamd_relay_step_checks_its_arguments_before_the_device():
    """the same texts through the C ABI, with no relay behind the handle: what needs no object is refused before the
    handle is followed, and a null relay is an error of its own"""
    from zerokit_amd._native import last_error, lib
    F = lib().rlnamd_relay_step

    def call(n, a, relay=None):
        first = (ctypes.c_uint64 * 1)()
        return F(relay, n, a[0], a[1], 5, a[2], 0, a[3], a[4], a[5], a[6], None, a[7], a[8], None, first)

    for have, text in CHECKS:
        rc = call(1, _check_args(have))
        assert rc != 0 and last_error() == (text or "rlnamd_relay_step: null relay"), have
    assert call(0, [None] * 6 + [0, None, None]) != 0 and last_error() == "rlnamd_relay_step: null relay"
    out = (ctypes.c_uint64 * 8)()
    assert lib().rlnamd_relay_info(None, out) != 0 and last_error() == "rlnamd_relay_info: null pointer"
    h = ctypes.c_void_p()
    assert lib().rlnamd_relay_new(None, None, None, 0, ctypes.byref(h)) != 0 and last_error() == "rlnamd_relay_new: null pointer"


def test_relay_header_under_asan_and_ubsan(L, tmp_path):
    """a stand-alone program of its own (tests/host/relay_main.cpp), built with the sanitizers and run as a child process
    on the single and the multi cases: one call and calls of 1, 63 and 1 000"""
    exe = str(tmp_path / "relay_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "relay_main.cpp"), "-o", exe])
    for k in (1, 4):
        c = cases.messages(k)
        n = len(c["rows"])
        want = cases.model(c["rows"], c["ok"], c["xs"], c["roots"], c["tags"], k, {}, 0)
        path = str(tmp_path / ("case%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<8Q", k, cases.n_values(k), n, 64, 4 * n, 23, 0, 0))
            f.write(cases.pack_rows(c["rows"]) + bytes(c["ok"]) + cases.pack_frs(c["xs"]) + cases.pack_frs(c["roots"]))
            f.write(struct.pack("<%dQ" % n, *c["tags"]))
            f.write(bytes(want[0]) + bytes(want[1]) + cases.pack_frs(want[2]) + struct.pack("<%dQ" % n, *want[3]))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "ok %d\n" % (4 * n), (r.stdout, r.stderr[-2000:])


def test_ffi_relay_step_checks_its_arguments_before_the_device():
    """the drop-in entries: n = 0 succeeds and looks at nothing; null arrays, a null object and a null log are refused, each
    with its own text, before anything is followed (the pattern of tests/test_members_host.py)"""
    from zerokit_amd._native import VecU8, lib
    from zerokit_amd.public import _err
    for name in ("ffi_relay_step", "ffi_rln_v3_relay_step"):
        F = getattr(lib(), name)

        def call(rln, log, proofs, n, signals, verdict, status):
            r = F(rln, log, proofs, n, signals, None, None, verdict, status, None, None)
            return bool(r.ok), (_err(r.err) if r.err.ptr else "")

        one = (ctypes.c_void_p * 1)(64)
        sig = (VecU8 * 1)(VecU8(None, 0, 0))
        out = ctypes.create_string_buffer(1)
        dummy, null_handle = ctypes.c_void_p(64), ctypes.c_void_p(None)
        assert call(None, None, None, 0, None, None, None) == (True, "")
        for hole in range(4):
            args = [one, sig, out, out]
            args[hole] = None
            assert call(ctypes.byref(dummy), dummy, args[0], 1, args[1], args[2], args[3]) == (False, "relay step: null argument"), hole
        assert call(None, dummy, one, 1, sig, out, out) == (False, "relay step: null RLN object")
        assert call(ctypes.byref(null_handle), dummy, one, 1, sig, out, out) == (False, "relay step: null RLN object")
