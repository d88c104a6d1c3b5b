"""The quota ledger on the CPU: the sequential text of zerokit_amd/csrc/quota_ledger.h (tests/host/quota.cpp, built with
g++ and loaded with ctypes) held to the dict model of tests/quota_cases.py; the same cases through a stand-alone
sanitizer program; the refusal texts, which come before anything touches a device; and the model itself checked for the
split property.  No GPU needed."""
import ctypes
import itertools
import os
import struct
import subprocess

import pytest

import quota_cases as cases
from quota_cases import E1, E2, E3, E4, OUTSIDE, NO_EPOCH, OK, OVER, U32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
CP = ctypes.c_char_p
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
DEPTH = 20
LAST = (1 << DEPTH) - 1


def pack(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libquotahost.so")
    src = os.path.join(HOST, "quota.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("quota_ledger.h", "nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.ql_new.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.ql_new.restype = ctypes.c_void_p
    lib.ql_free.argtypes = [ctypes.c_void_p]
    lib.ql_free.restype = None
    lib.ql_last.restype = CP
    lib.ql_new_refusal.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.ql_new_refusal.restype = CP
    lib.ql_epochs_refusal.argtypes = [CP, ctypes.c_size_t, ctypes.c_size_t]
    lib.ql_epochs_refusal.restype = CP
    lib.ql_draw_refusal.argtypes = [ctypes.c_size_t, U64P, CP, U32P, U32P, CP, ctypes.c_uint32]
    lib.ql_draw_refusal.restype = CP
    lib.ql_set_epochs.argtypes = [ctypes.c_void_p, CP, ctypes.c_size_t]
    lib.ql_epochs.argtypes = [ctypes.c_void_p, CP]
    lib.ql_epochs.restype = ctypes.c_size_t
    lib.ql_draw.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, U32P, CP]
    lib.ql_used.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, CP]
    lib.ql_used.restype = None
    lib.ql_info.argtypes = [ctypes.c_void_p, U64P]
    lib.ql_info.restype = None
    lib.ql_plan.argtypes = [ctypes.c_size_t, ctypes.c_uint32, U64P]
    lib.ql_plan.restype = None
    return lib


class HostLedger:
    """quota.cpp's ledger with the methods of zerokit_amd.batch.QuotaLedger"""

    def __init__(self, L, depth, max_epochs):
        self.L, self.h = L, L.ql_new(depth, max_epochs)
        assert self.h

    def close(self):
        self.L.ql_free(self.h)

    def set_epochs(self, exts):
        if self.L.ql_set_epochs(self.h, pack(exts), len(exts)) != 0:
            raise cases.Refused(self.L.ql_last().decode())

    def epochs(self):
        out = ctypes.create_string_buffer(32 * 64)
        k = self.L.ql_epochs(self.h, out)
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(k)]

    def draw(self, leaves, exts, limits):
        n = len(leaves)
        ids, status = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        if self.L.ql_draw(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0",
                          (ctypes.c_uint32 * max(n, 1))(*limits), ids, status) != 0:
            raise cases.Refused(self.L.ql_last().decode())
        return list(ids[:n]), list(status.raw[:n])

    def used(self, leaves, exts):
        n = len(leaves)
        out, inside = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        self.L.ql_used(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0", out, inside)
        return [int(out[i]) if inside.raw[i] else None for i in range(n)]

    def info(self):
        out = (ctypes.c_uint64 * 6)()
        self.L.ql_info(self.h, out)
        return list(out)


# ---------------------------------------------------------------------------------------------- the model itself
def test_the_model_has_the_split_property_with_one_limit_per_member():
    """one call over n requests = every split of it into two consecutive calls = drawing one by one, n <= 12.
    Exhaustive in the split points: all n + 1 of every sequence.  Exhaustive in the sequences over an alphabet of
    request kinds that shrinks as n grows, so that the count stays in the tens of thousands: four kinds (4^n sequences)
    up to n = 6, two kinds (2^n: one member that runs out and one that does not, the pair that decides the property)
    for n = 7 .. 12.  Beyond that alphabet, 120 seeded sequences per n = 7 .. 12 over four members, two open epochs and
    one outside the window: those are samples, not an enumeration."""
    def sequences(n):
        # (member, external nullifier, its limit)
        kinds = [(0, E1, 0), (1, E1, 1), (2, E1, 2), (1, OUTSIDE, 1)] if n <= 6 else [(3, E1, 4), (2, E1, 2)]
        for seq in itertools.product(kinds, repeat=n):
            yield [s[0] for s in seq], [s[1] for s in seq], [s[2] for s in seq]
        if n > 6:
            yield from cases.split_sequences(n, 120, n)

    def fresh():
        m = cases.Model(4, 2)
        m.set_epochs([E1, E2])
        m.draw([2, 1], [E1, E2], [2, 1])      # not from zero
        return m
    checked = 0
    for n in range(1, 13):
        for leaves, exts, limits in sequences(n):
            whole = fresh()
            want = whole.draw(leaves, exts, limits)
            single = fresh()
            assert single.draw_one_by_one(leaves, exts, limits) == want and single.used == whole.used
            for cut in range(n + 1):
                m = fresh()
                a = m.draw(leaves[:cut], exts[:cut], limits[:cut])
                b = m.draw(leaves[cut:], exts[cut:], limits[cut:])
                assert (a[0] + b[0], a[1] + b[1]) == want and m.used == whole.used, (leaves, exts, limits, cut)
                checked += 1
    assert checked > 130000


def test_the_model_with_two_limits_skips_but_never_repeats():
    m = cases.Model(DEPTH, 1)
    m.set_epochs([E1])
    assert m.draw([7] * 6, [E1] * 6, [1, 5, 1, 5, 5, 1]) == ([0, 1, 1, 3, 4, 1], [OK, OK, OVER, OK, OK, OVER])   # 2 is skipped
    assert m.used[(E1, 7)] == 5
    assert m.draw([7, 7], [E1, E1], [9, 5]) == ([5, 5], [OK, OVER]) and m.used[(E1, 7)] == 6


# --------------------------------------------------------------------------------------- the header's sequential text
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 2000])
def test_host_draws_equal_the_model(L, n):
    q, m = HostLedger(L, DEPTH, 4), cases.Model(DEPTH, 4)
    try:
        q.set_epochs([E1, E2, E3])
        m.set_epochs([E1, E2, E3])
        keys = []
        for leaves, exts, limits in cases.draw_shapes(n):
            cases.compare_draw(m, q, leaves, exts, limits)
            keys += list(zip(exts, leaves))
        cases.compare_counters(m, q, keys)
        assert q.info() == [3, m.draws, m.issued, m.over, m.no_epoch, 0]
        q.set_epochs([E4])
        ids, status = q.draw([5] * n, [E4] * n, [n // 2] * n)
        assert status == [OK] * (n // 2) + [OVER] * (n - n // 2) and ids[:n // 2] == list(range(n // 2))
        assert q.used([5], [E4]) == [n // 2] and q.info()[5] == 0
    finally:
        q.close()


@pytest.mark.parametrize("depth", [1, 9, 24])
def test_host_edge_leaves_and_depths(L, depth):
    last = (1 << depth) - 1
    q, m = HostLedger(L, depth, 3), cases.Model(depth, 3)
    try:
        q.set_epochs([E1, E2, E3])
        m.set_epochs([E1, E2, E3])
        leaves = [0, last, last, 0, 0, last, 0] * 11
        exts = [E1, E3, E1, E3, OUTSIDE, E2, E1] * 11
        for limits in ([3] * 77, [U32] * 77, [0] * 77):
            cases.compare_draw(m, q, leaves, exts, limits)
        cases.compare_counters(m, q, [(e, leaf) for e in (E1, E2, E3, OUTSIDE) for leaf in (0, last)])
    finally:
        q.close()


def test_host_two_limits_and_the_window(L):
    q, m = HostLedger(L, DEPTH, 3), cases.Model(DEPTH, 3)
    try:
        for impl in (q, m):
            impl.set_epochs([E1, E2])
        for leaves, exts, limits in cases.two_limits() * 2:
            cases.compare_draw(m, q, leaves, exts, limits)
        cases.compare_draw(m, q, [0, 0, LAST, 5], [E1, E1, E2, E2], [9] * 4)
        for impl in (q, m):
            impl.set_epochs([E3, E2, E3])
        assert q.epochs() == m.window == [E3, E2] and q.info()[5] == 0
        assert q.used([0, LAST, 5, 0, 7], [E3, E2, E2, E1, E3]) == [0, 1, 1, None, 0]
        cases.compare_draw(m, q, [0, LAST, 0, 3], [E3, E2, E1, E3], [9] * 4)
        cases.compare_counters(m, q, [(E3, 0), (E2, LAST), (E1, 0), (E3, 3), (E1, 7)])
        for impl in (q, m):
            impl.set_epochs([])
        assert q.epochs() == [] and q.draw([0], [E2], [9]) == ([9], [NO_EPOCH]) and q.info()[5] == 0
    finally:
        q.close()


def test_host_plan_is_the_librarys(L):
    from zerokit_amd.batch import QuotaLedger
    for depth in (1, 8, 9, 16, 17, 24):
        for n in (1, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1):
            out = (ctypes.c_uint64 * 4)()
            L.ql_plan(n, depth, out)
            assert tuple(out) == QuotaLedger.plan(n, depth)
    assert QuotaLedger.plan(65537, 20) == (4, 257, 3, 3) and QuotaLedger.plan(256, 8) == (2, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------ refusals
NEW_REFUSALS = [(0, 1), (25, 1), (10, 0), (10, 65), (1, 1), (24, 64)]
EPOCHS_REFUSALS = [   # (elements or None for a null pointer, k, max_epochs)
    (None, 1, 4), ([E1] * 5, 5, 4), ([E1, cases.R], 2, 4), ([cases.R + 1], 1, 1), ([E1] * 65, 65, 64), (None, 0, 4), ([E1, E1], 2, 2),
]


def test_refusal_texts_of_the_header(L):
    for depth, max_epochs in NEW_REFUSALS:
        assert L.ql_new_refusal(depth, max_epochs).decode() == cases.new_refusal(depth, max_epochs)
    assert cases.new_refusal(1, 1) == cases.new_refusal(24, 64) == ""
    for exts, k, max_epochs in EPOCHS_REFUSALS:
        m = cases.Model(4, max_epochs)
        want = m.epochs_refusal(exts or [0] * k, pointers=exts is not None)
        assert L.ql_epochs_refusal(None if exts is None else pack(exts), k, max_epochs).decode() == want, (k, max_epochs)
    m = cases.Model(10, 1)
    ids, st = (ctypes.c_uint32 * 3)(), ctypes.create_string_buffer(3)
    leaf, lim = (ctypes.c_uint64 * 3)(0, 1024, 1), (ctypes.c_uint32 * 3)(5, 5, 5)
    assert L.ql_draw_refusal(3, leaf, b"\0" * 96, lim, ids, st, 10).decode() == m.draw_refusal([0, 1024, 1]) != ""
    assert L.ql_draw_refusal(3, leaf, b"\0" * 96, lim, ids, st, 11).decode() == ""
    assert L.ql_draw_refusal(3, None, b"\0" * 96, lim, ids, st, 10).decode() == m.draw_refusal([0], pointers=False)
    assert L.ql_draw_refusal(1 << 32, leaf, b"\0" * 96, lim, ids, st, 10).decode() == \
        "quota ledger: a draw takes fewer than 2^32 requests, not 4294967296"
    assert L.ql_draw_refusal(0, None, None, None, None, None, 10).decode() == ""


def test_refused_calls_leave_the_host_ledger_as_it_was(L):
    q = HostLedger(L, 10, 2)
    try:
        q.set_epochs([E1, E2])
        q.draw([0, 1023, 0], [E1, E2, E1], [5, 5, 5])
        before = (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info())
        for exts in ([E1, E2, E3], [E3, cases.R]):
            with pytest.raises(cases.Refused):
                q.set_epochs(exts)
        with pytest.raises(cases.Refused):
            q.draw([0, 1024], [E1, E1], [5, 5])
        assert (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info()) == before
    finally:
        q.close()


def test_the_c_abi_refuses_before_it_touches_a_device():
    """the same texts through rlnamd_quota_* with no object behind the handle and no device asked for"""
    from zerokit_amd._native import last_error, lib
    out = ctypes.c_void_p()
    for depth, max_epochs in NEW_REFUSALS:
        if cases.new_refusal(depth, max_epochs):
            assert lib().rlnamd_quota_new(depth, max_epochs, ctypes.byref(out)) != 0 and not out.value
            assert last_error() == cases.new_refusal(depth, max_epochs)
    for exts, k, max_epochs in EPOCHS_REFUSALS:
        if max_epochs != 64 and exts is not None and k > max_epochs:
            continue                      # without an object the bound is the largest a ledger can have
        want = cases.Model(4, 64).epochs_refusal(exts or [0] * k, pointers=exts is not None)
        assert lib().rlnamd_quota_set_epochs(None, None if exts is None else pack(exts), k) != 0
        assert last_error() == (want or "rlnamd_quota_set_epochs: null ledger"), k
    ids, st = (ctypes.c_uint32 * 2)(), ctypes.create_string_buffer(2)
    leaf, lim = (ctypes.c_uint64 * 2)(0, 1 << 24), (ctypes.c_uint32 * 2)(5, 5)
    assert lib().rlnamd_quota_draw(None, 2, leaf, b"\0" * 64, lim, ids, st) != 0
    assert last_error() == "quota ledger: leaf index 16777216 of request 1 is outside a ledger of depth 24"
    assert lib().rlnamd_quota_draw(None, 2, leaf, None, lim, ids, st) != 0
    assert last_error() == "quota ledger: draw was given a null pointer for n > 0 requests"
    assert lib().rlnamd_quota_draw(None, 0, None, None, None, None, None) != 0 and last_error() == "rlnamd_quota_draw: null ledger"
    k = ctypes.c_size_t()
    assert lib().rlnamd_quota_epochs(None, None, ctypes.byref(k)) != 0 and last_error() == "rlnamd_quota_epochs: null pointer"
    assert lib().rlnamd_quota_info(None, None) != 0 and last_error() == "rlnamd_quota_info: null pointer"
    lib().rlnamd_quota_free(None)


def test_python_names():
    from zerokit_amd import batch
    assert (batch.QuotaLedger.OK, batch.QuotaLedger.OVER, batch.QuotaLedger.NO_EPOCH) == (OK, OVER, NO_EPOCH)
    assert batch.QuotaLedger.EPOCHS_MAX == batch.Relay.EPOCHS_MAX == 64
    for name in ("set_epochs", "epochs", "draw", "info", "used", "plan"):
        assert callable(getattr(batch.QuotaLedger, name))


# ------------------------------------------------------------------------------------------ the sanitizer program
def test_the_ledger_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/quota_main.cpp), built with the sanitizers and run as a child
    process: the cases above as one file of steps with the model's answers"""
    exe = str(tmp_path / "quota_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "quota_main.cpp"), "-o", exe])
    depth, max_epochs = 12, 3
    last = (1 << depth) - 1
    m = cases.Model(depth, max_epochs)
    steps, judged = [], 0

    def set_epochs(exts):
        refused = 1 if m.epochs_refusal(exts) else 0
        if not refused:
            m.set_epochs(exts)
        steps.append(struct.pack("<2Q", 0, len(exts)) + pack(exts) + struct.pack("<Q", refused))

    def draw(leaves, exts, limits):
        nonlocal judged
        ids, status = m.draw(leaves, exts, limits)
        n = len(leaves)
        steps.append(struct.pack("<2Q", 1, n) + struct.pack("<%dQ" % n, *leaves) + pack(exts) + struct.pack("<%dI" % n, *limits) +
                     struct.pack("<%dI" % n, *ids) + bytes(status))
        judged += n

    def counters(keys):
        nonlocal judged
        keys = sorted(set(keys))
        n = len(keys)
        inside = [k[0] in m.window for k in keys]
        want = [m.used.get(k, 0) if i else 0 for k, i in zip(keys, inside)]
        steps.append(struct.pack("<2Q", 2, n) + struct.pack("<%dQ" % n, *[k[1] for k in keys]) + pack([k[0] for k in keys]) +
                     struct.pack("<%dI" % n, *want) + bytes(inside))
        judged += n

    set_epochs([E1, E2, E3])
    keys = []
    for n in (1, 63, 64, 65, 256, 257):
        for leaves, exts, limits in cases.draw_shapes(n, depth):
            draw(leaves, exts, limits)
            keys += list(zip(exts, leaves))
    counters(keys)
    set_epochs([E1, E2, E3, E4])          # refused: four for a window of three
    set_epochs([E4, E2, E4])              # E1 and E3 leave, E4 takes a slot that was just zeroed
    for leaves, exts, limits in cases.two_limits():
        draw(leaves, [E4] * len(leaves), limits)
    draw([0, last, 0, last], [E4, E2, E1, E2], [U32, 0, 5, U32])
    counters(keys + [(E4, 7), (E4, 9), (E4, 0), (E2, last), (E1, 0)])
    set_epochs([])
    counters(keys[:50])
    path = str(tmp_path / "steps.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<3Q", depth, max_epochs, len(steps)) + b"".join(steps))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok %d\n" % judged, (r.stdout, r.stderr[-2000:])
