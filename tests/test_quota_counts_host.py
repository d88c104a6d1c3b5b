"""The quota ledger's draw by count on the CPU: SeqLedger::draw_counts of zerokit_amd/csrc/quota_ledger.h
(tests/host/quota_counts.cpp, built with g++ and loaded with ctypes) held to the model of tests/quota_counts_cases.py;
the properties the header states, each from the answers alone; the refusal texts; the chosen cases checked for what they
must contain; and the same cases through a stand-alone sanitizer program.  No GPU needed."""
import ctypes
import itertools
import os
import struct
import subprocess

import pytest

import quota_cases as cases
import quota_counts_cases as cc
from quota_cases import E1, E2, E3, E4, OUTSIDE, NO_EPOCH, OK, OVER, U32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]
CP = ctypes.c_char_p
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
DEPTH = 20
LAST = (1 << DEPTH) - 1


def pack(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libquotacountshost.so")
    srcs = [os.path.join(HOST, "quota_counts.cpp"), os.path.join(HOST, "quota.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("quota_ledger.h", "relay.h", "nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.ql_new.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.ql_new.restype = ctypes.c_void_p
    lib.ql_free.argtypes = [ctypes.c_void_p]
    lib.ql_free.restype = None
    lib.ql_last.restype = CP
    lib.ql_set_epochs.argtypes = [ctypes.c_void_p, CP, ctypes.c_size_t]
    lib.ql_draw.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, U32P, CP]
    lib.ql_draw_counts.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, CP, U32P, CP]
    lib.ql_used.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, CP]
    lib.ql_used.restype = None
    lib.ql_info.argtypes = [ctypes.c_void_p, U64P]
    lib.ql_info.restype = None
    lib.ql_count_refusal.argtypes = [ctypes.c_size_t, ctypes.c_uint64]
    lib.ql_count_refusal.restype = CP
    lib.ql_draw_counts_refusal.argtypes = [ctypes.c_size_t, U64P, CP, U32P, CP, U32P, CP, ctypes.c_uint32]
    lib.ql_draw_counts_refusal.restype = CP
    lib.ql_issue_counts.argtypes = [ctypes.c_uint32] * 4 + [U32P]
    lib.ql_issue_counts.restype = None
    lib.ql_advance_counts.argtypes = [ctypes.c_uint32] * 5
    lib.ql_advance_counts.restype = ctypes.c_uint32
    lib.ql_set_used.argtypes = [ctypes.c_void_p, ctypes.c_uint64, CP, ctypes.c_uint32]
    lib.ql_count_max.restype = ctypes.c_uint32
    return lib


class HostLedger:
    """quota_counts.cpp's ledger with the methods of zerokit_amd.batch.QuotaLedger"""

    def __init__(self, L, depth, max_epochs):
        self.L, self.h = L, L.ql_new(depth, max_epochs)
        assert self.h

    def close(self):
        self.L.ql_free(self.h)

    def set_epochs(self, exts):
        if self.L.ql_set_epochs(self.h, pack(exts), len(exts)) != 0:
            raise cases.Refused(self.L.ql_last().decode())

    def draw(self, leaves, exts, limits):
        n = len(leaves)
        ids, status = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        if self.L.ql_draw(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0",
                          (ctypes.c_uint32 * max(n, 1))(*limits), ids, status) != 0:
            raise cases.Refused(self.L.ql_last().decode())
        return list(ids[:n]), list(status.raw[:n])

    def draw_counts(self, leaves, exts, limits, counts):
        n = len(leaves)
        firsts, status = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        if self.L.ql_draw_counts(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0",
                                 (ctypes.c_uint32 * max(n, 1))(*limits), bytes(counts) or b"\0", firsts, status) != 0:
            raise cases.Refused(self.L.ql_last().decode())
        return list(firsts[:n]), list(status.raw[:n])

    def used(self, leaves, exts):
        n = len(leaves)
        out, inside = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        self.L.ql_used(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0", out, inside)
        return [int(out[i]) if inside.raw[i] else None for i in range(n)]

    def info(self):
        out = (ctypes.c_uint64 * 6)()
        self.L.ql_info(self.h, out)
        return list(out)


def _pair(L, depth=DEPTH, max_epochs=4, window=(E1, E2, E3)):
    q, m = HostLedger(L, depth, max_epochs), cc.CountsModel(depth, max_epochs)
    q.set_epochs(list(window))
    m.set_epochs(list(window))
    return q, m


# --------------------------------------------------------------------------------------------- the chosen cases
@pytest.mark.parametrize("n", sorted(cc.SEEDS))
def test_the_chosen_cases_hold_what_they_must(n):
    """OK, OVER and NO_EPOCH, every count 1 .. 4 and the count 255 occur in the randomised case of every size, by the
    model alone"""
    assert cc.preconditions_hold(cc.interleaved(n))
    assert set(cc.SIZES) <= set(cc.SEEDS)


def test_the_straddling_group_straddles():
    """sorted by key, the one member's requests begin inside the first workgroup and end in a later one, and both
    outcomes occur in the group"""
    for n in (257, 65537):
        leaves, exts, limits, counts = cc.straddling(n)
        member = LAST - 1
        order = sorted(range(n), key=lambda i: leaves[i])
        where = [j for j, i in enumerate(order) if leaves[i] == member]
        assert 0 < where[0] < 256 <= where[-1] and where == list(range(where[0], where[-1] + 1))
        m = cc.CountsModel(DEPTH, 1)
        m.set_epochs([E1])
        st = m.draw_counts(leaves, exts, limits, counts)[1]
        assert {s for s, leaf in zip(st, leaves) if leaf == member} == {OK, OVER} and set(counts) == {1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------- the model itself
def test_the_model_with_all_ones_is_draw_and_its_blocks_never_meet():
    """exhaustive over short sequences of (member, epoch, limit, count) kinds: all-ones equals Model.draw; the OK
    requests of a key are a prefix with one limit per member; the blocks are disjoint over two calls"""
    kinds = [(0, E1, 3, 1), (0, E1, 3, 2), (1, E1, 9, 4), (1, E1, 9, 1), (1, OUTSIDE, 9, 2)]
    checked = 0
    for n in range(1, 7):
        for seq in itertools.product(kinds, repeat=n):
            leaves, exts, limits, counts = ([s[k] for s in seq] for k in range(4))
            m, blocks = cc.CountsModel(4, 2), cc.Blocks()
            m.set_epochs([E1, E2])
            for _ in range(2):
                firsts, st = m.draw_counts(leaves, exts, limits, counts)
                blocks.add(leaves, exts, limits, counts, firsts, st)
                for key in set(zip(exts, leaves)):
                    mine = [s for s, e, leaf in zip(st, exts, leaves) if (e, leaf) == key]
                    assert mine == sorted(mine)          # OK (0) before OVER (1); NO_EPOCH (2) is a key of its own
            assert blocks.check() == m.issued
            a, b = cc.CountsModel(4, 2), cases.Model(4, 2)
            a.set_epochs([E1, E2])
            b.set_epochs([E1, E2])
            for _ in range(2):
                assert a.draw_counts(leaves, exts, limits, [1] * n) == b.draw(leaves, exts, limits)
            assert a.used == b.used and (a.issued, a.over, a.no_epoch) == (b.issued, b.over, b.no_epoch)
            checked += 1
    assert checked > 19000


def test_the_model_is_not_what_every_split_gives():
    """the header's caveat, as an example: a refused block of 4 pushes a request of 1 behind it over in the same call;
    split after the 4, the 1 is granted"""
    whole = cc.CountsModel(4, 1)
    whole.set_epochs([E1])
    assert whole.draw_counts([5, 5], [E1, E1], [3, 3], [4, 1]) == ([3, 3], [OVER, OVER]) and whole.used.get((E1, 5), 0) == 0
    split = cc.CountsModel(4, 1)
    split.set_epochs([E1])
    assert split.draw_counts([5], [E1], [3], [4]) == ([3], [OVER])
    assert split.draw_counts([5], [E1], [3], [1]) == ([0], [OK]) and split.used[(E1, 5)] == 1


# --------------------------------------------------------------------------------------- the header's sequential text
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2000])
def test_host_draws_by_count_equal_the_model(L, n):
    q, m = _pair(L)
    blocks = cc.Blocks()
    try:
        keys = []
        for leaves, exts, limits, counts in cc.counts_shapes(n):
            cc.compare_draw_counts(m, q, leaves, exts, limits, counts, blocks)
            keys += list(zip(exts, leaves))
        cases.compare_counters(m, q, keys)
        assert blocks.check() == m.issued
        assert q.info() == [3, m.draws, m.issued, m.over, m.no_epoch, 0]
    finally:
        q.close()


@pytest.mark.parametrize("n", [1, 64, 257, 2000])
def test_host_all_ones_is_draw_on_a_twin_ledger(L, n):
    a, b = HostLedger(L, DEPTH, 4), HostLedger(L, DEPTH, 4)
    try:
        a.set_epochs([E1, E2, E3])
        b.set_epochs([E1, E2, E3])
        keys = []
        for leaves, exts, limits in cases.draw_shapes(n):
            assert a.draw_counts(leaves, exts, limits, [1] * n) == b.draw(leaves, exts, limits)
            keys += list(zip(exts, leaves))
        keys = sorted(set(keys))
        assert a.used([k[1] for k in keys], [k[0] for k in keys]) == b.used([k[1] for k in keys], [k[0] for k in keys])
        assert a.info() == b.info()
    finally:
        a.close()
        b.close()


def test_host_a_block_that_ends_at_the_limit_is_granted(L):
    q, m = _pair(L)
    try:
        # first + count == limit: OK; the same block under limit - 1 ... that is, a limit one too low: OVER
        assert q.draw_counts([3, 3], [E1, E1], [7, 7], [3, 4]) == ([0, 3], [OK, OK]) and q.used([3], [E1]) == [7]
        assert q.draw_counts([4, 4], [E1, E1], [7, 6], [3, 4]) == ([0, 6], [OK, OVER]) and q.used([4], [E1]) == [3]
        assert q.draw_counts([6], [E2], [255], [255]) == ([0], [OK]) and q.draw_counts([8], [E2], [254], [255]) == ([254], [OVER])
        # limit + 1 ids in all: the last request is the one over
        assert q.draw_counts([9] * 3, [E3] * 3, [8] * 3, [4, 4, 1]) == ([0, 4, 8], [OK, OK, OVER]) and q.used([9], [E3]) == [8]
        for args in (([3, 3], [E1, E1], [7, 7], [3, 4]), ([4, 4], [E1, E1], [7, 6], [3, 4]), ([6], [E2], [255], [255]), ([8], [E2], [254], [255]),
                     ([9] * 3, [E3] * 3, [8] * 3, [4, 4, 1])):
            m.draw_counts(*args)
        cases.compare_counters(m, q, [(E1, 3), (E1, 4), (E2, 6), (E2, 8), (E3, 9)])
    finally:
        q.close()


def test_the_rule_does_not_wrap_around(L):
    out = (ctypes.c_uint32 * 2)()
    L.ql_issue_counts(U32 - 2, 0, 3, U32, out)          # used = 2^32 - 3, limit = 2^32 - 1: first + 3 = 2^32
    assert list(out) == [U32, OVER]
    L.ql_issue_counts(U32 - 2, 0, 2, U32, out)
    assert list(out) == [U32 - 2, OK]
    L.ql_issue_counts(U32, U32, 255, U32, out)          # every operand at its largest
    assert list(out) == [U32, OVER]
    L.ql_issue_counts(0, 0, 1, 0, out)
    assert list(out) == [0, OVER]
    assert L.ql_advance_counts(U32 - 2, 5, 6, 0, 2) == U32 and L.ql_advance_counts(17, 5, 5, 9, 9) == 17
    q, m = _pair(L)
    try:
        assert L.ql_set_used(q.h, 11, pack([E1]), U32 - 2) == 0
        m.used[(E1, 11)] = U32 - 2
        for counts in ([3, 2], [2, 1]):
            cc.compare_draw_counts(m, q, [11, 11], [E1, E1], [U32, U32], counts)
        assert q.used([11], [E1]) == [U32]
    finally:
        q.close()


def test_host_two_limits_in_both_orders(L):
    q, m = _pair(L)
    blocks = cc.Blocks()
    try:
        for leaves, exts, limits, counts in cc.two_limits_counts() * 2:
            cc.compare_draw_counts(m, q, leaves, exts, limits, counts, blocks)
        cases.compare_counters(m, q, [(E1, 7), (E1, 9)])
        assert blocks.check() == m.issued > 0 and m.over > 0
    finally:
        q.close()


def test_host_a_refused_block_counts_behind_it_in_its_call_only(L):
    q, m = _pair(L)
    try:
        # 4 does not fit under 3, and the 1 behind it would have: OVER in this call, OK in the next
        assert cc.compare_draw_counts(m, q, [5, 5], [E1, E1], [3, 3], [4, 1]) == ([3, 3], [OVER, OVER])
        assert q.used([5], [E1]) == [0]
        assert cc.compare_draw_counts(m, q, [5], [E1], [3], [1]) == ([0], [OK])
        assert q.used([5], [E1]) == [1]
    finally:
        q.close()


def test_host_set_epochs_zeroes_what_a_block_draw_advanced(L):
    q, m = _pair(L, max_epochs=2, window=(E1, E2))
    try:
        cc.compare_draw_counts(m, q, [0, LAST, 0], [E1, E2, E1], [600] * 3, [255, 4, 3])
        assert q.used([0, LAST], [E1, E2]) == [258, 4]
        for impl in (q, m):
            impl.set_epochs([E4, E2])
        assert q.used([0, LAST, 0], [E4, E2, E1]) == [0, 4, None]
        cc.compare_draw_counts(m, q, [0, LAST], [E4, E2], [600] * 2, [2, 2])
        assert q.used([0, LAST], [E4, E2]) == [2, 6] and q.info()[5] == 0
    finally:
        q.close()


# ------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_text(L):
    assert L.ql_count_max() == cc.COUNT_MAX == 255
    for i, c in ((0, 0), (7, 0), (3, 256), (0, 1 << 40), (5, 1), (5, 255)):
        assert L.ql_count_refusal(i, c).decode() == cc.count_refusal(i, c)
    assert cc.count_refusal(5, 1) == cc.count_refusal(5, 255) == "" and cc.count_refusal(7, 0) and cc.count_refusal(3, 256)
    m = cc.CountsModel(10, 1)
    firsts, st = (ctypes.c_uint32 * 3)(), ctypes.create_string_buffer(3)
    leaf, bad_leaf, lim = (ctypes.c_uint64 * 3)(0, 1, 2), (ctypes.c_uint64 * 3)(0, 1024, 1), (ctypes.c_uint32 * 3)(5, 5, 5)
    ext = b"\0" * 96

    def said(n, leaf_, ext_, lim_, counts_, firsts_, st_, depth=10):
        return L.ql_draw_counts_refusal(n, leaf_, ext_, lim_, counts_, firsts_, st_, depth).decode()
    assert said(3, leaf, ext, lim, bytes([1, 255, 4]), firsts, st) == ""
    assert said(0, None, None, None, None, None, None) == ""
    # what draw refuses, in draw's words
    for args in ((None, ext, lim, b"\1\1\1", firsts, st), (leaf, None, lim, b"\1\1\1", firsts, st), (leaf, ext, None, b"\1\1\1", firsts, st),
                 (leaf, ext, lim, b"\1\1\1", None, st), (leaf, ext, lim, b"\1\1\1", firsts, None)):
        assert said(3, *args) == m.draw_counts_refusal([0, 1, 2], [1, 1, 1], pointers=False) == m.draw_refusal([0], pointers=False)
    assert said(3, bad_leaf, ext, lim, b"\1\1\1", firsts, st) == m.draw_counts_refusal([0, 1024, 1], [1, 1, 1]) == \
        m.draw_refusal([0, 1024, 1]) != ""
    # its own
    assert said(3, leaf, ext, lim, None, firsts, st) == m.draw_counts_refusal([0, 1, 2], None, counts_pointer=False) == \
        "quota ledger: draw_counts was given a null pointer for the counts of n > 0 requests"
    assert said(3, leaf, ext, lim, bytes([1, 0, 0]), firsts, st) == m.draw_counts_refusal([0, 1, 2], [1, 0, 0]) == \
        "quota ledger: request 1 of draw_counts asks for no id (a count is 1 .. 255)"
    assert m.draw_counts_refusal([0, 1, 2], [1, 2, 256]) == "quota ledger: request 2 of draw_counts asks for 256 ids, more than 255"
    # n = 2^24, with arrays of three: refused before any of them is read; one request fewer is judged by its arrays
    for n in (1 << 24, 1 << 32, (1 << 24) + 1):
        assert said(n, leaf, ext, lim, b"\1\1\1", firsts, st) == m.draw_counts_refusal([], [], n=n) == \
            "quota ledger: a draw by count takes fewer than 2^24 requests, not %d" % n
    # the order: a bad leaf is named before a bad count
    assert said(3, bad_leaf, ext, lim, bytes([0, 1, 1]), firsts, st) == m.draw_refusal([0, 1024, 1])


def test_refused_calls_leave_the_host_ledger_as_it_was(L):
    q, _ = _pair(L, depth=10, max_epochs=2, window=(E1, E2))
    try:
        q.draw_counts([0, 1023, 0], [E1, E2, E1], [50, 50, 50], [4, 255, 2])
        before = (q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info())
        for leaves, counts in (([0, 1024], [1, 1]), ([0, 1], [1, 0]), ([0, 1], [0, 1])):
            with pytest.raises(cases.Refused):
                q.draw_counts(leaves, [E1, E1], [50, 50], counts)
        assert q.draw_counts([], [], [], []) == ([], [])
        assert (q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info()) == before
    finally:
        q.close()


def test_the_c_abi_refuses_before_it_touches_a_device():
    """the same texts through rlnamd_quota_draw_counts with no object behind the handle and no device asked for"""
    from zerokit_amd._native import last_error, lib
    firsts, st = (ctypes.c_uint32 * 2)(), ctypes.create_string_buffer(2)
    leaf, lim = (ctypes.c_uint64 * 2)(0, 1 << 24), (ctypes.c_uint32 * 2)(5, 5)
    f = lib().rlnamd_quota_draw_counts
    assert f(None, 2, leaf, b"\0" * 64, lim, b"\1\1", firsts, st) != 0
    assert last_error() == "quota ledger: leaf index 16777216 of request 1 is outside a ledger of depth 24"
    leaf[1] = 1
    assert f(None, 2, leaf, None, lim, b"\1\1", firsts, st) != 0
    assert last_error() == "quota ledger: draw was given a null pointer for n > 0 requests"
    assert f(None, 2, leaf, b"\0" * 64, lim, None, firsts, st) != 0
    assert last_error() == "quota ledger: draw_counts was given a null pointer for the counts of n > 0 requests"
    assert f(None, 2, leaf, b"\0" * 64, lim, b"\1\0", firsts, st) != 0 and last_error() == cc.count_refusal(1, 0)
    assert f(None, 1 << 24, leaf, b"\0" * 64, lim, b"\1\1", firsts, st) != 0
    assert last_error() == "quota ledger: a draw by count takes fewer than 2^24 requests, not 16777216"
    assert f(None, 2, leaf, b"\0" * 64, lim, b"\1\xff", firsts, st) != 0 and last_error() == "rlnamd_quota_draw_counts: null ledger"
    assert f(None, 0, None, None, None, None, None, None) != 0 and last_error() == "rlnamd_quota_draw_counts: null ledger"


def test_python_names():
    from zerokit_amd import batch
    assert batch.QuotaLedger.COUNT_MAX == cc.COUNT_MAX and callable(batch.QuotaLedger.draw_counts)


# ------------------------------------------------------------------------------------------ the sanitizer program
def test_draw_counts_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/quota_counts_main.cpp), built with the sanitizers and run as a child
    process: the cases above as one file of steps with the model's answers, then the program's own edge calls"""
    exe = str(tmp_path / "quota_counts_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "quota_counts_main.cpp"), "-o", exe])
    depth, max_epochs = 12, 3
    m = cc.CountsModel(depth, max_epochs)
    steps, judged = [], 0

    def set_epochs(exts):
        refused = 1 if m.epochs_refusal(exts) else 0
        if not refused:
            m.set_epochs(exts)
        steps.append(struct.pack("<2Q", 0, len(exts)) + pack(exts) + struct.pack("<Q", refused))

    def draw(leaves, exts, limits, counts):
        nonlocal judged
        firsts, status = m.draw_counts(leaves, exts, limits, counts)
        n = len(leaves)
        steps.append(struct.pack("<2Q", 3, n) + struct.pack("<%dQ" % n, *leaves) + pack(exts) + struct.pack("<%dI" % n, *limits) +
                     bytes(counts) + struct.pack("<%dI" % n, *firsts) + bytes(status))
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
        for leaves, exts, limits, counts in cc.counts_shapes(n, depth):
            draw(leaves, exts, limits, counts)
            keys += list(zip(exts, leaves))
    counters(keys)
    set_epochs([E4, E2, E4])              # E1 and E3 leave, E4 takes a slot that was just zeroed
    for leaves, exts, limits, counts in cc.two_limits_counts():
        draw(leaves, [E4] * len(leaves), limits, counts)
    counters(keys + [(E4, 7), (E4, 9)])
    set_epochs([])
    counters(keys[:50])
    path = str(tmp_path / "steps.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<3Q", depth, max_epochs, len(steps)) + b"".join(steps))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok %d\n" % judged, (r.stdout, r.stderr[-2000:])
