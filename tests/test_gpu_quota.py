"""The quota ledger on the device (rlnamd_quota_*, zerokit_amd/csrc/quota_ledger.hip) against the dict model of
tests/quota_cases.py: ids, statuses, the counters read back, the window, and the per-call buffers left at zero.  The
sizes are the wave and workgroup edges and every n at which the draw's own plan (rlnamd_quota_plan) takes another
workgroup, scan level or sort pass."""
import pytest

import quota_cases as cases
from quota_cases import E1, E2, E3, E4, OUTSIDE, NO_EPOCH, OK, OVER, U32

pytestmark = pytest.mark.gpu

DEPTH = 20
LAST = (1 << DEPTH) - 1


def _ledger(depth=DEPTH, max_epochs=4):
    from zerokit_amd.batch import QuotaLedger
    return QuotaLedger(depth, max_epochs)


def _plan_edges(depth, upto):
    """the n in [2, upto] at which the plan of n differs from the plan of n - 1 in anything but the workgroup count,
    found by bisection between powers of two (levels only ever rise with n)"""
    from zerokit_amd.batch import QuotaLedger

    def shape(n):
        p = QuotaLedger.plan(n, depth)
        return (p[0], p[2], p[3])
    edges, lo = [], 1
    while lo < upto:
        hi = min(2 * lo, upto)
        while shape(lo) != shape(hi):       # an edge in (lo, hi]
            a, b = lo, hi
            while b - a > 1:
                mid = (a + b) // 2
                if shape(mid) == shape(lo):
                    a = mid
                else:
                    b = mid
            edges.append(b)
            lo = b
        lo = hi
    return edges


def test_the_plan_names_its_edges():
    from zerokit_amd.batch import QuotaLedger
    assert _plan_edges(DEPTH, 1 << 17) == [257, 65537]                  # one more level for the bins and the requests
    assert [QuotaLedger.plan(1, d)[0] for d in (1, 8, 9, 16, 17, 24)] == [2, 2, 3, 3, 4, 4]   # the leaf's digits + the slot's
    assert QuotaLedger.plan(256, DEPTH)[1] == 1 and QuotaLedger.plan(257, DEPTH)[1] == 2


SIZES = [1, 63, 64, 65, 256, 257]


def _sizes():
    out = list(SIZES)
    for e in [257, 65537]:                  # test_the_plan_names_its_edges holds these to the plan
        out += [e - 1, e]
    return sorted(set(out))


@pytest.mark.parametrize("n", _sizes())
def test_draws_equal_the_model(n):
    q, m = _ledger(), cases.Model(DEPTH, 4)
    try:
        q.set_epochs([E1, E2, E3])
        m.set_epochs([E1, E2, E3])
        keys = []
        for leaves, exts, limits in cases.draw_shapes(n):
            ids, status = cases.compare_draw(m, q, leaves, exts, limits)
            keys += list(zip(exts, leaves))[:300] + list(zip(exts, leaves))[-300:]
            assert q.info()["residue"] == 0
        cases.compare_counters(m, q, keys[:900])
        info = q.info()
        assert (info["window"], info["draws"], info["issued"], info["over"], info["no_epoch"]) == \
            (3, m.draws, m.issued, m.over, m.no_epoch)
        # all n for one member with limit n // 2: the refusals are exactly the tail
        q.set_epochs([E4])
        ids, status = q.draw([5] * n, [E4] * n, [n // 2] * n)
        assert status == [OK] * (n // 2) + [OVER] * (n - n // 2) and ids[:n // 2] == list(range(n // 2))
        assert q.used([5], [E4]) == [n // 2]
    finally:
        q.close()


def test_the_sizes_cover_the_plan():
    assert set(_plan_edges(DEPTH, 1 << 17)) <= set(_sizes()) and {e - 1 for e in _plan_edges(DEPTH, 1 << 17)} <= set(_sizes())


@pytest.mark.parametrize("depth", [1, 9, 20, 24])
def test_every_sort_pass_count_and_the_edge_leaves(depth):
    """depth 1, 9, 20 and 24: two, three, four and four sort passes; leaf 0 and leaf 2^depth - 1 under the first and the
    last slot"""
    last = (1 << depth) - 1
    q, m = _ledger(depth, 3), cases.Model(depth, 3)
    try:
        q.set_epochs([E1, E2, E3])
        m.set_epochs([E1, E2, E3])
        leaves = [0, last, last, 0, 0, last, 0] * 11
        exts = [E1, E3, E1, E3, OUTSIDE, E2, E1] * 11
        for limits in ([3] * 77, [U32] * 77, [0] * 77):
            cases.compare_draw(m, q, leaves, exts, limits)
        cases.compare_counters(m, q, [(e, leaf) for e in (E1, E2, E3, OUTSIDE) for leaf in (0, last)])
        assert q.info()["residue"] == 0
    finally:
        q.close()


def test_limit_zero_and_limit_max():
    q = _ledger()
    try:
        q.set_epochs([E1])
        ids, status = q.draw([3, 3, 4, 4, 4], [E1] * 5, [0, 0, U32, U32, U32])
        assert status == [OVER, OVER, OK, OK, OK] and ids == [0, 0, 0, 1, 2]
        assert q.used([3, 4], [E1, E1]) == [0, 3]
    finally:
        q.close()


def test_two_limits_for_one_member_in_both_orders():
    q, m = _ledger(), cases.Model(DEPTH, 4)
    try:
        q.set_epochs([E1])
        m.set_epochs([E1])
        issued = {}
        for leaves, exts, limits in cases.two_limits() * 2:
            ids, status = cases.compare_draw(m, q, leaves, exts, limits)
            for leaf, i, s in zip(leaves, ids, status):
                if s == OK:
                    assert i not in issued.setdefault(leaf, set())      # skipped perhaps, never twice
                    issued[leaf].add(i)
        cases.compare_counters(m, q, [(E1, 7), (E1, 9)])
        assert issued[7] and issued[9]
    finally:
        q.close()


def test_three_draws_in_a_row_equal_one_draw_of_their_concatenation():
    a, b = _ledger(), _ledger()
    try:
        a.set_epochs([E1, E2])
        b.set_epochs([E1, E2])
        parts = [s for n in (65, 257, 30) for s in list(cases.split_sequences(n, 1, n))]
        whole = tuple(sum((p[k] for p in parts), []) for k in range(3))
        got = ([], [])
        for leaves, exts, limits in parts:
            i, s = a.draw(leaves, exts, limits)
            got = (got[0] + i, got[1] + s)
        assert got == b.draw(*whole)
        keys = sorted(set(zip(whole[1], whole[0])))
        assert a.used([k[1] for k in keys], [k[0] for k in keys]) == b.used([k[1] for k in keys], [k[0] for k in keys])
        assert {OK, OVER, NO_EPOCH} <= set(got[1])
    finally:
        a.close()
        b.close()


def test_set_epochs_keeps_zeroes_and_hands_over():
    q, m = _ledger(DEPTH, 3), cases.Model(DEPTH, 3)
    try:
        for impl in (q, m):
            impl.set_epochs([E1, E2])
            impl.draw([0, 0, LAST, 5], [E1, E1, E2, E2], [9] * 4)
        assert q.epochs() == [E1, E2] and q.used([0, LAST, 5], [E1, E2, E2]) == [2, 1, 1]
        for impl in (q, m):
            impl.set_epochs([E3, E2, E3])                 # E2 stays, E1 leaves, E3 takes E1's slot; the duplicate counts once
        assert q.epochs() == m.window == [E3, E2] and q.info()["window"] == 2
        assert q.used([0, LAST, 5, 0, LAST], [E3, E2, E2, E1, E3]) == [0, 1, 1, None, 0]
        cases.compare_draw(m, q, [0, LAST, 0, 3], [E3, E2, E1, E3], [9] * 4)
        cases.compare_counters(m, q, [(E3, 0), (E2, LAST), (E1, 0), (E3, 3)])
        for impl in (q, m):
            impl.set_epochs([])
        assert q.epochs() == [] and q.draw([0], [E2], [9]) == ([9], [NO_EPOCH])
        for impl in (q, m):
            impl.set_epochs([E2])                         # (what must not be done: E2 is back, and its counters are gone)
        assert q.used([LAST], [E2]) == [0]
    finally:
        q.close()


def test_every_refusal_leaves_counters_and_window_unchanged():
    import ctypes as C
    from zerokit_amd._native import RLNError, last_error, lib
    q, m = _ledger(10, 2), cases.Model(10, 2)
    try:
        q.set_epochs([E1, E2])
        m.set_epochs([E1, E2])
        cases.compare_draw(m, q, [0, 1023, 0], [E1, E2, E1], [5, 5, 5])
        before = (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info())
        for exts in ([E1, E2, E3], [E3, cases.R], [cases.R + 5]):
            with pytest.raises(RLNError) as err:
                _set_raw(q, exts)
            assert str(err.value) == m.epochs_refusal(exts) != ""
        assert lib().rlnamd_quota_set_epochs(q._h, None, 1) != 0 and last_error() == m.epochs_refusal([E1], pointers=False)
        with pytest.raises(RLNError) as err:
            q.draw([0, 1024, 1], [E1] * 3, [5] * 3)
        assert str(err.value).endswith(m.draw_refusal([0, 1024, 1]))
        ids, st = (C.c_uint32 * 2)(), C.create_string_buffer(2)
        leaf, lim = (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 2)(5, 5)
        for args in ((None, b"\0" * 64, lim, ids, st), (leaf, None, lim, ids, st), (leaf, b"\0" * 64, None, ids, st),
                     (leaf, b"\0" * 64, lim, None, st), (leaf, b"\0" * 64, lim, ids, None)):
            assert lib().rlnamd_quota_draw(q._h, 2, *args) != 0 and last_error() == m.draw_refusal([0, 1], pointers=False)
        assert lib().rlnamd_quota_draw(q._h, 1 << 32, leaf, b"\0" * 64, lim, ids, st) != 0
        assert last_error() == "quota ledger: a draw takes fewer than 2^32 requests, not 4294967296"
        assert q.draw([], [], []) == ([], [])                                          # n = 0 succeeds
        assert (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info()) == before
        cases.compare_draw(m, q, [0, 1023, 0], [E1, E2, E1], [5, 5, 5])                 # usable afterwards
    finally:
        q.close()
    from zerokit_amd.batch import QuotaLedger
    for depth, max_epochs in ((0, 1), (25, 1), (10, 0), (10, 65)):
        with pytest.raises(RLNError) as err:
            QuotaLedger(depth, max_epochs)
        assert str(err.value).endswith(cases.new_refusal(depth, max_epochs))


def _set_raw(q, exts):
    """set_epochs with elements that batch._b would refuse to pack (>= r)"""
    from zerokit_amd._native import check, lib
    check(lib().rlnamd_quota_set_epochs(q._h, b"".join(int(e).to_bytes(32, "little") for e in exts), len(exts)))
