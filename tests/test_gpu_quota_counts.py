"""The quota ledger's draw by count on the device (rlnamd_quota_draw_counts, zerokit_amd/csrc/quota_ledger.hip) against
the model of tests/quota_counts_cases.py, the ledger alone and no prover: firsts, statuses, the counters read back, the
blocks granted checked for overlap from the answers themselves, and the per-call buffers left at zero after every call.
The sizes are the workgroup edge and every n at which the draw's plan (rlnamd_quota_plan) takes another scan level --
the sum over the counts is a scan over the n requests with exactly those levels."""
import pytest

import quota_cases as cases
import quota_counts_cases as cc
from quota_cases import E1, E2, E3, E4, OUTSIDE, NO_EPOCH, OK, OVER, U32

pytestmark = pytest.mark.gpu

DEPTH = 20
LAST = (1 << DEPTH) - 1


def _ledger(depth=DEPTH, max_epochs=4):
    from zerokit_amd.batch import QuotaLedger
    return QuotaLedger(depth, max_epochs)


def _level_edges(upto):
    """the n in [2, upto] at which the scan over the requests, or the one over a pass's bins, takes another level"""
    from zerokit_amd.batch import QuotaLedger

    def shape(n):
        return QuotaLedger.plan(n, DEPTH)[2:]
    edges, lo = [], 1
    while lo < upto:
        hi = min(2 * lo, upto)
        while shape(lo) != shape(hi):
            a, b = lo, hi
            while b - a > 1:
                mid = (a + b) // 2
                a, b = (mid, b) if shape(mid) == shape(lo) else (a, mid)
            edges.append(b)
            lo = b
        lo = hi
    return edges


def _sizes():
    return cc.SIZES


def test_the_sizes_are_the_plans():
    from zerokit_amd.batch import QuotaLedger
    edges = _level_edges(1 << 17)
    assert edges == [257, 65537]
    assert set(_sizes()) == {1, 255, 256} | set(edges)
    assert [QuotaLedger.plan(n, DEPTH)[3] for n in _sizes()] == [1, 1, 1, 2, 3]
    assert [QuotaLedger.plan(n, DEPTH)[1] for n in (255, 256, 257)] == [1, 1, 2]


def _play(q, m, blocks, call, keys):
    leaves, exts, limits, counts = call
    got = cc.compare_draw_counts(m, q, leaves, exts, limits, counts, blocks)
    assert q.info()["residue"] == 0
    pairs = list(zip(exts, leaves))
    keys += pairs[:200] + pairs[-200:]
    return got


@pytest.fixture(params=cc.SIZES)
def n(request):
    return request.param


def _fresh():
    q, m = _ledger(), cc.CountsModel(DEPTH, 4)
    q.set_epochs([E1, E2, E3])
    m.set_epochs([E1, E2, E3])
    return q, m


def _finish(q, m, blocks, keys):
    cases.compare_counters(m, q, keys[:900])
    info = q.info()
    assert (info["window"], info["draws"], info["issued"], info["over"], info["no_epoch"], info["residue"]) == \
        (3, m.draws, m.issued, m.over, m.no_epoch, 0)
    assert blocks.check() == m.issued          # ids issued: the counts of the granted requests


def test_one_member_for_all_n_with_count_255(n):
    q, m = _fresh()
    blocks, keys = cc.Blocks(), []
    try:
        firsts, status = _play(q, m, blocks, cc.one_member_255(n), keys)
        # the member's limit is 255 * (n // 2) + 7: the first n // 2 blocks, one behind the other, and then the tail over
        assert status == [OK] * (n // 2) + [OVER] * (n - n // 2) and firsts[:n // 2] == [255 * i for i in range(n // 2)]
        assert q.used([LAST], [E2]) == [255 * (n // 2)]
        _finish(q, m, blocks, keys)
    finally:
        q.close()


def test_one_member_astride_a_workgroup_boundary_with_mixed_counts(n):
    q, m = _fresh()
    blocks, keys = cc.Blocks(), []
    try:
        call = cc.straddling(n)
        firsts, status = _play(q, m, blocks, call, keys)
        mine = [s for s, leaf in zip(status, call[0]) if leaf == LAST - 1]
        assert mine == sorted(mine) and (n < 64 or set(mine) == {OK, OVER})       # a prefix is granted
        _play(q, m, blocks, call, keys)                                           # and again: what is left of the limit
        _finish(q, m, blocks, keys)
    finally:
        q.close()


def test_all_distinct(n):
    q, m = _fresh()
    blocks, keys = cc.Blocks(), []
    try:
        _play(q, m, blocks, cc.all_distinct(n), keys)
        _finish(q, m, blocks, keys)
    finally:
        q.close()


def test_interleaved_epochs_one_outside_and_consecutive_calls(n):
    """the randomised case of size n: two and more consecutive calls over the same few members on one ledger"""
    q, m = _fresh()
    blocks, keys = cc.Blocks(), []
    try:
        calls = cc.interleaved(n)
        assert len(calls) >= 2
        seen = set()
        for call in calls:
            seen |= set(_play(q, m, blocks, call, keys)[1])
        assert seen == {OK, OVER, NO_EPOCH}
        _finish(q, m, blocks, keys)
    finally:
        q.close()


def test_every_shape_in_a_row_on_one_ledger(n):
    q, m = _fresh()
    blocks, keys = cc.Blocks(), []
    try:
        for call in cc.counts_shapes(n):
            _play(q, m, blocks, call, keys)
        _finish(q, m, blocks, keys)
    finally:
        q.close()


def test_all_ones_is_draw_on_a_twin_ledger(n):
    a, b = _ledger(), _ledger()
    try:
        a.set_epochs([E1, E2, E3])
        b.set_epochs([E1, E2, E3])
        keys = []
        for leaves, exts, limits in cases.draw_shapes(n):
            assert a.draw_counts(leaves, exts, limits, [1] * n) == b.draw(leaves, exts, limits)
            assert a.info()["residue"] == 0
            pairs = list(zip(exts, leaves))
            keys += pairs[:200] + pairs[-200:]
        keys = sorted(set(keys))[:900]
        assert a.used([k[1] for k in keys], [k[0] for k in keys]) == b.used([k[1] for k in keys], [k[0] for k in keys])
        assert a.info() == b.info()
    finally:
        a.close()
        b.close()


def test_a_refused_block_counts_behind_it_in_its_call_only():
    q, m = _fresh()
    try:
        assert cc.compare_draw_counts(m, q, [5, 5], [E1, E1], [3, 3], [4, 1]) == ([3, 3], [OVER, OVER])
        assert q.used([5], [E1]) == [0]
        assert cc.compare_draw_counts(m, q, [5], [E1], [3], [1]) == ([0], [OK])
        assert q.used([5], [E1]) == [1] and q.info()["residue"] == 0
    finally:
        q.close()


def test_blocks_at_the_limit_and_two_limits_in_both_orders():
    q, m = _fresh()
    blocks = cc.Blocks()
    try:
        assert cc.compare_draw_counts(m, q, [3, 3, 9, 9, 9], [E1] * 5, [7, 7, 8, 8, 8], [3, 4, 4, 4, 1], blocks) == \
            ([0, 3, 0, 4, 8], [OK, OK, OK, OK, OVER])                       # first + count == limit is granted
        assert cc.compare_draw_counts(m, q, [6, 8], [E2, E2], [255, 254], [255, 255], blocks) == ([0, 254], [OK, OVER])
        assert cc.compare_draw_counts(m, q, [4], [E3], [U32], [255], blocks) == ([0], [OK])
        for leaves, exts, limits, counts in cc.two_limits_counts() * 2:
            cc.compare_draw_counts(m, q, leaves, exts, limits, counts, blocks)
            assert q.info()["residue"] == 0
        cases.compare_counters(m, q, [(E1, 3), (E1, 9), (E2, 6), (E2, 8), (E3, 4), (E1, 7)])
        assert blocks.check() == m.issued == q.info()["issued"]
    finally:
        q.close()


def test_set_epochs_zeroes_what_a_block_draw_advanced():
    q, m = _ledger(DEPTH, 2), cc.CountsModel(DEPTH, 2)
    try:
        for impl in (q, m):
            impl.set_epochs([E1, E2])
        cc.compare_draw_counts(m, q, [0, LAST, 0], [E1, E2, E1], [600] * 3, [255, 4, 3])
        assert q.used([0, LAST], [E1, E2]) == [258, 4]
        for impl in (q, m):
            impl.set_epochs([E4, E2])                     # E1 leaves, E4 takes its slot
        assert q.used([0, LAST, 0], [E4, E2, E1]) == [0, 4, None]
        cc.compare_draw_counts(m, q, [0, LAST, 0], [E4, E2, E1], [600] * 3, [2, 2, 2])
        assert q.used([0, LAST], [E4, E2]) == [2, 6] and q.info()["residue"] == 0
        cases.compare_counters(m, q, [(E4, 0), (E2, LAST), (E1, 0)])
    finally:
        q.close()


def test_the_refusals_draw_nothing():
    import ctypes as C
    from zerokit_amd._native import RLNError, last_error, lib
    q, m = _ledger(10, 2), cc.CountsModel(10, 2)
    try:
        q.set_epochs([E1, E2])
        m.set_epochs([E1, E2])
        cc.compare_draw_counts(m, q, [0, 1023, 0], [E1, E2, E1], [50] * 3, [4, 255, 2])
        before = (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info())
        for leaves, counts in (([0, 1024, 1], [1, 1, 1]), ([0, 1, 2], [1, 0, 1]), ([0, 1, 2], [1, 2, 256])):
            with pytest.raises(RLNError) as err:
                q.draw_counts(leaves, [E1] * 3, [50] * 3, counts)
            assert str(err.value).endswith(m.draw_counts_refusal(leaves, counts)) and m.draw_counts_refusal(leaves, counts)
        firsts, st = (C.c_uint32 * 2)(), C.create_string_buffer(2)
        leaf, lim = (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 2)(50, 50)
        f = lib().rlnamd_quota_draw_counts
        for args in ((None, b"\0" * 64, lim, b"\1\1", firsts, st), (leaf, None, lim, b"\1\1", firsts, st),
                     (leaf, b"\0" * 64, None, b"\1\1", firsts, st), (leaf, b"\0" * 64, lim, b"\1\1", None, st),
                     (leaf, b"\0" * 64, lim, b"\1\1", firsts, None)):
            assert f(q._h, 2, *args) != 0 and last_error() == m.draw_refusal([0, 1], pointers=False)
        assert f(q._h, 2, leaf, b"\0" * 64, lim, None, firsts, st) != 0
        assert last_error() == m.draw_counts_refusal([0, 1], None, counts_pointer=False)
        for n in (1 << 24, 1 << 32):                                       # before any array is read: these hold two
            assert f(q._h, n, leaf, b"\0" * 64, lim, b"\1\1", firsts, st) != 0
            assert last_error() == "quota ledger: a draw by count takes fewer than 2^24 requests, not %d" % n
        assert q.draw_counts([], [], [], []) == ([], [])                   # n = 0 succeeds, and is no draw
        assert (q.epochs(), q.used([0, 1023, 0, 1023], [E1, E2, E2, E1]), q.info()) == before
        assert q.info()["draws"] == m.draws == 1
        cc.compare_draw_counts(m, q, [0, 1023, 0], [E1, E2, E1], [50] * 3, [4, 255, 2])      # usable afterwards
    finally:
        q.close()
