"""The variable-base MSM (zerokit_amd/csrc/msm_impl.h) at every branch its sizes decide, on inputs built by LAYOUT
(tests/msm_cases.py; its model is judged by tests/test_msm_cases_host.py, which proves that every case reaches the branch
it is named for).  Every comparison is exact equality of affine points, or of None, with the closed form
((sum_i s_i k_i) mod r) G of the oracle -- one big-integer sum and one scalar multiplication, no code shared with the
kernels.

  tiles         n = 1, 15, 16, 17, 31: empty tiles, the last tile short
  slice_walk    every outcome of k_slice_acc (buckets[], head[], tail[]; empty buckets skipped; the window edge), in the
                bottom, a middle and the top window
  signs         negative digits through the carry rule, 2^15 exactly, -(2^15 - 1), a zero digit under a carry, a carry
                through every window
  join_64_65    a bucket cut so that s1 - s0 is 64 (k_slice_fix's serial join) and 65 (listed for k_slice_fix_big), after
                0, 5 and 128 entries, ending inside a slice and exactly on a slice end
  cancel        the same with +d and -d of ONE base: heads and tails that are the point at infinity, an infinity entry
  stage_edge    k_part2 with a partition of exactly MSM_PART_CAP entries, one of MSM_PART_CAP + 1, and an unstaged one
                between two staged ones
  big_overflow  more buckets listed than MSM_BIG_CAP: the serial join of k_slice_fix's overflow branch
  stale state   a tiny and a mid-sized run directly after every many-slice run, on one object
  scatter       k_scatter, chosen by a CAPACITY above 2^24 alone, on the same bytes as the two-level placement
  refusals      the four messages of msm_impl.h, and that a refused call leaves the loaded points and n alone

Nothing depends on timing; every test prints its wall time."""
import random
import re
import time

import pytest

import msm_cases as mc
from oracle.pyref.bn254 import Q, R
from zerokit_amd._native import RLNError

pytestmark = pytest.mark.gpu

MID_WINDOW = mc.SLICE_WALK_WINDOWS[1]


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def msm_class(group):
    from zerokit_amd.batch import MsmG1, MsmG2
    return MsmG1 if group == 1 else MsmG2


def run(m, data):
    points, scalars, n, _ = data
    m.set_raw(points, scalars, n)
    return m.combine([m.run_windows()[0]])


def stale_order():
    """every small case; directly after each many-slice one (join, cancel, stage_edge) a one-point run and a mid-sized
    one: stale heads, tails, list entries, histograms or sorted entries of the long run would show"""
    tiny, mid = mc.tiles(1), mc.slice_walk("5_long_long", MID_WINDOW)
    out = []
    for lay in mc.small_cases():
        out.append(lay)
        if lay.n > 4096:
            out += [tiny, mid]
    return out


SMALL_CAPACITY = max(lay.n for lay in mc.small_cases())


def run_cases(group):
    m = msm_class(group)(SMALL_CAPACITY)
    wrong = []
    try:
        for lay in stale_order():
            data = mc.built(lay, group)
            if run(m, data) != data[3]:
                wrong.append(lay.name)
    finally:
        m.close()
    assert not wrong, wrong


def test_every_case_on_one_g1_object_in_stale_state_order():
    assert SMALL_CAPACITY < 1 << 17
    run_cases(1)


def test_every_case_on_one_g2_object():
    """the same cases on the twist, except big_overflow: the join and walk kernels are the same templates, and its
    275 MB of G2 points and threefold additions buy nothing the G1 run does not show"""
    run_cases(2)


def test_big_overflow_joins_the_buckets_beyond_the_list_serially():
    """4 112 listed buckets for a list of 4 096: which 16 take the serial join of k_slice_fix is the order of an atomic,
    and the result must not depend on it.  One upload, one run."""
    from zerokit_amd.batch import MsmG1
    t0 = time.perf_counter()
    lay = mc.big_overflow()
    points, scalars, n, expected = mc.build(lay)
    t1 = time.perf_counter()
    m = MsmG1(n)
    try:
        m.set_raw(points, scalars, n)
        t2 = time.perf_counter()
        blob, ms = m.run_windows()
        got = m.combine([blob])
        t3 = time.perf_counter()
    finally:
        m.close()
    print("big_overflow: n = %d; bytes and closed form %.2f s, upload %.2f s, run %.2f s %r" % (n, t1 - t0, t2 - t1, t3 - t2, ms))
    assert got == expected


def test_both_folds_on_join_and_cancel(monkeypatch):
    """every window but one (cancel: two) sums to infinity here, and some whole cases do: both folds take them"""
    from zerokit_amd.batch import MsmG1
    m = MsmG1(SMALL_CAPACITY)
    wrong = []
    try:
        for lay in mc.joins() + mc.joins(cancel=True):
            data = mc.built(lay)
            monkeypatch.setenv("RLNAMD_MSM_FOLD", "device")
            on_device = run(m, data)
            monkeypatch.delenv("RLNAMD_MSM_FOLD")
            on_host = run(m, data)
            if not on_device == on_host == data[3]:
                wrong.append(lay.name)
    finally:
        m.close()
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------ the scatter route
@pytest.fixture(scope="module")
def scatter_pair():
    """(an MsmG1 whose capacity is above 2^24 -- about 5 GB of workspace; only the capacity selects k_scatter -- and one
    of the two-level placement), made once"""
    from zerokit_amd.batch import MsmG1
    big = MsmG1((1 << 24) + 1)
    try:
        small = MsmG1(SMALL_CAPACITY)
        try:
            yield big, small
        finally:
            small.close()
    finally:
        big.close()


def scatter_inputs():
    rnd = random.Random(0x5CA7)
    rand = mc.Layout("random_3000", [([rnd.randrange(R) for _ in range(3000)], [i % 64 for i in range(3000)], 1)])
    out = [mc.tiles(n) for n in mc.TILE_SIZES] + [mc.signs()]
    out += [mc.slice_walk(name, w) for w in mc.SLICE_WALK_WINDOWS for name in mc.SLICE_WALKS]
    return out + mc.joins(cancel=True) + [mc.stage_edge(), rand]


def test_scatter_route_equals_the_oracle_and_the_two_level_placement(scatter_pair):
    """k_scatter places straight from the tile histograms: the same bytes through both routes, and both against the
    oracle.  No run has n > 2^24: point indices of 2^24 and above in `sorted` stay untested at this size."""
    from oracle.c import binding as ob
    big, small = scatter_pair
    assert SMALL_CAPACITY >= 1 << 14
    wrong = []
    for lay in scatter_inputs():
        data = mc.built(lay)
        one_pass, two_level = run(big, data), run(small, data)
        if not one_pass == two_level == data[3]:
            wrong.append((lay.name, one_pass == data[3], two_level == data[3]))
    seed, n = 0x5CA77E4, 1 << 14
    for mode in (0, 1, 2, 3):
        want = ob.msm_expected(seed, 0, n, mode)
        for m in (big, small):
            m.generate(seed, 0, n, mode)
            if m.combine([m.run_windows()[0]]) != want:
                wrong.append(("generate mode %d" % mode, m is big))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------ refusals
def _with(raw, at, value):
    return raw[:at] + value.to_bytes(32, "little") + raw[at + 32:]


@pytest.mark.parametrize("group", [1, 2])
def test_refusals_leave_the_loaded_points_alone(group):
    lay = mc.slice_walk("5_long_long", MID_WINDOW)
    points, scalars, n, expected = mc.built(lay, group)
    pb = mc.point_bytes(group)
    m = msm_class(group)(n)
    try:
        assert run(m, (points, scalars, n, expected)) == expected
        first, last = m.fetch(0, 1), m.fetch(n - 1, 1)

        def refused(message, call, *args):
            with pytest.raises(RLNError, match=re.escape(message)):
                call(*args)
            # the loaded data and n are what they were
            assert m.fetch(0, 1) == first and m.fetch(n - 1, 1) == last
            with pytest.raises(RLNError, match=re.escape("MSM fetch: range outside the loaded points")):
                m.fetch(n - 1, 2)
            assert m.combine([m.run_windows()[0]]) == expected, message

        # what a refused call must not load: other points (rotated by one) under other scalars, fewer of them
        k = n - 7
        other_p, other_s = (points[pb:] + points[:pb])[:pb * k], (scalars[32 * 3:] + scalars[:32 * 3])[:32 * k]
        refused("MSM larger than the workspace", m.set_raw, points + points[:pb], scalars + scalars[:32], n + 1)
        for coord in range(pb // 32):      # x, y on G1; x.c0, x.c1, y.c0, y.c1 on G2 -- in the LAST point
            refused("Non-canonical field element", m.set_raw, _with(other_p, pb * (k - 1) + 32 * coord, Q), other_s, k)
        refused("Non-canonical field element", m.set_raw, _with(other_p, 0, Q), other_s, k)
        refused("Non-canonical field element: value is not in [0, r-1]", m.set_raw, other_p, _with(other_s, 32 * (k - 1), R), k)
        refused("Non-canonical field element: value is not in [0, r-1]", m.set_raw, other_p[:2 * pb], _with(other_s[:64], 0, R), 2)
        refused("MSM fetch: range outside the loaded points", m.fetch, n - 1, 2)
        refused("MSM fetch: range outside the loaded points", m.fetch, n, 1)
        refused("MSM fetch: range outside the loaded points", m.fetch, (1 << 64) - 1, 2)    # first + count wraps to 1
        refused("MSM larger than the workspace", m.generate, 1, 0, n + 1)
        # and the other input, unspoiled, is accepted and replaces the first
        m.set_raw(other_p, other_s, k)
        assert m.fetch(0, 1) != first
        with pytest.raises(RLNError, match=re.escape("MSM fetch: range outside the loaded points")):
            m.fetch(k - 1, 2)
    finally:
        m.close()
