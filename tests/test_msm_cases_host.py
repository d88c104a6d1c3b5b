"""tests/msm_cases.py judged on the host: the recoding holds its identity, every named case makes the model report the
branch in its name, the cases together reach everything the model knows, and the closed form of the small cases equals
the oracle's naive MSM over the points and scalars read back from the bytes."""
import pytest

import msm_cases as mc
from oracle.pyref.bn254 import G1, G1_GEN, G2, R

C, NB, S = mc.MSM_C, mc.NB, mc.MSM_SLICE


def test_constants_are_the_headers():
    assert (mc.W, mc.NB, mc.PART_NB) == ((255 + C - 1) // C, 1 << (C - 1), (1 << (C - 1)) // mc.MSM_PARTS)
    assert mc.W * C >= 255 and mc.PART_NB * mc.MSM_PARTS == mc.NB
    if C == 16:
        assert mc.TOP_LIMIT == 0x3064


def test_recode_identity_and_range_on_the_edge_scalars():
    top = (1 << (C * (mc.W - 1))) - 1          # all-ones below the top window
    for s in (0, 1, NB, NB + 1, (1 << C) - 1, 0xFFFF8000FFFF, R - 1, top, top + 1, R - 2, NB - 1, (NB + 1) << C):
        d = mc.recode(s)
        assert len(d) == mc.W and sum(v << (C * w) for w, v in enumerate(d)) == s, hex(s)
        assert all(-NB < v <= NB for v in d), hex(s)
    assert mc.recode(NB)[:2] == [NB, 0]                         # the half stays positive
    assert mc.recode(NB + 1)[:2] == [-(NB - 1), 1]              # above it: negative, and a carry
    assert mc.recode((1 << C) - 1)[:2] == [-1, 1]
    assert mc.recode(0xFFFF8000FFFF)[:4] == [-1, -NB + 1, 0, 1] if C == 16 else True
    assert mc.recode(top) == [-1] + [0] * (mc.W - 2) + [1]      # the carry runs through every window
    assert mc.scalar_for({0: -5, 1: 1}) == (1 << C) - 5
    with pytest.raises(AssertionError):
        mc.scalar_for({0: -5})                                  # a negative digit needs its carry named
    with pytest.raises(AssertionError):
        mc.scalar_for({mc.W - 1: mc.TOP_LIMIT})                 # >= r


def test_plan_on_a_hand_made_input():
    """three scalars worked out by hand (c = 16 notation, but stated through the constants)"""
    sc = [mc.scalar_for({0: 3}), mc.scalar_for({0: 3, 2: 9}), mc.scalar_for({0: -4, 1: 1})]
    p = mc.plan(sc)
    assert p.n == 3 and p.total == 5
    assert dict(p.counts) == {(0, 2): 2, (0, 3): 1, (1, 0): 1, (2, 8): 1} and dict(p.neg) == {(0, 3): 1}
    assert p.offs == {(0, 2): 0, (0, 3): 2, (1, 0): 3, (2, 8): 4}
    assert p.parts == {(0, 0): (3, True), (1, 0): (1, True), (2, 0): (1, True)}
    assert all(v == (0, 0, "slice") for v in p.buckets.values()) and p.listed == 0 and p.overflow == 0
    assert p.slices == [("ends_at_slice_end", "inside", "last_slice_short", "skip_empty_in_walk", "skip_hundreds_empty")]
    assert p.tiles == [1, 1, 1] + [0] * (mc.MSM_TILES - 3)
    assert mc.plan({sc[0]: 2, sc[2]: 1}).counts == mc.plan([sc[0], sc[0], sc[2]]).counts


@pytest.mark.parametrize("n", mc.TILE_SIZES)
def test_tiles_reach_empty_short_and_full_tiles(n):
    p = mc.tiles(n).plan()
    T, tl = mc.MSM_TILES, -(-n // mc.MSM_TILES)
    assert p.n == n and sum(p.tiles) == n and max(p.tiles) == tl
    want = {1: {"tile_full", "tile_empty"}, T - 1: {"tile_full", "tile_empty"}, T: {"tile_full", "tiles_all_full"},
            T + 1: {"tile_full", "tile_short", "tile_empty"}, 2 * T - 1: {"tile_full", "tile_short"}}[n]
    assert p.tags & set(mc.TILE_TAGS) == want


SLICE_WALK_TAGS = {
    "one_full_slice": {"whole_slice_bucket", "ends_at_slice_end", "total_multiple_of_slice"},
    "s-1_1": {"inside", "ends_at_slice_end", "total_multiple_of_slice"},
    "1_s-1_s_3": {"inside", "ends_at_slice_end", "whole_slice_bucket", "skip_empty_at_slice_start", "skip_hundreds_empty",
                  "last_slice_short"},
    "5_long_2": {"inside", "tail", "slice_inside_bucket", "head_at_bucket_end", "skip_hundreds_empty", "last_slice_short"},
    "5_long_long": {"head_and_tail_in_one_slice", "head_ends_at_slice_end", "slice_inside_bucket"},
    "total_1": {"total_one", "ends_at_slice_end", "last_slice_short"},
    "two_slices_exactly": {"tail", "head_ends_at_slice_end", "total_multiple_of_slice", "skip_empty_in_walk"},
    "s_then_long": {"whole_slice_bucket", "tail_from_slice_start", "head_ends_at_slice_end", "skip_empty_at_slice_start"},
    "window_edge": {"window_crossing_adjacent", "inside", "tail"},
    "window_gap": {"skip_hundreds_empty", "inside"},
}


@pytest.mark.parametrize("w", mc.SLICE_WALK_WINDOWS)
@pytest.mark.parametrize("name", list(mc.SLICE_WALKS))
def test_slice_walk_layouts_are_the_sorted_list_and_reach_their_outcomes(name, w):
    lay = mc.slice_walk(name, w)
    p = lay.plan()
    spec = mc.SLICE_WALKS[name]
    w0 = min(w, mc.W - 1 - max(step for step, _, _ in spec))
    assert w0 == w or w == mc.W - 1
    # single-window scalars: the sorted list is exactly the layout
    assert dict(p.counts) == {(w0 + step, b): c for step, b, c in spec} and p.total == lay.n == sum(c for _, _, c in spec)
    assert not p.neg
    assert SLICE_WALK_TAGS[name] <= p.tags, SLICE_WALK_TAGS[name] - p.tags


def test_slice_walk_reaches_every_outcome_of_the_walk():
    for w in mc.SLICE_WALK_WINDOWS:
        reached = set()
        for name in mc.SLICE_WALKS:
            reached |= mc.slice_walk(name, w).plan().tags
        assert set(mc.SLICE_TAGS) <= reached, (w, set(mc.SLICE_TAGS) - reached)


def test_signs_show_the_carry_rule():
    lay = mc.signs()
    p = lay.plan()
    assert set(mc.DIGIT_TAGS) <= p.tags, set(mc.DIGIT_TAGS) - p.tags
    # -5 in window 0 is raw 2^c - 5 and leaves +1 in window 1's bucket 0
    q = mc.plan([mc.scalar_for({0: -5, 1: 1})])
    assert dict(q.counts) == {(0, 4): 1, (1, 0): 1} and dict(q.neg) == {(0, 4): 1}
    # raw all-ones under a carry: a zero digit (absent from the list) and the carry goes on
    q = mc.plan([mc.scalar_for({0: -3, 2: 1})])
    assert dict(q.counts) == {(0, 2): 1, (2, 0): 1} and "digit_zero_under_carry" in q.tags
    q = mc.plan([mc.scalar_for({0: -1, mc.W - 1: 1})])
    assert dict(q.counts) == {(0, 0): 1, (mc.W - 1, 0): 1} and "carry_through_every_window" in q.tags
    assert p.counts[(3, NB - 1)] >= 3 and p.neg[(3, NB - 2)] >= 3        # 2^(c-1) exactly, -(2^(c-1) - 1)


@pytest.mark.parametrize("cancel", [False, True])
def test_join_cases_sit_on_both_sides_of_the_listing_limit(cancel):
    seen = []
    for lay in mc.joins(cancel):
        _, diff, m0, end = lay.name.split("/")
        diff, m0 = int(diff), int(m0[1:])
        p = lay.plan()
        w = mc.JOIN_WINDOW
        s0, s1, how = p.buckets[(w, 11)]
        assert s1 - s0 == diff and how == ("listed" if diff > mc.MSM_BIG_SLICES else "serial"), lay
        assert p.counts[(w, 10)] == m0 and p.offs[(w, 11)] == m0
        L = p.counts[(w, 11)]
        assert 8000 < lay.n < 8700 + (L if cancel else 0)
        assert ((m0 + L) % S == 0) == (end == "exact")
        if end == "min":      # one entry fewer and the bucket is cut into one slice fewer
            assert (m0 + L - 2) // S - s0 == diff - 1
        if not cancel:        # (with cancel the carries' bucket in the next window is joined too)
            assert ("joined_bucket_starts_at_slice_start" in p.tags) == (m0 % S == 0)
            assert ("joined_bucket_ends_at_slice_end" in p.tags) == (end == "exact")
        assert p.listed == (diff > mc.MSM_BIG_SLICES) and p.overflow == 0
        if cancel:
            assert p.neg[(w, 11)] == (L - 1) // 2 and p.counts[(w + 1, 0)] == (L - 1) // 2
            assert sum(sl.count(None) for _, sl, _ in lay.segments) == 1
            small = mc.scalar_for({w: 11})
            assert {j for sc, sl, _ in lay.segments if sc[0] != small for j in sl} == {None, 17}     # ONE base
        seen.append((diff, m0, end))
    assert len(set(seen)) == 12 and {d for d, _, _ in seen} == {mc.MSM_BIG_SLICES, mc.MSM_BIG_SLICES + 1}


def test_stage_edge_partitions_sit_on_the_cap():
    lay = mc.stage_edge()
    p = lay.plan()
    assert 33000 <= lay.n <= 70000 or mc.MSM_PART_CAP != 32768
    (wa, wb, wc), (pa, pb, pc) = mc.STAGE_WINDOWS, mc.STAGE_PARTS
    assert p.parts[(wa, pa)] == (mc.MSM_PART_CAP, True)
    assert p.parts[(wb, pb)] == (mc.MSM_PART_CAP + 1, False)
    assert not p.parts[(wc, pc)][1] and p.parts[(wc, pc - 1)] == (100, True) and p.parts[(wc, pc + 1)] == (100, True)
    assert {"part_at_cap", "part_cap_plus_1", "part_unstaged_between_staged", "part_staged", "part_unstaged"} <= p.tags
    in_a = {b: c for (w, b), c in p.counts.items() if w == wa and b // mc.PART_NB == pa}
    assert len(in_a) >= 8 and len(set(in_a.values())) >= 8                  # spread unevenly
    assert {pa * mc.PART_NB, pa * mc.PART_NB + mc.PART_NB - 1} <= set(in_a)  # first and last bucket of the partition
    negs = [p.neg[(wa, b)] for b in in_a]
    assert any(v == in_a[b] for v, b in zip(negs, in_a)) and any(v == 0 for v in negs)   # both signs
    # staged and unstaged partitions side by side in one window
    assert p.parts[(wa, pa + 1)][1] and p.parts[(wb, pb - 1)][1]


def test_big_overflow_lists_more_than_the_list_holds():
    lay = mc.big_overflow()
    p = lay.plan()
    k = mc.MSM_BIG_CAP // mc.W + 1
    assert len(p.counts) == mc.W * k and p.listed == mc.W * k > mc.MSM_BIG_CAP and p.overflow >= 1
    assert all(how == "listed" for _, _, how in p.buckets.values())
    assert min(p.counts.values()) >= (mc.MSM_BIG_SLICES + 1) * S + 1 and not p.neg
    assert {b for _, b in p.counts} == set(range(k))                       # every window contiguous
    assert "join_overflow" in p.tags
    if (C, mc.MSM_BIG_CAP, mc.MSM_BIG_SLICES, S) == (16, 4096, 64, 128):
        assert lay.n == 2154688 and set(p.counts.values()) == {8384}
    # one scalar fewer and the list is no longer overflowed
    assert mc.W * (k - 1) <= mc.MSM_BIG_CAP


def test_the_cases_cover_the_plan():
    reached = set()
    for lay in mc.small_cases() + [mc.big_overflow()]:
        reached |= lay.plan().tags
    assert set(mc.ALL_TAGS) - reached == set() and reached - set(mc.ALL_TAGS) == set()


def test_closed_form_equals_the_naive_msm_over_the_materialised_points():
    """every case of at most 4 096 points, on G1; on G2 the tiles, the signs and one walk (the same builder)"""
    small = [lay for lay in mc.small_cases() if lay.n <= 4096]
    assert len(small) >= len(mc.TILE_SIZES) + 3 * len(mc.SLICE_WALKS) + 1
    for lay in small:
        pb, sb, n, expected = mc.built(lay)
        pts, sc = mc.materialise(pb, sb, n)
        assert n == lay.n and all(G1.on_curve(P) for P in pts[:64])
        assert sorted(sc) == sorted(lay.multiset().elements())
        assert G1.msm_naive(pts, sc) == expected, lay
    for lay in [mc.tiles(n) for n in mc.TILE_SIZES] + [mc.signs(), mc.slice_walk("5_long_2", 0)]:
        pb, sb, n, expected = mc.built(lay, 2)
        pts, sc = mc.materialise(pb, sb, n, 2)
        assert all(G2.on_curve(P) for P in pts[:16])
        assert G2.msm_naive(pts, sc) == expected, lay


def test_cancel_sums_and_the_infinity_entry():
    """the big bucket of a cancel case sums to infinity or to one point; the whole case is what the small bucket and
    the carries leave"""
    ks, _ = mc.bases(1)
    for lay in mc.joins(cancel=True)[:4]:
        _, _, n, expected = mc.built(lay)
        w, p = mc.JOIN_WINDOW, lay.plan()
        L, m0 = p.counts[(w, 11)], p.counts[(w, 10)]
        pairs = (L - 1) // 2
        big = 12 * ((L - 1) % 2) * ks[17] << (C * w)                        # what the +d / -d bucket leaves
        carries = pairs * ks[17] << (C * (w + 1))
        small = sum(11 * ks[j % 64] for j in range(m0)) << (C * w)
        v = (big + carries + small) % R
        assert expected == (G1.mul(G1_GEN, v) if v else None), lay
