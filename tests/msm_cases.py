"""Inputs of the variable-base MSM (zerokit_amd/csrc/msm_impl.h) chosen by LAYOUT -- which bucket of which window
receives how many entries -- and a host model of the plan the kernels derive from such an input.  No GPU here.

The constants are read from msm_impl.h, so a later change of one moves the cases with it.  plan() follows the comments
of the header (counting sort in window-major order, partitions of PART_NB buckets staged through LDS up to PART_CAP
entries, slices of SLICE sorted entries, buckets cut into more than BIG_SLICES slices listed up to BIG_CAP) and exists
to PROVE that a case reaches the branch it is named for: tests/test_msm_cases_host.py asserts its tags, the GPU tests
never look at it.  What a run must give is the closed form ((sum_i s_i k_i) mod r) G over bases k_j G with known k_j:
one big-integer sum and one scalar multiplication of oracle/pyref -- no code shared with the kernels."""
import os
import random
import re
from collections import Counter
from types import SimpleNamespace

from oracle.pyref.bn254 import G1, G1_GEN, G2, G2_GEN, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    src = open(os.path.join(ROOT, "zerokit_amd", "csrc", "msm_impl.h")).read()

    def one(pattern):
        return int(re.search(pattern, src).group(1))
    # the derived values below restate these three lines: notice when they change
    assert "MSM_W = (255 + MSM_C - 1) / MSM_C;" in src and "MSM_NB = 1u << (MSM_C - 1);" in src
    assert "MSM_PART_NB = MSM_NB / MSM_PARTS;" in src
    return (one(r"#define RLN_MSM_C (\d+)"), one(r"MSM_TILES = (\d+)[;,]"), one(r"MSM_PARTS = (\d+)[;,]"),
            one(r"MSM_PART_CAP = (\d+)[;,]"), one(r"MSM_SLICE = (\d+)[;,]"), one(r"MSM_BIG_SLICES = (\d+)[;,]"),
            one(r"MSM_BIG_CAP = (\d+)[;,]"))


MSM_C, MSM_TILES, MSM_PARTS, MSM_PART_CAP, MSM_SLICE, MSM_BIG_SLICES, MSM_BIG_CAP = _constants()
W = (255 + MSM_C - 1) // MSM_C
NB = 1 << (MSM_C - 1)
PART_NB = NB // MSM_PARTS
TOP_LIMIT = R >> (MSM_C * (W - 1))      # digits of the top window stay below this (0x3064 at c = 16)
_MASK = (1 << MSM_C) - 1


# ------------------------------------------------------------------------------------------ digits
def _recode(s):
    """-> (signed digits, raw digits before the carry, carry into each window)"""
    digits, raws, carries, carry = [], [], [], 0
    for w in range(W):
        raw = (s >> (MSM_C * w)) & _MASK
        raws.append(raw)
        carries.append(carry)
        raw += carry
        if raw > NB:                 # above the half: the negative digit and a carry; the half itself stays positive
            digits.append(raw - (1 << MSM_C))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
    assert carry == 0 and s >> (MSM_C * W) == 0, "scalar does not fit the windows"
    return digits, raws, carries


def recode(s):
    """signed digits d_w in (-2^(c-1), 2^(c-1)] with sum(d_w << (c * w)) == s, from the bottom window up"""
    return _recode(s)[0]


def scalar_for(digits):
    """the scalar whose recoding is exactly the {window: signed digit} plan (every other digit zero).  A negative digit
    is only reachable through the carry rule: the plan has to name what the carry leaves in the next window."""
    s = sum(d << (MSM_C * w) for w, d in digits.items())
    assert 0 <= s < R, "not a scalar: %r" % (digits,)
    assert digits.get(W - 1, 0) < TOP_LIMIT
    assert recode(s) == [digits.get(w, 0) for w in range(W)], "not a recoding: %r" % (digits,)
    return s


# ------------------------------------------------------------------------------------------ the model
SLICE_TAGS = (
    "inside",                      # a bucket that starts and ends inside the slice: flushed to buckets[] in the walk
    "head_at_bucket_end",          # a bucket from an earlier slice ends inside this one: head[s] in the walk
    "slice_inside_bucket",         # the slice lies wholly inside one bucket: head[s] at the slice end, the bucket runs on
    "head_ends_at_slice_end",      # a bucket from an earlier slice ends exactly at the slice end: head[s]
    "tail",                        # a bucket starts inside the slice and runs past it: tail[s]
    "tail_from_slice_start",       # ... and starts exactly at the slice start
    "ends_at_slice_end",           # a bucket that started here ends exactly at the slice end: buckets[] after the walk
    "whole_slice_bucket",          # ... and also started exactly at the slice start
    "head_and_tail_in_one_slice",
    "skip_empty_in_walk",          # empty buckets skipped at a boundary inside the slice
    "skip_hundreds_empty",
    "skip_empty_at_slice_start",   # a boundary on the slice start with empty buckets behind it (the search skips them)
    "window_crossing_adjacent",    # the last bucket of a window followed directly by the first of the next
    "last_slice_short",
    "total_multiple_of_slice",
    "total_one",
)
JOIN_TAGS = ("join_none", "join_serial", "join_serial_at_limit", "join_listed_just_above", "join_listed",
             "join_overflow", "joined_bucket_ends_at_slice_end", "joined_bucket_starts_at_slice_start")
PART_TAGS = ("part_staged", "part_at_cap", "part_cap_plus_1", "part_unstaged", "part_unstaged_between_staged")
DIGIT_TAGS = ("digit_negative", "carry_alone_fills_bucket_0", "digit_plus_half", "digit_most_negative",
              "digit_zero_under_carry", "carry_through_every_window")
TILE_TAGS = ("tile_full", "tile_short", "tile_empty", "tiles_all_full")
ALL_TAGS = SLICE_TAGS + JOIN_TAGS + PART_TAGS + DIGIT_TAGS + TILE_TAGS


def plan(scalars):
    """scalars: a list, or {scalar: how many points carry it}.  -> the plan: per (window, bucket) counts, negatives and
    offsets; per partition (length, staged); per bucket (s0, s1, how); listed / overflow; per slice its outcomes; and
    `tags`, everything reached."""
    mult = scalars if isinstance(scalars, dict) else Counter(scalars)
    n = sum(mult.values())
    counts, neg, tags = Counter(), Counter(), set()
    for s, k in mult.items():
        digits, raws, carries = _recode(s)
        for w, d in enumerate(digits):
            if d:
                counts[(w, abs(d) - 1)] += k
            if d < 0:
                neg[(w, -d - 1)] += k
                tags.add("digit_negative")
                if raws[w + 1] == 0 and digits[w + 1] == 1:
                    tags.add("carry_alone_fills_bucket_0")
            if d == NB:
                tags.add("digit_plus_half")
            if d == 1 - NB:
                tags.add("digit_most_negative")
            if d == 0 and raws[w] == _MASK and carries[w]:
                tags.add("digit_zero_under_carry")
        if all(carries[1:]):
            tags.add("carry_through_every_window")
    # tiles of the histogram and placement passes
    tile_len = -(-max(n, 1) // MSM_TILES)
    tiles = [max(0, min(n, (t + 1) * tile_len) - t * tile_len) for t in range(MSM_TILES)]
    for c in tiles:
        tags.add("tile_full" if c == tile_len else "tile_short" if c else "tile_empty")
    if all(c == tile_len for c in tiles):
        tags.add("tiles_all_full")
    # offsets: window-major, buckets ascending, zero digits absent
    keys = sorted(counts)
    offs, run = {}, 0
    for k in keys:
        offs[k] = run
        run += counts[k]
    total = run
    # partitions of the two-level placement
    parts = Counter()
    for (w, b), c in counts.items():
        parts[(w, b // PART_NB)] += c
    parts = {k: (c, c <= MSM_PART_CAP) for k, c in parts.items()}
    for (w, p), (c, staged) in parts.items():
        tags.add("part_staged" if staged else "part_unstaged")
        if c == MSM_PART_CAP:
            tags.add("part_at_cap")
        if c == MSM_PART_CAP + 1:
            tags.add("part_cap_plus_1")
        if not staged and all(parts.get((w, q), (0, False))[0] and parts[(w, q)][1] for q in (p - 1, p + 1)):
            tags.add("part_unstaged_between_staged")
    # joins
    buckets, listed = {}, 0
    for k in keys:
        s0, s1 = offs[k] // MSM_SLICE, (offs[k] + counts[k] - 1) // MSM_SLICE
        if s0 == s1:
            how = "slice"
            tags.add("join_none")
        elif s1 - s0 > MSM_BIG_SLICES:
            how = "listed"
            listed += 1
            tags.add("join_listed")
            if s1 - s0 == MSM_BIG_SLICES + 1:
                tags.add("join_listed_just_above")
        else:
            how = "serial"
            tags.add("join_serial")
            if s1 - s0 == MSM_BIG_SLICES:
                tags.add("join_serial_at_limit")
        if s0 != s1:
            if (offs[k] + counts[k]) % MSM_SLICE == 0:
                tags.add("joined_bucket_ends_at_slice_end")
            if offs[k] % MSM_SLICE == 0:
                tags.add("joined_bucket_starts_at_slice_start")
        buckets[k] = (s0, s1, how)
    overflow = max(0, listed - MSM_BIG_CAP)
    if overflow:
        tags.add("join_overflow")     # that many of the listed are joined serially; WHICH is the order of an atomic
    # the walk of every slice
    gkey = [w * NB + b for w, b in keys]
    slices, i = [], 0
    for s in range(-(-total // MSM_SLICE)):
        lo, hi = s * MSM_SLICE, min((s + 1) * MSM_SLICE, total)
        while offs[keys[i]] + counts[keys[i]] <= lo:
            i += 1
        out = set()
        if s and offs[keys[i]] == lo and gkey[i] - gkey[i - 1] > 1:
            out.add("skip_empty_at_slice_start")
        k = i
        while k < len(keys) and offs[keys[k]] < hi:
            st, en = offs[keys[k]], offs[keys[k]] + counts[keys[k]]
            before = st < lo
            if en < hi:
                out.add("head_at_bucket_end" if before else "inside")
                gap = gkey[k + 1] - gkey[k] - 1      # (en < hi <= total: a next bucket exists)
                if gap:
                    out.add("skip_empty_in_walk")
                if gap >= 100:
                    out.add("skip_hundreds_empty")
                if not gap and keys[k + 1][0] != keys[k][0]:
                    out.add("window_crossing_adjacent")
            elif en == hi:
                out.add("head_ends_at_slice_end" if before else "ends_at_slice_end")
                if st == lo and hi - lo == MSM_SLICE:
                    out.add("whole_slice_bucket")
            else:
                out.add("slice_inside_bucket" if before else "tail")
                if st == lo:
                    out.add("tail_from_slice_start")
            k += 1
        if "head_at_bucket_end" in out and "tail" in out:
            out.add("head_and_tail_in_one_slice")
        if hi - lo < MSM_SLICE:
            out.add("last_slice_short")
        slices.append(tuple(sorted(out)))
        tags |= out
    if total and total % MSM_SLICE == 0:
        tags.add("total_multiple_of_slice")
    if total == 1:
        tags.add("total_one")
    return SimpleNamespace(n=n, total=total, counts=counts, neg=neg, offs=offs, tiles=tiles, parts=parts, buckets=buckets,
                           listed=listed, overflow=overflow, slices=slices, tags=tags)


# ------------------------------------------------------------------------------------------ bases
N_BASES = {1: 64, 2: 16}
_BASES = {}


def bases(group):
    """-> (k_j, bytes of k_j G): 64 fixed multiples of the generator on G1, 16 on G2; slot j of a layout is base
    j mod that number"""
    if group not in _BASES:
        rnd = random.Random(0xBA5E5 + group)
        ks = [rnd.randrange(1, R) for _ in range(N_BASES[group])]
        if group == 1:
            raw = [b"".join(v.to_bytes(32, "little") for v in G1.mul(G1_GEN, k)) for k in ks]
        else:
            raw = [b"".join(v.to_bytes(32, "little") for xy in G2.mul(G2_GEN, k) for v in xy) for k in ks]
        _BASES[group] = (ks, raw)
    return _BASES[group]


def point_bytes(group):
    return 64 * group


# ------------------------------------------------------------------------------------------ layouts
class Layout:
    """segments: [(scalars, slots, repeat)] -- `repeat` copies of the points (base of slot, scalar); slot None is the
    all-zero encoding of the point at infinity"""

    def __init__(self, name, segments):
        self.name = name
        self.segments = [(list(sc), list(sl), rep) for sc, sl, rep in segments if rep and len(sc)]
        assert all(len(sc) == len(sl) for sc, sl, _ in self.segments)
        self.n = sum(len(sc) * rep for sc, _, rep in self.segments)

    def multiset(self):
        m = Counter()
        for sc, _, rep in self.segments:
            for s in sc:
                m[s] += rep
        return m

    def plan(self):
        return plan(self.multiset())

    def __repr__(self):
        return "%s (n = %d)" % (self.name, self.n)


def build(layout, group=1):
    """-> (points_bytes, scalars_bytes, n, expected); expected = ((sum_i s_i k_base(i)) mod r) G, None for infinity"""
    ks, raw = bases(group)
    nb, zero = len(ks), bytes(point_bytes(group))
    pts, scs, acc = [], [], 0
    for sc, sl, rep in layout.segments:
        pts.append(b"".join(zero if j is None else raw[j % nb] for j in sl) * rep)
        scs.append(b"".join(s.to_bytes(32, "little") for s in sc) * rep)
        acc += rep * sum(s * ks[j % nb] for s, j in zip(sc, sl) if j is not None)
    acc %= R
    if group == 1:
        expected = G1.mul(G1_GEN, acc) if acc else None
    else:
        expected = G2.mul(G2_GEN, acc) if acc else None
    return b"".join(pts), b"".join(scs), layout.n, expected


def materialise(points_bytes, scalars_bytes, n, group=1):
    """the bytes back as ([point or None], [scalar]) in the oracle's form"""
    pb = point_bytes(group)
    assert len(points_bytes) == pb * n and len(scalars_bytes) == 32 * n
    pts = []
    for i in range(n):
        v = [int.from_bytes(points_bytes[pb * i + 32 * k:pb * i + 32 * k + 32], "little") for k in range(pb // 32)]
        pts.append(None if not any(v) else (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3])))
    return pts, [int.from_bytes(scalars_bytes[32 * i:32 * i + 32], "little") for i in range(n)]


def _run(scalar, count, first_slot=0):
    """`count` points with one scalar on the slots first_slot, first_slot + 1, ...: whole periods of 64, then the rest"""
    slots = [(first_slot + j) % 64 for j in range(64)]
    return [([scalar] * 64, slots, count // 64), ([scalar] * (count % 64), slots[:count % 64], 1)]


# ---- tiles
TILE_SIZES = (1, MSM_TILES - 1, MSM_TILES, MSM_TILES + 1, 2 * MSM_TILES - 1)


def tiles(n):
    """n random scalars on distinct bases (G1; G2 has 16 bases): tile length ceil(n / TILES), empty and short tiles"""
    rnd = random.Random(0x711E5 + n)
    return Layout("tiles/%d" % n, [([rnd.randrange(R) for _ in range(n)], range(n), 1)])


# ---- slice_walk
_S = MSM_SLICE
# name -> [(window step, bucket, entries)]; single-window scalars, so the sorted list is exactly this
SLICE_WALKS = {
    "one_full_slice": [(0, 0, _S)],
    "s-1_1": [(0, 0, _S - 1), (0, 1, 1)],
    "1_s-1_s_3": [(0, 7, 1), (0, 300, _S - 1), (0, 301, _S), (0, 900, 3)],
    "5_long_2": [(0, 3, 5), (0, 4, 2 * _S + 44), (0, 700, 2)],
    "5_long_long": [(0, 3, 5), (0, 4, 2 * _S + 44), (0, 1200, _S + 72)],
    "total_1": [(0, 41, 1)],
    "two_slices_exactly": [(0, 0, _S - 28), (0, 2, _S + 28)],
    "s_then_long": [(0, 9, _S), (0, 600, _S + 72)],
    "window_edge": [(0, NB - 1, 70), (1, 0, 100)],
    "window_gap": [(0, 5, 10), (2, 9, 20)],
}
SLICE_WALK_WINDOWS = (0, W // 2 - 1, W - 1)


def slice_walk(name, w):
    """the layout `name` in window w.  The two layouts that cross windows start 1 (2) windows lower where w is the top
    window; NB - 1, the last bucket of a window, does not exist in the top one (digits < TOP_LIMIT)"""
    spec = SLICE_WALKS[name]
    w0 = min(w, W - 1 - max(step for step, _, _ in spec))
    segs = []
    for k, (step, bucket, entries) in enumerate(spec):
        segs += _run(scalar_for({w0 + step: bucket + 1}), entries, first_slot=5 * k)
    return Layout("slice_walk/%s/w%d" % (name, w), segs)


# ---- signs
def signs():
    half = NB
    plans = [{0: -5, 1: 1}, {3: half}, {3: -(half - 1), 4: 1}, {0: -3, 2: 1}, {0: -1, W - 1: 1},
             dict([(w, -7) for w in range(W - 1)] + [(W - 1, 5)]), {W - 2: -half + 1, W - 1: TOP_LIMIT - 1},
             {0: half, 1: half, 2: -2, 3: 1}]
    sc = [scalar_for(p) for p in plans] + [0, 1, half, half + 1, (1 << MSM_C) - 1, 0xFFFF8000FFFF, R - 1, R - 2]
    rnd = random.Random(0x5167)
    sc += [rnd.randrange(R) for _ in range(8)]
    return Layout("signs", [(sc, range(len(sc)), 1), (sc, range(7, 7 + len(sc)), 1), (sc[::-1], range(len(sc)), 1)])


# ---- join_64_65 and cancel
JOIN_WINDOW = W // 2
JOIN_SMALL = (0, 5, MSM_SLICE)


def join_length(diff, m0, exact_end):
    """the shortest bucket after m0 entries that is cut so that s1 - s0 == diff, or the one that also ends on a slice end"""
    s0 = m0 // MSM_SLICE
    return (s0 + diff + 1) * MSM_SLICE - m0 if exact_end else (s0 + diff) * MSM_SLICE + 1 - m0


def join(diff, m0, exact_end, cancel=False):
    w, L = JOIN_WINDOW, join_length(diff, m0, exact_end)
    segs = _run(scalar_for({w: 11}), m0)
    if not cancel:
        segs += _run(scalar_for({w: 12}), L, first_slot=3)
    else:
        # +d and -d of ONE base, and one entry that is the point at infinity; -d is a carry into the next window
        plus, minus = scalar_for({w: 12}), scalar_for({w: -12, w + 1: 1})
        segs += [([plus], [None], 1), ([plus, minus], [17, 17], (L - 1) // 2), ([plus] * ((L - 1) % 2), [17] * ((L - 1) % 2), 1)]
    return Layout("%s/%d/m%d/%s" % ("cancel" if cancel else "join", diff, m0, "exact" if exact_end else "min"), segs)


def joins(cancel=False):
    return [join(diff, m0, exact, cancel) for diff in (MSM_BIG_SLICES, MSM_BIG_SLICES + 1) for m0 in JOIN_SMALL
            for exact in (False, True)]


# ---- stage_edge
STAGE_WINDOWS = (0, W // 2 - 1, W - 1)
STAGE_PARTS = (300, 17, 100)


def _spread(total, sizes):
    return [total - sum(sizes)] + list(sizes)


def stage_edge():
    """every point has a digit in the bottom, a middle and the top window.  Bottom: partition 300 receives exactly
    PART_CAP entries over 8 of its buckets (first and last included), both signs; middle: partition 17 receives
    PART_CAP + 1 over 5; top: partition 100 lies above the cap between two small ones.  The rest of each window goes
    to a neighbouring partition."""
    n = MSM_PART_CAP + 432
    wa, wb, wc = STAGE_WINDOWS
    pa, pb, pc = STAGE_PARTS

    def digits(runs):
        out = []
        for d, c in runs:
            out += [d] * c
        assert len(out) == n
        return out
    a_sizes = _spread(MSM_PART_CAP, [1, 2, 37, 300, 1500, 4000, 9000])
    a = digits([((-1) ** k * (pa * PART_NB + off + 1), c) for k, (off, c) in enumerate(zip((0, 1, 5, 13, 31, 40, 62, 63), a_sizes))]
               + [((pa + 1) * PART_NB + 9, n - MSM_PART_CAP)])
    b_sizes = _spread(MSM_PART_CAP + 1, [3, 500, 6000, 10000])
    b = digits([((-1) ** k * (pb * PART_NB + off + 1), c) for k, (off, c) in enumerate(zip((63, 0, 20, 21, 50), b_sizes))]
               + [((pb - 1) * PART_NB + 64, n - MSM_PART_CAP - 1)])
    c_sizes = _spread(n - 200, [1, 777, 5000])
    c = digits([(pc * PART_NB + off + 1, k) for off, k in zip((2, 3, 33, 63), c_sizes)]
               + [((pc - 1) * PART_NB + 64, 100), ((pc + 1) * PART_NB + 1, 100)])
    sc = []
    for i in range(n):
        da, db = a[i], b[i * 7919 % n]
        d = {wa: da, wb: db, wc: c[i * 104729 % n]}
        if da < 0:
            d[wa + 1] = 1
        if db < 0:
            d[wb + 1] = 1
        sc.append(scalar_for(d))
    return Layout("stage_edge", [(sc, [i % 64 for i in range(n)], 1)])


# ---- big_overflow
def big_overflow():
    """more listed buckets than the list holds: BIG_CAP / W + 1 distinct scalars, the digits of scalar j a permutation
    of 1 .. that number which differs per window (no carries, every window contiguous), each scalar often enough that
    its bucket spans more than BIG_SLICES slices wherever it starts"""
    k = MSM_BIG_CAP // W + 1
    entries = (MSM_BIG_SLICES + 1) * MSM_SLICE + 1
    assert all(k % p for p in range(2, W + 2)), "the multipliers below must be units mod k"
    sc = [scalar_for({w: 1 + (j * (w + 1) + 3 * w) % k for w in range(W)}) for j in range(k)]
    period = 64 * k
    return Layout("big_overflow", [([sc[i % k] for i in range(period)], [i % 64 for i in range(period)], -(-entries // 64))])


def small_cases():
    """every named case but big_overflow, smallest first within its kind"""
    out = [tiles(n) for n in TILE_SIZES]
    out += [slice_walk(name, w) for w in SLICE_WALK_WINDOWS for name in SLICE_WALKS]
    out += [signs()] + joins() + joins(cancel=True) + [stage_edge()]
    return out


_BUILT = {}


def built(layout, group=1):
    """build(), once per (case, group) and session: shared by the tests, never written"""
    key = (layout.name, group)
    if key not in _BUILT:
        _BUILT[key] = build(layout, group)
    return _BUILT[key]
