"""The HBM-resident Poseidon tree (zerokit_amd/csrc/merkle.hip) at every size at which it chooses another kernel, against
the host model of tests/tree_model.py (oracle/c's Poseidon on a heap of Python ints; judged itself by
tests/test_tree_model_host.py).  Everything is bit-exact.

The trees hold pairwise distinct, non-default leaves (on an all-default tree every node of a level is equal and a wrong
node index still finds the right value), and the judge is assert_tree_equals: the root and the paths of ALL leaves.
Every node but the root is some leaf's sibling, so that compares the whole tree.

  range emission   k_proofs_lds when count * depth >= 2^(depth + 1) - 1, k_proofs below: both sides of that switch at an
                   odd first leaf, single paths, a block that straddles the middle of the tree, a short last block
  range rebuild    k_hash_parents_l3 up to 16 384 parents in a level, k_hash_parents above: 16 384, 16 385 and 20 001
                   parents from ragged ranges, one after the other on one handle
  fill_sequential  off leaf 0, values across the 32-bit limb boundary
  one handle       set / set_leaves (host chain and device pass) / set_range / fill_sequential mixed with reads
  edge operands    all ordered pairs of {0, 1, 2, r - 2, r - 1, 2^253} as siblings through the three hash forms
  the guard        first + count that wraps around 2^64 is refused on the host

The models are computed once per session and copied by the tests that write; the file's time is the C oracle's."""
import random

import pytest

from tree_model import R, TreeModel
from zerokit_amd._native import RLNError

pytestmark = pytest.mark.gpu

EDGE = [0, 1, 2, R - 2, R - 1, 1 << 253]
EDGE_PAIRS = [v for a in EDGE for b in EDGE for v in (a, b)]      # 36 ordered pairs as 72 sibling leaves

_BASE = {}


def distinct_leaves(rnd, n):
    leaves = [rnd.randrange(1, R) for _ in range(n)]
    assert len(set(leaves)) == n
    return leaves


def base(depth):
    """(leaves, model) of a full tree of distinct random leaves; shared, never written: writers take model.copy()"""
    if depth not in _BASE:
        leaves = distinct_leaves(random.Random(0x7EE0 + depth), 1 << depth)
        model = TreeModel(depth)
        model.set_range(0, leaves)
        _BASE[depth] = (leaves, model)
    return _BASE[depth]


def device_tree(depth):
    from zerokit_amd.batch import PoseidonTree
    dev = PoseidonTree(depth)
    dev.set_range(0, base(depth)[0])
    return dev


def assert_same_bytes(got, want, what):
    if got != want:
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        pytest.fail("%s: %d bytes for %d expected, first difference at byte %d" % (what, len(got), len(want), at))


def assert_range_equals(dev, model, first, count, what=""):
    elems, bits = dev.proofs_raw(first, count)
    want_elems, want_bits = model.proofs_bytes(first, count)
    assert_same_bytes(bits, want_bits, "%s path bits of [%d, +%d) at depth %d" % (what, first, count, model.depth))
    assert_same_bytes(elems, want_elems, "%s path elements of [%d, +%d) at depth %d" % (what, first, count, model.depth))


def assert_tree_equals(dev, model, what=""):
    assert dev.root() == model.root(), what
    assert_range_equals(dev, model, 0, 1 << model.depth, what)


# ------------------------------------------------------------------------------------------ range emission
def bulk_threshold(depth):
    """the smallest count that takes k_proofs_lds: count * depth >= 2^(depth + 1) - 1"""
    return -(-((2 << depth) - 1) // depth)


def emission_cases(depth):
    cap, mid, T = 1 << depth, 1 << (depth - 1), bulk_threshold(depth)
    cases = [(0, cap), (0, 1), (cap - 1, 1), ((mid | 1) % cap, 1)]
    if depth == 16:
        # (the whole tree and the switch at T = 8192 = 2^13 exactly; 8229 = 128 * 64 + 37 ends in a short block)
        cases += [(mid - 4097, 8229), (mid - 4097, 8191), (mid - 4097, 8192)]
        return cases
    # both sides of the switch at one odd first leaf (depths 1 and 2 have no room for an odd one: T >= cap there)
    first = ((cap - T) // 2) | 1 if cap - T >= 2 else 0
    cases += [(first, c) for c in (T, T - 1) if 0 < c <= cap - first]
    # odd first leaf, the first block of 64 straddles the middle of the tree, more than one block, the bulk kernel
    first = max(1, mid - 33) if depth > 1 else 0
    cases.append((first, min(cap - first, max(97, T + 31))))
    # full blocks, then a last block of 37 paths: 37 * depth is no multiple of 16 unless 16 divides depth, so the bit
    # stores end in the scalar tail (depth 7: first = 5, count = 101)
    count = max(T, 101) + (37 - max(T, 101)) % 64
    if 5 + count <= cap:
        cases.append((5, count))
    return cases


def test_emission_cases_cover_what_they_claim():
    for depth in list(range(1, 13)) + [16]:
        cap, T = 1 << depth, bulk_threshold(depth)
        assert T * depth >= 2 * cap - 1 > (T - 1) * depth
        cases = emission_cases(depth)
        assert all(c >= 1 and f + c <= cap for f, c in cases)
        if depth >= 3:
            assert any(f % 2 == 1 and c == T for f, c in cases) and any(f % 2 == 1 and c == T - 1 for f, c in cases)
            # (a block of 64 paths with the middle of the tree inside it, not at its start)
            assert any(f % 2 == 1 and c >= T and f < cap // 2 < f + c and (cap // 2 - f) % 64 for f, c in cases)
        if depth >= 7:
            assert any(f % 2 == 1 and c >= T and c > 64 and c % 64 == 37 for f, c in cases)
    assert (5, 101) in emission_cases(7) and (101 * 7) % 16 != 0
    assert (2**15 - 4097, 8229) in emission_cases(16) and (2**15 - 4097, 8191) in emission_cases(16)


@pytest.mark.parametrize("depth", list(range(1, 13)) + [16])
def test_range_emission_both_kernels_unaligned(depth):
    _, model = base(depth)
    dev = device_tree(depth)
    cap = 1 << depth
    assert dev.root() == model.root()
    for first, count in emission_cases(depth):
        assert_range_equals(dev, model, first, count)
    for first in (0, 1, cap - 1, cap):
        assert dev.proofs_raw(first, 0) == (b"", b"")
    for first, count in ((cap - 1, 2), (cap, 1), (0, cap + 1), (1, cap)):
        with pytest.raises(RLNError):
            dev.proofs_raw(first, count)
    assert dev.root() == model.root()
    dev.close()


# ------------------------------------------------------------------------------------------ range rebuild
def lowest_level_parents(start, n):
    return ((start + n - 1) >> 1) - (start >> 1) + 1


def test_ragged_rebuilds_across_the_rehash_switch():
    """depth 16, one handle: 16 384 parents in the lowest level (the last size of the four-lane kernel), 16 385 (the first
    of the one-lane kernel, both edge parents mixing a new child with an old one), 20 001 with the edge pairs in front"""
    depth = 16
    model = base(depth)[1].copy()
    dev = device_tree(depth)
    rnd = random.Random(0x4A66ED)
    plan = [(1000, 32768, 16384, 0, 1), (2001, 32768, 16385, 1, 0), (12345, 40001, 20001, 1, 1)]
    for start, n, parents, start_parity, end_parity in plan:
        assert lowest_level_parents(start, n) == parents
        assert start % 2 == start_parity and (start + n - 1) % 2 == end_parity
        leaves = distinct_leaves(rnd, n)
        if parents == 20001:
            leaves[1:1 + len(EDGE_PAIRS)] = EDGE_PAIRS      # leaf 12346 is a left child: the pairs are siblings
            assert (start + 1) % 2 == 0
        model.set_range(start, leaves)
        dev.set_range(start, leaves)
        assert_tree_equals(dev, model, "after set_range(%d, %d leaves)" % (start, n))
    dev.close()


# ------------------------------------------------------------------------------------------ fill_sequential
@pytest.mark.parametrize("depth,start,n", [(12, 777, 2222), (16, 4321, 40000)])
def test_fill_sequential_off_zero(depth, start, n):
    """odd start, even end, values 2^32 - 7 ... across the 32-bit limb boundary; at depth 16 the lowest level holds
    20 001 parents, the one-lane kernel"""
    assert start % 2 == 1 and (start + n - 1) % 2 == 0 and (depth < 16 or n > 32768)
    model = base(depth)[1].copy()
    dev = device_tree(depth)
    model.fill_sequential(start, n, 2**32 - 7)
    dev.fill_sequential(start, n, 2**32 - 7)
    assert dev.get(start) == 2**32 - 7 and dev.get(start + 7) == 2**32 and dev.get(start + n - 1) == 2**32 - 8 + n
    assert dev.get(start - 1) == model.get(start - 1) and dev.get(start + n) == model.get(start + n)
    assert_tree_equals(dev, model)
    with pytest.raises(RLNError):
        dev.fill_sequential((1 << depth) - 1, 2, 1)
    assert dev.root() == model.root()
    dev.close()


# ------------------------------------------------------------------------------------------ one handle, everything
SET_LEAVES_K = (1, 2, 11, 12, 16, 17, 64, 65, 300, 2000)


def mixed_plan(depth, rnd):
    cap = 1 << depth

    def set_leaves(k):
        idx = rnd.sample(range(cap), k)
        ups = [(i, rnd.randrange(1, R)) for i in idx]
        if k >= 2:                                   # rewrites; k stays the number of distinct leaves
            ups += [(idx[0], rnd.randrange(1, R)), (idx[k // 2], rnd.randrange(1, R)), (idx[0], rnd.randrange(1, R))]
        head = ups[:k]
        rnd.shuffle(head)                            # unsorted; the rewrites stay behind what they rewrite
        return ("set_leaves", head + ups[k:])

    def set_one():
        return ("set", rnd.randrange(cap), rnd.randrange(1, R))

    def set_range():
        start = rnd.randrange(cap - 1200) | 1
        return ("set_range", start, distinct_leaves(rnd, rnd.randrange(2, 1000) | 1))      # odd start, odd count: even end

    def fill():
        start = rnd.randrange(cap - 1200) | 1
        return ("fill_sequential", start, rnd.randrange(2, 1000) | 1, rnd.randrange(1, 1 << 40))

    # a host-chain pass (k <= 11: the root is then cached on the host) in front of each kind of device pass
    head = [set_leaves(2), set_range(), set_leaves(11), fill(), set_leaves(1), set_one(), set_leaves(5), set_leaves(12)]
    rest = [set_leaves(k) for k in SET_LEAVES_K * 2] + [set_one() for _ in range(6)] + [set_range() for _ in range(6)]
    rest += [fill() for _ in range(5)]
    rnd.shuffle(rest)
    return head + rest


def test_mixed_sequence_on_one_handle(monkeypatch):
    monkeypatch.delenv("RLNAMD_TREE_HOST_MAX", raising=False)
    depth = 12
    cap = 1 << depth
    rnd = random.Random(0x31BED)
    plan = mixed_plan(depth, rnd)
    assert len(plan) >= 40 and {len(dict(op[1])) for op in plan if op[0] == "set_leaves"} >= set(SET_LEAVES_K)
    model = base(depth)[1].copy()
    dev = device_tree(depth)
    paths_k = 1
    for step, op in enumerate(plan):
        getattr(model, op[0])(*op[1:])
        getattr(dev, op[0])(*op[1:])
        what = "step %d, %s" % (step, op[0])
        assert dev.root() == model.root(), what
        # reads in between; the scratch behind proof() and proofs_at() has to grow from call to call
        i = rnd.randrange(cap)
        assert dev.proof(i) == model.proof(i), what
        assert dev.get(i) == model.get(i), what
        idx = [rnd.randrange(cap) for _ in range(paths_k)]
        idx[-1] = idx[0]                              # a repeat
        assert dev.proofs_at(idx) == [model.proof(j) for j in idx], what
        paths_k += 1 + paths_k // 6
        assert dev.root() == model.root(), what
        if step % 4 == 3:
            assert_tree_equals(dev, model, what)
    assert paths_k > 1000
    assert_tree_equals(dev, model, "at the end")
    dev.close()


# ------------------------------------------------------------------------------------------ edge operands
_EDGE_MODEL = []


def edge_model():
    if not _EDGE_MODEL:
        model = TreeModel(7)
        model.set_range(0, EDGE_PAIRS)
        _EDGE_MODEL.append(model)
    return _EDGE_MODEL[0]


@pytest.mark.parametrize("form", ["set_range", "set_leaves_device", "set_leaves_host"])
def test_edge_operand_pairs_through_every_hash_form(form, monkeypatch):
    """set_range: the four-lane kernel; set_leaves with the host chain off: the list and tail kernels; with the host
    chain up to 4096 leaves: the host Poseidon of set_few"""
    from zerokit_amd.batch import PoseidonTree
    assert len(EDGE_PAIRS) == 72 and len({(EDGE_PAIRS[i], EDGE_PAIRS[i + 1]) for i in range(0, 72, 2)}) == 36
    if form == "set_range":
        monkeypatch.delenv("RLNAMD_TREE_HOST_MAX", raising=False)
    else:
        monkeypatch.setenv("RLNAMD_TREE_HOST_MAX", "0" if form == "set_leaves_device" else "4096")
    dev = PoseidonTree(7)
    if form == "set_range":
        dev.set_range(0, EDGE_PAIRS)
    else:
        dev.set_leaves(list(enumerate(EDGE_PAIRS)))
    assert [dev.get(i) for i in range(72)] == EDGE_PAIRS
    assert_tree_equals(dev, edge_model(), form)
    dev.close()


def test_edge_operand_pairs_through_the_list_kernel(monkeypatch):
    """a tree of 128 leaves has at most 64 dirty parents in a level, and those go to the tail kernel at once: at depth 9
    the pairs plus 150 scattered distinct leaves make 186 dirty parents, so the pairs pass k_hash_parents_l3_list"""
    from zerokit_amd.batch import PoseidonTree
    monkeypatch.setenv("RLNAMD_TREE_HOST_MAX", "0")
    rnd = random.Random(0xED6E)
    ups = list(enumerate(EDGE_PAIRS)) + list(zip(range(100, 100 + 2 * 150, 2), distinct_leaves(rnd, 150)))
    rnd.shuffle(ups)
    assert len({i >> 1 for i, _ in ups}) == 36 + 150 > 64
    model = TreeModel(9)
    model.set_leaves(ups)
    dev = PoseidonTree(9)
    dev.set_leaves(ups)
    assert_tree_equals(dev, model)
    dev.close()


# ------------------------------------------------------------------------------------------ the guard
def test_wrapping_range_is_refused_on_the_host():
    """first + count that wraps around 2^64 passes a plain `first + count > capacity` test; the refusal comes before any
    launch, and the handle goes on answering"""
    depth = 5
    _, model = base(depth)
    dev = device_tree(depth)
    for first, count in ((2**64 - 1, 2), (2**64 - 1, 1), (2**64 - 3, 4), (2**64 - 32, 33)):
        with pytest.raises(RLNError):
            dev.proofs_raw(first, count)
        with pytest.raises(RLNError):
            dev.fill_sequential(first, count, 1)
    assert_tree_equals(dev, model)
    dev.close()
