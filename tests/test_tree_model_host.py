"""The host model that judges the device tree (tests/tree_model.py) against the two oracles, so that the reference is not
the weak link: oracle/pyref's FullMerkleTree (Python Poseidon, a full rehash of every parent range) on small depths after
every step of a random sequence, and oracle/c's bottom-up root on a ragged range at depth 16."""
import random

import pytest

from tree_model import R, TreeModel


def _ref_proofs_bytes(ref, first, count):
    elems, bits = b"", b""
    for i in range(first, first + count):
        e, b = ref.proof(i)
        elems += b"".join(v.to_bytes(32, "little") for v in e)
        bits += bytes(b)
    return elems, bits


@pytest.mark.parametrize("depth", range(7))
def test_model_random_sequence_vs_pyref(depth):
    from oracle.pyref.rln import FullMerkleTree
    rnd = random.Random(1000 + depth)
    cap = 1 << depth
    model, ref = TreeModel(depth), FullMerkleTree(depth)
    assert model.root() == ref.root()
    for step in range(10):
        op = rnd.choice(("set_range", "set_leaves", "fill_sequential"))
        if op == "set_range":
            start = rnd.randrange(cap)
            leaves = [rnd.randrange(R) for _ in range(rnd.randrange(1, cap - start + 1))]
            model.set_range(start, leaves)
            ref.set_range(start, leaves)
        elif op == "set_leaves":
            ups = [(rnd.randrange(cap), rnd.randrange(R)) for _ in range(rnd.randrange(1, cap + 3))]
            ups += [(ups[0][0], rnd.randrange(R))]          # a rewrite: the later entry wins
            model.set_leaves(ups)
            for i, v in ups:
                ref.set(i, v)
        else:
            start = rnd.randrange(cap)
            n = rnd.randrange(1, cap - start + 1)
            first_value = rnd.choice((1, 2**32 - 2, 2**64 - 1 - n // 2))   # (the last one wraps the 64-bit counter)
            model.fill_sequential(start, n, first_value)
            ref.set_range(start, [(first_value + i) % 2**64 for i in range(n)])
        assert model.root() == ref.root(), (step, op)
        assert model.nodes == ref.nodes, (step, op)
        for i in range(cap):
            assert model.proof(i) == ref.proof(i), (step, op, i)
            assert model.get(i) == ref.get(i)
        assert model.proofs_bytes(0, cap) == _ref_proofs_bytes(ref, 0, cap), (step, op)
        first = rnd.randrange(cap)
        count = rnd.randrange(0, cap - first + 1)
        assert model.proofs_bytes(first, count) == _ref_proofs_bytes(ref, first, count), (step, op, first, count)


def test_model_refuses_what_the_tree_refuses():
    m = TreeModel(3)
    with pytest.raises(IndexError):
        m.set_range(7, [1, 2])
    with pytest.raises(IndexError):
        m.set_leaves([(8, 1)])
    with pytest.raises(IndexError):
        m.proofs_bytes(7, 2)
    with pytest.raises(IndexError):
        m.proof(8)
    with pytest.raises(ValueError):
        m.set(0, R)
    assert m.proofs_bytes(5, 0) == (b"", b"")
    assert m.root() == TreeModel(3).root()
    c = m.copy()
    c.set(1, 5)
    assert m.get(1) == 0 and c.get(1) == 5 and m.root() != c.root()


def test_model_ragged_range_depth16_vs_c_oracle():
    """40 001 leaves from an odd start: both edge parents of the lowest level mix a new child with a default one"""
    from oracle.c import binding as ob
    rnd = random.Random(16)
    depth, start, n = 16, 12345, 40001
    leaves = [rnd.randrange(R) for _ in range(n)]
    m = TreeModel(depth)
    m.set_range(start, leaves)
    assert m.root() == ob.tree_root(depth, [0] * start + leaves)
    # a second, overlapping write on top: the C oracle rebuilds from the merged leaves
    m.fill_sequential(start + n - 100, 201, 2**32 - 7)
    merged = [0] * start + leaves[:n - 100] + [2**32 - 7 + i for i in range(201)]
    assert m.root() == ob.tree_root(depth, merged)
