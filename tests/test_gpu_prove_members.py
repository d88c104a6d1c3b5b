"""Proving for tree members by leaf index: rlnamd_tree_proofs_at, rlnamd_prover_submit_members /
_prove_stream_members and ffi_generate_rln_proofs_for_members on the device.  Smallest tables (window_bits = 8), a depth-20
tree with a few dozen members.  Every comparison is byte for byte: the paths against single rlnamd_tree_proof calls and
the oracle's tree, the proofs against the same batch submitted with its paths in the inputs."""
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DEPTH = 20
LAST = (1 << DEPTH) - 1
LIMIT = 100
# member m sits at leaf MEMBER_LEAVES[m]: the first and the last leaf, both children of one parent (6, 7), neighbours
# across a subtree boundary (2^19 - 1, 2^19), the rest scattered
_rnd = random.Random(2024)
MEMBER_LEAVES = [0, LAST, 6, 7, (1 << 19) - 1, 1 << 19] + sorted(_rnd.sample(range(8, LAST - 1), 34))
SENTINEL = (R - 2).to_bytes(32, "little")


def _b(x):
    return int(x).to_bytes(32, "little")


@pytest.fixture(scope="module")
def members():
    """secrets and rate commitments (the leaves) of the members, hashed by the oracle"""
    from oracle.pyref.poseidon import poseidon
    rnd = random.Random(7)
    secrets = [rnd.randrange(1, R) for _ in MEMBER_LEAVES]
    leaves = [poseidon([poseidon([s]), LIMIT]) for s in secrets]
    return secrets, leaves


@pytest.fixture(scope="module")
def oracle_tree(members):
    from oracle.pyref.rln import FullMerkleTree
    t = FullMerkleTree(DEPTH)
    for leaf, v in zip(MEMBER_LEAVES, members[1]):
        t.set(leaf, v)
    return t


def _fresh_tree(members, depth=DEPTH):
    from zerokit_amd.batch import PoseidonTree
    t = PoseidonTree(depth)
    if depth == DEPTH:
        t.set_leaves(list(zip(MEMBER_LEAVES, members[1])))
    return t


@pytest.fixture(scope="module")
def tree(members):
    """never written to by a test (the ordering test takes a tree of its own)"""
    t = _fresh_tree(members)
    yield t
    t.close()


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, window_bits=8)
    yield p
    p.close()


@pytest.fixture(scope="module")
def prover128():
    """capacity 128: the 65-proof batches (two proof groups, the second ragged)"""
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=128, window_bits=8)
    yield p
    p.close()


def _index_list(k):
    """k leaf indices, unsorted, with repeats, holding leaf 0, the last leaf and both children of one parent whenever
    k allows"""
    base = [LAST, 7, 0, 6, 7, 1 << 19, LAST, (1 << 19) - 1, 12345, 0]     # (12345: a leaf nobody wrote)
    rnd = random.Random(k)
    out = [base[i] if i < len(base) else rnd.choice(MEMBER_LEAVES + [rnd.randrange(1 << DEPTH)]) for i in range(k)]
    return out if k > 1 else [LAST]


# ------------------------------------------------------------------------------------------------ 1. the paths
@pytest.mark.parametrize("k", [1, 13, 65])
def test_proofs_at_equals_single_proofs_and_the_oracle(tree, oracle_tree, k):
    """k x depth = 20, 260, 1 300 lanes: a partial block, one block and four lanes, several blocks with a ragged tail"""
    idx = _index_list(k)
    if k >= 13:
        assert {0, LAST, 6, 7} <= set(idx) and len(set(idx)) < k and idx != sorted(idx)
    got = tree.proofs_at(idx)
    assert len(got) == k
    for i, leaf in zip(range(k), idx):
        assert got[i] == tree.proof(leaf), (i, leaf)
        assert got[i] == tuple(oracle_tree.proof(leaf)), (i, leaf)
    e, b = tree.proofs_at_raw(idx)
    assert len(e) == k * DEPTH * 32 and len(b) == k * DEPTH and set(b) <= {0, 1}


def test_proofs_at_on_a_depth_10_tree_and_its_edges(members):
    from oracle.pyref.rln import FullMerkleTree
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import PoseidonTree
    t = PoseidonTree(10)
    o = FullMerkleTree(10)
    for leaf, v in [(0, 11), (1023, 12), (512, 13), (511, 14), (6, 15), (7, 16)]:
        t.set(leaf, v)
        o.set(leaf, v)
    for k in (1, 13, 65):
        rnd = random.Random(100 + k)
        idx = [1023, 7, 0, 6, 511, 512, 7][:k] + [rnd.randrange(1024) for _ in range(max(0, k - 7))]
        got = t.proofs_at(idx)
        assert got == [tuple(o.proof(leaf)) for leaf in idx] == [t.proof(leaf) for leaf in idx], k
    assert t.proofs_at([]) == []
    with pytest.raises(RLNError, match="InvalidLeaf: leaf index 1024 is outside a tree of depth 10"):
        t.proofs_at([3, 1024, 5])
    assert t.proofs_at([3]) == [t.proof(3)]          # usable afterwards
    t.close()


# ------------------------------------------------------------------------------------- 2. by index equals by path
def _witnesses(members, n, seed):
    """n proofs for members in an unsorted order with repeats -> (leaf indices, witnesses without a path, rs)"""
    secrets, _ = members
    rnd = random.Random(seed)
    who = [rnd.randrange(len(MEMBER_LEAVES)) for _ in range(n)]
    if n > 4:
        who[:4] = [1, 3, 0, 2]          # the last leaf, 7, leaf 0, 6
    ws = [dict(identity_secret=secrets[m], user_message_limit=LIMIT, message_id=i % LIMIT, x=rnd.randrange(R),
               external_nullifier=rnd.randrange(R)) for i, m in enumerate(who)]
    rs = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)]
    return [MEMBER_LEAVES[m] for m in who], ws, rs


def _inputs_by_path(p, t, leaves, ws, partial=False):
    full = []
    for leaf, w in zip(leaves, ws):
        elems, bits = t.proof(leaf)                      # one rlnamd_tree_proof call per proof
        w = dict(w, path_elements=elems, identity_path_index=bits)
        full.append(dict(w, message_id=0, x=0, external_nullifier=0) if partial else w)
    return p.pack_inputs(full)


def _inputs_with_sentinel(p, ws, partial=False):
    """what submit_members gets: a value that is neither a path element nor a bit in every path slot"""
    if partial:
        ws = [dict(w, message_id=0, x=0, external_nullifier=0) for w in ws]
    inp = bytearray(p.pack_member_inputs(ws))
    for i in range(len(ws)):
        for name in ("pathElements", "identityPathIndex"):
            off, ln = p.slots[name]
            for l in range(ln):
                o = (i * p.inputs_size + off + l) * 32
                inp[o:o + 32] = SENTINEL
    return bytes(inp)


@pytest.fixture(scope="module")
def by_path(prover, prover128, tree, members):
    """the reference of tests 2 and 5: submit() over inputs whose path slots were filled from rlnamd_tree_proof, computed
    once per size and left unchanged"""
    out = {}
    for n in (1, 25, 65):
        p = prover128 if n > 64 else prover
        leaves, ws, rs = _witnesses(members, n, seed=n)
        rsb = p.pack_rs(rs)
        raw = p.collect_raw(*p.submit(_inputs_by_path(p, tree, leaves, ws), rsb))
        part = p.collect_partial(*p.submit(_inputs_by_path(p, tree, leaves, ws, partial=True), bytes(64 * n), 1))
        out[n] = dict(leaves=leaves, ws=ws, rs=rs, rsb=rsb, raw=raw, partial=part)
    return out


@pytest.mark.parametrize("n", [1, 25, 65])
def test_submit_members_equals_submit_with_the_paths(prover, prover128, tree, by_path, n):
    """n = 1: the host route (the batch is interpreted as segments behind hints hashed from the path); 25: the first
    size past RLNAMD_HINTS, gathered on the device; 65: two proof groups, the second ragged"""
    p = prover128 if n > 64 else prover
    ref = by_path[n]
    before = p.hint_stats()
    t, k = p.submit_members(tree, ref["leaves"], _inputs_with_sentinel(p, ref["ws"]), ref["rsb"])
    proofs, values, errs = p.collect_raw(t, k)
    after = p.hint_stats()
    assert errs == [0] * n == ref["raw"][2]
    assert values == ref["raw"][1]
    assert proofs == ref["raw"][0]
    root = tree.root()
    pub = [[int.from_bytes(values[160 * i + 32 * j:160 * i + 32 * j + 32], "little") for j in range(5)] for i in range(n)]
    assert all(v[1] == root for v in pub)
    assert list(p.verify_many([proofs[128 * i:128 * i + 128] for i in range(n)], pub)) == [True] * n
    # which route the batch took: segments behind hints for the lone proof only
    assert after["hinted_batches"] - before["hinted_batches"] == (1 if n == 1 else 0)
    assert after["fallbacks"] == before["fallbacks"]


@pytest.mark.parametrize("n", [1, 25, 65])
def test_partial_submit_members_equals_partial_submit_with_the_paths(prover, prover128, tree, by_path, n):
    p = prover128 if n > 64 else prover
    ref = by_path[n]
    t, k = p.submit_members(tree, ref["leaves"], _inputs_with_sentinel(p, ref["ws"], partial=True), bytes(64 * n), 1)
    assert p.collect_partial(t, k) == ref["partial"]
    assert len(set(ref["partial"])) == len(set(ref["leaves"]))       # one partial proof per member


def test_prove_stream_members_over_capacity_plus_one(prover, prover128, tree, by_path):
    """65 proofs through a capacity of 64: two chunks, both at the tree's one root"""
    ref = by_path[65]
    assert int(prover.info.capacity) == 64
    proofs, values, errs = prover.prove_members_raw(tree, ref["leaves"], _inputs_with_sentinel(prover, ref["ws"]), ref["rsb"])
    assert (proofs, values, errs) == ref["raw"]
    out = prover.prove_members(tree, ref["leaves"][:3], ref["ws"][:3], ref["rs"][:3])
    assert b"".join(o["proof"] for o in out) == ref["raw"][0][:3 * 128]


# ------------------------------------------------------------------------------------------------ 3. ordering
def _root_of(p, ticket_n):
    _, values, errs = p.collect_raw(*ticket_n)
    assert errs == [0] * ticket_n[1]
    roots = {values[160 * i + 32:160 * i + 64] for i in range(ticket_n[1])}
    assert len(roots) == 1            # one root per batch
    return int.from_bytes(roots.pop(), "little")


def test_a_batch_sees_the_writes_before_it_and_none_after_it(prover, members):
    """The only check of the two event edges (tree stream -> gather, gather -> tree stream).  A race can pass by luck: a
    gather that did NOT wait may still run after the write it should have waited for, and a write that did not wait for
    the gather may still land after it.  What the test pins is the observable rule -- a write made before the call is seen
    by the whole batch, a write made after it returns by none of it -- on both tree write paths (the device pass above 11
    leaves, the host chain of set_few with its scatter left behind on the stream)."""
    t = _fresh_tree(members)
    n = 25                                   # gathered on the device
    leaves, ws, rs = _witnesses(members, n, seed=77)
    inp, rsb = _inputs_with_sentinel(prover, ws), prover.pack_rs(rs)
    free = [l for l in range(100, 200) if l not in MEMBER_LEAVES]
    root0 = t.root()
    assert _root_of(prover, prover.submit_members(t, leaves, inp, rsb)) == root0
    # the device pass (more than 11 leaves), then the batch at once
    t.set_leaves([(l, 1000 + l) for l in free[:16]])
    tk = prover.submit_members(t, leaves, inp, rsb)
    root1 = t.root()
    assert root1 != root0 and _root_of(prover, tk) == root1
    # one leaf through set_few, then the batch at once
    t.set_leaves([(free[20], 5)])
    tk = prover.submit_members(t, leaves, inp, rsb)
    root2 = t.root()
    assert root2 not in (root0, root1) and _root_of(prover, tk) == root2
    # submit, write before collect: the batch keeps the old root, the next batch has the new one -- both write paths
    for write in ([(free[21], 6)], [(l, 2000 + l) for l in free[30:46]]):
        before = t.root()
        tk = prover.submit_members(t, leaves, inp, rsb)
        t.set_leaves(write)
        after = t.root()
        assert after != before
        assert _root_of(prover, tk) == before
        assert _root_of(prover, prover.submit_members(t, leaves, inp, rsb)) == after
    # the same on the host route (a lone proof)
    before = t.root()
    tk = prover.submit_members(t, leaves[:1], _inputs_with_sentinel(prover, ws[:1]), prover.pack_rs(rs[:1]))
    t.set_leaves([(free[50], 9)])
    assert _root_of(prover, tk) == before
    t.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_have_their_own_texts_and_enqueue_nothing(prover, tree, members, by_path):
    from zerokit_amd._native import RLNError
    ref = by_path[25]
    inp = _inputs_with_sentinel(prover, ref["ws"])
    info0 = prover.hint_stats()
    # a ticket handed out now and the one after the refusals are consecutive: nothing was enqueued in between
    t0, _ = prover.submit_members(tree, ref["leaves"], inp, ref["rsb"])
    prover.collect_raw(t0, 25)
    bad = list(ref["leaves"])
    bad[13] = 1 << DEPTH
    with pytest.raises(RLNError, match="leaf index 1048576 is outside a tree of depth 20"):
        prover.submit_members(tree, bad, inp, ref["rsb"])
    with pytest.raises(RLNError, match="leaf index 1048576 is outside a tree of depth 20"):
        prover.prove_members_raw(tree, bad, inp, ref["rsb"])
    small = _fresh_tree(members, depth=10)
    with pytest.raises(RLNError, match=r"the tree's depth \(10\) is not the circuit's \(20\)"):
        prover.submit_members(small, [l % 1024 for l in ref["leaves"]], inp, ref["rsb"])
    small.close()
    with pytest.raises(RLNError, match="full and partial proofs only"):
        prover.submit_members(tree, ref["leaves"], inp, ref["rsb"], mode=2)
    t1, k = prover.submit_members(tree, ref["leaves"], inp, ref["rsb"])
    assert t1 == t0 + 1
    assert prover.collect_raw(t1, k) == ref["raw"]           # usable afterwards
    assert prover.hint_stats()["fallbacks"] == info0["fallbacks"]


# ------------------------------------------------------------------------------------------------ 5. residue
@pytest.mark.parametrize("n", [1, 25])
def test_no_residue_behind_the_collect_of_a_members_batch(prover, tree, by_path, n):
    """entry [5] covers the staged inputs, (r, s) and the leaf indices, device and pinned copy; n = 1 host route, 25 device"""
    ref = by_path[n]
    inp = _inputs_with_sentinel(prover, ref["ws"])
    t, k = prover.submit_members(tree, ref["leaves"], inp, ref["rsb"])
    assert prover.collect_raw(t, k) == ref["raw"]
    assert set(prover.residue().values()) == {0}, prover.residue()


# ------------------------------------------------------------------------------------------------ 6. the FFI
def _ffi_object(tmp_path, members):
    from zerokit_amd.public import RLN
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"profile": "small"}))        # window_bits 8, max_batch 64
    rln = RLN(DEPTH, tree_config=str(cfgp))
    assert int(rln.prover_info().capacity) == 64
    for leaf, v in zip(MEMBER_LEAVES, members[1]):            # single writes: they wait in the tree's pending set
        rln.set_leaf(leaf, v)
    return rln


def _ffi_by_path(rln, leaves, ws, rs):
    from zerokit_amd.public import RLNWitnessInput
    wi = []
    for leaf, w in zip(leaves, ws):
        elems, bits = rln.get_merkle_proof(leaf)
        wi.append(RLNWitnessInput(w["identity_secret"], w["user_message_limit"], w["message_id"], elems, bits, w["x"],
                                  w["external_nullifier"]))
    return rln.generate_rln_proofs_batch(wi, rs)


def _ffi_for_members(rln, leaves, ws, rs):
    return rln.generate_rln_proofs_for_members(leaves, [w["identity_secret"] for w in ws],
                                               [w["user_message_limit"] for w in ws], [w["message_id"] for w in ws],
                                               [w["x"] for w in ws], [w["external_nullifier"] for w in ws], rs)


def test_ffi_proofs_for_members_equal_the_batch_over_merkle_proofs(tmp_path, members, tree):
    """n = 3 (one batch, the host route) and n = 65 on a max_batch 64 object (streamed: 64 + 1); on a forced sparse tree
    (the child process of the test below) every size takes the host route"""
    from zerokit_amd.public import RLNError
    rln = _ffi_object(tmp_path, members)
    for n in (3, 65):
        leaves, ws, rs = _witnesses(members, n, seed=300 + n)
        got = _ffi_for_members(rln, leaves, ws, rs)           # first: its paths come behind the flush of the pending writes
        ref = _ffi_by_path(rln, leaves, ws, rs)
        assert [p.to_bytes_le() for p in got] == [p.to_bytes_le() for p in ref], n
        assert all(p.values.root == tree.root() for p in got)
        assert all(rln.verify_rln_proof(p, w["x"]) for p, w in zip(got, ws))
    assert rln.generate_rln_proofs_for_members([], [], [], [], [], []) == []
    leaves, ws, rs = _witnesses(members, 3, seed=1)
    ws[1] = dict(ws[1], message_id=LIMIT)
    with pytest.raises(RLNError, match=r"Message id \(100\) is not within user_message_limit \(100\)"):
        _ffi_for_members(rln, leaves, ws, rs)
    ws[1] = dict(ws[1], message_id=1)
    with pytest.raises(RLNError, match="leaf index 1048576 is outside a tree of depth 20"):
        _ffi_for_members(rln, [leaves[0], 1 << DEPTH, leaves[2]], ws, rs)
    assert len(_ffi_for_members(rln, leaves, ws, None)) == 3          # random blinding; usable after the refusals


def test_ffi_proofs_for_members_refuse_a_multi_message_id_object():
    from zerokit_amd.batch import resource_paths
    from zerokit_amd.public import RLN, RLNError
    zp, gp = resource_paths(20, multi=True)
    rln = RLN.new_with_params(20, open(zp, "rb").read(), open(gp, "rb").read())
    with pytest.raises(RLNError, match="ffi_generate_rln_proofs_for_members: single message-id circuits only"):
        rln.generate_rln_proofs_for_members([0], [1], [LIMIT], [0], [5], [6])


def test_the_ffi_members_test_on_a_forced_sparse_tree():
    """RLNAMD_TREE_SPARSE_ABOVE=0 in a child process: the object's tree is the sparse one, whose paths the call fetches on
    the host (SparseTree::proof in a loop) at any n -- same bytes as the batch over ffi_get_merkle_proof.

    A deviation from the issue, which asks for the proofs_at comparison itself on a sparse tree: rlnamd_tree wraps the
    dense MerkleTreeDev only, so rlnamd_tree_proofs_at never meets a sparse tree.  The sparse tree exists behind the FFI
    object alone (TreeAny), and this is the one way to reach its loop."""
    env = dict(os.environ, RLNAMD_TREE_SPARSE_ABOVE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", os.path.abspath(__file__), "-k",
                        "test_ffi_proofs_for_members_equal_the_batch_over_merkle_proofs"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "1 passed" in r.stdout
