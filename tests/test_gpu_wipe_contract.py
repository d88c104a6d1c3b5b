"""Nothing secret outlives a batch -- in ANY buffer of the slot the batch used.  rlnamd_prover_residue_slot counts, per
workspace slot, what rlnamd_prover_residue counts plus the pinned staging buffer, the pinned hints and the interpreter's
stored values (the table above `struct Slot` in prover.hip names every buffer as counted or exempt).  One batch per path a
batch can take -- sizes read from rlnamd_prover_describe -- on one prover (max_batch 192, smallest tables); inputs are the
golden depth-20 cases, and every proof and public input that comes back is compared with the golden bytes, so a wipe that
comes too early shows as well.

Per batch: before the wiping collect, rlnamd_prover_collect_public (which does not wipe) and the tap -- the control that
the tap sees something: staging and stored values not zero, hints not zero exactly when the batch was hinted; after the
collect every field of the batch's slot zero and rlnamd_prover_fetch_witness all zero (every lane up to 48 proofs, lanes
0, n // 2 and n - 1 above).  What no test can see: the `Fr hv[64]` stack arrays of the hint hashing (zeroed with
secure_zero) and the hints of a prover that is freed with batches uncollected (~Prover clears them before hipHostFree):
after rlnamd_prover_free there is nothing to tap."""
import ctypes as C
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["cases"]


def _w(case):
    w = case["witness"]
    return dict(identity_secret=int(w["identity_secret"]), user_message_limit=int(w["user_message_limit"]),
                message_id=int(w["message_id"]), path_elements=[int(t) for t in w["path_elements"]],
                identity_path_index=[int(t) for t in w["identity_path_index"]], x=int(w["x"]),
                external_nullifier=int(w["external_nullifier"]))


def _tuning(text):
    return {k: v for k, v in (kv.split("=", 1) for kv in text.split() if "=" in kv)}


class _Rig:
    def __init__(self):
        from zerokit_amd.batch import BatchProver
        self.p = BatchProver(max_batch=192, window_bits=8)
        self.cases = _cases()
        self.partial = {c["name"]: bytes.fromhex(c["partial320"]) for c in
                        json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_partial.json")))["cases"]}
        self.tune = _tuning(self.p.describe())
        self.enqueued = 0                # batches so far: consecutive batches take consecutive slots
        self.ns = int(self.p.info.num_signals)

    def pack(self, idx):
        cs = [self.cases[i] for i in idx]
        return self.p.pack_inputs([_w(c) for c in cs]), self.p.pack_rs([(int(c["r"]), int(c["s"])) for c in cs])

    def slot(self):
        """the slot the batch submitted NEXT takes"""
        return self.enqueued % self.p.n_slots()

    def control(self, t, idx, k, hinted):
        """before the wiping collect: the public signals are the golden ones, and the tap sees the batch"""
        from zerokit_amd import lib
        from zerokit_amd._native import check
        p, n = self.p, len(idx)
        buf = C.create_string_buffer(32 * p.num_public * n)
        check(lib().rlnamd_prover_collect_public(p._h, t, n, buf))
        for lane, i in enumerate(idx):
            got = [int.from_bytes(buf.raw[32 * (lane * p.num_public + j):32 * (lane * p.num_public + j + 1)], "little")
                   for j in range(p.num_public)]
            assert [str(v) for v in got] == self.cases[i]["public_inputs"], (lane, self.cases[i]["name"])
        res = p.residue_slot(k)
        print("slot %d, %d proofs, hinted %s, before the collect: %s" % (k, n, hinted, res))
        assert res["staging"] > 0 and res["v29"] > 0 and res["inputs"] > 0 and res["reserved"] == 0, res
        assert (res["hints"] > 0) == hinted, (hinted, res)

    def golden(self, out, idx):
        for lane, (o, i) in enumerate(zip(out, idx)):
            c = self.cases[i]
            assert o["error"] == 0 and o["proof"].hex() == c["proof_compressed"], (lane, c["name"])
            assert [str(v) for v in o["public_inputs"]] == c["public_inputs"], (lane, c["name"])

    def nothing_left(self, k, n):
        from zerokit_amd import lib
        from zerokit_amd._native import check
        res = self.p.residue_slot(k)
        print("slot %d, %d proofs, after the collect: %s" % (k, n, res))
        assert set(res.values()) == {0}, (k, n, res)
        buf = C.create_string_buffer(32 * self.ns)
        for lane in (range(n) if n <= 48 else (0, n // 2, n - 1)):
            check(lib().rlnamd_prover_fetch_witness(self.p._h, lane, buf))
            assert buf.raw == bytes(32 * self.ns), (n, lane)

    def full(self, idx, hinted, submit=None):
        """one full-proof batch of the cases idx through submit (or `submit`), with every check of the module"""
        p = self.p
        k, before = self.slot(), p.hint_stats()["hinted_batches"]
        inp, rsb = self.pack(idx)
        t, n = submit(inp, rsb) if submit else p.submit(inp, rsb)
        self.enqueued += 1
        was = p.hint_stats()["hinted_batches"] - before == 1
        assert hinted is None or was == hinted, (len(idx), p.hint_stats())     # (None: read, not assumed)
        self.control(t, idx, k, was)
        self.golden(p.collect(t, n), idx)
        assert p.hint_stats()["fallbacks"] == 0
        self.nothing_left(k, n)


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.p.close()


def _idx(n, first=0):
    return [(first + j) % 6 for j in range(n)]


def test_the_tap_names_its_fields_and_refuses_a_slot_that_is_not_there(rig):
    from zerokit_amd._native import RLNError
    p = rig.p
    assert len(rig.cases) == 6 and 2 <= p.n_slots() <= 6
    for k in range(p.n_slots()):
        res = p.residue_slot(k)
        assert list(res) == list(p.RESIDUE_SLOT) and len(res) == 10, (k, res)
        # the constructor clears every buffer the tap counts (hipMalloc may hand out what an earlier prover freed)
        assert set(res.values()) == {0}, (k, res)
    for k in (p.n_slots(), 6, -1):
        with pytest.raises(RLNError):
            p.residue_slot(k)


@pytest.mark.parametrize("which", ["lone", "tiny", "lanechunk_walk", "ntt_lg_max+1", "lanechunk+1"])
def test_a_batch_of_this_shape_leaves_nothing_in_its_slot(rig, which):
    t = rig.tune
    n = {"lone": 1, "tiny": int(t["tiny"]), "lanechunk_walk": int(t["lanechunk_walk"]),
         "ntt_lg_max+1": int(t["ntt_lg_max"]) + 1, "lanechunk+1": int(t["lanechunk"]) + 1}[which]
    assert 1 <= n <= int(rig.p.info.capacity), (which, n)
    # a lone batch of at most RLNAMD_HINTS proofs hashes its hints inside submit; above it the members' chains would have to
    # be remembered (every golden member has been seen after the first batches): read, not assumed, above RLNAMD_HINTS
    rig.full(_idx(n, 1), True if n <= int(t["hints"]) else False if n > 64 else None)


def test_a_hinted_batch_through_submit_leaves_no_hints(rig):
    n = min(24, int(rig.tune["hints"]))
    assert n >= 2
    rig.full(_idx(n, 2), True)


def test_a_batch_with_hints_brought_by_the_caller_leaves_no_hints(rig):
    p = rig.p
    idx = _idx(40, 3)
    hints = p.hints_for(rig.pack(idx)[0])
    assert hints is not None and len(hints) == 40
    rig.full(idx, True, submit=lambda inp, rsb: p.submit_hinted(inp, rsb, hints))


def _partial_inputs(rig, names):
    by = {c["name"]: c for c in rig.cases}
    return rig.p.pack_inputs([dict(_w(by[nm]), message_id=0, x=0, external_nullifier=0) for nm in names])


def test_a_partial_batch_leaves_nothing_in_its_slot(rig):
    """(collect_public does not apply to a partial batch -- its witness has no public signals yet -- so the control before
    the collect is skipped here; the partial points are compared with the fixture)"""
    p = rig.p
    names = sorted(rig.partial) * 3
    k = rig.slot()
    t, n = p.submit(_partial_inputs(rig, names), bytes(64 * len(names)), 1)
    rig.enqueued += 1
    assert p.collect_partial(t, n) == [rig.partial[nm] for nm in names]
    rig.nothing_left(k, n)


def test_a_finish_batch_with_its_points_given_leaves_nothing_in_its_slot(rig):
    p = rig.p
    names = sorted(rig.partial) * 3
    idx = [[c["name"] for c in rig.cases].index(nm) for nm in names]
    before = p.hint_stats()["hinted_batches"]
    k = rig.slot()
    inp, rsb = rig.pack(idx)
    t, n = p.submit(inp, rsb, 2, [rig.partial[nm] for nm in names])
    rig.enqueued += 1
    rig.control(t, idx, k, p.hint_stats()["hinted_batches"] - before == 1)
    rig.golden(p.collect(t, n), idx)
    rig.nothing_left(k, n)


def test_a_finish_batch_through_cached_handles_leaves_nothing_in_its_slot_or_its_entries(rig):
    p = rig.p
    names = sorted(rig.partial) * 3
    idx = [[c["name"] for c in rig.cases].index(nm) for nm in names]
    k = rig.slot()
    t, n = p.submit(_partial_inputs(rig, names), bytes(64 * len(names)), 1)
    rig.enqueued += 1
    parts, handles, errs = p.collect_partial_cached(t, n)
    assert parts == [rig.partial[nm] for nm in names] and all(handles) and not any(errs)
    rig.nothing_left(k, n)
    cone0, hinted0 = p.partial_cache_info()["cone_batches"], p.hint_stats()["hinted_batches"]
    k = rig.slot()
    inp, rsb = rig.pack(idx)
    t, n = p.submit_finish(inp, rsb, parts, handles)
    rig.enqueued += 1
    assert p.partial_cache_info()["cone_batches"] == cone0 + 1 and p.hint_stats()["hinted_batches"] == hinted0
    rig.control(t, idx, k, False)
    rig.golden(p.collect(t, n), idx)
    rig.nothing_left(k, n)
    p.release_partial(handles)
    info = p.partial_cache_info()
    assert info["in_use"] == 0 and info["residue_in_free_entries"] == 0, info


def test_a_members_batch_leaves_nothing_in_its_slot(rig):
    """members of a depth-20 tree by leaf index, paths gathered on the device: the golden case whose path IS a tree's
    (config1_bench_witness: leaf 3 of a tree that holds its rate commitment and nothing else), 33 times"""
    from oracle.pyref.poseidon import poseidon
    from zerokit_amd.batch import PoseidonTree
    p = rig.p
    i = [c["name"] for c in rig.cases].index("config1_bench_witness")
    c = rig.cases[i]
    w = _w(c)
    leaf = sum(b << l for l, b in enumerate(w["identity_path_index"]))
    n = 33
    assert n > int(rig.tune["hints"])                # (at most RLNAMD_HINTS lone members fetch their paths to the host)
    tree = PoseidonTree(20)
    try:
        tree.set(leaf, poseidon([poseidon([w["identity_secret"]]), w["user_message_limit"]]))
        assert str(tree.root()) == json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["tree_root_config1"]
        before = p.hint_stats()["hinted_batches"]
        k = rig.slot()
        t, m = p.submit_members(tree, [leaf] * n, p.pack_member_inputs([w] * n), p.pack_rs([(int(c["r"]), int(c["s"]))] * n))
        rig.enqueued += 1
        assert p.hint_stats()["hinted_batches"] == before
        rig.control(t, [i] * n, k, False)
        rig.golden(p.collect(t, m), [i] * n)
        rig.nothing_left(k, m)
    finally:
        tree.close()


def test_every_slot_is_clean_at_the_end(rig):
    assert rig.enqueued >= rig.p.n_slots()           # every slot was used, most by batches of several shapes
    for k in range(rig.p.n_slots()):
        res = rig.p.residue_slot(k)
        assert set(res.values()) == {0}, (k, res)
