"""Proving on the multi-message-id circuit with blocks of message ids drawn on the device:
rlnamd_prover_submit_members_drawn_counts / _prove_stream_members_drawn_counts and
ffi_generate_rln_proofs_for_members_drawn_multi, on the smallest tables and a depth-20 tree with a dozen members.
Members repeat, a proof uses 1 .. 4 message slots, and some requests run past their member's limit.  A granted row is
byte for byte -- proof and all 15 public values -- what submit_members gives for the ids and selectors the model
(tests/quota_counts_cases.py) names and the same (r, s); a refused row yields an error code and nothing else; and a
relay's NullifierLog fed every used slot of every proof says NEW to all.  Before that, the call the drawn one is
measured against: submit_members on a multi prover with the caller's ids, against submit with the paths in the inputs."""
import json
import random

import pytest

import quota_cases as cases
import quota_counts_cases as cc
from quota_cases import NO_EPOCH, OK, OVER

pytestmark = pytest.mark.gpu

R = cases.R
DEPTH = 20
LAST = (1 << DEPTH) - 1
K = 4                                    # max_out of the shipped multi-message-id circuit
NV = 3 * K + 3                           # ys | root | nullifiers | x | external nullifier | selectors
_rnd = random.Random(4242)
MEMBER_LEAVES = [0, LAST, 6, 7, (1 << 19) - 1, 1 << 19] + sorted(_rnd.sample(range(8, LAST - 1), 6))
MEMBER_LIMITS = [1, 2, 3, 100, 2, 1, 100, 3, 100, 1, 2, 100]
EA, EB, E_OUT = 0xA11CE, R - 2, 0xBAD


@pytest.fixture(scope="module")
def members():
    from oracle.pyref.poseidon import poseidon
    rnd = random.Random(11)
    secrets = [rnd.randrange(1, R) for _ in MEMBER_LEAVES]
    leaves = [poseidon([poseidon([s]), lim]) for s, lim in zip(secrets, MEMBER_LIMITS)]
    return secrets, leaves


@pytest.fixture(scope="module")
def tree(members):
    from zerokit_amd.batch import PoseidonTree
    t = PoseidonTree(DEPTH)
    t.set_leaves(list(zip(MEMBER_LEAVES, members[1])))
    yield t
    t.close()


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, window_bits=8, multi=True)
    assert p.num_public == NV and int(p.info.max_out) == K and int(p.info.capacity) == 64
    yield p
    p.close()


def _ledger():
    from zerokit_amd.batch import QuotaLedger
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    m = cc.CountsModel(DEPTH, 4)
    m.set_epochs([EA, EB])
    return q, m


def _requests(members, n, seed, who=None, counts=None):
    """n requests: members in an unsorted order with repeats, two open epochs and one the ledger does not sign under,
    1 .. 4 message slots a proof -> (leaf indices, witnesses without path, ids and selectors, rs, counts)"""
    rnd = random.Random(seed)
    who = who or [rnd.randrange(len(MEMBER_LEAVES)) for _ in range(n)]
    exts = [rnd.choice([EA, EA, EB, E_OUT] if n > 4 else [EA]) for _ in range(n)]
    ws = [dict(identity_secret=members[0][m], user_message_limit=MEMBER_LIMITS[m], x=rnd.randrange(R), external_nullifier=e)
          for m, e in zip(who, exts)]
    rs = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)]
    return [MEMBER_LEAVES[m] for m in who], ws, rs, counts or [rnd.randrange(1, K + 1) for _ in range(n)]


def _with_ids(w, first, count):
    return dict(w, message_id=[first + k if k < count else 0 for k in range(K)], selector_used=[int(k < count) for k in range(K)])


def _drawn_inputs(p, ws):
    """what the drawn calls get: ids no request may end up with in every message slot, and every selector set"""
    return p.pack_member_inputs([dict(w, message_id=[R - 5 - k for k in range(K)], selector_used=[1] * K) for w in ws])


def _collect(p, ticket, k):
    pub = p.collect_public(ticket, k)              # before the collect that ends the batch
    proofs, _five, errs = p.collect_raw(ticket, k)
    return proofs, pub, errs


def _field(pub, i, j):
    return int.from_bytes(pub[32 * (NV * i + j):32 * (NV * i + j + 1)], "little")


def _check(p, tree, m, leaves, ws, rs, counts, got, status):
    """got = (proofs, public values, errs) of a drawn call, status its statuses; m: the model BEFORE the call"""
    n = len(leaves)
    proofs, pub, errs = got
    root = tree.root()
    firsts, want_status = m.draw_counts(leaves, [w["external_nullifier"] for w in ws], [w["user_message_limit"] for w in ws], counts)
    assert status == want_status
    made = [i for i in range(n) if status[i] == OK]
    if made:
        ref = p.prove_members_public_raw(tree, [leaves[i] for i in made],
                                         p.pack_member_inputs([_with_ids(ws[i], firsts[i], counts[i]) for i in made]),
                                         p.pack_rs([rs[i] for i in made]))
        assert ref[2] == [0] * len(made)
        for k, i in enumerate(made):
            assert errs[i] == 0, i
            assert pub[32 * NV * i:32 * NV * (i + 1)] == ref[1][32 * NV * k:32 * NV * (k + 1)], i
            assert proofs[128 * i:128 * i + 128] == ref[0][128 * k:128 * k + 128], i
            assert [_field(pub, i, 2 * K + 3 + t) for t in range(K)] == [int(t < counts[i]) for t in range(K)], i   # the selectors: a prefix
            for t in range(counts[i], K):                                                    # an unused slot gives nothing
                assert _field(pub, i, t) == 0 and _field(pub, i, K + 1 + t) == 0, (i, t)
            assert _field(pub, i, K) == root and _field(pub, i, 2 * K + 2) == ws[i]["external_nullifier"]
    for i in range(n):
        if status[i] != OK:
            assert errs[i] != 0 and proofs[128 * i:128 * i + 128] == bytes(128), i
            assert pub[32 * NV * i:32 * NV * (i + 1)] == bytes(32 * NV), i
    return made, firsts


def _shares(pub, made, counts):
    """every used slot of every proof made: (nullifier_k, x, y_k, external nullifier)"""
    out = []
    for i in made:
        for t in range(counts[i]):
            out.append((_field(pub, i, K + 1 + t), _field(pub, i, 2 * K + 1), _field(pub, i, t), _field(pub, i, 2 * K + 2)))
    return out


# ---------------------------------------------------------------------------------- members by index, the caller's ids
def test_members_by_index_equal_members_by_path_on_the_multi_circuit(prover, tree, members):
    """n = 25 through submit_members with the caller's ids and selectors: proofs and all 15 public values are those of
    submit with the paths from the tree in the inputs"""
    p = prover
    rnd = random.Random(76)
    who = [rnd.choice([3, 6, 8, 11]) for _ in range(25)]          # the members with a limit of 100: ids up to 75
    leaves, ws, rs, counts = _requests(members, 25, seed=77, who=who)
    full = [_with_ids(w, 3 * i, c) for i, (w, c) in enumerate(zip(ws, counts))]
    rsb = p.pack_rs(rs)
    paths = tree.proofs_at(leaves)
    by_path = p.pack_inputs([dict(w, path_elements=e, identity_path_index=b) for w, (e, b) in zip(full, paths)])
    want = _collect(p, *p.submit(by_path, rsb))
    got = _collect(p, *p.submit_members(tree, leaves, p.pack_member_inputs(full), rsb))
    assert want[2] == [0] * 25 and got[2] == want[2]
    assert got[0] == want[0] and got[1] == want[1] and len(got[1]) == 25 * 32 * NV
    root = tree.root()
    assert all(_field(got[1], i, K) == root for i in range(25))
    # the stream form's sibling with every public value a row gives the same bytes
    stream = p.prove_members_public_raw(tree, leaves, p.pack_member_inputs(full), rsb)
    assert stream[0] == want[0] and stream[1] == want[1] and stream[2] == want[2]
    assert set(p.residue().values()) == {0}


# ------------------------------------------------------------------------------------------------------- drawn
@pytest.mark.parametrize("n", [1, 25])
def test_drawn_blocks_equal_batches_with_the_models_ids(prover, tree, members, n):
    """n = 1: a lone batch; 25: the device route, ids and selectors written by a kernel behind the staging.  Two calls on
    one ledger, every used slot into one NullifierLog."""
    from zerokit_amd.batch import NullifierLog
    p = prover
    q, m = _ledger()
    log = NullifierLog(8 * n + 64)
    blocks = cc.Blocks()
    try:
        seen = set()
        for call in range(2):
            leaves, ws, rs, counts = _requests(members, n, seed=100 * n + call, who=[3] if n == 1 else None,
                                               counts=[3 + call] if n == 1 else None)
            t, k, status = p.submit_members_drawn_counts(tree, q, leaves, _drawn_inputs(p, ws), p.pack_rs(rs), counts)
            got = _collect(p, t, k)
            assert set(p.residue().values()) == {0} and q.info()["residue"] == 0
            made, firsts = _check(p, tree, m, leaves, ws, rs, counts, got, status)
            blocks.add(leaves, [w["external_nullifier"] for w in ws], [w["user_message_limit"] for w in ws], counts, firsts, status)
            seen |= set(status)
            if made:
                st, _secrets, _first = log.observe(_shares(got[1], made, counts))
                assert st == [NullifierLog.NEW] * sum(counts[i] for i in made)      # the ledger exists so that the log never says SPAM
            cases.compare_counters(m, q, [(w["external_nullifier"], leaf) for leaf, w in zip(leaves, ws)])
        if n == 1:
            assert q.used([MEMBER_LEAVES[3]], [EA]) == [7]                          # blocks 0 .. 2 and 3 .. 6
            leaves, ws, rs, counts = _requests(members, 1, seed=5, who=[2], counts=[4])   # member 2: limit 3, a block of 4
            t, k, status = p.submit_members_drawn_counts(tree, q, leaves, _drawn_inputs(p, ws), p.pack_rs(rs), counts)
            made, _ = _check(p, tree, m, leaves, ws, rs, counts, _collect(p, t, k), status)
            assert status == [OVER] and not made and q.used([MEMBER_LEAVES[2]], [EA]) == [0]
        else:
            assert seen == {OK, OVER, NO_EPOCH}
        info = q.info()
        assert (info["issued"], info["over"], info["no_epoch"]) == (m.issued, m.over, m.no_epoch)
        assert blocks.check() == m.issued
    finally:
        log.close()
        q.close()


def test_the_stream_form_draws_once_for_both_chunks(prover, tree, members):
    """65 requests through a capacity of 64: ONE draw, two chunks; member 3 (limit 100) sits on both sides of the chunk
    boundary (requests 60 .. 63 | 64) and member 2 (limit 3) runs out inside the first chunk"""
    from zerokit_amd.batch import NullifierLog
    p = prover
    q, m = _ledger()
    log = NullifierLog(1024)
    try:
        rnd = random.Random(65)
        who = [rnd.randrange(len(MEMBER_LEAVES)) for _ in range(65)]
        who[60:65] = [3] * 5
        who = [8 if w == 2 else w for w in who]                 # member 2 asks nowhere else in this call
        who[50:56] = [2] * 6
        leaves, ws, rs, counts = _requests(members, 65, seed=66, who=who)
        counts[60:65] = [4, 1, 3, 4, 2]
        counts[50:56] = [2, 2, 1, 1, 1, 1]                      # limit 3: the first is granted, the second is over with it ...
        for i in list(range(50, 56)) + list(range(60, 65)):
            ws[i]["external_nullifier"] = EA
        proofs, pub, errs, status = p.prove_members_drawn_counts_raw(tree, q, leaves, _drawn_inputs(p, ws), p.pack_rs(rs), counts)
        made, firsts = _check(p, tree, m, leaves, ws, rs, counts, (proofs, pub, errs), status)
        assert status[60:65] == [OK] * 5 and [firsts[i + 1] - firsts[i] for i in range(60, 64)] == counts[60:64]
        assert status[50:56] == [OK] + [OVER] * 5               # ... and so is every smaller one behind it, in this call
        assert set(p.residue().values()) == {0} and q.info()["residue"] == 0 and q.info()["draws"] == 1
        st, _s, _f = log.observe(_shares(pub, made, counts))
        assert st == [NullifierLog.NEW] * len(st) and len(made) > 10
        # the next call grants member 2 the one id that was left
        out, st = p.prove_members_drawn_counts(tree, q, leaves[52:53], ws[52:53], rs[52:53], [1])
        assert st == [OK] == m.draw_counts(leaves[52:53], [EA], [3], [1])[1]
        assert out[0]["error"] == 0 and out[0]["public_inputs"][2 * K + 3:] == [1, 0, 0, 0]
        out, st = p.prove_members_drawn_counts(tree, q, leaves[50:53], ws[50:53], rs[50:53], [1, 1, 1])
        assert st == [OVER] * 3 and all(o["error"] != 0 and o["proof"] == bytes(128) and set(o["public_inputs"]) == {0} for o in out)
    finally:
        log.close()
        q.close()


def test_on_a_single_message_id_prover_counts_of_one_give_what_the_plain_drawn_call_gives(tree, members):
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, window_bits=8)
    (qa, _ma), (qb, _mb) = _ledger(), _ledger()
    try:
        for n in (1, 25):
            leaves, ws, rs, _ = _requests(members, n, seed=900 + n)
            inp, rsb = p.pack_member_inputs([dict(w, message_id=R - 5) for w in ws]), p.pack_rs(rs)
            ta, k, sa = p.submit_members_drawn_counts(tree, qa, leaves, inp, rsb, [1] * n)
            a = p.collect_raw(ta, k)
            tb, k, sb = p.submit_members_drawn(tree, qb, leaves, inp, rsb)
            b = p.collect_raw(tb, k)
            assert sa == sb and a == b and any(e == 0 for e in a[2])
            keys = sorted(set((w["external_nullifier"], leaf) for leaf, w in zip(leaves, ws)))
            assert qa.used([k[1] for k in keys], [k[0] for k in keys]) == qb.used([k[1] for k in keys], [k[0] for k in keys])
        assert qa.info() == qb.info()
        from zerokit_amd._native import RLNError
        with pytest.raises(RLNError, match="proof 0 asks for 2 message ids, the circuit has 1 message slots"):
            p.submit_members_drawn_counts(tree, qa, leaves[:1], inp[:p.inputs_size * 32], rsb[:64], [2])
    finally:
        qa.close()
        qb.close()
        p.close()


def test_refusals_have_their_own_texts_and_draw_nothing(prover, tree, members):
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import QuotaLedger
    p = prover
    q, m = _ledger()
    shallow = QuotaLedger(10, 2)
    try:
        leaves, ws, rs, counts = _requests(members, 25, seed=9)
        inp, rsb = _drawn_inputs(p, ws), p.pack_rs(rs)
        t, k, status = p.submit_members_drawn_counts(tree, q, leaves, inp, rsb, counts)
        _check(p, tree, m, leaves, ws, rs, counts, _collect(p, t, k), status)
        # a ticket handed out now and the one after the refusals are consecutive: nothing was enqueued in between
        t0, k = p.submit_members(tree, leaves[:2], p.pack_member_inputs([_with_ids(w, 0, 1) for w in ws[:2]]), p.pack_rs(rs[:2]))
        p.collect_raw(t0, k)
        before = (q.info(), q.used(leaves, [w["external_nullifier"] for w in ws]))
        for call in (p.submit_members_drawn_counts, p.prove_members_drawn_counts_raw):
            with pytest.raises(RLNError, match=r"proof 11 asks for 5 message ids, the circuit has 4 message slots \(max_out\)"):
                call(tree, q, leaves, inp, rsb, counts[:11] + [5] + counts[12:])
            with pytest.raises(RLNError, match=r"request 4 of draw_counts asks for no id \(a count is 1 \.\. 255\)"):
                call(tree, q, leaves, inp, rsb, counts[:4] + [0] + counts[5:])
            with pytest.raises(RLNError, match=r"the ledger's depth \(10\) is not the tree's \(20\)"):
                call(tree, shallow, leaves, inp, rsb, counts)
            wide = _drawn_inputs(p, ws[:7] + [dict(ws[7], user_message_limit=1 << 32)] + ws[8:])
            with pytest.raises(RLNError, match="the message limit of proof 7 is 2\\^32 or more"):
                call(tree, q, leaves, wide, rsb, counts)
            bad = list(leaves)
            bad[13] = 1 << DEPTH
            with pytest.raises(RLNError, match="leaf index 1048576 is outside a tree of depth 20"):
                call(tree, q, bad, inp, rsb, counts)
        assert (q.info(), q.used(leaves, [w["external_nullifier"] for w in ws])) == before and shallow.info()["draws"] == 0
        t1, k, status = p.submit_members_drawn_counts(tree, q, leaves, inp, rsb, counts)      # nothing was enqueued in between
        assert t1 == t0 + 1
        _check(p, tree, m, leaves, ws, rs, counts, _collect(p, t1, k), status)                 # usable afterwards
    finally:
        shallow.close()
        q.close()


# ------------------------------------------------------------------------------------------------------ the FFI
def test_the_ffi_entry_gives_what_a_multi_witness_with_the_models_ids_gives(tmp_path, members):
    """n = 3 (one chunk) and 65 on a max_batch 64 object (two chunks)"""
    from zerokit_amd.batch import resource_paths
    from zerokit_amd.public import RLN, RLNError, RLNWitnessInput
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"profile": "small"}))        # window_bits 8, max_batch 64
    zp, gp = resource_paths(20, multi=True)
    rln = RLN.new_with_params(DEPTH, open(zp, "rb").read(), open(gp, "rb").read(), tree_config=str(cfgp))
    for leaf, v in zip(MEMBER_LEAVES, members[1]):
        rln.set_leaf(leaf, v)
    q, m = _ledger()
    try:
        for n in (3, 65):
            leaves, ws, rs, counts = _requests(members, n, seed=300 + n, who=[3, 2, 2] if n == 3 else None,
                                               counts=[4, 2, 2] if n == 3 else None)
            cols = [[w[k] for w in ws] for k in ("identity_secret", "user_message_limit", "x", "external_nullifier")]
            got, status = rln.generate_rln_proofs_for_members_drawn_multi(q, leaves, cols[0], cols[1], counts, cols[2], cols[3], rs)
            firsts, want = m.draw_counts(leaves, cols[3], cols[1], counts)
            assert status == want
            made = [i for i in range(n) if status[i] == OK]
            assert [got[i] is not None for i in range(n)] == [s == OK for s in status] and made and len(made) < n
            for i in made[:6] + made[-2:]:                  # (a proof a call: the first few and the last of the second chunk)
                path = rln.get_merkle_proof(leaves[i])
                w = RLNWitnessInput.new_multi(cols[0][i], cols[1][i], [firsts[i] + k if k < counts[i] else 0 for k in range(K)],
                                              path[0], path[1], cols[2][i], cols[3][i], [k < counts[i] for k in range(K)])
                assert got[i].to_bytes_le() == rln.generate_rln_proof_with_rs(w, *rs[i]).to_bytes_le(), (n, i)
            assert q.info()["residue"] == 0
        assert rln.generate_rln_proofs_for_members_drawn_multi(q, [], [], [], [], [], []) == ([], [])
        with pytest.raises(RLNError, match="ffi_generate_rln_proofs_for_members_drawn_multi: null ledger"):
            rln.generate_rln_proofs_for_members_drawn_multi(None, [0], [1], [100], [1], [5], [6])
        with pytest.raises(RLNError, match="User message limit cannot be zero"):
            rln.generate_rln_proofs_for_members_drawn_multi(q, [0], [1], [0], [1], [5], [6])
    finally:
        q.close()
    single = RLN(DEPTH, tree_config=str(cfgp))
    q = _ledger()[0]
    try:
        with pytest.raises(RLNError, match="ffi_generate_rln_proofs_for_members_drawn_multi: multi message-id circuits only"):
            single.generate_rln_proofs_for_members_drawn_multi(q, [0], [1], [100], [1], [5], [6])
        assert q.info()["draws"] == 0
    finally:
        q.close()
