"""Proving with message ids drawn on the device: rlnamd_prover_submit_members_drawn / _prove_stream_members_drawn and
ffi_generate_rln_proofs_for_members_drawn, on the fixtures of test_gpu_prove_members.py (smallest tables, a depth-20
tree with a dozen members).  Members repeat and some run past their limit.  The proofs of the granted requests are byte
for byte those of prove_members_raw given the model's ids (tests/quota_cases.py) and the same (r, s); a refused request
yields an error code, no proof bytes and its status; and a relay's NullifierLog fed every proof made says NEW to all."""
import json
import random

import pytest

import quota_cases as cases
from quota_cases import NO_EPOCH, OK, OVER

pytestmark = pytest.mark.gpu

R = cases.R
DEPTH = 20
LAST = (1 << DEPTH) - 1
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
    p = BatchProver(max_batch=64, window_bits=8)
    yield p
    p.close()


@pytest.fixture(scope="module")
def prover128():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=128, window_bits=8)
    yield p
    p.close()


def _ledger():
    from zerokit_amd.batch import QuotaLedger
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    m = cases.Model(DEPTH, 4)
    m.set_epochs([EA, EB])
    return q, m


def _requests(members, n, seed, who=None):
    """n requests: members in an unsorted order with repeats, two open epochs and one the ledger does not sign under"""
    rnd = random.Random(seed)
    who = who or [rnd.randrange(len(MEMBER_LEAVES)) for _ in range(n)]
    exts = [rnd.choice([EA, EA, EB, E_OUT] if n > 4 else [EA]) for _ in range(n)]
    ws = [dict(identity_secret=members[0][m], user_message_limit=MEMBER_LIMITS[m], message_id=0, x=rnd.randrange(R),
               external_nullifier=e) for m, e in zip(who, exts)]
    rs = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)]
    return [MEMBER_LEAVES[m] for m in who], ws, rs


def _drawn_inputs(p, ws):
    """what the drawn calls get: a message id that no request may end up with in every messageId slot"""
    return p.pack_member_inputs([dict(w, message_id=R - 5) for w in ws])


def _check(p, tree, m, leaves, ws, rs, got, status):
    """got = (proofs, values, errs) of a drawn call, status its statuses; m: the model BEFORE the call"""
    n = len(leaves)
    proofs, values, errs = got
    ids, want_status = m.draw(leaves, [w["external_nullifier"] for w in ws], [w["user_message_limit"] for w in ws])
    assert status == want_status
    made = [i for i in range(n) if status[i] == OK]
    if made:
        ref = p.prove_members_raw(tree, [leaves[i] for i in made], p.pack_member_inputs([dict(ws[i], message_id=ids[i]) for i in made]),
                                  p.pack_rs([rs[i] for i in made]))
        assert ref[2] == [0] * len(made)
        for k, i in enumerate(made):
            assert errs[i] == 0, i
            assert values[160 * i:160 * i + 160] == ref[1][160 * k:160 * k + 160], i
            assert proofs[128 * i:128 * i + 128] == ref[0][128 * k:128 * k + 128], i
    for i in range(n):
        if status[i] != OK:
            assert errs[i] != 0 and proofs[128 * i:128 * i + 128] == bytes(128), i
            # no public values either: every refused row is evaluated with ONE message id, so the y of two refused
            # requests of one member under one external nullifier would be two shares on one line
            assert values[160 * i:160 * i + 160] == bytes(160), i
    return made


def _shares(values, made):
    out = []
    for i in made:
        y, _root, nul, x, ext = (int.from_bytes(values[160 * i + 32 * j:160 * i + 32 * j + 32], "little") for j in range(5))
        out.append((nul, x, y, ext))
    return out


@pytest.mark.parametrize("n", [1, 25, 65])
def test_drawn_batches_equal_batches_with_the_models_ids(prover, prover128, tree, members, n):
    """n = 1: the host route (one copy back of the id); 25: the device route, the ids written by a kernel behind the
    staging; 65: one over a wave.  Two calls on one ledger: the second starts where the first left the counters."""
    from zerokit_amd.batch import NullifierLog
    p = prover128 if n > 64 else prover
    q, m = _ledger()
    log = NullifierLog(4 * n + 16)
    try:
        seen = set()
        for call in range(2):
            leaves, ws, rs = _requests(members, n, seed=100 * n + call, who=[3] if n == 1 and call == 0 else [0] if n == 1 else None)
            t, k, status = p.submit_members_drawn(tree, q, leaves, _drawn_inputs(p, ws), p.pack_rs(rs))
            got = p.collect_raw(t, k)
            assert set(p.residue().values()) == {0} and q.info()["residue"] == 0
            made = _check(p, tree, m, leaves, ws, rs, got, status)
            seen |= set(status)
            if made:
                st, _secrets, _first = log.observe(_shares(got[1], made))
                assert st == [NullifierLog.NEW] * len(made)         # the ledger exists so that the log never says SPAM
            cases.compare_counters(m, q, [(w["external_nullifier"], leaf) for leaf, w in zip(leaves, ws)])
        if n == 1:                                                   # a lone request past its member's limit (member 0: limit 1)
            leaves, ws, rs = _requests(members, 1, seed=5, who=[0])
            for _ in range(2):
                t, k, status = p.submit_members_drawn(tree, q, leaves, _drawn_inputs(p, ws), p.pack_rs(rs))
                made = _check(p, tree, m, leaves, ws, rs, p.collect_raw(t, k), status)
                seen |= set(status)
            assert status == [OVER] and not made
        else:
            assert seen == {OK, OVER, NO_EPOCH}
        info = q.info()
        assert (info["issued"], info["over"], info["no_epoch"]) == (m.issued, m.over, m.no_epoch)
    finally:
        log.close()
        q.close()


def test_the_stream_form_keeps_the_meaning_across_chunks(prover, tree, members):
    """65 requests through a capacity of 64: ONE draw, two chunks; member 3 (limit 100) sits on both sides of the chunk
    boundary (requests 60 .. 63 | 64) and member 2 (limit 3) runs out inside the first chunk"""
    assert int(prover.info.capacity) == 64
    q, m = _ledger()
    try:
        rnd = random.Random(65)
        who = [rnd.randrange(len(MEMBER_LEAVES)) for _ in range(65)]
        who[60:65] = [3, 3, 3, 3, 3]
        who[50:56] = [2] * 6
        leaves, ws, rs = _requests(members, 65, seed=66, who=who)
        for i in list(range(50, 56)) + list(range(60, 65)):
            ws[i]["external_nullifier"] = EA
        proofs, values, errs, status = prover.prove_members_drawn_raw(tree, q, leaves, _drawn_inputs(prover, ws), prover.pack_rs(rs))
        made = _check(prover, tree, m, leaves, ws, rs, (proofs, values, errs), status)
        assert status[60:65] == [OK] * 5 and status[50:56].count(OVER) >= 3
        nullifiers = [values[160 * i + 64:160 * i + 96] for i in range(60, 65)]
        assert len(set(nullifiers)) == 5                             # five message ids of one member under one epoch
        assert set(prover.residue().values()) == {0} and q.info()["residue"] == 0 and q.info()["draws"] == 1
        out, st = prover.prove_members_drawn(tree, q, leaves[:3], ws[:3], rs[:3])
        assert st == m.draw(leaves[:3], [w["external_nullifier"] for w in ws[:3]], [w["user_message_limit"] for w in ws[:3]])[1]
        assert len(out) == 3 and len(made) > 40
        # member 2 has used its limit under EA: six more requests, all OVER, and nothing of them reaches the caller
        out, st = prover.prove_members_drawn(tree, q, leaves[50:56], ws[50:56], rs[50:56])
        assert st == [OVER] * 6 == m.draw(leaves[50:56], [EA] * 6, [3] * 6)[1]
        assert all(o["error"] != 0 and o["proof"] == bytes(128) and set(o["public_inputs"]) == {0} for o in out)
    finally:
        q.close()


def test_refusals_have_their_own_texts_and_draw_nothing(prover, tree, members):
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import PoseidonTree, QuotaLedger
    q, m = _ledger()
    shallow = QuotaLedger(10, 2)
    try:
        leaves, ws, rs = _requests(members, 25, seed=9)
        inp, rsb = _drawn_inputs(prover, ws), prover.pack_rs(rs)
        t, k, status = prover.submit_members_drawn(tree, q, leaves, inp, rsb)
        _check(prover, tree, m, leaves, ws, rs, prover.collect_raw(t, k), status)
        # a ticket handed out now and the one after the refusals are consecutive: nothing was enqueued in between
        t0, k = prover.submit_members(tree, leaves[:2], prover.pack_member_inputs(ws[:2]), prover.pack_rs(rs[:2]))
        prover.collect_raw(t0, k)
        before = (q.info(), q.used(leaves, [w["external_nullifier"] for w in ws]))
        with pytest.raises(RLNError, match=r"the ledger's depth \(10\) is not the tree's \(20\)"):
            prover.submit_members_drawn(tree, shallow, leaves, inp, rsb)
        bad = list(leaves)
        bad[13] = 1 << DEPTH
        with pytest.raises(RLNError, match="leaf index 1048576 is outside a tree of depth 20"):
            prover.submit_members_drawn(tree, q, bad, inp, rsb)
        wide = _drawn_inputs(prover, ws[:7] + [dict(ws[7], user_message_limit=1 << 32)] + ws[8:])
        for call in (prover.submit_members_drawn, prover.prove_members_drawn_raw):
            with pytest.raises(RLNError, match="the message limit of proof 7 is 2\\^32 or more"):
                call(tree, q, leaves, wide, rsb)
        small = PoseidonTree(10)
        with pytest.raises(RLNError, match=r"the tree's depth \(10\) is not the circuit's \(20\)"):
            prover.submit_members_drawn(small, shallow, [leaf % 1024 for leaf in leaves], inp, rsb)
        small.close()
        assert (q.info(), q.used(leaves, [w["external_nullifier"] for w in ws])) == before
        assert shallow.info()["draws"] == 0
        t1, k, status = prover.submit_members_drawn(tree, q, leaves, inp, rsb)      # nothing was enqueued in between
        assert t1 == t0 + 1
        _check(prover, tree, m, leaves, ws, rs, prover.collect_raw(t1, k), status)   # usable afterwards
    finally:
        shallow.close()
        q.close()


def test_a_multi_message_id_prover_is_refused():
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import BatchProver, PoseidonTree, QuotaLedger
    p, t, q = BatchProver(max_batch=64, window_bits=8, multi=True), PoseidonTree(DEPTH), QuotaLedger(DEPTH, 1)
    try:
        n_in = p.inputs_size * 32
        with pytest.raises(RLNError, match="names no single messageId input"):
            p.submit_members_drawn(t, q, [0], bytes(n_in), bytes(64))
        assert q.info()["draws"] == 0
    finally:
        q.close()
        t.close()
        p.close()


# ------------------------------------------------------------------------------------------------------ the FFI
def test_the_ffi_entry_gives_what_the_batch_call_gives(tmp_path, members, tree):
    """n = 3 (one batch, the host route) and 65 on a max_batch 64 object (streamed: 64 + 1)"""
    from zerokit_amd.public import RLN
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"profile": "small"}))        # window_bits 8, max_batch 64
    rln = RLN(DEPTH, tree_config=str(cfgp))
    for leaf, v in zip(MEMBER_LEAVES, members[1]):
        rln.set_leaf(leaf, v)
    q, m = _ledger()
    try:
        for n in (3, 65):
            leaves, ws, rs = _requests(members, n, seed=300 + n, who=[3, 0, 0] if n == 3 else None)
            cols = [[w[k] for w in ws] for k in ("identity_secret", "user_message_limit", "x", "external_nullifier")]
            got, status = rln.generate_rln_proofs_for_members_drawn(q, leaves, *cols, rs)
            ids, want = m.draw(leaves, cols[3], cols[1])
            assert status == want
            made = [i for i in range(n) if status[i] == OK]
            assert [got[i] is not None for i in range(n)] == [s == OK for s in status] and made and len(made) < n
            ref = rln.generate_rln_proofs_for_members([leaves[i] for i in made], [cols[0][i] for i in made], [cols[1][i] for i in made],
                                                      [ids[i] for i in made], [cols[2][i] for i in made], [cols[3][i] for i in made],
                                                      [rs[i] for i in made])
            assert [got[i].to_bytes_le() for i in made] == [r.to_bytes_le() for r in ref], n
            assert all(got[i].values.root == tree.root() for i in made)
            assert q.info()["residue"] == 0
        assert rln.generate_rln_proofs_for_members_drawn(q, [], [], [], [], []) == ([], [])
    finally:
        q.close()


def test_the_ffi_entry_refuses_a_multi_message_id_object():
    from zerokit_amd.batch import QuotaLedger, resource_paths
    from zerokit_amd.public import RLN, RLNError
    zp, gp = resource_paths(20, multi=True)
    rln = RLN.new_with_params(20, open(zp, "rb").read(), open(gp, "rb").read())
    q = QuotaLedger(DEPTH, 1)
    try:
        with pytest.raises(RLNError, match="ffi_generate_rln_proofs_for_members_drawn: single message-id circuits only"):
            rln.generate_rln_proofs_for_members_drawn(q, [0], [1], [100], [5], [6])
        with pytest.raises(RLNError, match="ffi_generate_rln_proofs_for_members_drawn: null ledger"):
            rln.generate_rln_proofs_for_members_drawn(None, [0], [1], [100], [5], [6])
    finally:
        q.close()
