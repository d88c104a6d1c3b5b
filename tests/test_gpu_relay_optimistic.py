"""The relay step with the combined pairing check (rlnamd_relay_new_ex: RLNAMD_RELAY_OPTIMISTIC [| _TEAMS]) against the
exact relay (flags = 0) on twin logs: verdicts, statuses, secrets and first tags byte-equal, the logs equal in every
record, and the verifier's counters (rlnamd_verify_gpu_optimistic_stats, rlnamd_verify_gpu_passes) saying which path a
chunk took.  And the scalars' derivation on the device (rlnamd_verify_gpu_aggregate_seeded) against the host's
(rlnamd_verify_agg_scalars) through the two aggregate entries that take scalars.

The helpers and the generated proofs are those of test_gpu_relay.py, taken from that module."""
import ctypes as C

import pytest

import test_gpu_relay as tr
import verify_cases as vc
from test_gpu_relay import (BAD_PROOF, BAD_ROOT, BAD_SIGNAL, DUPLICATE, NEW, OK, SKIPPED, SPAM, generated, hasher,  # noqa: F401
                            prover)
from verify_cases import GT_ONE, le

pytestmark = pytest.mark.gpu

SEED32 = bytes((7 * i + 3) & 0xFF for i in range(32))
STAT_KEYS = ("combined", "accepted", "fell_back", "skipped_in_cooldown", "refused_proofs", "combined_team")


@pytest.fixture(autouse=True)
def _quiet(request):
    """every test starts outside a cool-down, with cool-down 0, and leaves the default behind"""
    p = request.getfixturevalue("prover") if "prover" in request.fixturenames else None
    if p is not None:
        p.verify_set_cooldown(0)
    yield
    if p is not None:
        p.verify_set_cooldown(0)
        p.verify_set_cooldown(16)


def raw(v):
    return (int(v) % (1 << 256)).to_bytes(32, "little")


def named_rejects(case):
    return dict((nm.split("/")[1], (pr, b"".join(raw(v) for v in pu))) for nm, pr, pu in vc.rejects(*case))


@pytest.fixture(scope="module")
def pool(generated):
    """valid rows (proof, values): the golden depth-20 proofs and the generated ones; `forged`: proof 1's points under
    proof 0's values (every per-proof check passes, the pairing does not); `refused`: a non-canonical encoding"""
    g = vc.golden_h20()
    valid = [(c[1], b"".join(raw(v) for v in c[2])) for c in g] + [(r[0], r[1]) for r in generated["rows"]]
    rj = named_rejects(g[2])
    return dict(valid=valid, forged=(valid[1][0], valid[0][1]), refused=rj["A_noncanonical_x"], input0=rj["input0"],
                off_curve=rj["A_off_curve"])


def valid_rows(pool, n, shift=0):
    v = pool["valid"]
    return [v[(i + shift) % len(v)] for i in range(n)]


def pack(rows):
    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[1][96:128] for r in rows)


def stats(p):
    s = p.verify_optimistic_stats()
    return {k: s[k] for k in STAT_KEYS}, p.verify_gpu_passes()


def pair(prover, seed_share, lanes, rows, optimistic=True, team_checks=False, xs=None, roots=b"", tags=None, nv=5,
         capacity=None):
    """one step of an optimistic relay and of an exact relay over the same rows on fresh twin logs -> (the step's
    results, the change of the optimistic counters and of the passes over the optimistic step, its info).  Results and
    logs must be equal."""
    from zerokit_amd.batch import Relay
    n = len(rows)
    logs = tr.twin_logs(capacity or max(n, 16), seed_share)
    opt = Relay(prover, logs[0], None, lanes, optimistic=optimistic, team_checks=team_checks)
    exact = Relay(prover, logs[1], None, lanes)
    try:
        proofs, values, own = pack(rows)
        kw = dict(xs=own if xs is None else xs, roots=roots, tags=tags)
        s0, p0 = stats(prover)
        got = tr.relay_step(opt, n, proofs, values, nv, **kw)
        s1, p1 = stats(prover)
        want = tr.relay_step(exact, n, proofs, values, nv, **kw)
        assert got[0] == want[0] and got[1] == want[1]
        assert got == want
        tr.logs_equal(*logs)
        info = opt.info()
        assert info["residue_words"] == 0 and info["messages"] == n and info["reserved"] == 0
        return got, {k: s1[k] - s0[k] for k in s0}, (p1[0] - p0[0], p1[1] - p0[1]), info
    finally:
        opt.close()
        exact.close()
        for log in logs:
            log.close()


# ------------------------------------------------------------------------------------------- the seeded aggregate

def chunk_scalars(n, step):
    from zerokit_amd.batch import agg_scalars
    out = []
    for c, off in enumerate(range(0, n, step)):
        out += agg_scalars(SEED32, c, min(step, n - off))
    return out


def aggregates(prover, rows, lanes):
    """(seeded on the device, rlnamd_verify_gpu_aggregate_ex under the host's scalars, the host twin under them)"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    proofs, values, _xs = pack(rows)
    sc = b"".join(s.to_bytes(16, "little") for s in chunk_scalars(n, 8192 if lanes == 8 else 65536))
    out = []
    for which in range(3):
        gt, rej = C.create_string_buffer(384), C.create_string_buffer(b"\x07" * n, n)
        if which == 0:
            check(lib().rlnamd_verify_gpu_aggregate_seeded(prover._h, n, proofs, values, 5, SEED32, lanes, gt, rej))
        elif which == 1:
            check(lib().rlnamd_verify_gpu_aggregate_ex(prover._h, n, proofs, values, 5, sc, lanes, gt, rej))
        else:
            z = vc.zkey_bytes(20)
            check(lib().rlnamd_verify_aggregate_with_zkey(z, len(z), n, proofs, values, 5, sc, gt, rej))
        out.append((gt.raw, rej.raw[:n]))
    return out


@pytest.mark.parametrize("lanes,n", [(8, 1), (8, 9), (8, 65), (8, 8193), (1, 65), (1, 4097)])
def test_seeded_aggregate_equals_the_supplied_scalars(prover, pool, lanes, n):
    """the group of 8, the fold of 64, a second chunk whose counter is 1 (lanes = 8: chunks of 8 192), the third fold
    level (lanes = 1).  Value and reject flags of the three entries agree; with one refused and one forged proof in the
    set the value is not 1, and all-valid sets give 1.  (n = 1 holds one row: valid, refused and forged in turn.)"""
    rows = valid_rows(pool, n, shift=n % 5)
    seeded, supplied, host = aggregates(prover, rows, lanes)
    assert seeded == supplied == host == (GT_ONE, bytes(n))
    if n == 1:
        for bad, flag, one in ((pool["refused"], b"\x01", True), (pool["forged"], b"\x00", False)):
            seeded, supplied, host = aggregates(prover, [bad], lanes)
            assert seeded == supplied == host and seeded[1] == flag and (seeded[0] == GT_ONE) == one
        return
    rows[n // 3], rows[n - 1] = pool["refused"], pool["forged"]   # the forged one in the last group, and in chunk 1
    seeded, supplied, host = aggregates(prover, rows, lanes)
    assert seeded[1] == supplied[1] == host[1] and sum(seeded[1]) == 1 and seeded[1][n // 3] == 1
    assert seeded[0] == supplied[0] == host[0] and seeded[0] != GT_ONE


def test_seeded_aggregate_errors(prover, pool):
    from zerokit_amd import RLNError
    pr, pu = [pool["valid"][0][0]], [[int.from_bytes(pool["valid"][0][1][32 * j:32 * j + 32], "little") for j in range(5)]]
    assert prover.verify_aggregate_seeded(pr, pu, SEED32, lanes=8) == (GT_ONE, [False])
    assert prover.verify_aggregate_seeded([], [], SEED32)[0] == GT_ONE
    with pytest.raises(RLNError, match="lanes must be 1 or 8"):
        prover.verify_aggregate_seeded(pr, pu, SEED32, lanes=0)
    with pytest.raises(RLNError, match="32 bytes"):
        prover.verify_aggregate_seeded(pr, pu, SEED32[:31])


# ------------------------------------------------------------------------------------------------ the relay step

@pytest.mark.parametrize("lanes,teams,n", [(8, True, 1), (8, True, 64), (8, True, 65), (8, True, 257), (8, True, 8192),
                                           (8, True, 8193), (1, False, 4097), (1, False, 65537)])
def test_all_valid_chunks_are_accepted_without_an_exact_pass(prover, generated, pool, lanes, teams, n):
    rows = valid_rows(pool, n, shift=n % 3)
    got, d, passes, info = pair(prover, generated["seed"], lanes, rows, team_checks=teams, tags=[50 + i for i in range(n)])
    chunks = -(-n // (8192 if lanes == 8 else 65536))
    assert list(got[0]) == [OK] * n and SKIPPED not in got[1]
    assert d == dict(combined=chunks, accepted=chunks, fell_back=0, skipped_in_cooldown=0, refused_proofs=0,
                     combined_team=chunks if lanes == 8 else 0)
    assert passes == (0, 0)
    assert info["chunks"] == chunks and info["accepted"] == n


@pytest.mark.parametrize("lanes,teams,n,at", [(8, True, 65, 64), (1, False, 4097, 2048), (8, True, 8193, 8192)])
def test_one_forged_proof_falls_back_to_the_exact_pass(prover, generated, pool, lanes, teams, n, at):
    """proof 1's points under proof 0's values with cool-down 0: its chunk falls back, the exact pass of the same shape
    runs once over the resident inputs, and the message is BAD_PROOF although its root is outside the window too"""
    rows = valid_rows(pool, n)
    rows[at] = pool["forged"]
    roots = b"".join(sorted(set(r[1][32:64] for r in pool["valid"][1:])))
    assert pool["forged"][1][32:64] not in [roots[o:o + 32] for o in range(0, len(roots), 32)]
    got, d, passes, _info = pair(prover, generated["seed"], lanes, rows, team_checks=teams, roots=roots)
    chunks = -(-n // (8192 if lanes == 8 else 65536))
    assert got[0][at] == BAD_PROOF and got[1][at] == SKIPPED
    assert [i for i in range(n) if got[0][i] == BAD_PROOF] == [at]
    assert set(got[0]) == {OK, BAD_PROOF, BAD_ROOT}   # the valid rows under the first proof's root are outside the window
    assert (d["combined"], d["accepted"], d["fell_back"], d["skipped_in_cooldown"]) == (chunks, chunks - 1, 1, 0)
    assert passes == ((0, 1) if lanes == 8 else (1, 0))


def test_a_refused_proof_is_named_without_an_exact_pass(prover, generated, pool):
    """a non-canonical encoding and a point off the curve among valid rows: the chunk is accepted, those messages are
    BAD_PROOF, stats[4] counts them, nothing falls back"""
    rows = valid_rows(pool, 70)
    rows[5], rows[69] = pool["refused"], pool["off_curve"]
    got, d, passes, _info = pair(prover, generated["seed"], 8, rows, team_checks=True)
    assert [i for i in range(70) if got[0][i] != OK] == [5, 69] and got[0][5] == got[0][69] == BAD_PROOF
    assert got[1][5] == got[1][69] == SKIPPED
    assert d == dict(combined=1, accepted=1, fell_back=0, skipped_in_cooldown=0, refused_proofs=2, combined_team=1)
    assert passes == (0, 0)


def test_wrong_root_or_signal_on_valid_proofs(prover, generated, pool):
    """the chunk is accepted; the gate names the root and the signal, in that order, and their statuses are SKIPPED"""
    n = 40
    rows = valid_rows(pool, n)
    _p, _v, own = pack(rows)
    xs = bytearray(own)
    wrong_signal = [3, 17, 39]
    for i in wrong_signal:
        xs[32 * i:32 * i + 32] = le(777000 + i)
    first_root = pool["valid"][0][1][32:64]
    roots = b"".join(sorted(set(r[1][32:64] for r in pool["valid"]) - {first_root}))
    got, d, passes, _info = pair(prover, generated["seed"], 8, rows, team_checks=True, xs=bytes(xs), roots=roots)
    for i in range(n):
        want = BAD_ROOT if rows[i][1][32:64] == first_root else BAD_SIGNAL if i in wrong_signal else OK
        assert got[0][i] == want, i
        assert (got[1][i] == SKIPPED) == (want != OK)
    assert {OK, BAD_ROOT, BAD_SIGNAL} == set(got[0])
    assert (d["combined"], d["accepted"], d["fell_back"], d["refused_proofs"]) == (1, 1, 0, 0) and passes == (0, 0)


def test_cooldown_two_skips_two_chunks(prover, generated, pool):
    """a rejected chunk, then three all-valid steps on the same relay: two run the exact team pass uncombined, the
    third is checked combined again; every step equals the exact relay's"""
    from zerokit_amd.batch import Relay
    prover.verify_set_cooldown(2)
    logs = tr.twin_logs(1024, generated["seed"])
    opt = Relay(prover, logs[0], None, 8, optimistic=True, team_checks=True)
    exact = Relay(prover, logs[1], None, 8)
    try:
        seen = []
        for step in range(4):
            rows = valid_rows(pool, 65, shift=step)
            if step == 0:
                rows[33] = pool["forged"]
            proofs, values, xs = pack(rows)
            s0, p0 = stats(prover)
            got = tr.relay_step(opt, 65, proofs, values, 5, xs=xs)
            s1, p1 = stats(prover)
            assert got == tr.relay_step(exact, 65, proofs, values, 5, xs=xs)
            tr.logs_equal(*logs)
            assert (got[0].count(BAD_PROOF), got[0].count(OK)) == ((1, 64) if step == 0 else (0, 65))
            seen.append((s1["combined"] - s0["combined"], s1["accepted"] - s0["accepted"], s1["fell_back"] - s0["fell_back"],
                         s1["skipped_in_cooldown"] - s0["skipped_in_cooldown"], p1[1] - p0[1], p1[0] - p0[0]))
        assert seen == [(1, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 0), (0, 0, 0, 1, 1, 0), (1, 1, 0, 0, 0, 0)]
        assert opt.info()["residue_words"] == 0
    finally:
        opt.close()
        exact.close()
        for log in logs:
            log.close()


def test_teams_without_the_teams_flag_are_the_exact_pass(prover, generated, pool):
    rows = valid_rows(pool, 65)
    _got, d, passes, _info = pair(prover, generated["seed"], 8, rows, team_checks=False)
    assert d == dict(combined=0, accepted=0, fell_back=0, skipped_in_cooldown=0, refused_proofs=0, combined_team=0)
    assert passes == (0, 1)
    _got, d, passes, _info = pair(prover, generated["seed"], 0, rows, team_checks=False)   # lanes = 0: teams at this n
    assert d["combined"] == 0 and passes == (0, 1)


def test_the_multi_message_id_circuit(hasher):
    """n_values = 15: used and unused slots and one SPAM pair, both flags; results equal the exact relay's"""
    from zerokit_amd.batch import BatchProver
    p = BatchProver(depth=20, multi=True, max_batch=64, window_bits=8)
    try:
        nv = p.num_public
        assert nv == 15
        sig = tr.SIGNALS
        named = [tr._multi(0, [1, 2, 3, 4], [1, 0, 0, 0], sig[0], tr.EXT1),    # NEW
                 tr._multi(0, [5, 6, 1, 7], [1, 0, 1, 0], sig[1], tr.EXT1),    # slot 2: id 1 under another x, SPAM
                 tr._multi(1, [1, 2, 3, 4], [0, 1, 1, 0], sig[3], tr.EXT1),    # two NEW
                 tr._multi(2, [1, 2, 3, 4], [1, 1, 1, 1], sig[4], tr.EXT1)]    # four NEW
        gp, gv = tr._prove_public(p, named)
        rows = [(gp[128 * i:128 * i + 128], gv[32 * nv * i:32 * nv * (i + 1)]) for i in range(len(named))]
        rows.append(rows[0])   # DUPLICATE
        xs = b"".join(r[1][32 * 9:32 * 10] for r in rows)
        p.verify_set_cooldown(0)
        for lanes, teams in ((8, True), (1, False)):
            got, d, passes, _info = pair(p, le(1) + le(2) + le(3) + le(4), lanes, rows, team_checks=teams, xs=xs, nv=nv,
                                         capacity=64)
            assert list(got[0]) == [OK] * 5 and list(got[1]) == [NEW, SPAM, NEW, NEW, DUPLICATE]
            assert got[2][32:64] == le(tr.SECRETS[0])
            assert (d["combined"], d["accepted"], d["fell_back"]) == (1, 1, 0) and passes == (0, 0)
    finally:
        p.close()


def test_every_refusal_leaves_everything_as_it_was(prover, hasher, generated):
    """the refusals of test_gpu_relay.py::test_every_refusal_leaves_the_log_as_it_was on optimistic relays: the log,
    the hasher, the passes and the optimistic counters do not move"""
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import NullifierLog, Relay
    n, proofs, values, signals, offsets, xs = tr._signals_case(generated, [0, 1, 2, 3])
    logs = tr.twin_logs(16, generated["seed"])
    kw = dict(optimistic=True, team_checks=True)
    with_hasher, without = Relay(prover, logs[0], hasher, 0, **kw), Relay(prover, logs[0], None, 0, **kw)
    small = NullifierLog(3, tr.SEED)
    tight = Relay(prover, small, None, 0, **kw)
    exact = Relay(prover, logs[1], hasher, 0)
    try:
        first = tr.relay_step(with_hasher, 2, proofs[:256], values[:320], 5, signals=signals[:offsets[2]], offsets=offsets[:3])
        assert first == tr.relay_step(exact, 2, proofs[:256], values[:320], 5, signals=signals[:offsets[2]], offsets=offsets[:3])
        state = lambda: (logs[0].info(), logs[0].retire_info(), tr.records(logs[0]), hasher.info()["calls"],   # noqa: E731
                         prover.verify_gpu_passes(), prover.verify_optimistic_stats())
        before = state()
        assert before[5]["combined"] >= 1
        for relay, rkw, text in (
                (with_hasher, dict(xs=None), "neither signals nor xs_le"),
                (with_hasher, dict(xs=xs, signals=signals, offsets=offsets), "both signals and xs_le"),
                (without, dict(signals=signals, offsets=offsets), "made without a hasher"),
                (with_hasher, dict(signals=signals, offsets=[0, 5, 3, 6, 7]), "offsets decrease"),
                (with_hasher, dict(signals=signals[:-1], offsets=offsets), "the last offset lies beyond data_len"),
                (with_hasher, dict(xs=xs, nv=4), "n_values is not the key's"),
                (with_hasher, dict(xs=xs, roots=bytes(32 * 65)), "at most 64 roots")):
            nv = rkw.pop("nv", 5)
            with pytest.raises(RLNError, match=text):
                tr.relay_step(relay, n, proofs, values[:32 * nv * n], nv, **rkw)
        null = (C.c_uint64 * 1)()
        assert tr._lib().rlnamd_relay_step(with_hasher._h, n, None, values, 5, None, 0, None, xs, None, 0, None, proofs, proofs,
                                           None, null) != 0 and "null pointer for n > 0" in tr._err()
        with pytest.raises(RLNError, match="4 messages of up to 1 shares do not fit: 3 of 3 records are left"):
            tr.relay_step(tight, n, proofs, values, 5, xs=xs)
        assert small.info()[1] == 0
        assert state() == before
        # and the next steps work, on the tight log too
        assert tr.relay_step(with_hasher, 0, b"", b"", 5, xs=b"") == (b"", b"", b"", [])
        got = tr.relay_step(with_hasher, n, proofs, values, 5, signals=signals, offsets=offsets)
        assert got == tr.relay_step(exact, n, proofs, values, 5, signals=signals, offsets=offsets)
        tr.logs_equal(*logs)
        assert list(tr.relay_step(tight, 3, proofs[:384], values[:480], 5, xs=xs[:96])[1]) == [NEW, NEW, SPAM]
    finally:
        for r in (with_hasher, without, tight, exact):
            r.close()
        small.close()
        for log in logs:
            log.close()


# ------------------------------------------------------------------------------------------- the drop-in boundary

def _objects(tmp_path, make, count=3):
    import json
    objs = []
    for k, cfg in enumerate(({"verify_optimistic": True, "verify_optimistic_cooldown": 0, "relay_gpu_min": 1},
                             {"relay_gpu_min": 1},
                             {"verify_optimistic": True, "verify_optimistic_teams": True, "verify_optimistic_cooldown": 0,
                              "relay_gpu_min": 1})[:count]):
        cfgp = tmp_path / ("opt%d.json" % k)
        cfgp.write_text(json.dumps(cfg))
        objs.append(make(str(cfgp)))
    return objs


def test_ffi_relay_step_of_an_optimistic_object(tmp_path):
    """the nine messages of test_the_drop_in_entries_equal_the_existing_calls through ffi_relay_step of an object with
    "verify_optimistic" and of one without, both on the device route, on twin logs: the same verdicts, statuses, secrets
    and first tags with a roots window and with roots = None; the optimistic object's step ran a combined check; and it
    refuses 9 messages on a log of 8 records, which only the device route does"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.batch import NullifierLog
    from zerokit_amd.public import RLN, RLNWitnessInput
    objs = _objects(tmp_path, lambda cfg: RLN(20, tree_config=cfg))
    secret = hashers.hash_to_field_le(b"relay-step-member")
    for obj in objs:
        obj.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = objs[0].get_merkle_proof(3)
    signals = [b"relay message %d " % i * (1 + 9 * i) for i in range(8)]
    signals[5] = b""
    xs = [hashers.hash_to_field_le(s) for s in signals]
    ids = [0, 1, 2, 3, 1, 4, 5, 0]
    ws = [RLNWitnessInput(secret, 100, ids[i], path[0], path[1], xs[i], 4242) for i in range(8)]
    proofs = objs[0].generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(8)])
    proofs.append(proofs[6])
    signals.append(signals[6])
    root = proofs[0].values.root
    sent = list(signals)
    sent[2] = sent[2][:4] + bytes([sent[2][4] ^ 1]) + sent[2][5:]
    tags = [100 + i for i in range(9)]
    for roots in (None, [12345, root]):
        logs = NullifierLog(64, tr.SEED), NullifierLog(64, tr.SEED), NullifierLog(64, tr.SEED)
        try:
            for tg in (tags, None):
                got = objs[0].relay_step(logs[0], proofs, sent, roots, tg)
                want = objs[1].relay_step(logs[1], proofs, sent, roots, tg)
                assert got == want
                # 9 messages take teams: with "verify_optimistic_teams" the step is checked combined, and accepted
                s0 = objs[2].verify_stats()
                assert objs[2].relay_step(logs[2], proofs, sent, roots, tg) == want
                s1 = objs[2].verify_stats()
                assert [s1[k] - s0[k] for k in ("combined", "accepted", "fell_back", "combined_team", "team_passes")] == [1, 1, 0, 1, 0]
                if tg is not None:
                    assert got[0] == [OK, OK, BAD_SIGNAL] + [OK] * 6
                    assert got[1] == [NEW, NEW, SKIPPED, NEW, SPAM, NEW, NEW, SPAM, DUPLICATE]
                    assert got[2][4] == secret and got[2][7] == secret and got[3][8] == 106
            tr.logs_equal(logs[0], logs[1])
            tr.logs_equal(logs[2], logs[1])
        finally:
            for log in logs:
                log.close()
    assert objs[0].verify_stats()["combined"] == 0 and objs[0].verify_stats()["team_passes"] >= 4   # teams, no teams flag
    log = NullifierLog(8, tr.SEED)
    try:
        with pytest.raises(RLNError, match="9 messages of up to 1 shares do not fit"):
            objs[0].relay_step(log, proofs, sent, [])
        assert log.info()[1] == 0
    finally:
        log.close()


def test_the_v3_entry_of_an_optimistic_object(tmp_path):
    from zerokit_amd import hashers
    from zerokit_amd.batch import NullifierLog, resource_paths
    from zerokit_amd.public_v3 import RLNV3, RLNWitnessInputV3
    zp, gp = resource_paths(20)
    z, g = open(zp, "rb").read(), open(gp, "rb").read()
    objs = _objects(tmp_path, lambda cfg: RLNV3.stateful(20, z, g, tree="pm", config_path=cfg), count=2)
    secret = 777
    for obj in objs:
        obj.set_next_leaf(5)
        obj.set_next_leaf(hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 10))
    elems, bits = objs[0].get_merkle_proof(1)
    msgs = [b"v3 message %d" % i * (1 + 40 * i) for i in range(4)]
    xs = [hashers.hash_to_field_le(s) for s in msgs]
    ids = [0, 1, 2, 0]
    proofs = [objs[0].generate_proof(RLNWitnessInputV3.new_single(secret, 10, ids[i], elems, bits, xs[i], 55)) for i in range(4)]
    sent = list(msgs)
    sent[1] = sent[1] + b"!"
    logs = NullifierLog(32, tr.SEED), NullifierLog(32, tr.SEED)
    try:
        got = objs[0].relay_step(logs[0], proofs, sent, None, [7, 8, 9, 10])
        assert got == objs[1].relay_step(logs[1], proofs, sent, None, [7, 8, 9, 10])
        assert got[0] == [OK, BAD_SIGNAL, OK, OK] and got[1] == [NEW, SKIPPED, NEW, SPAM] and got[2][3] == secret
        tr.logs_equal(*logs)
    finally:
        for log in logs:
            log.close()
