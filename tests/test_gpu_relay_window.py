"""The relay step's epoch window on the device (rlnamd_relay_set_epochs, rlnamd_relay_epochs, RLNAMD_RELAY_BAD_EPOCH;
ffi_relay_set_epochs and its V3 twin).  The yardstick is the composition: rlnamd_verify_many_gpu_ex, the model's gate
on the host -- tests/test_gpu_relay.py's, with one more check behind the three: OK and an external nullifier outside the
window is BAD_EPOCH -- and ONE observe(take) on a twin log with the same seed.  Verdicts, statuses, secrets and first
tags must be byte-equal and the logs equal afterwards.

Proofs are made in the module's fixture under three external nullifiers, two of which the window holds; FOREIGN needs a
nullifier under two external nullifiers that both pass, which no valid proof gives, so both logs start with one
hand-made record."""
import ctypes as C

import pytest

import test_gpu_relay as tr
import verify_cases as vc
from test_gpu_relay import (BAD_PROOF, BAD_ROOT, BAD_SIGNAL, DUPLICATE, FOREIGN, NEW, OK, SECRETS, SEED, SIGNALS, SKIPPED, SPAM,  # noqa: F401
                            hasher, prover)
from verify_cases import le

pytestmark = pytest.mark.gpu

BAD_EPOCH = 4
EA, EB, EC = 9101, 9102, 9103
GEN = [(0, 1, 0, EA), (1, 1, 1, EA), (0, 1, 2, EA), (2, 1, 3, EB), (2, 1, 4, EB), (3, 1, 5, EC), (3, 2, 0, EC), (1, 1, 1, EB)]
# in arrival order under the window {EA, EB}: NEW, NEW, SPAM, NEW, SPAM, BAD_EPOCH, BAD_EPOCH, FOREIGN (the seeded record)


def window_of(k, inside=(EA, EB)):
    """a window of k elements whose only matching ones come last"""
    inside = list(inside)[-k:]
    return [70000 + j for j in range(k - len(inside))] + inside


@pytest.fixture(scope="module")
def generated(prover):
    proofs, values = tr._prove(prover, [tr._single(m, j, SIGNALS[s], e) for m, j, s, e in GEN])
    rows = [(proofs[128 * i:128 * i + 128], values[160 * i:160 * i + 160], SIGNALS[GEN[i][2]]) for i in range(len(GEN))]
    seed_share = rows[7][1][64:96] + le(5) + le(7) + le(EA)   # the nullifier of row 7 (under EB) recorded under EA
    return dict(rows=rows, seed=seed_share)


@pytest.fixture(scope="module")
def base(generated):
    """the tile: every golden depth-20 case with its rejects (their external nullifier is in no window here), the
    generated rows and two replays; xs is each row's own x except in every 11th row.  Computed once, never changed."""
    rows, valid = [], []
    for name, proof, pub in vc.golden_h20():
        valid.append(len(rows))
        for _nm, pr, pu in [(name, proof, pub)] + vc.rejects(name, proof, pub):
            rows.append((pr, b"".join((int(v) % (1 << 256)).to_bytes(32, "little") for v in pu), None))
    valid += range(len(rows), len(rows) + len(generated["rows"]))
    rows += generated["rows"] + [generated["rows"][0], generated["rows"][3], generated["rows"][5]]
    xs = [le(12345 + i) if i % 11 == 10 else r[1][96:128] for i, r in enumerate(rows)]
    return dict(n=len(rows), proofs=b"".join(r[0] for r in rows), values=b"".join(r[1] for r in rows), xs=b"".join(xs),
                roots=sorted(set(rows[i][1][32:64] for i in valid[1:])))


def compose(p, log, lanes, n, proofs, values, nv, k, xs, roots, tags, window):
    """verify, the model's gate with the window on the host, observe(take) -- over packed rows"""
    from zerokit_amd._native import check, lib
    ok = C.create_string_buffer(max(n, 1))
    check(lib().rlnamd_verify_many_gpu_ex(p._h, n, proofs, values, nv, lanes, ok, None))
    ok = ok.raw
    root_set = set(roots[o:o + 32] for o in range(0, len(roots), 32))
    win = set(le(e) for e in window)
    one, zero = le(1), le(0)
    verdict, counts, shares, share_tags = bytearray(n), [], [], []
    for i in range(n):
        v = values[32 * nv * i:32 * nv * (i + 1)]
        val = lambda j: v[32 * j:32 * j + 32]   # noqa: E731
        if k == 1:
            ys, root, nuls, x, ext, sel = [val(0)], val(1), [val(2)], val(3), val(4), [one]
        else:
            ys, root, nuls = [val(s) for s in range(k)], val(k), [val(k + 1 + s) for s in range(k)]
            x, ext, sel = val(2 * k + 1), val(2 * k + 2), [val(2 * k + 3 + s) for s in range(k)]
        if not ok[i] or any(s not in (one, zero) for s in sel):
            verdict[i] = BAD_PROOF
        elif root_set and root not in root_set:
            verdict[i] = BAD_ROOT
        elif xs[32 * i:32 * i + 32] != x:
            verdict[i] = BAD_SIGNAL
        elif win and ext not in win:
            verdict[i] = BAD_EPOCH
        used = [s for s in range(k) if sel[s] == one] if verdict[i] == OK else []
        counts.append(len(used))
        for s in used:
            shares.append(nuls[s] + x + ys[s] + ext)
            if tags is not None:
                share_tags.append(tags[i])
    st, sec, ft = log.observe_raw(b"".join(shares), share_tags if tags is not None else None) if shares else (b"", b"", [])
    status, secrets, first, at = bytearray(n), bytearray(32 * n), [0] * n, 0
    for i, c in enumerate(counts):
        status[i] = SKIPPED
        for want in (SPAM, FOREIGN, DUPLICATE, NEW):
            hit = [j for j in range(at, at + c) if st[j] == want]
            if hit:
                status[i], secrets[32 * i:32 * i + 32], first[i] = want, sec[32 * hit[0]:32 * hit[0] + 32], ft[hit[0]]
                break
        at += c
    return bytes(verdict), bytes(status), bytes(secrets), first


def same_logs(a, b):
    """tests/test_gpu_relay.py's logs_equal without retire_info[4], the longest walk of the last rebuild, which depends on
    the order in which the rebuild's lanes take their slots and not on what the log holds"""
    ia, ib = a.info(), b.info()
    assert ia[1] == ib[1] and ia[3] == ib[3] and ia[6] == 0 and ib[6] == 0
    assert a.retire_info()[1:4] == b.retire_info()[1:4]
    assert tr.records(a) == tr.records(b)


def clean(relay, log):
    """the residue counters: nothing of a step stays in the relay's or the log's result buffers"""
    assert relay.info()["residue_words"] == 0 and log.info()[6] == 0


SIZES = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (8, 8193), (1, 257)]


@pytest.mark.parametrize("lanes,n", SIZES)
def test_a_step_with_a_window_equals_the_composition(prover, generated, base, lanes, n):
    """one chunk, a lane per proof, and two team chunks (the window holds across chunks), each under windows of 1, 33
    and 64 elements whose matching ones come last"""
    from zerokit_amd.batch import Relay
    roots = b"".join(base["roots"])
    proofs, values, xs = tr.tile(base, n, n % 7)
    tags = [1000 + i for i in range(n)]
    for k in ((1, 33, 64) if n <= 257 else (33,)):   # (the logs are compared record by record: one window at 8 193)
        window = window_of(k)
        logs = tr.twin_logs(max(n, 16), generated["seed"])
        relay = Relay(prover, logs[0], None, lanes)
        try:
            # {EB} alone sweeps the hand-made record under EA, and then row 7 is NEW, not FOREIGN
            assert relay.set_epochs(window) == logs[1].retain(window) == (1 if k == 1 else 0) and relay.epochs() == window
            got = tr.relay_step(relay, n, proofs, values, 5, xs=xs, roots=roots, tags=tags)
            want = compose(prover, logs[1], lanes, n, proofs, values, 5, 1, xs, roots, tags, window)
            assert got == want
            same_logs(*logs)
            info = relay.info()
            assert info["bad_epoch"] == got[0].count(BAD_EPOCH) and info["accepted"] == got[0].count(OK)
            assert info["shares"] == logs[0].info()[1] - (0 if k == 1 else 1)
            clean(relay, logs[0])
            assert logs[0].retain(window) == 0               # everything the relay recorded lies in the window
            if n >= 257:
                assert set(got[0]) == {OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_EPOCH}
                assert set(got[1]) == ({NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED} if k > 1 else {NEW, DUPLICATE, SPAM, SKIPPED})
        finally:
            relay.close()
            for log in logs:
                log.close()


def test_without_a_window_the_step_is_what_it_was(prover, hasher, generated, base):
    """byte for byte the step of tests/test_gpu_relay.py's composition, and info[7] stays 0; so it is again after
    set_epochs([])"""
    from zerokit_amd.batch import Relay
    n = 257
    roots = b"".join(base["roots"])
    proofs, values, xs = tr.tile(base, n, 5)
    for switch_off in (False, True):
        logs = tr.twin_logs(n, generated["seed"])
        relay = Relay(prover, logs[0], None, 0)
        try:
            if switch_off:
                assert relay.set_epochs([EA]) == 0 and relay.set_epochs([]) == 0
            assert relay.epochs() == []
            got = tr.both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, xs=xs, roots=roots)
            same_logs(*logs)
            assert BAD_EPOCH not in got[0] and relay.info()["bad_epoch"] == 0
            clean(relay, logs[0])
        finally:
            relay.close()
            for log in logs:
                log.close()


def test_the_multi_message_id_circuit():
    from zerokit_amd.batch import BatchProver, Relay
    p = BatchProver(depth=20, multi=True, max_batch=64, window_bits=8)
    try:
        nv, k = p.num_public, 4
        sig = SIGNALS
        named = [tr._multi(0, [1, 2, 3, 4], [1, 0, 0, 0], sig[0], EA),    # NEW
                 tr._multi(0, [5, 6, 1, 7], [1, 0, 1, 0], sig[1], EA),    # slot 0 NEW, slot 2 SPAM
                 tr._multi(1, [1, 2, 3, 4], [0, 1, 1, 0], sig[3], EC),    # outside the window
                 tr._multi(2, [1, 2, 3, 4], [1, 1, 1, 1], sig[4], EB),    # four NEW
                 tr._multi(1, [9, 3, 8, 2], [0, 1, 1, 0], sig[5], EC)]    # outside the window
        gp, gv = tr._prove_public(p, named)
        rows = [(gp[128 * i:128 * i + 128], gv[32 * nv * i:32 * nv * (i + 1)]) for i in range(len(named))]
        rows.append((rows[3][0], rows[3][1][:32 * 11] + le(2) + rows[3][1][32 * 12:]))   # a selector of 2: a bad proof
        rows = [rows[i % len(rows)] for i in range(65)]
        n, proofs, values = len(rows), b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
        xs = b"".join(le(77) if i % 13 == 12 else r[1][32 * 9:32 * 10] for i, r in enumerate(rows))
        window = window_of(33)
        logs = tr.twin_logs(8 * n, le(1) + le(2) + le(3) + le(EA))
        relay = Relay(p, logs[0], None, 0)
        try:
            relay.set_epochs(window)
            got = tr.relay_step(relay, n, proofs, values, nv, xs=xs)
            assert got == compose(p, logs[1], 0, n, proofs, values, nv, k, xs, b"", None, window)
            same_logs(*logs)
            assert list(got[0][:6]) == [OK, OK, BAD_EPOCH, OK, BAD_EPOCH, BAD_PROOF] and BAD_SIGNAL in got[0]
            assert list(got[1][:6]) == [NEW, SPAM, SKIPPED, NEW, SKIPPED, SKIPPED]
            assert relay.info()["bad_epoch"] == got[0].count(BAD_EPOCH)
            clean(relay, logs[0])
        finally:
            relay.close()
            for log in logs:
                log.close()
    finally:
        p.close()


@pytest.mark.parametrize("lanes,n,teams,valid_only", [(1, 257, False, True), (1, 257, False, False), (0, 65, True, True),
                                                      (0, 65, True, False)])
def test_the_combined_relay_equals_the_exact_one_under_the_same_window(prover, generated, base, lanes, n, teams, valid_only):
    """valid_only: every proof is valid, so the combined check accepts the chunk and the gate reads reject flags;
    otherwise the chunk holds bad proofs and runs the exact kernels behind the rejected combined check"""
    from zerokit_amd.batch import Relay
    prover.verify_set_cooldown(0)
    try:
        if valid_only:
            g = generated["rows"]
            rows = [g[(3 * i + i // 8) % len(g)] for i in range(n)]
            proofs, values = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
            xs = b"".join(le(5) if i % 10 == 9 else r[1][96:128] for i, r in enumerate(rows))
            roots = b""
        else:
            proofs, values, xs = tr.tile(base, n, base["n"] - 30)   # the generated rows lie at the end of the tile
            roots = b"".join(base["roots"])
        window = window_of(64)
        logs = tr.twin_logs(n, generated["seed"])
        opt = Relay(prover, logs[0], None, lanes, optimistic=True, team_checks=teams)
        exact = Relay(prover, logs[1], None, lanes)
        try:
            s0 = prover.verify_optimistic_stats()
            for r in (opt, exact):
                assert r.set_epochs(window) == 0
            got = tr.relay_step(opt, n, proofs, values, 5, xs=xs, roots=roots)
            s1 = prover.verify_optimistic_stats()
            want = tr.relay_step(exact, n, proofs, values, 5, xs=xs, roots=roots)
            assert got == want
            same_logs(*logs)
            assert s1["combined"] - s0["combined"] == 1
            if valid_only:
                assert s1["accepted"] - s0["accepted"] == 1
            assert {OK, BAD_SIGNAL, BAD_EPOCH} <= set(got[0]) and {NEW, SPAM, DUPLICATE, SKIPPED} <= set(got[1])
            assert opt.info()["bad_epoch"] == exact.info()["bad_epoch"] == got[0].count(BAD_EPOCH)
            clean(opt, logs[0])
            clean(exact, logs[1])
        finally:
            opt.close()
            exact.close()
            for log in logs:
                log.close()
    finally:
        prover.verify_set_cooldown(0)
        prover.verify_set_cooldown(16)


def _rows(generated, order):
    rows = [generated["rows"][i] for i in order]
    return len(rows), b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[1][96:128] for r in rows)


def test_set_epochs_sweeps_the_log_and_closes_the_late_share_hole(prover, generated):
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import Relay
    logs = tr.twin_logs(64, generated["seed"])
    relay, plain = Relay(prover, logs[0], None, 0), Relay(prover, logs[1], None, 0)
    try:
        # both logs take everything while no window is set: EA x 3 (+ the seed record), EB x 3, EC x 2
        n, proofs, values, xs = _rows(generated, range(8))
        for r in (relay, plain):
            assert list(tr.relay_step(r, n, proofs, values, 5, xs=xs)[0]) == [OK] * 8
        assert logs[0].info()[1] == 9
        # the window {EB, EC}: what lies outside goes -- the three EA records and the seed record
        assert relay.set_epochs([EB, EC]) == 4 and relay.epochs() == [EB, EC]
        assert logs[0].info()[1] == 5 and logs[0].retire_info()[:2] == [1, 4]
        assert logs[1].retire([EA]) == 4
        same_logs(*logs)
        # moved again: {EC} alone
        assert relay.set_epochs([EC]) == 3 and logs[0].info()[1] == 2 and logs[1].retire([EB]) == 3
        same_logs(*logs)
        # a late share of a dropped epoch: BAD_EPOCH, and the log does not move ...
        late = _rows(generated, [3, 5])          # EB (dropped), EC (a replay in the window)
        held = logs[0].info()[1]
        got = tr.relay_step(relay, late[0], late[1], late[2], 5, xs=late[3])
        assert list(got[0]) == [BAD_EPOCH, OK] and list(got[1]) == [SKIPPED, DUPLICATE]
        assert logs[0].info()[1] == held + 1 and relay.info()["bad_epoch"] == 1
        # ... where the relay without a window takes it as NEW: the record that would never be removed
        got = tr.relay_step(plain, late[0], late[1], late[2], 5, xs=late[3])
        assert list(got[0]) == [OK, OK] and list(got[1]) == [NEW, DUPLICATE]
        # a refused call leaves the window and the log as they were
        before = (relay.epochs(), logs[0].info(), logs[0].retire_info(), tr.records(logs[0]))
        from zerokit_amd._native import check, lib
        for raw, k, text in ((b"".join(le(1) for _ in range(65)), 65, "a window holds at most 64"),
                             (le(EA) + le(vc.R), 2, "external nullifier 1 of the retain is not canonical"),
                             (None, 3, "null pointer for k > 0")):
            with pytest.raises(RLNError, match=text):
                check(lib().rlnamd_relay_set_epochs(relay._h, raw, k, None))
        assert (relay.epochs(), logs[0].info(), logs[0].retire_info(), tr.records(logs[0])) == before
        # k = 0 switches the window off and removes nothing
        assert relay.set_epochs([]) == 0 and relay.epochs() == [] and logs[0].info() == before[1]
        got = tr.relay_step(relay, late[0], late[1], late[2], 5, xs=late[3])
        assert list(got[0]) == [OK, OK] and list(got[1]) == [NEW, DUPLICATE]
        # a direct observe brings a stranger in; the next set_epochs sweeps it
        assert logs[0].observe([(123456, 5, 6, 31337)])[0] == [NEW]
        assert relay.set_epochs([EC, EB]) == 1
        clean(relay, logs[0])
    finally:
        relay.close()
        plain.close()
        for log in logs:
            log.close()


def _ffi_case(make_proofs, secret, n):
    """n messages of one member under EA, EB and EC in turn: message ids rise, every 9th (under EB) repeats an id under
    another x (SPAM), every 14th is a replay, and one signal is not the proof's"""
    from zerokit_amd import hashers
    signals, ids, exts = [], [], []
    for i in range(n):
        signals.append(b"window message %d" % i)
        exts.append((EA, EB, EC)[i % 3])
        ids.append(i // 3 if i % 9 != 7 else (i - 6) // 3)
    xs = [hashers.hash_to_field_le(s) for s in signals]
    proofs = make_proofs(secret, ids, xs, exts)
    for i in range(13, n, 14):
        proofs[i], signals[i] = proofs[i - 3], signals[i - 3]
    sent = list(signals)
    sent[4] = sent[4] + b"?"
    return proofs, sent


def _either_side_of_the_threshold(obj, make_proofs, secret):
    from zerokit_amd.batch import NullifierLog
    proofs, sent = _ffi_case(make_proofs, secret, 65)
    results = []
    for n in (63, 65):           # below and above "relay_gpu_min": 64
        log = NullifierLog(256, SEED)
        try:
            assert log.observe([(11, 12, 13, 4242), (14, 15, 16, EA)], [1, 2])[0] == [NEW, NEW]
            assert obj.relay_set_epochs(log, [EA, EB]) == 1          # before any device relay exists for the pair
            got = obj.relay_step(log, proofs[:n], sent[:n], [], list(range(500, 500 + n)))
            results.append(got)
            v, st = got[0], got[1]
            assert all((v[i] == BAD_EPOCH) == (i % 3 == 2) for i in range(n))     # a replay keeps its epoch
            assert v[4] == BAD_SIGNAL and {OK, BAD_EPOCH, BAD_SIGNAL} == set(v)
            assert {NEW, SPAM, DUPLICATE, SKIPPED} == set(st) and all(st[i] == SKIPPED for i in range(n) if v[i] != OK)
            assert all(s == secret for s, t in zip(got[2], st) if t == SPAM)
            assert log.info()[1] == 1 + sum(1 for x in v if x == OK)
            # the window moves: EA leaves, EC comes; then the same messages again
            gone = obj.relay_set_epochs(log, [EB, EC])
            assert gone == 1 + sum(1 for i in range(n) if v[i] == OK and _ext(proofs[i]) == EA)
            again = obj.relay_step(log, proofs[:n], sent[:n], [], list(range(900, 900 + n)))
            results.append(again)
            assert all(again[0][i] == BAD_EPOCH for i in range(n) if _ext(proofs[i]) == EA and i != 4)
            assert obj.relay_set_epochs(log, []) == 0
            assert BAD_EPOCH not in obj.relay_step(log, proofs[:8], sent[:8], [], None)[0]
        finally:
            log.close()
    # the same messages give the same answers on either side: the first 63 of the larger call are the smaller call
    for small, large in ((results[0], results[2]), (results[1], results[3])):
        assert [list(x[:63]) for x in large[:2]] == [list(x) for x in small[:2]]
        assert list(large[2][:63]) == list(small[2]) and list(large[3][:63]) == list(small[3])


def _ext(proof):
    return proof.values.external_nullifier


def test_ffi_relay_set_epochs_on_either_side_of_relay_gpu_min(tmp_path):
    import json
    from zerokit_amd import hashers
    from zerokit_amd.public import RLN, RLNWitnessInput
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"relay_gpu_min": 64}))
    obj = RLN(20, tree_config=str(cfgp))
    secret = hashers.hash_to_field_le(b"window-member")
    obj.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = obj.get_merkle_proof(3)

    def make(secret, ids, xs, exts):
        ws = [RLNWitnessInput(secret, 100, ids[i], path[0], path[1], xs[i], exts[i]) for i in range(len(ids))]
        out = []
        for o in range(0, len(ws), 32):
            out += obj.generate_rln_proofs_batch(ws[o:o + 32], [(11 + i, 23 + i) for i in range(o, o + len(ws[o:o + 32]))])
        return out

    _either_side_of_the_threshold(obj, make, secret)


def test_ffi_rln_v3_relay_set_epochs_on_either_side_of_relay_gpu_min(tmp_path):
    import json
    from zerokit_amd import hashers
    from zerokit_amd.batch import resource_paths
    from zerokit_amd.public_v3 import RLNV3, RLNWitnessInputV3
    zp, gp = resource_paths(20)
    cfgp = tmp_path / "v3cfg.json"
    cfgp.write_text(json.dumps({"relay_gpu_min": 64}))
    obj = RLNV3.stateful(20, open(zp, "rb").read(), open(gp, "rb").read(), tree="pm", config_path=str(cfgp))
    secret = 777
    obj.set_next_leaf(5)
    obj.set_next_leaf(hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    elems, bits = obj.get_merkle_proof(1)

    def make(secret, ids, xs, exts):
        return [obj.generate_proof(RLNWitnessInputV3.new_single(secret, 100, ids[i], elems, bits, xs[i], exts[i]))
                for i in range(len(ids))]

    _either_side_of_the_threshold(obj, make, secret)
