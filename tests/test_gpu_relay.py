"""The relay step on the device (rlnamd_relay_*: zerokit_amd/csrc/relay.hip) against the composition of the existing
calls, which is the yardstick: rlnamd_hasher_hash_to_field, rlnamd_verify_many_gpu_ex and ONE
rlnamd_nullifier_log_observe on a twin log with the same seed.  Verdicts, statuses, secrets and first tags must be
byte-equal, and afterwards the two logs must be equal in info[1], info[3], retire_info and every get(seq).

Rows are the golden depth-20 cases with verify_cases.rejects, plus proofs made in the fixture so that NEW, DUPLICATE,
SPAM (same member, epoch and message id, another x) and FOREIGN all occur (FOREIGN needs the nullifier of a valid proof
under another external nullifier, which no valid proof gives: both logs start with one hand-made record that holds
it), tiled at a shifting offset."""
import ctypes as C

import pytest

import verify_cases as vc
from verify_cases import R, le

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 0xA5, 64
OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL = range(4)
NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED = range(5)
SEED = 0x5EED0001
PATH = [1000 + 17 * t for t in range(20)]
BITS = [t & 1 for t in range(20)]
SECRETS = [111111, 222222, 333333, 444444]
EXT1, EXT2 = 9001, 9002
SIGNALS = [b"", b"a", bytes(range(135)), b"b" * 136, b"c" * 137, bytes(range(256)) * 4]   # 0, 1, 135, 136, 137, 1 024


def _lib():
    from zerokit_amd import lib
    return lib()


def _err():
    from zerokit_amd._native import last_error
    return last_error()


def _x(signal):
    from zerokit_amd import hashers
    return hashers.hash_to_field_le(signal)


def _prove(p, named):
    rs = [(7 + 2 * i, 9 + 2 * i) for i in range(len(named))]
    t, n = p.submit(p.pack_named_inputs(named), p.pack_rs(rs))
    proofs, values, errs = p.collect_raw(t, n)
    assert not any(errs)
    return proofs, values


def _prove_public(p, named):
    """any circuit: the proofs and every public value (collect_raw returns the five of the single-message circuit)"""
    k = p.upload(p.pack_named_inputs(named), [(7 + 2 * i, 9 + 2 * i) for i in range(len(named))])
    p.run(k)
    out, pub = p.download(k), p.download_public(k)
    assert not any(o["error"] for o in out)
    return b"".join(o["proof"] for o in out), b"".join(le(v) for row in pub for v in row)


def _single(member, msg_id, signal, ext):
    return {"identitySecret": [SECRETS[member]], "userMessageLimit": [100], "messageId": [msg_id], "pathElements": PATH,
            "identityPathIndex": BITS, "x": [_x(signal)], "externalNullifier": [ext]}


def _multi(member, ids, sel, signal, ext):
    w = _single(member, 0, signal, ext)
    w["messageId"], w["selectorUsed"] = list(ids), list(sel)
    return w


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, window_bits=8)
    yield p
    p.close()


@pytest.fixture(scope="module")
def hasher():
    from zerokit_amd.batch import Hasher
    h = Hasher()
    yield h
    h.close()


GEN = [(0, 1, 0, EXT1), (1, 1, 1, EXT1), (0, 1, 2, EXT1), (2, 1, 3, EXT1), (1, 2, 4, EXT1), (2, 1, 5, EXT1), (3, 1, 1, EXT2)]
# in arrival order: NEW, NEW, SPAM (member 0 again, another x), NEW, NEW, SPAM (member 2), FOREIGN (the seeded record)


@pytest.fixture(scope="module")
def generated(prover):
    """the proofs of GEN as rows (proof, values, signal), and the hand-made record both logs start with"""
    proofs, values = _prove(prover, [_single(m, j, SIGNALS[s], e) for m, j, s, e in GEN])
    rows = [(proofs[128 * i:128 * i + 128], values[160 * i:160 * i + 160], SIGNALS[GEN[i][2]]) for i in range(len(GEN))]
    seed_share = rows[6][1][64:96] + le(5) + le(7) + le(EXT1)   # the nullifier of row 6 under the other epoch
    return dict(rows=rows, seed=seed_share)


@pytest.fixture(scope="module")
def base(generated):
    """the tile: every golden depth-20 case with its rejects, then the generated rows, a replay of the first of them, as
    (proofs, values, xs, signals); xs is each row's own x except in every 11th row.  Computed once, never changed."""
    rows, valid = [], []
    for name, proof, pub in vc.golden_h20():
        valid.append(len(rows))
        for _nm, pr, pu in [(name, proof, pub)] + vc.rejects(name, proof, pub):
            rows.append((pr, b"".join((int(v) % (1 << 256)).to_bytes(32, "little") for v in pu), None))
    valid += range(len(rows), len(rows) + len(generated["rows"]))
    rows += generated["rows"] + [generated["rows"][0], generated["rows"][2]]
    xs = [le(12345 + i) if i % 11 == 10 else r[1][96:128] for i, r in enumerate(rows)]
    return dict(n=len(rows), proofs=b"".join(r[0] for r in rows), values=b"".join(r[1] for r in rows), xs=b"".join(xs),
                roots=sorted(set(rows[i][1][32:64] for i in valid[1:])))   # of the valid rows, but for the first golden case


def twin_logs(capacity, seed_share):
    from zerokit_amd.batch import NullifierLog
    a, b = NullifierLog(capacity + 1, SEED), NullifierLog(capacity + 1, SEED)
    for log in (a, b):
        assert log.observe_raw(seed_share, [999])[0] == bytes([NEW])
    return a, b


def relay_step(relay, n, proofs, values, nv, signals=None, offsets=None, xs=None, roots=b"", tags=None):
    """rlnamd_relay_step on raw bytes -> (verdict, status, secrets, first tags); every output buffer is PAD rows longer
    than n, filled with a sentinel, and must be untouched beyond row n - 1.  Raises RLNError with the step's text."""
    from zerokit_amd._native import check
    off = None if offsets is None else (C.c_uint64 * (n + 1))(*offsets)
    tg = None if tags is None else (C.c_uint64 * max(n, 1))(*tags)
    fill = bytes([SENTINEL])
    verdict, status = C.create_string_buffer(fill * (n + PAD)), C.create_string_buffer(fill * (n + PAD))
    secrets = C.create_string_buffer(fill * (32 * (n + PAD)))
    first = (C.c_uint64 * (n + PAD))(*([0xA5A5A5A5A5A5A5A5] * (n + PAD)))
    check(_lib().rlnamd_relay_step(relay._h, n, proofs, values, nv, signals, len(signals) if signals is not None else 0, off, xs,
                                   roots if roots else None, len(roots) // 32, tg, verdict, status, secrets, first))
    assert verdict.raw[n:n + PAD] == fill * PAD and status.raw[n:n + PAD] == fill * PAD
    assert secrets.raw[32 * n:32 * (n + PAD)] == fill * (32 * PAD) and list(first[n:]) == [0xA5A5A5A5A5A5A5A5] * PAD
    return verdict.raw[:n], status.raw[:n], secrets.raw[:32 * n], list(first[:n])


def compose(prover, log, hasher, lanes, n, proofs, values, nv, k, signals=None, offsets=None, xs=None, roots=b"", tags=None):
    """the three existing calls and the host glue between them, over packed rows"""
    from zerokit_amd._native import check
    if xs is None:
        xs = hasher.hash_to_field_raw(signals, offsets)
    ok = C.create_string_buffer(max(n, 1))
    check(_lib().rlnamd_verify_many_gpu_ex(prover._h, n, proofs, values, nv, lanes, ok, None))
    ok = ok.raw
    root_set = set(roots[o:o + 32] for o in range(0, len(roots), 32))
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


def records(log):
    """every get(seq) of the log, an error's text where a record was retired"""
    from zerokit_amd._native import RLNError
    out = []
    for seq in range(log.retire_info()[2]):
        try:
            out.append(log.get(seq))
        except RLNError as e:
            out.append(str(e))
    return out


def logs_equal(a, b):
    ia, ib = a.info(), b.info()
    assert ia[1] == ib[1] and ia[3] == ib[3] and ia[6] == 0 and ib[6] == 0
    assert a.retire_info()[1:5] == b.retire_info()[1:5]
    assert records(a) == records(b)


def tile(base, n, off):
    reps = (off + n) // base["n"] + 1
    cut = lambda b, w: (b * reps)[w * off:w * (off + n)]   # noqa: E731
    return cut(base["proofs"], 128), cut(base["values"], 160), cut(base["xs"], 32)


def both(relay, prover, hasher, lanes, logs, n, proofs, values, nv, k, **kw):
    got = relay_step(relay, n, proofs, values, nv, **kw)
    want = compose(prover, logs[1], hasher, lanes, n, proofs, values, nv, k, **kw)
    assert got == want
    return got


@pytest.mark.parametrize("lanes,sizes", [(0, (0, 1, 63, 64, 65, 257)), (8, (8191, 8192, 8193)), (1, (65537,))])
def test_any_n_equals_the_composition(prover, hasher, generated, base, lanes, sizes):
    """every n on fresh twin logs: one chunk, the team-chunk boundary, two lane-per-proof passes"""
    from zerokit_amd.batch import Relay
    roots = b"".join(base["roots"])   # the root of the first golden case is not in the window
    for n in sizes:
        logs = twin_logs(max(n, 16), generated["seed"])
        relay = Relay(prover, logs[0], None, lanes)
        try:
            proofs, values, xs = tile(base, n, n % 7)
            tags = [1000 + i for i in range(n)]
            v, st, _sec, _ft = both(relay, prover, hasher, lanes, logs, n, proofs, values, 5, 1, xs=xs, roots=roots, tags=tags)
            logs_equal(*logs)
            if n >= 257:
                assert set(v) == {OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL} and set(st) == {NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED}
            info = relay.info()
            chunk = 8192 if (lanes == 8 or (lanes == 0 and n <= 1024)) else 65536
            assert info["messages"] == n and info["chunks"] == -(-n // chunk) and info["accepted"] == v.count(OK)
            assert info["shares"] == logs[0].info()[1] - 1 and info["residue_words"] == 0
        finally:
            relay.close()
            for log in logs:
                log.close()


def _signals_case(generated, order):
    rows = [generated["rows"][i] for i in order]
    signals = b"".join(r[2] for r in rows)
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + len(r[2]))
    return (len(rows), b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), signals, offsets,
            b"".join(r[1][96:128] for r in rows))


def test_signals_give_what_xs_gives(prover, hasher, generated):
    """lengths 0, 1, 135, 136, 137 and 1 024 mixed in arrival order, so that the device's lane order is not the message
    order; one signal is not the proof's; a hasher with lane_max_blocks = 1 sends the long message down the host route"""
    from zerokit_amd.batch import Hasher, Relay
    order = [3, 0, 5, 1, 6, 2, 4, 0, 5, 3, 1]
    n, proofs, values, signals, offsets, xs = _signals_case(generated, order)
    # message 4 of the call brings the signal of another row: its x is not the proof's
    wrong = list(offsets)
    bad_signals = signals[:offsets[4]] + b"zz" + signals[offsets[5]:]
    for j in range(5, n + 1):
        wrong[j] = offsets[j] - (offsets[5] - offsets[4]) + 2
    short = Hasher(lane_max_blocks=1)
    results, host_route = [], []
    try:
        for h, sig, off in ((hasher, signals, offsets), (short, signals, offsets), (hasher, bad_signals, wrong)):
            logs = twin_logs(64, generated["seed"])
            relay = Relay(prover, logs[0], h, 0)
            try:
                got = both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, signals=sig, offsets=off)
                logs_equal(*logs)
                results.append(got)
                # the step's plan is the plan of the composition's hash call with the same hasher
                assert h is short or relay.info()["host_hashed"] == hasher.info()["host_messages"]
                host_route.append(relay.info()["host_hashed"])
            finally:
                relay.close()
                for log in logs:
                    log.close()
        logs = twin_logs(64, generated["seed"])
        relay = Relay(prover, logs[0], None, 0)
        try:
            with_xs = both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, xs=xs)
        finally:
            relay.close()
            for log in logs:
                log.close()
        assert results[0] == with_xs and results[1] == with_xs
        assert host_route[1] > host_route[0] and host_route[1] >= 2   # one block a lane: the two long messages at least
        assert list(with_xs[0]) == [OK] * n
        assert list(with_xs[1]) == [NEW, NEW, SPAM, NEW, FOREIGN, SPAM, NEW, DUPLICATE, SPAM, DUPLICATE, DUPLICATE]
        assert with_xs[2][32 * 5:32 * 6] == le(SECRETS[0])
        assert list(results[2][0]) == [OK] * 4 + [BAD_SIGNAL] + [OK] * 6 and results[2][1][4] == SKIPPED
    finally:
        short.close()


def test_roots_and_the_order_of_the_checks(prover, hasher, generated):
    """no root: any; one; 64; 65 are refused.  Hand-made rows: proof before root before signal, every pair and all three"""
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import Relay
    a, b = generated["rows"][0], generated["rows"][1]   # two valid proofs with different roots
    bad = lambda r: (r[0], le((int.from_bytes(r[1][:32], "little") + 1) % R) + r[1][32:], r[2])   # noqa: E731
    rows = [a, bad(a), b, a, bad(b), b, bad(a), bad(b)]
    xs = [r[1][96:128] for r in rows]
    for i in (3, 5, 6, 7):
        xs[i] = le(4242)
    n, proofs, values, xs = len(rows), b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(xs)
    root_a = a[1][32:64]
    for roots, want in ((b"", [OK, BAD_PROOF, OK, BAD_SIGNAL, BAD_PROOF, BAD_SIGNAL, BAD_PROOF, BAD_PROOF]),
                        (root_a, [OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_PROOF, BAD_ROOT, BAD_PROOF, BAD_PROOF]),
                        (b"".join(le(77 + t) for t in range(63)) + root_a,
                         [OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_PROOF, BAD_ROOT, BAD_PROOF, BAD_PROOF])):
        logs = twin_logs(16, generated["seed"])
        relay = Relay(prover, logs[0], None, 0)
        try:
            got = both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, xs=xs, roots=roots)
            assert list(got[0]) == want
            logs_equal(*logs)
            with pytest.raises(RLNError, match="at most 64 roots"):
                relay_step(relay, n, proofs, values, 5, xs=xs, roots=b"".join(le(t) for t in range(65)))
        finally:
            relay.close()
            for log in logs:
                log.close()


def test_the_multi_message_id_circuit(hasher):
    """the golden case of rln_other_circuits.json with its rejects, and generated proofs with the selector patterns 0000,
    1000, 0110, 1111 and 1010; a SPAM in a higher slot returns that slot's secret.

    A message without a used slot is SKIPPED and leaves no record.  The proof the shipped circuit gives for selector 0000
    is REFUSED by the device verifier (measured on an MI355X: rlnamd_verify_many_gpu_ex gives ok = 0 for it, with the
    patterns 1000, 0110, 1010 and 1111 of the same member accepted), so on the device that row is a bad proof for the
    step and for the composition alike, and "verdict OK, status SKIPPED, no record" for an ACCEPTED proof without a used
    slot is held by the CPU build of the same source (tests/test_relay_host.py, whose verdicts are inputs)."""
    from zerokit_amd.batch import BatchProver, Relay
    p = BatchProver(depth=20, multi=True, max_batch=64, window_bits=8)
    try:
        nv, k = p.num_public, 4
        assert nv == 15
        sig = SIGNALS
        named = [_multi(0, [1, 2, 3, 4], [1, 0, 0, 0], sig[0], EXT1),    # NEW
                 _multi(0, [5, 6, 1, 7], [1, 0, 1, 0], sig[1], EXT1),    # slot 0 NEW, slot 2: id 1 under another x, SPAM
                 _multi(1, [1, 2, 3, 4], [0, 0, 0, 0], sig[2], EXT1),    # no used slot
                 _multi(1, [1, 2, 3, 4], [0, 1, 1, 0], sig[3], EXT1),    # two NEW
                 _multi(2, [1, 2, 3, 4], [1, 1, 1, 1], sig[4], EXT1),    # four NEW
                 _multi(1, [9, 3, 8, 2], [0, 1, 1, 0], sig[5], EXT1)]    # slot 1: id 3 SPAM, slot 2: id 8 NEW
        gp, gv = _prove_public(p, named)
        rows = [(gp[128 * i:128 * i + 128], gv[32 * nv * i:32 * nv * (i + 1)]) for i in range(len(named))]
        rows.append(rows[0])                                             # DUPLICATE
        two = le(2)
        rows.append((rows[4][0], rows[4][1][:32 * 11] + two + rows[4][1][32 * 12:]))   # a selector of 2: a bad proof
        for name, d, m, pr, pu in vc.golden_other():
            if (d, m) == (20, True):
                for _nm, rp, ru in [(name, pr, pu)] + vc.rejects(name, pr, pu):
                    rows.append((rp, b"".join((int(v) % (1 << 256)).to_bytes(32, "little") for v in ru)))
        n, proofs, values = len(rows), b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
        xs = b"".join(r[1][32 * 9:32 * 10] for r in rows)
        for lanes in (0, 1):
            for cut in (n, 3):   # one call, and calls of 3
                logs = twin_logs(8 * n, le(1) + le(2) + le(3) + le(4))
                relay = Relay(p, logs[0], None, lanes)
                try:
                    got = ([], [], [], [])
                    for o in range(0, n, cut):
                        c = min(cut, n - o)
                        part = both(relay, p, hasher, lanes, logs, c, proofs[128 * o:128 * (o + c)],
                                    values[32 * nv * o:32 * nv * (o + c)], nv, k, xs=xs[32 * o:32 * (o + c)])
                        got = tuple(x + (list(y) if not isinstance(y, list) else y) for x, y in zip(got, part))
                    logs_equal(*logs)
                    assert got[0][:8] == [OK, OK, BAD_PROOF, OK, OK, OK, OK, BAD_PROOF]   # selector 0000: refused, see above
                    assert got[1][:8] == [NEW, SPAM, SKIPPED, NEW, NEW, SPAM, DUPLICATE, SKIPPED]
                    sec = bytes(got[2])
                    assert sec[32:64] == le(SECRETS[0]) and sec[32 * 5:32 * 6] == le(SECRETS[1]) and sec[64:96] == bytes(32)
                    assert got[0][8] == OK and got[0][9:].count(OK) == 0   # the golden case is accepted, its rejects are not
                    golden_slots = sum(1 for t in range(4) if rows[8][1][32 * (11 + t):32 * (12 + t)] == le(1))
                    assert logs[0].info()[1] == 1 + 1 + 2 + 0 + 2 + 4 + 2 + 1 + golden_slots   # the seed record, every used slot
                finally:
                    relay.close()
                    for log in logs:
                        log.close()
    finally:
        p.close()


def test_a_log_that_has_retired_an_epoch(prover, hasher, generated, base):
    """once rows and sequence numbers have parted the step writes the sequence numbers too: a step after a retire equals
    the composition, default tags included, and retire_info is equal"""
    from zerokit_amd.batch import Relay
    logs = twin_logs(1024, generated["seed"])
    relay = Relay(prover, logs[0], None, 0)
    try:
        for step_no, n in enumerate((150, 130)):
            proofs, values, xs = tile(base, n, 3 + step_no)
            both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, xs=xs)
            logs_equal(*logs)
            if step_no == 0:
                gone = [log.retire([EXT1]) for log in logs]
                assert gone[0] == gone[1] and gone[0] > 0
                assert logs[0].retire_info() == logs[1].retire_info()
        assert logs[0].retire_info() == logs[1].retire_info() and logs[0].retire_info()[1] > 0
        assert any(isinstance(r, str) for r in records(logs[0]))
    finally:
        relay.close()
        for log in logs:
            log.close()


def test_every_refusal_leaves_the_log_as_it_was(prover, hasher, generated, base):
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import NullifierLog, Relay
    n, proofs, values, signals, offsets, xs = _signals_case(generated, [0, 1, 2, 3])
    logs = twin_logs(16, generated["seed"])
    with_hasher, without = Relay(prover, logs[0], hasher, 0), Relay(prover, logs[0], None, 0)
    small = NullifierLog(3, SEED)
    tight = Relay(prover, small, None, 0)
    try:
        both(with_hasher, prover, hasher, 0, logs, 2, proofs[:256], values[:320], 5, 1, signals=signals[:offsets[2]],
             offsets=offsets[:3])
        before = (logs[0].info(), logs[0].retire_info(), records(logs[0]), hasher.info()["calls"], prover.verify_gpu_passes())
        down = [0, 5, 3, 6, 7]
        for relay, kw, text in (
                (with_hasher, dict(xs=None), "neither signals nor xs_le"),
                (with_hasher, dict(xs=xs, signals=signals, offsets=offsets), "both signals and xs_le"),
                (without, dict(signals=signals, offsets=offsets), "made without a hasher"),
                (with_hasher, dict(signals=signals, offsets=down), "offsets decrease"),
                (with_hasher, dict(signals=signals[:-1], offsets=offsets), "the last offset lies beyond data_len"),
                (with_hasher, dict(xs=xs, nv=4), "n_values is not the key's"),
                (with_hasher, dict(xs=xs, roots=bytes(32 * 65)), "at most 64 roots")):
            nv = kw.pop("nv", 5)
            with pytest.raises(RLNError, match=text):
                relay_step(relay, n, proofs, values[:32 * nv * n], nv, **kw)
        null = (C.c_uint64 * 1)()
        assert _lib().rlnamd_relay_step(with_hasher._h, n, None, values, 5, None, 0, None, xs, None, 0, None, proofs, proofs,
                                        None, null) != 0 and "null pointer for n > 0" in _err()
        with pytest.raises(RLNError, match="4 messages of up to 1 shares do not fit: 3 of 3 records are left"):
            relay_step(tight, n, proofs, values, 5, xs=xs)
        assert small.info()[1] == 0
        assert (logs[0].info(), logs[0].retire_info(), records(logs[0]), hasher.info()["calls"], prover.verify_gpu_passes()) == before
        # n = 0 succeeds and writes nothing; the next steps work, on the tight log too
        assert relay_step(with_hasher, 0, b"", b"", 5, xs=b"") == (b"", b"", b"", [])
        both(with_hasher, prover, hasher, 0, logs, n, proofs, values, 5, 1, signals=signals, offsets=offsets)
        logs_equal(*logs)
        assert list(relay_step(tight, 3, proofs[:384], values[:480], 5, xs=xs[:96])[1]) == [NEW, NEW, SPAM]
    finally:
        for r in (with_hasher, without, tight):
            r.close()
        small.close()
        for log in logs:
            log.close()


def test_nothing_of_a_secret_stays_behind(prover, hasher, generated):
    """after a step with SPAM results the relay's device and pinned buffers hold no non-zero word, nor do the log's"""
    from zerokit_amd.batch import Relay
    n, proofs, values, signals, offsets, _xs = _signals_case(generated, [0, 2, 3, 5, 1])
    logs = twin_logs(16, generated["seed"])
    relay = Relay(prover, logs[0], hasher, 0)
    try:
        got = both(relay, prover, hasher, 0, logs, n, proofs, values, 5, 1, signals=signals, offsets=offsets, tags=[5, 6, 7, 8, 9])
        assert list(got[1]) == [NEW, SPAM, NEW, SPAM, NEW]
        assert got[2][32:64] == le(SECRETS[0]) and got[2][96:128] == le(SECRETS[2]) and got[3] == [5, 5, 7, 7, 9]
        info = relay.info()
        assert info["residue_words"] == 0 and info["steps"] == 1 and info["shares"] == 5 and info["reserved"] == 0
        assert logs[0].info()[6] == 0 and logs[0].info()[4] == 2   # the seeding observe, and one chunk that recorded
    finally:
        relay.close()
        for log in logs:
            log.close()


def test_the_drop_in_entries_equal_the_existing_calls(tmp_path, generated):
    """ffi_relay_step == ffi_verify_rln_signals_batch + ffi_nullifier_log_observe(take = ok): on the device ("relay_gpu_min":
    1) and as the composition (the default at this n), with roots = NULL (the object's current root), a window and an
    empty window; verdict[i] == 0 exactly where ok[i]; one signal has a flipped byte, one member signals twice under one
    message id.  (ffi_rln_v3_relay_step: the next test.)"""
    import json
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.batch import NullifierLog
    from zerokit_amd.public import RLN, RLNWitnessInput, observe_proof_values
    objs = []
    for k, cfg in enumerate(({"relay_gpu_min": 1}, {})):
        cfgp = tmp_path / ("cfg%d.json" % k)
        cfgp.write_text(json.dumps(cfg))
        objs.append(RLN(20, tree_config=str(cfgp)))
    secret = hashers.hash_to_field_le(b"relay-step-member")
    for obj in objs:
        obj.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = objs[0].get_merkle_proof(3)
    signals = [b"relay message %d " % i * (1 + 9 * i) for i in range(8)]
    signals[5] = b""
    xs = [hashers.hash_to_field_le(s) for s in signals]
    ids = [0, 1, 2, 3, 1, 4, 5, 0]   # message ids 1 and 0 twice: SPAM
    ws = [RLNWitnessInput(secret, 100, ids[i], path[0], path[1], xs[i], 4242) for i in range(8)]
    proofs = objs[0].generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(8)])
    proofs.append(proofs[6])              # a replay: DUPLICATE
    signals.append(signals[6])
    root = proofs[0].values.root
    sent = list(signals)
    sent[2] = sent[2][:4] + bytes([sent[2][4] ^ 1]) + sent[2][5:]
    tags = [100 + i for i in range(9)]
    for roots in (None, [12345, root], [], [12345]):
        for obj in objs:
            logs = NullifierLog(64, SEED), NullifierLog(64, SEED)
            try:
                for tg in (tags, None):   # a second step on the same logs, default tags: everything seen before
                    ok = obj.verify_rln_signals_batch(proofs, sent, roots)
                    want = observe_proof_values(logs[1], [p.values for p in proofs], take=ok, tags=tg)
                    verdict, status, secrets, first = obj.relay_step(logs[0], proofs, sent, roots, tg)
                    assert [v == OK for v in verdict] == ok
                    assert (status, secrets, first) == want
                    if roots == [12345]:
                        assert verdict == [BAD_ROOT] * 9
                    elif tg is not None:
                        assert verdict == [OK, OK, BAD_SIGNAL] + [OK] * 6
                        assert status == [NEW, NEW, SKIPPED, NEW, SPAM, NEW, NEW, SPAM, DUPLICATE]
                        assert secrets[4] == secret and secrets[7] == secret and first[8] == 106
                logs_equal(*logs)
            finally:
                for log in logs:
                    log.close()
    log = NullifierLog(8, SEED)
    try:
        assert objs[0].relay_step(log, [], []) == ([], [], [], [])
        with pytest.raises(RLNError, match="9 messages of up to 1 shares do not fit: 8 of 8 records are left"):
            objs[0].relay_step(log, proofs, sent, [])
        assert log.info()[1] == 0
    finally:
        log.close()
    for bad in (-2, 1000000001):
        cfgp = tmp_path / "bad.json"
        cfgp.write_text(json.dumps({"relay_gpu_min": bad}))
        with pytest.raises(RLNError, match="Configuration error: relay_gpu_min"):
            RLN(20, tree_config=str(cfgp))


def _signals_batch(obj_ref, proofs, signals, roots):
    """ffi_verify_rln_signals_batch on raw handles (a V3 object and V3 proofs are the same records) -> list of bools"""
    from zerokit_amd._native import VecU8
    from zerokit_amd.public import _ok_bool, _vec_cfr, _vec_u8
    n = len(proofs)
    hs = (C.c_void_p * n)(*[p._h.value for p in proofs])
    keep = [_vec_u8(s) for s in signals]
    vecs = (VecU8 * n)(*[v if len(s) else VecU8(None, 0, 0) for (v, _k), s in zip(keep, signals)])
    rp = None
    if roots is not None:
        v, _k2 = _vec_cfr(list(roots))
        rp = C.byref(v)
    ok = (C.c_bool * n)()
    _ok_bool(_lib().ffi_verify_rln_signals_batch(obj_ref, hs, n, vecs, rp, ok))
    return [bool(b) for b in ok]


def test_the_v3_entry_equals_the_existing_calls(tmp_path):
    """ffi_rln_v3_relay_step == ffi_verify_rln_signals_batch + ffi_rln_v3_nullifier_log_observe(take = ok) over V3 objects:
    on the device ("relay_gpu_min": 1, a stateful object made with a config file) and as the composition (the default at
    this n), with roots = NULL (the object's current root), a window, an empty window and a window without the root; one
    signal is not the proof's, one member signals twice under one message id, one message is a replay.  Two logs in turn
    on one object: each gets a relay of its own."""
    import json
    from zerokit_amd import hashers
    from zerokit_amd.batch import NullifierLog, resource_paths
    from zerokit_amd.public_v3 import RLNV3, RLNWitnessInputV3, observe_proof_values as observe_v3
    zp, gp = resource_paths(20)
    z, g = open(zp, "rb").read(), open(gp, "rb").read()
    objs = []
    for k, cfg in enumerate(({"relay_gpu_min": 1}, {})):
        cfgp = tmp_path / ("v3cfg%d.json" % k)
        cfgp.write_text(json.dumps(cfg))
        objs.append(RLNV3.stateful(20, z, g, tree="pm", config_path=str(cfgp)))
    secret = 777
    for obj in objs:
        obj.set_next_leaf(5)
        obj.set_next_leaf(hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 10))
    elems, bits = objs[0].get_merkle_proof(1)
    msgs = [b"v3 message %d" % i * (1 + 40 * i) for i in range(5)]
    msgs[3] = b""
    xs = [hashers.hash_to_field_le(s) for s in msgs]
    ids = [0, 1, 2, 0, 3]
    proofs = [objs[0].generate_proof(RLNWitnessInputV3.new_single(secret, 10, ids[i], elems, bits, xs[i], 55)) for i in range(5)]
    proofs.append(proofs[2])
    msgs.append(msgs[2])
    root = objs[0].get_root()
    assert proofs[0].values.root == root == objs[1].get_root()
    sent = list(msgs)
    sent[1] = sent[1] + b"!"
    tags = [7, 8, 9, 10, 11, 12]
    for obj in objs:
        for roots in (None, [12345, root], [], [12345]):
            logs = NullifierLog(32, SEED), NullifierLog(32, SEED)
            try:
                for tg in (tags, None):   # a second step on the same logs, default tags: everything seen before
                    ok = _signals_batch(obj._ref(), proofs, sent, roots)
                    want = observe_v3(logs[1], [p.values for p in proofs], take=ok, tags=tg)
                    verdict, status, secrets, first = obj.relay_step(logs[0], proofs, sent, roots, tg)
                    assert [v == OK for v in verdict] == ok
                    assert (status, secrets, first) == want
                    if roots == [12345]:
                        assert verdict == [BAD_ROOT] * 6
                    elif tg is not None:
                        assert verdict == [OK, BAD_SIGNAL, OK, OK, OK, OK]
                        assert status == [NEW, SKIPPED, NEW, SPAM, NEW, DUPLICATE]
                        assert secrets[3] == secret and first[3] == 7 and first[5] == 9
                logs_equal(*logs)
            finally:
                for log in logs:
                    log.close()
