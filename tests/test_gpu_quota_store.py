"""The quota ledger opened on a directory (rlnamd_quota_open, QuotaLedger.open): every draw journalled from the device
before an id of it is returned, and a reopen that restores window and counters.  Judged by the dict models of
tests/quota_cases.py and tests/quota_counts_cases.py; the journal is parsed here, in Python, from the format that
zerokit_amd/csrc/quota_store.h states.  Small ledgers (depth 12 and below) except where a case needs 65 537 distinct
members or the prover's depth-20 tree."""
import os
import random
import shutil
import stat
import struct

import pytest

import quota_cases as cases
import quota_counts_cases as cc
from quota_cases import E1, E2, E3, E4, OUTSIDE, NO_EPOCH, OK, OVER, U32

pytestmark = pytest.mark.gpu

DEPTH = 12
SNAP, WAL = "rlnamd_quota.bin", "rlnamd_quota.wal"
WAL_HEADER = 36
# set_epochs([E1, E2, E3]) on a fresh ledger: new external nullifiers take the lowest free slots in the order given
# (quota::next_window), which is what the keys of a journal's advance records are read with below
SLOT = {E1: 0, E2: 1, E3: 2}


def _open(path, depth=DEPTH, max_epochs=4, journal_max_bytes=0, window=(E1, E2, E3)):
    from zerokit_amd.batch import QuotaLedger
    q = QuotaLedger.open(path, depth, max_epochs, journal_max_bytes)
    m = cc.CountsModel(depth, max_epochs)
    if window is not None:
        q.set_epochs(list(window))
        m.set_epochs(list(window))
    return q, m


def _records(path):
    """the journal's records: ("window", [external nullifiers]) and ("advance", {key: used})"""
    b = open(os.path.join(path, WAL), "rb").read()
    at, out = WAL_HEADER, []
    while at < len(b):
        (length,) = struct.unpack_from("<Q", b, at)
        payload = b[at + 8:at + 8 + length]
        at += 12 + length
        (count,) = struct.unpack_from("<Q", payload, 1)
        if payload[0] == 2:
            pairs = list(struct.iter_unpack("<II", payload[9:]))
            assert len(pairs) == count and len({k for k, _ in pairs}) == count       # one pair a key
            out.append(("advance", dict(pairs)))
        else:
            out.append(("window", [int.from_bytes(payload[9 + 32 * j:41 + 32 * j], "little") for j in range(count)]))
    assert at == len(b)
    return out


def _keys(leaves, exts):
    return [(e, leaf) for leaf, e in zip(leaves, exts)]


def test_reopen_equals_continue(tmp_path):
    """fails without the feature: there is no QuotaLedger.open"""
    from zerokit_amd.batch import QuotaLedger
    d = tmp_path / "ledger"
    q, m = _open(d)
    keys = []
    for n in (1, 63, 64, 65, 256, 257):
        for leaves, exts, limits in cases.draw_shapes(n, DEPTH):
            cases.compare_draw(m, q, leaves, exts, limits)
            keys += _keys(leaves, exts)
    leaves, exts, limits, counts = cc.interleaved(65, DEPTH)[0]
    cc.compare_draw_counts(m, q, leaves, exts, limits, counts)
    keys += _keys(leaves, exts)
    assert q.info()["residue"] == 0 and q.store_info()["generation"] == 1
    q.close()                                        # compacts, then closes
    q = QuotaLedger.open(d, DEPTH, 4)
    try:
        info = q.store_info()
        assert info["generation"] == 2 and info["replayed"] == 0 and info["journal_bytes"] == WAL_HEADER
        assert info["restored_pairs"] == sum(1 for v in m.used.values() if v)
        assert q.epochs() == [E1, E2, E3]
        cases.compare_counters(m, q, keys)
        leaves, exts, limits = cases.draw_shapes(65, DEPTH)[2]
        cases.compare_draw(m, q, leaves, exts, limits)                       # the next draw gives the model's ids
        leaves, exts, limits, counts = cc.interleaved(65, DEPTH)[1]
        cc.compare_draw_counts(m, q, leaves, exts, limits, counts)
        cases.compare_counters(m, q, keys + _keys(leaves, exts))
    finally:
        q.close()


def test_durable_at_return_without_a_close(tmp_path):
    """the directory copied from under the open ledger is what a crash at that moment leaves"""
    from zerokit_amd.batch import QuotaLedger
    d = tmp_path / "ledger"
    q, m = _open(d)

    def crashed_copy(k):
        c = tmp_path / ("copy%d" % k)
        shutil.copytree(d, c)
        return QuotaLedger.open(c, DEPTH, 4)

    try:
        keys = []
        calls = cases.draw_shapes(65, DEPTH) + cases.draw_shapes(257, DEPTH)[:2]
        for k, (leaves, exts, limits) in enumerate(calls):
            cases.compare_draw(m, q, leaves, exts, limits)
            keys += _keys(leaves, exts)
            if k % 2 == 0 or k == len(calls) - 1:
                c = crashed_copy(k)
                try:
                    assert c.epochs() == [E1, E2, E3] and c.store_info()["torn_bytes"] == 0
                    cases.compare_counters(m, c, keys)
                finally:
                    c.close()
        leaves, exts, limits, counts = cc.interleaved(64, DEPTH)[0]
        cc.compare_draw_counts(m, q, leaves, exts, limits, counts)
        keys += _keys(leaves, exts)
        q.set_epochs([E1, E3, E4])                   # E2 leaves, E4 comes in
        m.set_epochs([E1, E3, E4])
        keys += [(E4, leaf) for _, leaf in keys[:40]]
        c = crashed_copy(99)
        try:
            assert c.epochs() == [E1, E3, E4]
            got = dict(zip(sorted(set(keys)), c.used([k[1] for k in sorted(set(keys))], [k[0] for k in sorted(set(keys))])))
            assert all(v is None for k, v in got.items() if k[0] == E2)          # gone
            assert all(v == 0 for k, v in got.items() if k[0] == E4)             # a zeroed slot
            assert any(v for k, v in got.items() if k[0] == E1) and any(v for k, v in got.items() if k[0] == E3)
            cases.compare_counters(m, c, keys)                                   # `used` right for every epoch
            leaves, exts, limits = [keys[0][1]] * 3, [E4, E1, E2], [U32] * 3
            cases.compare_draw(m, c, leaves, exts, limits)
        finally:
            c.close()
        assert q.info()["residue"] == 0
    finally:
        q.close()


def _delta_shapes(n, depth):
    last = (1 << depth) - 1
    shapes = [([last] * n, [E2] * n, [U32] * n),                                 # n requests of one member: one pair
              (random.Random(n).sample(range(1 << depth), n), [E1] * n, [5] * n)]   # n distinct members: n pairs
    return shapes + cases.draw_shapes(n, depth)


def _check_delta(d, q, m, call, by_count=False):
    """one draw; the journal's last record holds one pair per key that was granted something, with the model's counter"""
    before, info = dict(m.used), q.store_info()
    if by_count:
        cc.compare_draw_counts(m, q, *call)
    else:
        cases.compare_draw(m, q, *call)
    moved = {k: v for k, v in m.used.items() if before.get(k, 0) != v}
    after = q.store_info()
    if not moved:                                    # nothing granted: no record and no sync
        assert (after["records"], after["syncs"], after["journal_bytes"]) == (info["records"], info["syncs"], info["journal_bytes"])
        return 0
    assert (after["records"], after["syncs"]) == (info["records"] + 1, info["syncs"] + 1)
    assert after["journal_bytes"] == info["journal_bytes"] + 12 + 9 + 8 * len(moved) == os.path.getsize(os.path.join(d, WAL))
    kind, pairs = _records(d)[-1]
    assert kind == "advance" and pairs == {SLOT[e] << 24 | leaf: v for (e, leaf), v in moved.items()}
    return len(moved)


@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_the_delta_is_exactly_the_moved_counters(tmp_path, n):
    d = tmp_path / "ledger"
    q, m = _open(d, journal_max_bytes=1 << 30)
    try:
        shapes = _delta_shapes(n, DEPTH)
        assert _check_delta(d, q, m, shapes[0]) == 1
        assert _check_delta(d, q, m, shapes[1]) == n
        for call in shapes[2:]:
            _check_delta(d, q, m, call)
        members = shapes[1][0]
        assert _check_delta(d, q, m, (members, [E1] * n, [0] * n)) == 0          # all OVER
        assert _check_delta(d, q, m, (members, [OUTSIDE] * n, [U32] * n)) == 0   # all NO_EPOCH
        for call in cc.counts_shapes(n, DEPTH)[:3]:
            _check_delta(d, q, m, call, by_count=True)
        assert _check_delta(d, q, m, (members, [E3] * n, [3] * n, [4] * n), by_count=True) == 0    # all OVER, by count
        assert q.info()["residue"] == 0 and q.store_info()["compactions"] == 0
    finally:
        q.close()


def test_the_delta_at_the_scan_level_edge(tmp_path):
    """65 537 requests: one more level of block sums over the flags, as over the ranks (rlnamd_quota_plan)"""
    from zerokit_amd.batch import QuotaLedger
    n, depth = 65537, 20
    assert QuotaLedger.plan(n, depth)[3] == QuotaLedger.plan(n - 1, depth)[3] + 1
    d = tmp_path / "ledger"
    q, m = _open(d, depth=depth, journal_max_bytes=1 << 30)
    try:
        shapes = _delta_shapes(n, depth)
        assert _check_delta(d, q, m, shapes[0]) == 1
        assert _check_delta(d, q, m, shapes[1]) == n
        _check_delta(d, q, m, shapes[4])
        assert _check_delta(d, q, m, (shapes[1][0], [OUTSIDE] * n, [U32] * n)) == 0
        _check_delta(d, q, m, cc.all_distinct(n, depth), by_count=True)
        assert q.info()["residue"] == 0
    finally:
        q.close()


@pytest.mark.parametrize("depth", [8, 9, 16, 17])
def test_snapshot_kernels_at_their_edges(tmp_path, depth):
    """2^depth counters a slot: one workgroup, two, and either side of the scan's 65 537 edge"""
    from zerokit_amd.batch import QuotaLedger
    last, mid = (1 << depth) - 1, 1 << (depth - 1)
    every = list(range(1 << depth)) if depth <= 9 else None
    patterns = {"zero": [], "leaf 0": [(E1, 0)], "the last leaf": [(E1, last)],
                "two live slots, a dead one between": [(E1, 0), (E1, 5), (E2, 7), (E3, last), (E3, 0), (E3, mid - 1), (E3, mid)]}
    if every:
        patterns["every leaf"] = [(E1, leaf) for leaf in every]
    for name, keys in patterns.items():
        d = tmp_path / name.replace(" ", "_").replace(",", "")
        q, m = _open(d, depth=depth, max_epochs=3)
        try:
            if keys:
                rnd = random.Random(depth)
                call = ([k[1] for k in keys] * 2, [k[0] for k in keys] * 2, [rnd.choice([1, 2, U32]) for _ in keys] * 2)
                cases.compare_draw(m, q, *call)
            q.set_epochs([E1, E3])                   # slot 1 is dead between slots 0 and 2
            m.set_epochs([E1, E3])
            gen = q.store_info()["generation"]
            q.compact()
            info = q.store_info()
            assert info["generation"] == gen + 1 and info["journal_bytes"] == WAL_HEADER == os.path.getsize(d / WAL), name
            snap = open(d / SNAP, "rb").read()
            assert len(snap) == 40 + 2 * 40 + 2 * 8 + 8 * sum(1 for v in m.used.values() if v) + 4, name
        finally:
            q.close()
        q = QuotaLedger.open(d, depth, 3)
        try:
            info = q.store_info()
            assert info["generation"] == gen + 1 and info["replayed"] == 0 and q.epochs() == [E1, E3], name
            assert info["restored_pairs"] == sum(1 for v in m.used.values() if v), name
            probe = keys + [(E1, 1), (E3, 1), (E2, 0), (E1, last - 1), (E3, last)]
            cases.compare_counters(m, q, probe)
            cases.compare_draw(m, q, [0, last, 0], [E1, E3, E3], [U32] * 3)
        finally:
            q.close()


def test_automatic_compaction(tmp_path):
    d = tmp_path / "ledger"
    q, m = _open(d, journal_max_bytes=2000)
    try:
        keys, rose = [], 0
        for k in range(12):
            leaves = random.Random(k).sample(range(1 << DEPTH), 64)              # a record of 12 + 9 + 8 * 64 bytes
            before = q.store_info()
            cases.compare_draw(m, q, leaves, [E1] * 64, [U32] * 64)
            keys += _keys(leaves, [E1] * 64)
            info = q.store_info()
            if info["compactions"] > before["compactions"]:                     # behind the draw that crossed the threshold
                assert before["journal_bytes"] + 533 > 2000 and info["journal_bytes"] == WAL_HEADER
                assert info["generation"] == before["generation"] + 1
                rose += 1
            else:
                assert info["journal_bytes"] <= 2000
            cases.compare_counters(m, q, keys[-64:] + keys[:64])
        assert rose >= 2 and q.info()["residue"] == 0
        cases.compare_counters(m, q, keys)
    finally:
        q.close()


def test_refusals_each_with_its_own_text(tmp_path):
    from zerokit_amd.batch import QuotaLedger, RLNError
    d = tmp_path / "ledger"
    q, m = _open(d, journal_max_bytes=1 << 30)
    try:
        with pytest.raises(RLNError, match="is in use by another ledger"):
            QuotaLedger.open(d, DEPTH, 4)
        for k in range(4):
            cases.compare_draw(m, q, [k, k + 1], [E1, E2], [U32, U32])
        broken = tmp_path / "broken"
        shutil.copytree(d, broken)
        assert q.info()["residue"] == 0              # ... behind a failed open too
    finally:
        q.close()
    for name in (SNAP, WAL):
        assert stat.S_IMODE(os.stat(d / name).st_mode) == 0o600
    with pytest.raises(RLNError, match="holds a ledger of depth %d and max_epochs 4, not of depth %d" % (DEPTH, DEPTH + 1)):
        QuotaLedger.open(d, DEPTH + 1, 4)
    with pytest.raises(RLNError, match="holds a ledger of depth %d and max_epochs 4, not of depth %d and max_epochs 5" % (DEPTH, DEPTH)):
        QuotaLedger.open(d, DEPTH, 5)
    # a flipped byte in a middle record: records behind it would be dropped, and counters lowered below issued ids
    wal = bytearray(open(broken / WAL, "rb").read())
    second = WAL_HEADER + 12 + 9 + 32 * 3            # behind the window record: the first draw's record
    wal[second + 8 + 9 + 4] ^= 0x01                  # its first pair's counter
    open(broken / WAL, "wb").write(bytes(wal))
    with pytest.raises(RLNError, match="corrupt .*damaged record at offset %d with records behind it" % second):
        QuotaLedger.open(broken, DEPTH, 4)
    assert open(broken / WAL, "rb").read() == bytes(wal)
    q = QuotaLedger.open(d, DEPTH, 4)                # the store that was not damaged still opens
    try:
        cases.compare_counters(m, q, [(E1, k) for k in range(5)] + [(E2, k) for k in range(6)])
    finally:
        q.close()


def test_no_change_without_a_store(tmp_path, monkeypatch):
    from zerokit_amd.batch import QuotaLedger, RLNError
    monkeypatch.chdir(tmp_path)
    q = QuotaLedger(DEPTH, 4)
    try:
        m = cases.Model(DEPTH, 4)
        q.set_epochs([E1, E2, E3])
        m.set_epochs([E1, E2, E3])
        for call in cases.draw_shapes(65, DEPTH):
            cases.compare_draw(m, q, *call)
        assert set(q.store_info().values()) == {0} and q.info()["residue"] == 0
        with pytest.raises(RLNError, match="has no store"):
            q.compact()
    finally:
        q.close()
    assert os.listdir(tmp_path) == []


# ------------------------------------------------------------------------------------------------------ proving
R = cases.R
PROVE_DEPTH = 20
MEMBER_LEAVES = [0, (1 << PROVE_DEPTH) - 1, 6]
MEMBER_LIMITS = [100, 100, 100]
EA = 0xA11CE


@pytest.fixture(scope="module")
def members():
    from oracle.pyref.poseidon import poseidon
    rnd = random.Random(11)
    secrets = [rnd.randrange(1, R) for _ in MEMBER_LEAVES]
    return secrets, [poseidon([poseidon([s]), lim]) for s, lim in zip(secrets, MEMBER_LIMITS)]


@pytest.fixture(scope="module")
def tree(members):
    from zerokit_amd.batch import PoseidonTree
    t = PoseidonTree(PROVE_DEPTH)
    t.set_leaves(list(zip(MEMBER_LEAVES, members[1])))
    yield t
    t.close()


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, window_bits=8)
    yield p
    p.close()


def test_proving_across_a_reopen(tmp_path, prover, tree, members):
    """three proofs from an opened ledger, a reopen, three more for the same members: the ids are the model's, no member
    gets one twice, and every proof verifies"""
    from zerokit_amd.batch import QuotaLedger
    p, d = prover, tmp_path / "ledger"
    q, m = _open(d, depth=PROVE_DEPTH, window=(EA,))
    rnd = random.Random(5)
    ids_of = {leaf: [] for leaf in MEMBER_LEAVES}
    try:
        for call in range(2):
            who = [0, 1, 0] if call == 0 else [0, 1, 1]
            leaves = [MEMBER_LEAVES[w] for w in who]
            ws = [dict(identity_secret=members[0][w], user_message_limit=MEMBER_LIMITS[w], x=rnd.randrange(R), external_nullifier=EA)
                  for w in who]
            rs = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in who]
            syncs = q.store_info()["syncs"]
            results, status = p.prove_members_drawn(tree, q, leaves, ws, rs)
            assert q.store_info()["syncs"] == syncs + 1 and q.info()["residue"] == 0     # a held draw: one sync, wiped at release
            ids, want = m.draw(leaves, [EA] * 3, [w["user_message_limit"] for w in ws])
            assert status == want == [OK] * 3
            ref = p.prove_members_raw(tree, leaves, p.pack_member_inputs([dict(w, message_id=i) for w, i in zip(ws, ids)]), p.pack_rs(rs))
            for i, r in enumerate(results):
                assert r["error"] == 0 and p.verify(r["proof"], r["public_inputs"]), (call, i)
                assert r["proof"] == ref[0][128 * i:128 * i + 128], (call, i)            # proved with the model's id
                ids_of[leaves[i]].append(ids[i])
            if call == 0:
                q.close()
                q = QuotaLedger.open(d, PROVE_DEPTH, 4)
                assert q.epochs() == [EA]
        assert ids_of == {MEMBER_LEAVES[0]: [0, 1, 2], MEMBER_LEAVES[1]: [0, 1, 2], MEMBER_LEAVES[2]: []}
        assert all(len(set(v)) == len(v) for v in ids_of.values())
    finally:
        q.close()


def _listing(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


@pytest.mark.parametrize("where", ["init", "restore"])
def test_a_failed_open_never_writes_a_snapshot(tmp_path, monkeypatch, where):
    """the store opens and holds records, then the device side of the open fails (RLNAMD_QUOTA_OPEN_FAULT: behind the
    allocation, or with the image restored in part): the directory is byte for byte what the crash left, and the next
    open restores everything"""
    from zerokit_amd.batch import QuotaLedger, RLNError
    d, crashed = tmp_path / "ledger", tmp_path / "crashed"
    q, m = _open(d)
    try:
        leaves, exts, limits = cases.draw_shapes(65, DEPTH)[2]
        cases.compare_draw(m, q, leaves, exts, limits)
        cases.compare_draw(m, q, list(range(300)), [E1] * 300, [U32] * 300)
        shutil.copytree(d, crashed)                  # the journal holds records, as after a crash
    finally:
        q.close()
    before = _listing(crashed)
    monkeypatch.setenv("RLNAMD_QUOTA_OPEN_FAULT", where)
    with pytest.raises(RLNError, match="RLNAMD_QUOTA_OPEN_FAULT=" + where):
        QuotaLedger.open(crashed, DEPTH, 4)
    monkeypatch.delenv("RLNAMD_QUOTA_OPEN_FAULT")
    assert _listing(crashed) == before
    q = QuotaLedger.open(crashed, DEPTH, 4)
    try:
        assert q.store_info()["replayed"] == 3 and q.epochs() == [E1, E2, E3]
        cases.compare_counters(m, q, _keys(leaves, exts) + [(E1, k) for k in range(300)])
    finally:
        q.close()


def test_a_failed_append_fails_the_call_and_burns_its_ids(tmp_path, prover, tree, members):
    """the journal may not grow (RLIMIT_FSIZE at its present size): draw, draw_counts and a held draw fail, the caller's
    arrays are untouched, every per-call buffer is wiped, the counters stay advanced, and the ledger goes on"""
    import ctypes as C
    import resource
    import signal
    from zerokit_amd import lib
    from zerokit_amd.batch import QuotaLedger, RLNError
    signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
    d = tmp_path / "ledger"
    q, m = _open(d, depth=PROVE_DEPTH, window=(EA,))
    leaves = [MEMBER_LEAVES[0], MEMBER_LEAVES[1], MEMBER_LEAVES[0]]
    ws = [dict(identity_secret=members[0][w], user_message_limit=100, x=5 + w, external_nullifier=EA) for w in (0, 1, 0)]
    rs = [(11, 12), (13, 14), (15, 16)]
    try:
        cases.compare_draw(m, q, leaves, [EA] * 3, [100] * 3)
        size, info = os.path.getsize(d / WAL), q.store_info()
        ids, status = (C.c_uint32 * 3)(7, 7, 7), C.create_string_buffer(b"\x07\x07\x07", 3)
        idx, ext, lim = (C.c_uint64 * 3)(*leaves), b"".join(EA.to_bytes(32, "little") for _ in range(3)), (C.c_uint32 * 3)(100, 100, 100)
        soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
        resource.setrlimit(resource.RLIMIT_FSIZE, (size + 5, hard))
        try:
            assert lib().rlnamd_quota_draw(q._h, 3, idx, ext, lim, ids, status) != 0
            assert lib().rlnamd_quota_draw_counts(q._h, 3, idx, ext, lim, bytes([2, 1, 2]), ids, status) != 0
            with pytest.raises(RLNError, match="quota ledger: cannot append to"):
                prover.prove_members_drawn(tree, q, leaves, ws, rs)            # a held draw: nothing is staged for proving
            with pytest.raises(RLNError, match="quota ledger: cannot append to"):
                q.set_epochs([EA, E1])
        finally:
            resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
        assert list(ids) == [7, 7, 7] and status.raw == b"\x07\x07\x07"
        assert q.info()["residue"] == 0 and set(prover.residue().values()) == {0}
        after = q.store_info()
        assert os.path.getsize(d / WAL) == size and (after["records"], after["syncs"]) == (info["records"], info["syncs"])
        assert q.epochs() == [EA]
        m.draw(leaves, [EA] * 3, [100] * 3)                                    # burnt: 2 + 1 ids,
        m.draw_counts(leaves, [EA] * 3, [100] * 3, [2, 1, 2])                  # 4 + 1,
        m.draw(leaves, [EA] * 3, [100] * 3)                                    # and 2 + 1 again
        cases.compare_counters(m, q, [(EA, leaf) for leaf in leaves])
        results, st = prover.prove_members_drawn(tree, q, leaves, ws, rs)      # usable, and above everything burnt
        assert st == m.draw(leaves, [EA] * 3, [100] * 3)[1] == [OK] * 3 and all(r["error"] == 0 for r in results)
        assert q.info()["residue"] == 0
    finally:
        q.close()
    q = QuotaLedger.open(d, PROVE_DEPTH, 4)
    try:
        cases.compare_counters(m, q, [(EA, leaf) for leaf in leaves])
    finally:
        q.close()
