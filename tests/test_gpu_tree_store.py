"""The durable store of a persistent tree through the C ABI (zerokit_amd/csrc/tree_store.h behind ffi.cpp's open_tree):
timed syncs, a flush that costs what the update costs, a torn journal tail, a damaged snapshot, a long replay and the
refusal of a second object on one path.  A crash is simulated by copying the store's directory from under a live object;
no process that holds the GPU is killed.  The store's formats and every cut and flipped byte of them are judged on the CPU
in test_tree_store_host.py."""
import json
import os
import random
import shutil
import time

import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SNAP, WAL = "rlnamd_tree.bin", "rlnamd_tree.wal"
WAL_HEADER = 28
GEN, JOURNAL_BYTES, RECORDS, SYNCS, COMPACTIONS, REPLAYED, TORN, UNSYNCED = range(8)


def _open(tmp_path, store, name="cfg.json", **keys):
    """an RLN object on the persistent tree at `store` (the "small" profile: the tree is the subject)"""
    from zerokit_amd.public import RLN
    cfg = tmp_path / name
    cfg.write_text(json.dumps(dict({"profile": "small", "path": str(store), "temporary": False}, **keys)))
    return RLN(20, str(cfg))


def _leaves(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R) for _ in range(n)]


def _wait_synced(r):
    deadline = time.monotonic() + 5.0        # a cap on the poll, not a measurement
    while r.tree_store_info()[UNSYNCED] and time.monotonic() < deadline:
        time.sleep(0.005)
    assert r.tree_store_info()[UNSYNCED] == 0, "the flusher did not sync within 5 s"


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """one live object, stopped before and after its last operation: `crashed` is its directory copied while it lived
    (journal synced by the flusher, nothing compacted), `closed` the directory after the object was freed"""
    tmp = tmp_path_factory.mktemp("stores")
    live = tmp / "live"
    leaves = _leaves(21, 11)
    r = _open(tmp, live, flush_every_ms=50)
    r.set_leaves_from(0, leaves)
    r.delete_leaf(5)
    r.set_metadata(b"block 1234567")
    before = dict(root=r.get_root(), n=r.leaves_set(), info=r.tree_store_info())
    r.set_leaf(40, 77)
    after = dict(root=r.get_root(), n=r.leaves_set(), info=r.tree_store_info())
    _wait_synced(r)
    shutil.copytree(live, tmp / "crashed")
    r.close()
    return dict(tmp=tmp, crashed=tmp / "crashed", closed=live, leaves=leaves, before=before, after=after)


def test_timed_sync_makes_unflushed_updates_durable(tmp_path):
    """flush_every_ms is honoured: four kinds of update and no flush(), the flusher syncs the journal, and a copy of the
    directory taken then opens at the live object's state -- which is the oracle's for the same leaves"""
    from oracle.pyref import rln as o
    leaves = _leaves(11, 11)
    r = _open(tmp_path, tmp_path / "db", flush_every_ms=50)
    assert r.tree_store_info()[:3] == [1, WAL_HEADER, 0]
    r.set_leaves_from(0, leaves)
    r.delete_leaf(5)
    r.set_metadata(b"block 1234567")
    r.set_leaf(67, 77)
    assert r.tree_store_info()[RECORDS] == 4
    _wait_synced(r)
    assert r.tree_store_info()[SYNCS] >= 1
    shutil.copytree(tmp_path / "db", tmp_path / "copy")
    c = _open(tmp_path, tmp_path / "copy", name="copy.json")
    assert c.tree_store_info()[REPLAYED] == 4 and c.tree_store_info()[TORN] == 0
    assert c.get_root() == r.get_root() and c.leaves_set() == r.leaves_set() == 68
    assert c.get_metadata() == r.get_metadata() == b"block 1234567"
    for i in (0, 4, 5, 6, 10, 11, 66, 67):
        assert c.get_leaf(i) == r.get_leaf(i), i
    assert c.get_leaf(5) == 0 and c.get_leaf(4) == leaves[4] and c.get_leaf(67) == 77
    want = o.SparseMerkleTree(20)
    for i, v in enumerate(leaves):
        want.set(i, v)
    want.set(5, 0)
    want.set(67, 77)
    assert c.get_root() == want.root()
    c.close()
    r.close()


def test_flush_is_incremental(tmp_path):
    """a flush after one update leaves the snapshot alone and grows the journal by one small record"""
    db = tmp_path / "db"
    r = _open(tmp_path, db)
    r.set_leaves_from(0, _leaves(12, 1 << 16))
    r.flush()
    snap = os.stat(db / SNAP)
    journal = os.path.getsize(db / WAL)
    r.set_leaf(123, 456)
    r.flush()
    info = r.tree_store_info()
    now = os.stat(db / SNAP)
    assert (now.st_ino, now.st_mtime_ns, now.st_size) == (snap.st_ino, snap.st_mtime_ns, snap.st_size)
    grown = os.path.getsize(db / WAL) - journal
    assert 0 < grown < 256 and info[UNSYNCED] == 0 and info[JOURNAL_BYTES] == journal + grown
    root = r.get_root()
    r.close()
    r = _open(tmp_path, db)
    assert r.get_root() == root and r.leaves_set() == 1 << 16 and r.get_leaf(123) == 456
    r.close()


def test_torn_tail_through_the_ffi(stores):
    """the journal cut inside its last record: the store opens at the state before that operation"""
    d = stores["tmp"] / "torn"
    shutil.copytree(stores["crashed"], d)
    lo, hi = stores["before"]["info"][JOURNAL_BYTES], stores["after"]["info"][JOURNAL_BYTES]
    assert os.path.getsize(d / WAL) == hi > lo
    with open(d / WAL, "r+b") as f:
        f.truncate((lo + hi) // 2)
    r = _open(stores["tmp"], d, name="torn.json")
    info = r.tree_store_info()
    assert info[TORN] == (lo + hi) // 2 - lo > 0 and info[REPLAYED] == stores["before"]["info"][RECORDS] == 3
    assert r.get_root() == stores["before"]["root"] and r.leaves_set() == stores["before"]["n"] == 11
    assert r.get_leaf(40) == 0 and r.get_metadata() == b"block 1234567"
    r.close()
    # the whole copy, for comparison: every operation is there
    d = stores["tmp"] / "whole"
    shutil.copytree(stores["crashed"], d)
    r = _open(stores["tmp"], d, name="whole.json")
    assert r.get_root() == stores["after"]["root"] and r.leaves_set() == 41 and r.tree_store_info()[TORN] == 0
    r.close()


def test_corrupt_snapshot_is_refused(stores):
    """one byte of the snapshot's leaf area flipped: the open fails, and says why"""
    d = stores["tmp"] / "flipped"
    shutil.copytree(stores["closed"], d)
    snap = bytearray(open(d / SNAP, "rb").read())
    assert snap[:8] == b"RLNAMDT2" and len(snap) == 72 + 13 + 41 * 32 + 4       # compacted when the object was freed
    assert os.path.getsize(d / WAL) == WAL_HEADER
    snap[72 + 13 + 32 * 7 + 3] ^= 0x40
    (d / SNAP).write_bytes(bytes(snap))
    with pytest.raises(Exception, match=r"Merkle tree error: .*rlnamd_tree\.bin is corrupt \(checksum\)"):
        _open(stores["tmp"], d, name="flipped.json")


def test_replay_at_length(tmp_path):
    """300 single-leaf calls over 64 indices (repeats, overwrites, deletes) replayed as ONE upload; after a clean close
    nothing is replayed and the stored root is checked against the rebuilt tree"""
    db = tmp_path / "db"
    rnd = random.Random(5)
    r = _open(tmp_path, db)
    model = {}
    for k in range(300):
        i = rnd.randrange(64)
        if k % 3 == 2 and i < r.leaves_set():
            r.delete_leaf(i)
            model[i] = 0
        else:
            model[i] = rnd.randrange(1, R)
            r.set_leaf(i, model[i])
    root, n = r.get_root(), r.leaves_set()
    assert r.tree_store_info()[RECORDS] == 300 and r.tree_store_info()[COMPACTIONS] == 0
    r.flush()
    shutil.copytree(db, tmp_path / "copy")
    c = _open(tmp_path, tmp_path / "copy", name="copy.json")
    assert c.tree_store_info()[REPLAYED] == 300 and c.get_root() == root and c.leaves_set() == n
    assert all(c.get_leaf(i) == v for i, v in model.items())
    c.close()
    r.close()
    r = _open(tmp_path, db)
    info = r.tree_store_info()
    assert info[REPLAYED] == 0 and info[GEN] == 2 and info[JOURNAL_BYTES] == WAL_HEADER
    assert r.get_root() == root and r.leaves_set() == n
    r.close()


def test_second_object_on_one_path_is_refused(tmp_path):
    db = tmp_path / "db"
    first = _open(tmp_path, db)
    first.set_leaf(0, 5)
    with pytest.raises(Exception, match="Merkle tree error: store .* is in use"):
        _open(tmp_path, db, name="second.json")
    first.set_tree(20)                        # detaches the store: the object goes on with a temporary tree
    assert first.tree_store_info() == [0] * 8
    second = _open(tmp_path, db, name="second.json")
    assert second.get_leaf(0) == 5 and second.leaves_set() == 1
    second.close()
    first.close()
