"""The durable tree store (zerokit_amd/csrc/tree_store.h: checksummed snapshot + write-ahead journal) built for the CPU
and judged by a model: a Python dict of leaves + metadata + next index, advanced by the same operations.  Depth 5 and at
most 40 operations keep the files to a few KB, so EVERY offset of the journal is cut and EVERY byte of journal and
snapshot takes a flipped bit.  The stand-alone programs of tests/host/treestore_main.cpp cover a killed writer and the
sanitizers.  No GPU needed."""
import ctypes
import os
import random
import shutil
import signal
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-pthread", "-I", CSRC]
U64P = ctypes.POINTER(ctypes.c_uint64)
DEPTH = 5
CAP = 1 << DEPTH
WAL_HEADER = 28
SNAP, WAL = "rlnamd_tree.bin", "rlnamd_tree.wal"


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libtreestore.so")
    src = os.path.join(HOST, "treestore.cpp")
    deps = [src, os.path.join(CSRC, "tree_store.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.ts_crc32c.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.ts_crc32c.restype = ctypes.c_uint32
    lib.ts_open.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p,
                            ctypes.c_size_t]
    lib.ts_open.restype = ctypes.c_void_p
    lib.ts_close.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ts_set_range.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
    lib.ts_set_scatter.argtypes = [ctypes.c_void_p, ctypes.c_uint64, U64P, ctypes.c_char_p]
    lib.ts_set_meta.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64]
    lib.ts_sync.argtypes = [ctypes.c_void_p]
    lib.ts_info.argtypes = [ctypes.c_void_p, U64P]
    lib.ts_info.restype = None
    lib.ts_error.argtypes = [ctypes.c_void_p]
    lib.ts_error.restype = ctypes.c_char_p
    lib.ts_next.argtypes = [ctypes.c_void_p]
    lib.ts_next.restype = ctypes.c_uint64
    lib.ts_meta_len.argtypes = [ctypes.c_void_p]
    lib.ts_meta_len.restype = ctypes.c_uint64
    lib.ts_state.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.ts_state.restype = None
    return lib


class StoreRefused(Exception):
    pass


class Tree:
    """one open store; `flusher=False` keeps the tests free of timing"""

    def __init__(self, L, path, depth=DEPTH, flush_every_ms=500, journal_max_bytes=0, flusher=False):
        self.L = L
        err = ctypes.create_string_buffer(512)
        self.h = L.ts_open(str(path).encode(), depth, flush_every_ms, journal_max_bytes, int(flusher), err, len(err))
        if not self.h:
            raise StoreRefused(err.value.decode())

    def close(self, compact=False):
        if self.h:
            rc = self.L.ts_close(self.h, int(compact))
            self.h = None
            assert rc == 0

    def info(self):
        out = (ctypes.c_uint64 * 8)()
        self.L.ts_info(self.h, out)
        return list(out)

    def state(self):
        n, m = self.L.ts_next(self.h), self.L.ts_meta_len(self.h)
        leaves, meta = ctypes.create_string_buffer(max(32 * n, 1)), ctypes.create_string_buffer(max(m, 1))
        self.L.ts_state(self.h, leaves, meta)
        return n, meta.raw[:m], leaves.raw[:32 * n]

    def apply(self, op):
        kind = op[0]
        if kind == "range":
            rc = self.L.ts_set_range(self.h, op[1], len(op[2]), b"".join(op[2]))
        elif kind == "scatter":
            idx = (ctypes.c_uint64 * len(op[1]))(*op[1])
            rc = self.L.ts_set_scatter(self.h, len(op[1]), idx, b"".join(op[2]))
        else:
            rc = self.L.ts_set_meta(self.h, op[1], len(op[1]))
        assert rc == 0, self.L.ts_error(self.h)


class Model:
    def __init__(self):
        self.leaves, self.meta, self.next = {}, b"", 0

    def apply(self, op):
        if op[0] == "range":
            for k, leaf in enumerate(op[2]):
                self.leaves[op[1] + k] = leaf
            self.next = max(self.next, op[1] + len(op[2]))
        elif op[0] == "scatter":
            for i, leaf in zip(op[1], op[2]):
                self.leaves[i] = leaf
                self.next = max(self.next, i + 1)
        else:
            self.meta = op[1]

    def state(self):
        return self.next, self.meta, b"".join(self.leaves.get(i, bytes(32)) for i in range(self.next))


def operations(seed=7, count=40):
    """ranges, single sets, deletes (a zero leaf), one-record atomic operations (removals and insertions together, as a
    range or as scattered leaves) and metadata"""
    rnd = random.Random(seed)
    leaf = lambda: rnd.randrange(1, 1 << 250).to_bytes(32, "little")
    ops = []
    for k in range(count):
        pick = k % 5
        if pick == 0:
            start = rnd.randrange(CAP - 6)
            ops.append(("range", start, [leaf() for _ in range(rnd.randrange(1, 7))]))
        elif pick == 1:
            ops.append(("scatter", [rnd.randrange(CAP)], [leaf()]))
        elif pick == 2:
            ops.append(("scatter", [rnd.randrange(CAP)], [bytes(32)]))
        elif pick == 3:
            idx = sorted(rnd.sample(range(CAP), 4))
            ops.append(("scatter", idx, [bytes(32), bytes(32), leaf(), leaf()]))       # two removals + two insertions
        else:
            ops.append(("meta", bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 20)))))
    return ops


@pytest.fixture(scope="module")
def written(L, tmp_path_factory):
    """a live store's directory after 40 operations, copied from under the open object (what a crash leaves), with the
    journal's end offset and the model's state after each operation"""
    live = tmp_path_factory.mktemp("live") / "store"
    t, m = Tree(L, live), Model()
    ends, states = [t.info()[1]], [m.state()]
    assert ends[0] == WAL_HEADER
    for op in operations():
        t.apply(op)
        m.apply(op)
        ends.append(t.info()[1])
        states.append(m.state())
    assert t.state() == states[-1] and t.info()[2] == 40 and t.info()[0] == 1
    crashed = tmp_path_factory.mktemp("crashed") / "store"
    shutil.copytree(live, crashed)
    t.close()
    assert os.path.getsize(crashed / WAL) == ends[-1] and ends == sorted(set(ends))
    return crashed, ends, states


def variant(written_dir, dst, wal=None, snap=None):
    """a copy of the store with another journal and / or snapshot"""
    if os.path.exists(dst):
        shutil.rmtree(dst)
    shutil.copytree(written_dir, dst)
    for name, data in ((WAL, wal), (SNAP, snap)):
        if data is not None:
            with open(os.path.join(dst, name), "wb") as f:
                f.write(data)
    return dst


def test_crc32c_check_value(L):
    assert L.ts_crc32c(b"123456789", 9) == 0xE3069283
    assert L.ts_crc32c(b"", 0) == 0


def test_torn_writes_at_every_offset(L, written, tmp_path):
    src, ends, states = written
    wal = open(src / WAL, "rb").read()
    for cut in range(WAL_HEADER, len(wal) + 1):
        d = variant(src, tmp_path / "cut", wal=wal[:cut])
        kept = max(k for k, e in enumerate(ends) if e <= cut)
        t = Tree(L, d)
        info = t.info()
        assert t.state() == states[kept], cut
        assert info[5] == kept and info[6] == cut - ends[kept] and info[1] == ends[kept], (cut, info)
        t.close()
        t = Tree(L, d)                      # the tail was cut off for good
        assert t.info()[6] == 0 and t.info()[5] == kept and t.state() == states[kept], cut
        t.close()


def test_bit_flips_in_the_journal_yield_a_prefix(L, written, tmp_path):
    src, ends, states = written
    wal = bytearray(open(src / WAL, "rb").read())
    rnd = random.Random(3)
    for at in range(len(wal)):
        bad = bytearray(wal)
        bad[at] ^= 1 << rnd.randrange(8)
        t = Tree(L, variant(src, tmp_path / "flip", wal=bytes(bad)))
        got, info = t.state(), t.info()
        # the records before the damaged one, and nothing else
        whole = 0 if at < WAL_HEADER else max(k for k, e in enumerate(ends) if e <= at)
        assert got == states[whole] and info[5] == whole and info[6] > 0, at
        t.close()


def test_bit_flips_in_the_snapshot_are_refused(L, written, tmp_path):
    src, ends, states = written
    d = variant(src, tmp_path / "compacted")
    t = Tree(L, d)
    t.close(compact=True)                    # a T2 snapshot with metadata and leaves
    snap = open(d / SNAP, "rb").read()
    assert snap[:8] == b"RLNAMDT2" and len(snap) == 72 + len(states[-1][1]) + 32 * states[-1][0] + 4
    wal = open(d / WAL, "rb").read()
    rnd = random.Random(4)
    for at in range(len(snap)):
        bad = bytearray(snap)
        bad[at] ^= 1 << rnd.randrange(8)
        with pytest.raises(StoreRefused, match="corrupt"):
            Tree(L, variant(d, tmp_path / "flip", snap=bytes(bad)))
        assert open(tmp_path / "flip" / WAL, "rb").read() == wal       # a refused open leaves the store as it was
    # a snapshot that is whole but not the tree its root was taken from: a leaf changed under a fresh checksum
    bad = bytearray(snap)
    bad[-5] ^= 0x10
    bad[-4:] = struct.pack("<I", L.ts_crc32c(bytes(bad[:-4]), len(bad) - 4))
    with pytest.raises(StoreRefused, match=r"corrupt \(root\)"):
        Tree(L, variant(d, tmp_path / "flip", snap=bytes(bad)))
    t = Tree(L, d)
    assert t.state() == states[-1] and t.info()[5] == 0
    t.close()


def test_stale_journal_leftover_tmp_and_old_snapshot_form(L, written, tmp_path):
    src, ends, states = written
    # a crash between the two renames of a compaction: the new snapshot beside the journal of the generation before
    d = variant(src, tmp_path / "stale")
    old_wal = open(d / WAL, "rb").read()
    t = Tree(L, d)
    t.close(compact=True)
    assert open(d / WAL, "rb").read() != old_wal
    d = variant(d, tmp_path / "stale2", wal=old_wal)
    (d / (SNAP + ".tmp")).write_bytes(b"half a snapshot")
    (d / (WAL + ".tmp")).write_bytes(b"")
    t = Tree(L, d)
    info = t.info()
    assert t.state() == states[-1] and info[0] == 2 and info[5] == 0 and info[6] == 0 and info[1] == WAL_HEADER
    assert not (d / (SNAP + ".tmp")).exists() and not (d / (WAL + ".tmp")).exists()
    t.close()
    # RLNAMDT1, built by hand: magic | depth | next | meta_len | meta | leaves
    n, meta, leaves = states[17]
    d = tmp_path / "t1"
    d.mkdir()
    (d / SNAP).write_bytes(b"RLNAMDT1" + struct.pack("<QQQ", DEPTH, n, len(meta)) + meta + leaves)
    t = Tree(L, d)
    assert t.state() == states[17] and t.info()[0] == 0
    t.apply(("scatter", [3], [b"\x07" * 32]))
    assert open(d / SNAP, "rb").read(8) == b"RLNAMDT1"
    t.close(compact=True)
    assert open(d / SNAP, "rb").read(8) == b"RLNAMDT2"
    t = Tree(L, d)
    got = t.state()
    assert t.info()[0] == 1 and got[2][96:128] == b"\x07" * 32 and got[:2] == (max(n, 4), meta)
    t.close()
    with pytest.raises(StoreRefused, match="Tree depth"):
        Tree(L, d, depth=DEPTH + 1)
    (d / SNAP).write_bytes(b"RLNAMDT1" + struct.pack("<QQQ", DEPTH, n + 1, len(meta)) + meta + leaves)   # short
    with pytest.raises(StoreRefused, match="corrupt"):
        Tree(L, d)


def test_an_atomic_record_cut_in_half_shows_nothing_of_itself(L, written, tmp_path):
    src, ends, states = written
    ops = operations()
    k = next(i for i, op in enumerate(ops) if op[0] == "scatter" and len(op[1]) == 4 and i > 10)
    wal = open(src / WAL, "rb").read()
    t = Tree(L, variant(src, tmp_path / "half", wal=wal[:(ends[k] + ends[k + 1]) // 2]))
    n, _, leaves = t.state()
    assert (n, _, leaves) == states[k]
    before = states[k][2].ljust(32 * CAP, b"\0")
    leaves = leaves.ljust(32 * CAP, b"\0")
    for i in ops[k][1]:                       # neither the removals nor the insertions
        assert leaves[32 * i:32 * i + 32] == before[32 * i:32 * i + 32]
    t.close()


def test_compaction(L, tmp_path):
    d = tmp_path / "store"
    t, m = Tree(L, d, journal_max_bytes=600), Model()
    assert (d / SNAP).exists() and t.info()[:3] == [1, WAL_HEADER, 0]
    gens = [1]
    for op in operations(seed=9):
        before = t.info()
        t.apply(op)
        m.apply(op)
        info = t.info()
        if info[4] > before[4]:
            assert info[0] == before[0] + 1 and info[1] == WAL_HEADER and info[2] == 0
            assert os.path.getsize(d / WAL) == WAL_HEADER and before[1] <= 600
            gens.append(info[0])
        else:
            assert info[1] <= 600 and info[0] == before[0]
        assert t.state() == m.state()
    assert len(gens) > 3 and t.info()[4] == len(gens) - 1
    if t.info()[2] == 0:
        t.apply(("meta", b"last"))
        m.apply(("meta", b"last"))
    gen = t.info()[0]
    t.close(compact=True)                    # as freeing the object does
    assert os.path.getsize(d / WAL) == WAL_HEADER
    t = Tree(L, d)
    assert t.state() == m.state() and t.info()[:3] == [gen + 1, WAL_HEADER, 0] and t.info()[5] == 0
    t.close(compact=True)                    # nothing to compact: the generation stays
    t = Tree(L, d)
    assert t.info()[0] == gen + 1
    t.close()


def test_second_open_is_refused_while_the_first_is_attached(L, tmp_path):
    d = tmp_path / "store"
    t = Tree(L, d, journal_max_bytes=300)
    with pytest.raises(StoreRefused, match="Merkle tree error: store .* is in use"):
        Tree(L, d)
    for op in operations(seed=5, count=15):      # across compactions: the journal's name never leads to an unlocked file
        t.apply(op)
        with pytest.raises(StoreRefused, match="is in use"):
            Tree(L, d)
    assert t.info()[4] > 0
    # another process is refused as well
    code = ("import ctypes,sys; l=ctypes.CDLL(sys.argv[1]); l.ts_open.restype=ctypes.c_void_p; e=ctypes.create_string_buffer(300);"
            "h=l.ts_open(sys.argv[2].encode(),ctypes.c_uint64(5),ctypes.c_uint64(500),ctypes.c_uint64(0),0,e,ctypes.c_size_t(300));"
            "print(bool(h), e.value.decode())")
    import sys
    r = subprocess.run([sys.executable, "-c", code, os.path.join(HOST, "libtreestore.so"), str(d)], capture_output=True,
                       text=True, timeout=60)
    assert r.stdout.startswith("False") and "is in use" in r.stdout, (r.stdout, r.stderr)
    state = t.state()
    t.close()
    t = Tree(L, d)
    assert t.state() == state
    t.close()


def test_sync_accounting_and_the_flusher(L, tmp_path):
    t = Tree(L, tmp_path / "manual")
    t.apply(("scatter", [1], [b"\x01" * 32]))
    info = t.info()
    assert info[7] == info[1] - WAL_HEADER > 0 and info[3] == 0
    assert L.ts_sync(t.h) == 0 and t.info()[7] == 0 and t.info()[3] == 1
    t.close()
    t = Tree(L, tmp_path / "every", flush_every_ms=0)          # every call syncs before it returns
    for k in range(3):
        t.apply(("scatter", [k], [b"\x02" * 32]))
        assert t.info()[7] == 0 and t.info()[3] == k + 1
    t.close()
    t = Tree(L, tmp_path / "timed", flush_every_ms=5, flusher=True)
    t.apply(("meta", b"timed"))
    import time
    deadline = time.monotonic() + 5.0          # a cap, not a measurement
    while t.info()[7] and time.monotonic() < deadline:
        time.sleep(0.002)
    assert t.info()[7] == 0 and t.info()[3] >= 1
    t.close()                                   # joins the thread


def _program(tmp_path, name, sanitize):
    exe = str(tmp_path / name)
    extra = ["-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + extra + FLAGS + [os.path.join(HOST, "treestore_main.cpp"), "-o", exe])
    return exe


def test_killed_writer_keeps_every_acknowledged_operation(L, tmp_path):
    """CPU only.  The child syncs every record before it prints the operation's number; it is killed with SIGKILL after k
    lines and the store must hold at least those k operations and be a prefix of the sequence."""
    exe = _program(tmp_path, "treestore_crash", None)
    d = tmp_path / "store"
    child = subprocess.Popen([exe, "crash", str(d)], stdout=subprocess.PIPE, text=True)
    try:
        k = 0
        for line in child.stdout:
            k = int(line)
            if k >= 150:
                break
    finally:
        child.send_signal(signal.SIGKILL)
        child.wait(timeout=60)
        child.stdout.close()
    assert k == 150 and child.returncode == -signal.SIGKILL
    t = Tree(L, d)
    n, meta, leaves = t.state()
    vals = [int.from_bytes(leaves[32 * i:32 * i + 32], "little") for i in range(n)]
    done = max(vals)
    assert done >= k and n == min(done, 32) and meta == b""
    # operation i wrote i to leaf (i - 1) mod 32: after `done` operations leaf s holds the last i <= done on it
    assert vals == [done - ((done - 1 - s) % 32) for s in range(n)]
    assert t.info()[0] > 1                      # compactions were under way as well
    t.close()


def test_mutated_stores_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (tests/host/treestore_main.cpp) built with the sanitizers: 20 000 mutated journals and snapshots"""
    exe = _program(tmp_path, "treestore_asan", "address,undefined")
    r = subprocess.run([exe, "fuzz", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok fuzz: 20000 mutations"), (r.stdout, r.stderr[-2000:])


def test_flusher_appender_and_syncer_under_tsan(tmp_path):
    """the same program built with -fsanitize=thread: the flusher at 1 ms against an appending and a syncing thread"""
    exe = _program(tmp_path, "treestore_tsan", "thread")
    r = subprocess.run([exe, "threads", str(tmp_path / "store")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok threads"), (r.stdout, r.stderr[-2000:])
