"""The durable quota store (zerokit_amd/csrc/quota_store.h: checksummed snapshot + write-ahead journal) built for the CPU,
driven by quota::SeqLedger (tests/host/quotastore.cpp) and judged by the dict models of tests/quota_cases.py and
tests/quota_counts_cases.py.  Depth 5 and about 40 small records keep the files to a few KB, so EVERY offset of the journal
is cut and EVERY byte of journal and snapshot takes a flipped bit.  The rule under test is the one the tree store does not
have: a ledger never goes backwards -- a bad record is cut off only where nothing follows it, and refused otherwise.
The stand-alone programs of tests/host/quotastore_main.cpp cover a killed writer and the sanitizers.  No GPU needed."""
import ctypes
import os
import random
import shutil
import signal
import stat
import struct
import subprocess
import sys

import pytest

import quota_cases as cases
import quota_counts_cases as cc
from quota_cases import E1, E2, E3, E4, OUTSIDE, U32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]
DEPS = [os.path.join(CSRC, h) for h in ("quota_store.h", "tree_store.h", "quota_ledger.h", "relay.h", "nullifier_log.h", "field.h",
                                        "modinv30.h")]
CP = ctypes.c_char_p
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
DEPTH, MAX_EPOCHS = 5, 4
CAP = 1 << DEPTH
WAL_HEADER, REC_FRAME = 36, 12
SNAP, WAL = "rlnamd_quota.bin", "rlnamd_quota.wal"
GENERATION, JOURNAL_BYTES, RECORDS, SYNCS, COMPACTIONS, REPLAYED, TORN, RESTORED = range(8)


def pack(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libquotastore.so")
    src = os.path.join(HOST, "quotastore.cpp")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + DEPS):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.qs_crc32c.argtypes = [CP, ctypes.c_size_t]
    lib.qs_crc32c.restype = ctypes.c_uint32
    lib.qs_open.argtypes = [CP, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, CP, ctypes.c_size_t]
    lib.qs_open.restype = ctypes.c_void_p
    lib.qs_close.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.qs_compact.argtypes = [ctypes.c_void_p]
    lib.qs_error.argtypes = [ctypes.c_void_p]
    lib.qs_error.restype = CP
    lib.qs_set_epochs.argtypes = [ctypes.c_void_p, CP, ctypes.c_size_t]
    lib.qs_draw.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, U32P, CP]
    lib.qs_draw_counts.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64P, CP, U32P, CP, U32P, CP]
    lib.qs_info.argtypes = [ctypes.c_void_p, U64P]
    lib.qs_info.restype = None
    lib.qs_window.argtypes = [ctypes.c_void_p, CP, U32P]
    lib.qs_window.restype = ctypes.c_size_t
    lib.qs_counters.argtypes = [ctypes.c_void_p, U32P, ctypes.c_size_t]
    lib.qs_counters.restype = ctypes.c_size_t
    return lib


class StoreRefused(Exception):
    pass


class Ledger:
    """one open store with the sequential ledger on it, with the methods of zerokit_amd.batch.QuotaLedger"""

    def __init__(self, L, path, depth=DEPTH, max_epochs=MAX_EPOCHS, journal_max_bytes=0):
        self.L, self.depth, self.max_epochs = L, depth, max_epochs
        err = ctypes.create_string_buffer(512)
        self.h = L.qs_open(os.fsencode(str(path)), depth, max_epochs, journal_max_bytes, err, len(err))
        if not self.h:
            raise StoreRefused(err.value.decode())

    def close(self, compact=0):
        if self.h:
            rc = self.L.qs_close(self.h, compact)
            self.h = None
            assert rc == 0

    def _check(self, rc):
        if rc != 0:
            raise cases.Refused(self.L.qs_error(self.h).decode())

    def compact(self):
        self._check(self.L.qs_compact(self.h))

    def info(self):
        out = (ctypes.c_uint64 * 8)()
        self.L.qs_info(self.h, out)
        return list(out)

    def set_epochs(self, exts):
        self._check(self.L.qs_set_epochs(self.h, pack(exts), len(exts)))

    def draw(self, leaves, exts, limits):
        n = len(leaves)
        ids, status = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        self._check(self.L.qs_draw(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0",
                                   (ctypes.c_uint32 * max(n, 1))(*limits), ids, status))
        return list(ids[:n]), list(status.raw[:n])

    def draw_counts(self, leaves, exts, limits, counts):
        n = len(leaves)
        firsts, status = (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1))
        self._check(self.L.qs_draw_counts(self.h, n, (ctypes.c_uint64 * max(n, 1))(*leaves), pack(exts) or b"\0",
                                          (ctypes.c_uint32 * max(n, 1))(*limits), bytes(counts) or b"\0", firsts, status))
        return list(firsts[:n]), list(status.raw[:n])

    def window(self):
        """[(external nullifier, slot)] in the order set_epochs was given"""
        ext, slots = ctypes.create_string_buffer(32 * 64), (ctypes.c_uint32 * 64)()
        k = self.L.qs_window(self.h, ext, slots)
        return [(int.from_bytes(ext.raw[32 * j:32 * j + 32], "little"), int(slots[j])) for j in range(k)]

    def state(self):
        """(the window with its slots, {(external nullifier, leaf): used} of every counter that is not zero)"""
        window = self.window()
        ext_of = {s: e for e, s in window}
        cap = self.max_epochs << self.depth
        out = (ctypes.c_uint32 * (2 * cap))()
        m = self.L.qs_counters(self.h, out, cap)
        return window, {(ext_of[out[2 * i] >> 24], out[2 * i] & 0xFFFFFF): int(out[2 * i + 1]) for i in range(m)}


def model_state(m):
    return list(m.window), {k: v for k, v in m.used.items() if v and k[0] in m.window}


def same(got, want):
    """a Ledger.state() against a model_state(): window order and every counter"""
    return [e for e, _ in got[0]] == want[0] and got[1] == want[1]


def not_below(got, floor):
    """THE NEVER-BACKWARDS RULE: every counter of `floor` (a model_state) whose external nullifier is still in the opened
    window is at or above it there"""
    window = [e for e, _ in got[0]]
    return all(got[1].get(k, 0) >= v for k, v in floor[1].items() if k[0] in window)


def operations(seed=11, count=52):
    """windows and small draws of both kinds; every draw of a few requests over 32 members, so a record is a few dozen
    bytes.  Some draws grant nothing: they append nothing."""
    rnd = random.Random(seed)
    ops = [("window", [E1, E2, E3])]
    limit_of = [rnd.choice([0, 2, 9, U32]) for _ in range(CAP)]
    for k in range(1, count):
        n = rnd.randrange(1, 6)
        leaves = [rnd.randrange(CAP) for _ in range(n)]
        exts = [rnd.choice([E1, E2, E3, E4, OUTSIDE]) for _ in range(n)]
        if k in (15, 30):
            ops.append(("window", [E3, E1, E4] if k == 15 else [E4, E2, E1, E3]))   # E2 leaves (and later comes in anew)
        elif k % 3 == 0:
            ops.append(("counts", leaves, exts, [limit_of[v] for v in leaves], [rnd.choice([1, 2, 3, 4]) for _ in range(n)]))
        elif k % 11 == 0:
            ops.append(("draw", leaves, [OUTSIDE] * n, [limit_of[v] for v in leaves]))   # all NO_EPOCH: no record
        else:
            ops.append(("draw", leaves, exts, [limit_of[v] for v in leaves]))
    return ops


def play(q, m, op):
    if op[0] == "window":
        q.set_epochs(op[1])
        m.set_epochs(op[1])
    elif op[0] == "draw":
        assert q.draw(*op[1:]) == m.draw(*op[1:])
    else:
        assert q.draw_counts(*op[1:]) == m.draw_counts(*op[1:])


@pytest.fixture(scope="module")
def written(L, tmp_path_factory):
    """a live store's directory after the operations, copied from under the open object (what a crash leaves): the
    journal's end offset and the model's state after each RECORD, and the live ledger's slots at the end"""
    live = tmp_path_factory.mktemp("live") / "store"
    q, m = Ledger(L, live), cc.CountsModel(DEPTH, MAX_EPOCHS)
    ends, states = [q.info()[JOURNAL_BYTES]], [model_state(m)]
    assert ends[0] == WAL_HEADER
    silent = 0
    for op in operations():
        before = q.info()
        play(q, m, op)
        info = q.info()
        assert same(q.state(), model_state(m))
        if info[JOURNAL_BYTES] == before[JOURNAL_BYTES]:      # nothing granted: nothing appended, nothing synced
            assert op[0] != "window" and model_state(m) == states[-1] and info[SYNCS] == before[SYNCS]
            silent += 1
            continue
        assert info[SYNCS] == before[SYNCS] + 1 and info[RECORDS] == before[RECORDS] + 1
        ends.append(info[JOURNAL_BYTES])
        states.append(model_state(m))
    assert silent >= 2 and len(ends) >= 38 and q.info()[GENERATION] == 1 and q.info()[COMPACTIONS] == 0
    slots = q.window()
    crashed = tmp_path_factory.mktemp("crashed") / "store"
    shutil.copytree(live, crashed)
    q.close()
    assert os.path.getsize(crashed / WAL) == ends[-1] and ends == sorted(set(ends)) and ends[-1] < 8192
    return crashed, ends, states, slots


def variant(src, dst, wal=None, snap=None):
    """a copy of the store with another journal and / or snapshot"""
    if os.path.exists(dst):
        shutil.rmtree(dst)
    shutil.copytree(src, dst)
    for name, data in ((WAL, wal), (SNAP, snap)):
        if data is not None:
            with open(os.path.join(dst, name), "wb") as f:
                f.write(data)
    return dst


def record(payload, L):
    body = struct.pack("<Q", len(payload)) + payload
    return body + struct.pack("<I", L.qs_crc32c(body, len(body)))


def test_crc32c_check_value(L):
    assert L.qs_crc32c(b"123456789", 9) == 0xE3069283


def test_round_trip_compaction_and_a_stale_journal(L, written, tmp_path):
    src, ends, states, slots = written
    d = variant(src, tmp_path / "a")
    q = Ledger(L, d)                                   # what the crash left: the journal replayed
    info = q.info()
    assert same(q.state(), states[-1]) and q.window() == slots
    assert info[REPLAYED] == len(ends) - 1 and info[TORN] == 0 and info[GENERATION] == 1 and info[RESTORED] == len(states[-1][1])
    old_wal = open(d / WAL, "rb").read()
    q.compact()
    assert q.info()[GENERATION] == 2 and q.info()[JOURNAL_BYTES] == WAL_HEADER == os.path.getsize(d / WAL)
    assert same(q.state(), states[-1])
    q.close(compact=1)                                 # no record in the journal: nothing to compact
    q = Ledger(L, d)
    assert same(q.state(), states[-1]) and q.window() == slots and q.info()[GENERATION] == 2 and q.info()[REPLAYED] == 0
    m = cc.CountsModel(DEPTH, MAX_EPOCHS)              # and it goes on from there as the model does
    m.window, m.used = list(states[-1][0]), dict(states[-1][1])
    play(q, m, ("draw", [3, 3, 7], [E1, E1, E4], [U32] * 3))
    assert same(q.state(), model_state(m))
    q.close(compact=1)                                 # as freeing the ledger does
    assert os.path.getsize(d / WAL) == WAL_HEADER
    after = model_state(m)
    # a crash between the two renames of a compaction: the new snapshot beside the journal of the generation before
    d = variant(d, tmp_path / "stale", wal=old_wal)
    (d / (SNAP + ".tmp")).write_bytes(b"half a snapshot")
    (d / (WAL + ".tmp")).write_bytes(b"")
    q = Ledger(L, d)
    info = q.info()
    assert same(q.state(), after) and info[GENERATION] == 3 and info[REPLAYED] == 0 and info[JOURNAL_BYTES] == WAL_HEADER
    assert not (d / (SNAP + ".tmp")).exists() and not (d / (WAL + ".tmp")).exists()
    q.close()
    for name in (SNAP, WAL):
        assert stat.S_IMODE(os.stat(d / name).st_mode) == 0o600


def test_cut_at_every_offset(L, written, tmp_path):
    src, ends, states, _ = written
    wal = open(src / WAL, "rb").read()
    for cut in range(WAL_HEADER, len(wal) + 1):
        d = variant(src, tmp_path / "cut", wal=wal[:cut])
        kept = max(k for k, e in enumerate(ends) if e <= cut)   # the records that lie wholly below the cut
        q = Ledger(L, d)
        info = q.info()
        assert same(q.state(), states[kept]), cut
        assert info[REPLAYED] == kept and info[TORN] == cut - ends[kept] and info[JOURNAL_BYTES] == ends[kept], (cut, info)
        q.close()
        assert os.path.getsize(d / WAL) == ends[kept]           # the tail was cut off for good
    # the header is synced before the journal takes its name: a short one is damage, and so is an empty file beside
    # any snapshot but the first
    for cut in range(1, WAL_HEADER):
        with pytest.raises(StoreRefused, match="corrupt.*offset 0"):
            Ledger(L, variant(src, tmp_path / "cut", wal=wal[:cut]))
    q = Ledger(L, variant(src, tmp_path / "cut", wal=b""))      # a first open that got no further
    assert same(q.state(), states[0]) and q.info()[GENERATION] == 1
    q.close()
    d = variant(src, tmp_path / "cut")
    q = Ledger(L, d)
    q.close(compact=2)
    with pytest.raises(StoreRefused, match="corrupt.*empty"):
        Ledger(L, variant(d, tmp_path / "cut2", wal=b""))


def test_flipped_at_every_byte_of_the_journal(L, written, tmp_path):
    src, ends, states, _ = written
    wal = open(src / WAL, "rb").read()
    rnd = random.Random(3)
    last = len(ends) - 2                                         # the index of the last record
    opened = 0
    for at in range(len(wal)):
        bad = bytearray(wal)
        bad[at] ^= 1 << rnd.randrange(8)
        d = variant(src, tmp_path / "flip", wal=bytes(bad))
        whole = 0 if at < WAL_HEADER else max(k for k, e in enumerate(ends) if e <= at)   # records wholly before the flip
        if at < ends[last]:                                      # the header, or any record but the last: refused
            with pytest.raises(StoreRefused, match="corrupt.*offset %d" % (0 if at < WAL_HEADER else ends[whole])):
                Ledger(L, d)
            assert open(d / WAL, "rb").read() == bytes(bad)      # a refused open leaves the store as it was
            continue
        q = Ledger(L, d)                                         # the last record: a torn tail, by all the store can know
        got = q.state()
        assert whole == last and same(got, states[last]) and q.info()[REPLAYED] == last and q.info()[TORN] == ends[-1] - ends[last]
        assert not_below(got, states[whole]), at                 # never backwards
        q.close()
        opened += 1
    assert opened == ends[-1] - ends[last]


def test_flipped_at_every_byte_of_the_snapshot(L, written, tmp_path):
    src, ends, states, _ = written
    d = variant(src, tmp_path / "compacted")
    q = Ledger(L, d)
    q.close(compact=1)
    snap = open(d / SNAP, "rb").read()
    window, used = states[-1]
    assert snap[:8] == b"RLNAMDQ1" and len(snap) == 40 + 40 * len(window) + 8 * len(window) + 8 * len(used) + 4
    assert struct.unpack_from("<QQQQ", snap, 8) == (DEPTH, MAX_EPOCHS, 2, len(window))
    wal = open(d / WAL, "rb").read()
    rnd = random.Random(4)
    for at in range(len(snap)):
        bad = bytearray(snap)
        bad[at] ^= 1 << rnd.randrange(8)
        with pytest.raises(StoreRefused, match="corrupt"):
            Ledger(L, variant(d, tmp_path / "flip", snap=bytes(bad)))
        assert open(tmp_path / "flip" / WAL, "rb").read() == wal
    # whole by its checksum, and still not a snapshot this library wrote: a counter of zero, a leaf beyond the depth
    at = 40 + 40 * len(window)
    while struct.unpack_from("<Q", snap, at)[0] == 0:           # the first slot that has a pair
        at += 8
    at += 8
    for edit in (lambda b: b.__setitem__(slice(at + 4, at + 8), bytes(4)), lambda b: b.__setitem__(slice(at, at + 4), b"\xff\0\0\0")):
        bad = bytearray(snap)
        edit(bad)
        bad[-4:] = struct.pack("<I", L.qs_crc32c(bytes(bad[:-4]), len(bad) - 4))
        with pytest.raises(StoreRefused, match="corrupt"):
            Ledger(L, variant(d, tmp_path / "flip", snap=bytes(bad)))
    q = Ledger(L, d)
    assert same(q.state(), states[-1])
    q.close()


def test_an_ill_formed_payload_under_a_good_crc(L, written, tmp_path):
    """what the CRC lets through and this code never wrote: refused where something is behind it, a torn tail at the end"""
    src, ends, states, _ = written
    r = next(k for k, s in enumerate(states) if s[0] == [E3, E1, E4]) + 3        # three of the four slots are live there
    assert states[r][0] == [E3, E1, E4]
    wal, ends, states = open(src / WAL, "rb").read()[:ends[r]], ends[:r + 1], states[:r + 1]
    q = Ledger(L, variant(src, tmp_path / "ill", wal=wal))
    slots = q.window()
    q.close()
    live = {s for _, s in slots}
    dead = next(s for s in range(MAX_EPOCHS) if s not in live)
    a_live = min(live)
    advance = lambda m, pairs: bytes([2]) + struct.pack("<Q", m) + b"".join(struct.pack("<II", k, u) for k, u in pairs)
    payloads = {
        "a dead slot": advance(1, [(dead << 24 | 3, 5)]),
        "a slot beyond max_epochs": advance(1, [(MAX_EPOCHS << 24 | 3, 5)]),
        "a leaf beyond the depth": advance(1, [(a_live << 24 | CAP, 5)]),
        "m above the length": advance(3, [(a_live << 24 | 1, 5), (a_live << 24 | 2, 5)]),
        "m below the length": advance(1, [(a_live << 24 | 1, 5), (a_live << 24 | 2, 5)]),
        "a counter of zero": advance(1, [(a_live << 24 | 1, 0)]),
        "a window above max_epochs": bytes([1]) + struct.pack("<Q", MAX_EPOCHS + 1) + pack(range(1, MAX_EPOCHS + 2)),
        "an element that is no field element": bytes([1]) + struct.pack("<Q", 1) + pack([cases.R]),
        "an unknown kind": bytes([3]) + struct.pack("<Q", 0),
    }
    behind = record(advance(1, [(a_live << 24 | 4, 1000)]), L)
    for name, payload in payloads.items():
        with pytest.raises(StoreRefused, match="corrupt.*ill-formed.*offset %d" % ends[-1]):
            Ledger(L, variant(src, tmp_path / "ill", wal=wal + record(payload, L) + behind))
        with pytest.raises(StoreRefused, match="corrupt.*offset %d" % ends[-1]):       # any byte behind a framed record counts
            Ledger(L, variant(src, tmp_path / "ill", wal=wal + record(payload, L) + b"\x01"))
        q = Ledger(L, variant(src, tmp_path / "ill", wal=wal + record(payload, L)))   # nothing behind it: cut off
        assert same(q.state(), states[-1]) and q.info()[TORN] == len(record(payload, L)), name
        q.close()
    q = Ledger(L, variant(src, tmp_path / "ill", wal=wal + behind))                   # the record behind is a good one
    assert q.state()[1][(dict((s, e) for e, s in slots)[a_live], 4)] == 1000
    q.close()
    # an unsynced append may leave zero bytes where the record was to be: a torn tail
    q = Ledger(L, variant(src, tmp_path / "ill", wal=wal + bytes(100)))
    assert same(q.state(), states[-1]) and q.info()[TORN] == 100
    q.close()


def test_other_shapes_and_a_second_open_are_refused(L, written, tmp_path):
    src, ends, states, _ = written
    d = variant(src, tmp_path / "store")
    with pytest.raises(StoreRefused, match="holds a ledger of depth 5 and max_epochs 4, not of depth 6 and max_epochs 4"):
        Ledger(L, d, depth=DEPTH + 1)
    with pytest.raises(StoreRefused, match="holds a ledger of depth 5 and max_epochs 4, not of depth 5 and max_epochs 3"):
        Ledger(L, d, max_epochs=MAX_EPOCHS - 1)
    (tmp_path / "orphan").mkdir()
    shutil.copy(src / WAL, tmp_path / "orphan" / WAL)
    with pytest.raises(StoreRefused, match="has no snapshot beside it"):
        Ledger(L, tmp_path / "orphan")
    q = Ledger(L, d, journal_max_bytes=300)
    with pytest.raises(StoreRefused, match="store .* is in use by another ledger"):
        Ledger(L, d)
    m = cc.CountsModel(DEPTH, MAX_EPOCHS)
    m.window, m.used = list(states[-1][0]), dict(states[-1][1])
    for k in range(12):                              # across compactions: the journal's name never leads to an unlocked file
        play(q, m, ("draw", [k, k + 1, k], [E1, E4, E1], [U32] * 3))
        with pytest.raises(StoreRefused, match="is in use"):
            Ledger(L, d)
    assert q.info()[COMPACTIONS] > 0 and same(q.state(), model_state(m))
    code = ("import ctypes,sys; l=ctypes.CDLL(sys.argv[1]); l.qs_open.restype=ctypes.c_void_p; e=ctypes.create_string_buffer(300);"
            "h=l.qs_open(sys.argv[2].encode(),ctypes.c_uint64(5),ctypes.c_uint64(4),ctypes.c_uint64(0),e,ctypes.c_size_t(300));"
            "print(bool(h), e.value.decode())")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(HOST, "libquotastore.so"), str(d)], capture_output=True, text=True,
                       timeout=60)
    assert r.stdout.startswith("False") and "is in use" in r.stdout, (r.stdout, r.stderr)
    q.close()
    q = Ledger(L, d)
    assert same(q.state(), model_state(m))
    q.close()


def test_automatic_compaction_keeps_the_state(L, tmp_path):
    d = tmp_path / "store"
    q, m = Ledger(L, d, journal_max_bytes=400), cc.CountsModel(DEPTH, MAX_EPOCHS)
    assert (d / SNAP).exists() and q.info()[:3] == [1, WAL_HEADER, 0]
    crossings = 0
    for op in operations(seed=9):
        before = q.info()
        play(q, m, op)
        info = q.info()
        if info[COMPACTIONS] > before[COMPACTIONS]:   # behind the call that crossed the threshold
            assert info[GENERATION] == before[GENERATION] + 1 and info[JOURNAL_BYTES] == WAL_HEADER and before[JOURNAL_BYTES] <= 400
            crossings += 1
        else:
            assert info[JOURNAL_BYTES] <= 400 and info[GENERATION] == before[GENERATION]
        assert same(q.state(), model_state(m))
    assert crossings >= 2
    q.close()
    q = Ledger(L, d)
    assert same(q.state(), model_state(m)) and q.info()[GENERATION] == 1 + crossings
    q.close()


def _program(tmp_path, name, sanitize):
    exe = str(tmp_path / name)
    extra = ["-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + extra + FLAGS + [os.path.join(HOST, "quotastore_main.cpp"), "-o", exe])
    return exe


def test_killed_writer_keeps_every_acknowledged_draw(L, tmp_path):
    """CPU only.  The child prints a draw's number once the draw has returned -- so behind its record's sync; it is killed
    with SIGKILL after k lines and the reopened ledger must hold at least those k draws and be a prefix of the sequence."""
    exe = _program(tmp_path, "quotastore_crash", None)
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
    q = Ledger(L, d)
    window, used = q.state()
    assert [e for e, _ in window] == [E1]
    done = sum(used.values())                    # draw i (1-based) took one id of member (i - 1) mod 32
    assert done >= k and used == {(E1, s): (done - s + CAP - 1) // CAP for s in range(CAP)}
    assert q.info()[GENERATION] > 1              # compactions were under way as well
    q.close()


def test_the_cases_and_mutated_stores_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (tests/host/quotastore_main.cpp) built with the sanitizers: the round trip, the cut at every
    offset and the flip at every byte again, then seeded mutations of journal and snapshot"""
    exe = _program(tmp_path, "quotastore_asan", "address,undefined")
    r = subprocess.run([exe, "cases", str(tmp_path / "cases")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok cases"), (r.stdout, r.stderr[-2000:])
    r = subprocess.run([exe, "fuzz", str(tmp_path / "fuzz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok fuzz: 8000 mutations"), (r.stdout, r.stderr[-2000:])


def _listing(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def test_an_open_that_is_refused_or_abandoned_leaves_the_directory_as_it_was(L, written, tmp_path):
    src, ends, states, _ = written
    # opened and closed with nothing written in between -- what a ledger does whose device side could not be built: the
    # journal that holds the truth is still there, byte for byte (a failed open never writes a snapshot)
    d = variant(src, tmp_path / "abandoned")
    before = _listing(d)
    q = Ledger(L, d)
    q.close(compact=0)
    assert _listing(d) == before
    # a snapshot of a later generation with no journal beside it: refused, and no journal file is left behind
    q = Ledger(L, d)
    q.close(compact=2)
    os.unlink(d / WAL)
    before = _listing(d)
    with pytest.raises(StoreRefused, match="corrupt.*empty"):
        Ledger(L, d)
    assert _listing(d) == before and list(before) == [SNAP]
    # a directory that holds other files and no store: refused before anything is put into it
    other = tmp_path / "other"
    other.mkdir()
    (other / "notes.txt").write_bytes(b"not a ledger")
    with pytest.raises(StoreRefused, match="is not empty and holds no ledger store"):
        Ledger(L, other)
    assert _listing(other) == {"notes.txt": b"not a ledger"}
    # an empty directory and an absent one are where a store is created
    (tmp_path / "empty").mkdir()
    for d in (tmp_path / "empty", tmp_path / "absent"):
        q = Ledger(L, d)
        assert q.info()[GENERATION] == 1 and sorted(os.listdir(d)) == [SNAP, WAL]
        q.close()


def test_a_failed_append_is_taken_back_and_the_ledger_stays_usable(L, tmp_path):
    """the journal may not grow (RLIMIT_FSIZE at its present size): the append fails, the file is cut back to where it
    was, the call fails with the caller's arrays untouched -- and the counters stay advanced: those ids are burnt"""
    import resource
    signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
    d = tmp_path / "store"
    q, m = Ledger(L, d), cc.CountsModel(DEPTH, MAX_EPOCHS)
    play(q, m, ("window", [E1, E2]))
    play(q, m, ("draw", [1, 2, 1], [E1, E1, E2], [U32] * 3))
    size, info = os.path.getsize(d / WAL), q.info()
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    ids, status = (ctypes.c_uint32 * 3)(7, 7, 7), ctypes.create_string_buffer(b"\x07\x07\x07", 3)
    resource.setrlimit(resource.RLIMIT_FSIZE, (size + 5, hard))           # five bytes of the record fit, the rest does not
    try:
        rc = L.qs_draw(q.h, 3, (ctypes.c_uint64 * 3)(1, 2, 1), pack([E1, E1, E2]), (ctypes.c_uint32 * 3)(U32, U32, U32), ids, status)
        with pytest.raises(cases.Refused, match="quota ledger: cannot append to"):
            q.set_epochs([E1, E2, E3])
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
    assert rc != 0 and "cannot append to" in L.qs_error(q.h).decode()
    assert list(ids) == [7, 7, 7] and status.raw == b"\x07\x07\x07"          # nothing was handed out
    assert os.path.getsize(d / WAL) == size and q.info()[:4] == info[:4]    # taken back: no record, no sync counted
    assert [e for e, _ in q.window()] == [E1, E2]                            # the refused window was not applied
    m.draw([1, 2, 1], [E1, E1, E2], [U32] * 3)                               # the ids of the failed call are burnt
    play(q, m, ("draw", [1, 2], [E1, E1], [U32] * 2))                        # usable: the next record carries absolute values
    assert same(q.state(), model_state(m))
    q.close()
    # After a reopen a burnt id that no later record covered may be there again: it never left a call.  What holds is the
    # guarantee: no counter below what was handed out, none above what the live ledger had.
    handed = cc.CountsModel(DEPTH, MAX_EPOCHS)
    handed.set_epochs([E1, E2])
    handed.draw([1, 2, 1], [E1, E1, E2], [U32] * 3)
    handed.used[(E1, 1)], handed.used[(E1, 2)] = m.used[(E1, 1)], m.used[(E1, 2)]   # the last draw's ids lie above the burnt ones
    q = Ledger(L, d)
    got = q.state()
    assert not_below(got, model_state(handed)) and all(v <= m.used[k] for k, v in got[1].items())
    assert got[1] == {(E1, 1): 3, (E1, 2): 3, (E2, 1): 1}
    q.close()
