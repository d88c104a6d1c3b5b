"""The nullifier log's retire (zerokit_amd/csrc/nullifier_log.h: the keep predicate, the sequential retire over the
one-thread policy and the sequence-number lookup), built for the CPU and judged by the flow of
tests/nullifier_retire_cases.py, and once more in a stand-alone sanitizer program.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

import nullifier_log_cases as cases
import nullifier_retire_cases as rcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
U64P = ctypes.POINTER(ctypes.c_uint64)
HALF = rcases.HALF


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libnullifierretire.so")
    src = os.path.join(HOST, "nullifierretire.cpp")
    deps = [src, os.path.join(HOST, "nullifierlog.cpp")] + [os.path.join(CSRC, h) for h in ("nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.nr_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.nr_new.restype = ctypes.c_void_p
    lib.nr_free.argtypes = [ctypes.c_void_p]
    lib.nr_free.restype = None
    lib.nr_observe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, U64P, ctypes.c_char_p, ctypes.c_char_p, U64P]
    lib.nr_observe.restype = ctypes.c_int
    lib.nr_retire.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, U64P]
    lib.nr_retire.restype = ctypes.c_int
    lib.nr_get.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, U64P]
    lib.nr_get.restype = ctypes.c_int
    lib.nr_info.argtypes = [ctypes.c_void_p, U64P]
    lib.nr_info.restype = None
    lib.nr_check_table.argtypes = [ctypes.c_void_p]
    lib.nr_check_table.restype = ctypes.c_int64
    lib.nr_seqs_ascend.argtypes = [ctypes.c_void_p]
    lib.nr_seqs_ascend.restype = ctypes.c_int
    return lib


class Log:
    def __init__(self, L, capacity, seed):
        self.L, self.h = L, L.nr_new(capacity, seed)

    def close(self):
        self.L.nr_free(self.h)

    def observe(self, shares, tags, chunk=None):
        """-> (rc of the last call, (status bytes, secrets bytes, [first tags]))"""
        got, rc = (b"", b"", []), 0
        chunk = chunk or max(len(shares), 1)
        for o in range(0, len(shares), chunk):
            part = shares[o:o + chunk]
            n = len(part)
            status = ctypes.create_string_buffer(n)
            secrets = ctypes.create_string_buffer(32 * n)
            first = (ctypes.c_uint64 * n)()
            tg = None if tags is None else (ctypes.c_uint64 * n)(*tags[o:o + chunk])
            rc = self.L.nr_observe(self.h, n, cases.pack(part), tg, status, secrets, first)
            if rc != 0:
                break
            got = tuple(a + b for a, b in zip(got, (status.raw[:n], secrets.raw[:32 * n], list(first[:n]))))
        return rc, got

    def retire(self, exts):
        """-> (rc, removed)"""
        removed = ctypes.c_uint64()
        packed = b"".join(int(e).to_bytes(32, "little") for e in exts)
        return self.L.nr_retire(self.h, len(exts), packed, ctypes.byref(removed)), removed.value

    def get(self, seq):
        """-> (rc, share, tag)"""
        out = ctypes.create_string_buffer(128)
        tag = ctypes.c_uint64()
        rc = self.L.nr_get(self.h, seq, out, ctypes.byref(tag))
        return rc, tuple(int.from_bytes(out.raw[32 * k:32 * k + 32], "little") for k in range(4)), tag.value

    def info(self):
        out = (ctypes.c_uint64 * 6)()
        self.L.nr_info(self.h, out)
        return list(out)

    def taken(self):
        return self.L.nr_check_table(self.h)


@pytest.mark.parametrize("chunk", [4096, 1, 63, 1000])
def test_sequential_retire_matches_the_model(L, chunk):
    flow = rcases.flow()          # asserts first what the flow exercises
    shares, tags, _ = cases.stream()
    log = Log(L, 4096, 11)
    try:
        rc, got = log.observe(shares[:HALF], tags[:HALF], chunk)
        assert rc == 0 and got == cases.flat(flow["first"])
        assert log.retire([flow["ext"]]) == (0, 1014)
        # the rebuild: one slot per key, every key reachable from its home slot without an empty slot on the way
        assert log.taken() == len({k[0][0] for k in flow["kept"]})
        assert L.nr_seqs_ascend(log.h) == 1
        info = log.info()
        assert info[:5] == [4096, 1034, 8192, log.taken(), HALF] and 1 <= info[5] <= 8192
        rc, got = log.observe(shares[HALF:], tags[HALF:], chunk)
        assert rc == 0 and got == cases.flat(flow["second"])
        assert log.taken() == flow["distinct"]
        assert log.info()[:5] == [4096, 1034 + HALF, 8192, flow["distinct"], 4096]
    finally:
        log.close()


def test_retire_of_an_absent_of_both_and_twice_in_a_row(L):
    flow = rcases.flow()
    shares, tags, _ = cases.stream()
    exts = sorted({s[3] for s in shares}, key=lambda e: e != flow["ext"])      # the retired one first
    assert len(exts) == 2
    log = Log(L, 4096, 12)
    try:
        assert log.observe(shares[:HALF], tags[:HALF])[0] == 0
        before = (log.info(), log.taken())
        assert log.retire([12345]) == (0, 0) and log.retire([]) == (0, 0)       # nobody's, and none at all
        assert (log.info(), log.taken()) == before
        rc, got = log.observe(shares[HALF:HALF + 100], tags[HALF:HALF + 100])
        assert got == tuple(p[n:] for p, n in zip(cases.flat(cases.model(shares[:HALF + 100], tags[:HALF + 100])), (HALF, 32 * HALF, HALF)))
        # two retires in a row: the first external nullifier, then the second; together they leave nothing
        n0 = sum(1 for s in shares[:HALF + 100] if s[3] == exts[0])
        assert log.retire([exts[0]]) == (0, n0)
        assert log.retire([exts[1]]) == (0, HALF + 100 - n0)
        assert log.info()[:5] == [4096, 0, 8192, 0, HALF + 100] and log.taken() == 0
        # what an empty log says, and default tags go on from the counter
        rc, got = log.observe(shares[:50], None)
        want = cases.flat(cases.model(shares[:50], range(HALF + 100, HALF + 150)))
        assert rc == 0 and got == want
    finally:
        log.close()
    # both in one call, a duplicate among them
    log = Log(L, 4096, 13)
    try:
        assert log.observe(shares, tags)[0] == 0
        assert log.retire([exts[1], exts[0], exts[1]]) == (0, 4096)
        assert log.info()[:5] == [4096, 0, 8192, 0, 4096] and log.taken() == 0
    finally:
        log.close()


def test_room_after_a_retire(L):
    """retire, then fill to capacity exactly, then one share more is refused"""
    shares, tags = rcases.synthetic(1100, classes=2)
    log = Log(L, 1024, 14)
    try:
        assert log.observe(shares[:1024], tags[:1024])[0] == 0
        assert log.observe(shares[1024:1025], tags[1024:1025])[0] == 1
        assert log.retire([1001]) == (0, 512)
        more = [(5000 + i, 1, 2, 1000) for i in range(513)]
        assert log.observe(more, None)[0] == 1                      # 513 do not fit, and leave nothing behind
        assert log.info()[:2] == [1024, 512]
        rc, got = log.observe(more[:512], None)
        assert rc == 0 and got[0] == bytes(512) and got[2] == list(range(1024, 1536))
        assert log.observe(more[512:], None)[0] == 1
        assert log.info()[:5] == [1024, 1024, 2048, 1024, 1536] and log.taken() == 1024
    finally:
        log.close()


def test_get_of_a_kept_a_retired_and_a_never_issued_sequence_number(L):
    flow = rcases.flow()
    shares, tags, _ = cases.stream()
    log = Log(L, 4096, 15)
    try:
        assert log.observe(shares[:HALF], tags[:HALF])[0] == 0
        assert log.get(HALF - 1)[0] == 0 and log.get(HALF)[0] == 1            # before any retire: row == sequence number
        assert log.retire([flow["ext"]])[0] == 0
        kept = {k[2] for k in flow["kept"]}
        for seq in range(HALF):
            rc, share, tag = log.get(seq)
            assert (rc, share, tag) == (0, shares[seq], tags[seq]) if seq in kept else rc == 2, seq
        assert log.get(HALF)[0] == 1 and log.get(2 ** 40)[0] == 1
        assert log.observe(shares[HALF:HALF + 3], None)[0] == 0
        assert log.get(HALF + 2) == (0, shares[HALF + 2], HALF + 2) and log.get(HALF + 3)[0] == 1
    finally:
        log.close()


def test_refusals_leave_the_log_as_it_was(L):
    shares, tags, _ = cases.stream()
    log = Log(L, 64, 16)
    try:
        assert log.observe(shares[:64], tags[:64])[0] == 0
        before = (log.info(), log.taken())
        removed = ctypes.c_uint64()
        assert L.nr_retire(log.h, 1, None, ctypes.byref(removed)) == 1
        assert log.retire([shares[0][3]] * 65)[0] == 2
        assert log.retire([shares[0][3], 5, cases.R, cases.R + 1]) == (3, 2)    # names the first one >= r
        assert (log.info(), log.taken()) == before
        assert log.retire([shares[0][3]] * 64)[0] == 0
    finally:
        log.close()


def test_retire_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/nullifierretire_main.cpp), built with the sanitizers and run once"""
    exe = str(tmp_path / "nullifierretire_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "nullifierretire_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])
