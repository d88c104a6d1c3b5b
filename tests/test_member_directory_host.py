"""The member directory on the CPU: the sequential text of zerokit_amd/csrc/member_directory.h (tests/host/memberdir.cpp,
built with g++ and loaded with ctypes) held to the dict model of tests/member_directory_cases.py on every case the GPU
tests use; an 8-thread run of the insert and commit passes over std::atomic; the same cases through a stand-alone
sanitizer program; the refusal texts, which come before anything touches a device; and the model itself checked for
order independence.  No GPU needed."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

import member_directory_cases as cases
from member_directory_cases import FOUND, KNOWN, NO_INDEX, OCCUPIED, OK, R, REMOVED, SKIPPED, UNKNOWN, VACANT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
CP = ctypes.c_char_p
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
VP, SZ, U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64


def pack(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def u64s(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def u32s(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "libmemberdirhost.so")
    src = os.path.join(HOST, "memberdir.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("member_directory.h", "nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    sig = {
        "md_last": (CP, []),
        "md_new_refusal": (CP, [U64, U64]),
        "md_register_refusal": (CP, [SZ, U64P, CP, U32P, CP, U64]),
        "md_find_refusal": (CP, [SZ, CP, CP, U64P, U32P]),
        "md_resolve_refusal": (CP, [CP, SZ, CP, CP, CP, U64P, U32P]),
        "md_remove_refusal": (CP, [SZ, U64P, CP, U64]),
        "md_get_refusal": (CP, [SZ, U64P, CP, CP, U32P, U64]),
        "md_new": (VP, [U64, U64]),
        "md_free": (None, [VP]),
        "md_register": (ctypes.c_int, [VP, SZ, U64P, CP, U32P, CP]),
        "md_register_threads": (ctypes.c_int, [VP, SZ, U64P, CP, U32P, CP, ctypes.c_uint]),
        "md_find": (ctypes.c_int, [VP, SZ, CP, CP, U64P, U32P]),
        "md_resolve": (ctypes.c_int, [VP, SZ, CP, CP, CP, CP, U64P, U32P]),
        "md_slash": (ctypes.c_int, [VP, SZ, CP, CP, CP, CP, U64P, U32P, U64P]),
        "md_remove": (ctypes.c_int, [VP, SZ, U64P, CP]),
        "md_get": (ctypes.c_int, [VP, SZ, U64P, CP, CP, U32P]),
        "md_info": (None, [VP, U64P]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


class HostDirectory:
    """memberdir.cpp's directory with the methods of zerokit_amd.batch.MemberDirectory"""

    def __init__(self, L, capacity, seed=1, threads=0):
        self.L, self.h, self.threads = L, L.md_new(capacity, seed), threads
        assert self.h

    def close(self):
        self.L.md_free(self.h)

    def _check(self, rc):
        if rc != 0:
            raise cases.Refused(self.L.md_last().decode())

    def register(self, members):
        n = len(members)
        status = ctypes.create_string_buffer(max(n, 1))
        args = (self.h, n, u64s([m[0] for m in members]), pack(m[1] for m in members) or b"\0", u32s([m[2] for m in members]), status)
        self._check(self.L.md_register_threads(*args, self.threads) if self.threads else self.L.md_register(*args))
        return list(status.raw[:n])

    def _out(self, n):
        return ctypes.create_string_buffer(max(n, 1)), u64s([0] * n), u32s([0] * n)

    def find(self, idcs):
        n = len(idcs)
        status, index, limit = self._out(n)
        self._check(self.L.md_find(self.h, n, pack(idcs) or b"\0", status, index, limit))
        return list(status.raw[:n]), list(index[:n]), list(limit[:n])

    def _secrets(self, secrets, take):
        # the header has no Poseidon: the commitments of the canonical secrets come from the oracle
        keys = cases.commitments([s if s < R else 0 for s in secrets])
        return pack(secrets) or b"\0", pack(keys) or b"\0", None if take is None else bytes(1 if t else 0 for t in take) or b"\0"

    def resolve(self, secrets, take=None):
        n = len(secrets)
        status, index, limit = self._out(n)
        self._check(self.L.md_resolve(self.h, n, *self._secrets(secrets, take), status, index, limit))
        return list(status.raw[:n]), list(index[:n]), list(limit[:n])

    def slash(self, secrets, take=None):
        n = len(secrets)
        status, index, limit = self._out(n)
        removed = ctypes.c_uint64()
        self._check(self.L.md_slash(self.h, n, *self._secrets(secrets, take), status, index, limit, ctypes.byref(removed)))
        return list(status.raw[:n]), list(index[:n]), list(limit[:n]), int(removed.value)

    def remove(self, indices):
        n = len(indices)
        status = ctypes.create_string_buffer(max(n, 1))
        self._check(self.L.md_remove(self.h, n, u64s(indices), status))
        return list(status.raw[:n])

    def get(self, indices):
        n = len(indices)
        live, idcs, limits = ctypes.create_string_buffer(max(n, 1)), ctypes.create_string_buffer(max(32 * n, 1)), u32s([0] * n)
        self._check(self.L.md_get(self.h, n, u64s(indices), live, idcs, limits))
        return [(bool(live.raw[i]), int.from_bytes(idcs.raw[32 * i:32 * i + 32], "little"), int(limits[i])) for i in range(n)]

    def info(self):
        out = (ctypes.c_uint64 * 8)()
        self.L.md_info(self.h, out)
        return list(out)


# ---------------------------------------------------------------------------------------------- the model itself
def test_the_model_does_not_depend_on_the_order_of_a_call():
    """every permutation of a six-request call that meets each status (720), and 200 shuffles of the nine-request one:
    the same status per request, the same rows, the same root"""
    import itertools
    first, second, want, _ = cases.every_status()

    def run(reqs):
        m = cases.Model(5)
        m.register(list(first))
        return m, m.register(reqs)
    base, status = run(list(second))
    assert status == list(want)
    by_request = dict(zip(second, status))
    six = list(second[:6])
    ref, st6 = run(six)
    want6 = dict(zip(six, st6))
    assert set(st6) == {OK, OCCUPIED, KNOWN}
    for perm in itertools.permutations(six):
        m, st = run(list(perm))
        assert dict(zip(perm, st)) == want6 and m.rows == ref.rows and m.root() == ref.root()
    rnd = random.Random(9)
    for _ in range(200):
        reqs = list(second)
        rnd.shuffle(reqs)
        m, st = run(reqs)
        assert dict(zip(reqs, st)) == by_request and m.rows == base.rows and m.root() == base.root()


def test_the_model_slash_is_resolve_then_remove_and_a_split_differs():
    mem, indices = cases.small()
    a, b = cases.Model(5), cases.Model(5)
    for m in (a, b):
        assert m.register([(i, x[1], x[2]) for i, x in zip(indices, mem)]) == [OK] * 20
    secrets = [mem[0][0], mem[0][0], mem[3][0], 12345]
    out = a.slash(secrets)
    st, ix, lm = b.resolve(secrets)
    assert out == (st, ix, lm, 2) and st == [FOUND, FOUND, FOUND, UNKNOWN] and ix[0] == ix[1] == indices[0]
    assert b.remove(sorted({i for s, i in zip(st, ix) if s == FOUND})) == [REMOVED] * 2
    assert a.rows == b.rows and a.root() == b.root()
    # in one call the lowest index wins; across calls the first call wins
    idc = mem[0][1]
    one, two = cases.Model(5), cases.Model(5)
    assert one.register([(9, idc, 1), (2, idc, 1)]) == [KNOWN, OK]
    assert two.register([(9, idc, 1)]) + two.register([(2, idc, 1)]) == [OK, KNOWN]


# --------------------------------------------------------------------------------------- the header's sequential text
def test_host_small_directory(L):
    mem, indices = cases.small()
    d, m = HostDirectory(L, 32), cases.Model(5, 32)
    try:
        reqs = [(i, x[1], x[2]) for i, x in zip(indices, mem)]
        cases.compare_register(m, d, reqs)
        cases.compare_state(m, d, list(range(32)) + [5, 5])
        assert d.find([x[1] for x in mem] + [7]) == m.find([x[1] for x in mem] + [7])
        assert d.info()[:5] == [32, 20, 64, 20, 0]
    finally:
        d.close()


@pytest.mark.parametrize("shuffle", [None, 1, 2, 3])
def test_host_every_status_in_any_order(L, shuffle):
    first, second, want, _ = cases.every_status()
    reqs = list(second)
    if shuffle:
        random.Random(shuffle).shuffle(reqs)
    d, m = HostDirectory(L, 32), cases.Model(5, 32)
    try:
        cases.compare_register(m, d, list(first))
        got = d.register(reqs)
        assert got == m.register(reqs) and dict(zip(reqs, got)) == dict(zip(second, want))
        cases.compare_state(m, d, list(range(32)))
    finally:
        d.close()


@pytest.mark.parametrize("chunk", [5000, 1, 63, 64, 65, 257])
def test_host_big_call_and_its_splits(L, chunk):
    reqs = list(cases.big())
    if chunk == 1:
        reqs = reqs[:300] + reqs[-300:]     # (one by one: the ends, where the equal keys sit)
    d, m = HostDirectory(L, 1 << 13, seed=3), cases.Model(13)
    try:
        for o in range(0, len(reqs), chunk):
            cases.compare_register(m, d, reqs[o:o + chunk])
        cases.compare_state(m, d, [r[0] for r in reqs])
        idcs = sorted({r[1] for r in reqs})[:500]
        assert d.find(idcs) == m.find(idcs)
    finally:
        d.close()


def test_host_threads_give_the_sequential_statuses(L):
    """8 threads over std::atomic entries, every key eight times on average: the statuses, the rows and the longest walk's
    bound are those of the one-thread run"""
    reqs = cases.duplicate_heavy()
    seq, par, m = HostDirectory(L, 1 << 12, seed=11), HostDirectory(L, 1 << 12, seed=11, threads=8), cases.Model(12)
    try:
        want = m.register(reqs)
        assert want.count(KNOWN) > 3000
        for _ in range(3):                  # (a second and third call: everything is KNOWN or OCCUPIED by then)
            assert seq.register(reqs) == par.register(reqs) == want
            want = m.register(reqs)
        everything = list(range(1 << 12))
        assert seq.get(everything) == par.get(everything) == m.get(everything)
        assert seq.info()[:5] == par.info()[:5]
    finally:
        seq.close()
        par.close()


def test_host_resolve_slash_and_reregistration(L):
    mem, indices = cases.small()
    d, m = HostDirectory(L, 32), cases.Model(5, 32)
    try:
        cases.compare_register(m, d, [(i, x[1], x[2]) for i, x in zip(indices, mem)])
        assert d.remove([indices[4], 31 if 31 not in indices else indices[5]]) == m.remove([indices[4], 31 if 31 not in indices else indices[5]])
        secrets = [mem[0][0], mem[4][0], 999, mem[7][0]]
        assert d.resolve(secrets) == m.resolve(secrets)
        take = [1, 0, 1, 0]
        got = d.resolve(secrets, take)
        assert got == m.resolve(secrets, take) and got[0] == [FOUND, SKIPPED, UNKNOWN, SKIPPED] and got[1][1] == NO_INDEX
        assert d.resolve([R, 5], [0, 1]) == m.resolve([R, 5], [0, 1])          # a secret that is not taken is not read
        with pytest.raises(cases.Refused) as e:
            d.resolve([5, R + 1])
        assert str(e.value) == cases.resolve_refusal("resolve", [5, R + 1]) != ""
        sl = [mem[0][0], mem[1][0], mem[0][0], 31337, mem[1][0], mem[2][0]]
        assert d.slash(sl) == m.slash(sl)
        cases.compare_state(m, d, list(range(32)))
        again = [(indices[0], mem[0][1], 3), (indices[4], mem[1][1], 4)]        # the same index, and another one
        assert d.register(again) == m.register(again) == [OK, OK]
        assert d.resolve([mem[0][0], mem[1][0]]) == m.resolve([mem[0][0], mem[1][0]])
        cases.compare_state(m, d, list(range(32)))
    finally:
        d.close()


def test_host_churn_needs_the_rebuild(L):
    d, m = HostDirectory(L, 8), cases.Model(3, 8)
    try:
        for reqs in cases.churn_rounds():
            assert d.register(reqs) == m.register(reqs) == [OK] * 8
            assert d.info()[3] <= d.info()[2] // 2
            idcs = [r[1] for r in reqs]
            assert d.find(idcs + [1]) == m.find(idcs + [1])
            assert d.remove(list(range(8))) == m.remove(list(range(8))) == [REMOVED] * 8
            assert d.info()[3] <= d.info()[2] // 2 and d.find(idcs)[0] == [UNKNOWN] * 8
        info = d.info()
        assert info[2] == 16 and info[4] >= 1 and info[1] == 0 and info[5] <= 16
        assert d.remove([0]) == [VACANT]
    finally:
        d.close()


def test_the_seed_moves_walks_not_statuses(L):
    """2 000 members in 4 096 slots: the longest walk differs between seeds, no status does"""
    reqs = [(i, r[1], r[2]) for i, r in enumerate(cases.big()[:2000])]
    want = cases.Model(11).register(reqs)
    walks = set()
    for seed in (1, 2, 3, 4, 5, 6):
        d = HostDirectory(L, 1 << 11, seed=seed)
        assert d.register(reqs) == want
        walks.add(d.info()[5])
        d.close()
    assert len(walks) > 1 and all(1 <= w <= 1 << 12 for w in walks)


# ------------------------------------------------------------------------------------------------------ refusals
REGISTER_REFUSALS = [      # (members, capacity)
    ([(32, 1, 1)], 32), ([(1, 1, 1), (5, 2, 1), (1, 3, 1)], 32), ([(0, R, 1)], 32), ([(0, 1, 1), (1, 2, 0)], 32),
    ([(3, R + 5, 0), (3, 1, 1)], 32),          # the index rules come first
    ([(1 << 31, 1, 1)], 1 << 31),
]


def test_refusal_texts_of_the_header(L):
    for capacity, depth in [(0, 5), ((1 << 31) + 1, 40), (33, 5), (32, 5), (1, 0), (1 << 31, 31)]:
        assert L.md_new_refusal(capacity, depth).decode() == cases.new_refusal(capacity, depth)
    assert cases.new_refusal(32, 5) == cases.new_refusal(1, 0) == ""
    st = ctypes.create_string_buffer(8)
    for members, capacity in REGISTER_REFUSALS:
        want = cases.register_refusal(members, capacity)
        got = L.md_register_refusal(len(members), u64s([m[0] for m in members]), pack(m[1] for m in members),
                                    u32s([m[2] for m in members]), st, capacity).decode()
        assert got == want != "", members
    assert L.md_register_refusal(1, None, b"\0" * 32, u32s([1]), st, 8).decode() == cases.null_refusal("register")
    assert L.md_register_refusal(0, None, None, None, None, 8).decode() == ""
    ix, lm = u64s([0] * 4), u32s([0] * 4)
    assert L.md_find_refusal(1, None, st, ix, lm).decode() == cases.null_refusal("find")
    assert L.md_resolve_refusal(b"resolve", 2, None, None, st, ix, lm).decode() == cases.null_refusal("resolve", "secrets")
    assert L.md_resolve_refusal(b"slash", 2, pack([1, R]), None, st, ix, lm).decode() == cases.resolve_refusal("slash", [1, R]) != ""
    assert L.md_resolve_refusal(b"slash", 2, pack([1, R]), bytes([1, 0]), st, ix, lm).decode() == ""
    assert L.md_remove_refusal(2, u64s([4, 4]), st, 8).decode() == cases.indices_refusal("remove", [4, 4], 8) != ""
    assert L.md_remove_refusal(2, u64s([4, 8]), st, 8).decode() == cases.indices_refusal("remove", [4, 8], 8) != ""
    assert L.md_remove_refusal(1, None, st, 8).decode() == cases.null_refusal("remove")
    assert L.md_get_refusal(2, u64s([4, 4]), st, st, lm, 8).decode() == ""
    assert L.md_get_refusal(2, u64s([4, 9]), st, st, lm, 8).decode() == cases.indices_refusal("get", [4, 9], 8, False) != ""


def test_refused_calls_leave_the_host_directory_as_it_was(L):
    mem, indices = cases.small()
    d = HostDirectory(L, 32)
    try:
        d.register([(i, x[1], x[2]) for i, x in zip(indices, mem)])
        before = (d.get(list(range(32))), d.info())
        for members, capacity in REGISTER_REFUSALS[:5]:
            with pytest.raises(cases.Refused):
                d.register(members)
        with pytest.raises(cases.Refused):
            d.remove([1, 1])
        with pytest.raises(cases.Refused):
            d.slash([mem[0][0], R])
        assert (d.get(list(range(32))), d.info()) == before
    finally:
        d.close()


def test_the_c_abi_refuses_before_it_touches_a_device():
    """the same texts through rlnamd_directory_* with no object behind the handle and no device asked for"""
    from zerokit_amd._native import last_error, lib
    out = ctypes.c_void_p()
    assert lib().rlnamd_directory_new(None, 0, 0, ctypes.byref(out)) != 0 and last_error() == cases.new_refusal(0, 5)
    assert lib().rlnamd_directory_new(None, 8, 0, ctypes.byref(out)) != 0 and last_error() == "rlnamd_directory_new: null pointer"
    st, ix, lm = ctypes.create_string_buffer(8), u64s([0] * 4), u32s([0] * 4)
    for members, capacity in REGISTER_REFUSALS:
        if capacity != 1 << 31:
            continue                      # without an object the bound is the largest a directory can have
        assert lib().rlnamd_directory_register(None, 1, u64s([m[0] for m in members]), pack(m[1] for m in members),
                                               u32s([m[2] for m in members]), st) != 0
        assert last_error() == cases.register_refusal(members, capacity)
    assert lib().rlnamd_directory_register(None, 1, u64s([0]), pack([R]), u32s([1]), st) != 0
    assert last_error() == cases.register_refusal([(0, R, 1)], 1 << 31)
    assert lib().rlnamd_directory_register(None, 1, u64s([0]), pack([1]), u32s([1]), st) != 0
    assert last_error() == "rlnamd_directory_register: null directory"
    assert lib().rlnamd_directory_resolve(None, 2, pack([1, R]), None, st, ix, lm) != 0
    assert last_error() == cases.resolve_refusal("resolve", [1, R])
    removed = ctypes.c_uint64()
    assert lib().rlnamd_directory_slash(None, 2, pack([1, R]), None, st, ix, lm, ctypes.byref(removed)) != 0
    assert last_error() == cases.resolve_refusal("slash", [1, R])
    assert lib().rlnamd_directory_slash(None, 2, pack([1, R]), bytes([1, 0]), st, ix, lm, None) != 0
    assert last_error() == "rlnamd_directory_slash: null directory"
    assert lib().rlnamd_directory_remove(None, 2, u64s([7, 7]), st) != 0 and last_error() == cases.indices_refusal("remove", [7, 7], 1 << 31)
    assert lib().rlnamd_directory_find(None, 1, None, st, ix, lm) != 0 and last_error() == cases.null_refusal("find")
    assert lib().rlnamd_directory_get(None, 1, u64s([1 << 31]), st, st, lm) != 0
    assert last_error() == cases.indices_refusal("get", [1 << 31], 1 << 31, False)
    assert lib().rlnamd_directory_info(None, None) != 0 and last_error() == "rlnamd_directory_info: null pointer"
    lib().rlnamd_directory_free(None)


def test_python_names():
    from zerokit_amd import batch
    D = batch.MemberDirectory
    assert (D.OK, D.OCCUPIED, D.KNOWN, D.FOUND, D.UNKNOWN, D.SKIPPED, D.REMOVED, D.VACANT) == \
        (OK, OCCUPIED, KNOWN, FOUND, UNKNOWN, SKIPPED, REMOVED, VACANT)
    assert D.NO_INDEX == NO_INDEX
    for name in ("register", "find", "resolve", "resolve_raw", "slash", "slash_raw", "remove", "get", "info"):
        assert callable(getattr(D, name))


# ------------------------------------------------------------------------------------------ the sanitizer program
def test_the_directory_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/memberdir_main.cpp), built with the sanitizers and run as a child
    process: the cases above as one file of steps with the model's answers"""
    exe = str(tmp_path / "memberdir_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "memberdir_main.cpp"), "-o", exe])
    depth = 13
    m = cases.Model(depth)
    steps, judged = [], 0

    def q(fmt, vals):
        return struct.pack("<%d%s" % (len(vals), fmt), *vals)

    def register(reqs, threads=False):
        nonlocal judged
        refused = 1 if cases.register_refusal(reqs, m.capacity) else 0
        status = [] if refused else m.register(reqs)
        steps.append(struct.pack("<2Q", 7 if threads else 0, len(reqs)) + q("Q", [r[0] for r in reqs]) + pack(r[1] for r in reqs) +
                     q("I", [r[2] for r in reqs]) + struct.pack("<Q", refused) + bytes(status or [0] * len(reqs)))
        judged += len(reqs)

    def find(idcs):
        nonlocal judged
        st, ix, lm = m.find(idcs)
        steps.append(struct.pack("<2Q", 1, len(idcs)) + pack(idcs) + bytes(st) + q("Q", ix) + q("I", lm))
        judged += len(idcs)

    def resolve(secrets, take, slash=False):
        nonlocal judged
        n = len(secrets)
        refused = 1 if cases.resolve_refusal("x", secrets, take) else 0
        out = ([0] * n, [0] * n, [0] * n, 0) if refused else (m.slash(secrets, take) if slash else m.resolve(secrets, take) + (0,))
        keys = cases.commitments([s if s < R else 0 for s in secrets])
        steps.append(struct.pack("<2Q", 3 if slash else 2, n) + pack(secrets) + pack(keys) + bytes(take) + struct.pack("<Q", refused) +
                     bytes(out[0]) + q("Q", out[1]) + q("I", out[2]) + (struct.pack("<Q", out[3]) if slash else b""))
        judged += n

    def remove(indices):
        nonlocal judged
        refused = 1 if cases.indices_refusal("remove", indices, m.capacity) else 0
        status = [0] * len(indices) if refused else m.remove(indices)
        steps.append(struct.pack("<2Q", 4, len(indices)) + q("Q", indices) + struct.pack("<Q", refused) + bytes(status))
        judged += len(indices)

    def get(indices):
        nonlocal judged
        rows = m.get(indices)
        steps.append(struct.pack("<2Q", 5, len(indices)) + q("Q", indices) + bytes(1 if r[0] else 0 for r in rows) +
                     pack(r[1] for r in rows) + q("I", [r[2] for r in rows]))
        judged += len(indices)

    def info():
        nonlocal judged
        steps.append(struct.pack("<3Q", 6, 0, m.live()))
        judged += 1

    first, second, _, mem12 = cases.every_status()
    register([(i, idc, lim) for i, idc, lim in first])
    register(list(second))
    big = list(cases.big())
    register(big[:2500])
    register(big[2500:], threads=True)
    register([(1 << depth, 1, 1)])                       # refused
    register([(1, R, 1)])                                # refused
    info()
    get([r[0] for r in big[::7]] + [0, 0, (1 << depth) - 1])
    find([r[1] for r in big[::5]] + [1, 2, R])
    secrets = [x[0] for x in mem12]
    resolve(secrets, [1] * 12)
    resolve(secrets + [R], [1, 0] * 6 + [0])
    resolve(secrets + [R], [1] * 13)                     # refused
    resolve(secrets[:6] + secrets[:3] + [4242], [1] * 10, slash=True)
    remove([r[0] for r in big[:1000]] + [big[0][0]])     # refused: twice
    remove([r[0] for r in big[:1000]])
    remove([r[0] for r in big[:10]])                     # VACANT
    register(big[:1000])                                 # the removed come back (those whose commitment is not live elsewhere)
    for reqs in cases.churn_rounds(6, 8, 5):             # churn at the low indices, whatever lives there
        remove([r[0] for r in reqs])
        register(reqs)
    info()
    get(list(range(0, 1 << depth, 13)))
    path = str(tmp_path / "steps.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<3Q", 1 << depth, 77, len(steps)) + b"".join(steps))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok %d\n" % judged, (r.stdout, r.stderr[-2000:])
