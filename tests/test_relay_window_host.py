"""The relay step's epoch window and the nullifier log's retain on the CPU: relay::gate with a window and the one-thread
retain of zerokit_amd/csrc/nullifier_log.h (tests/host/relaywindow.cpp), judged by the model of
tests/relay_window_cases.py; the same cases through a stand-alone sanitizer program; and the refusal texts of retain and
set_epochs, which come before anything touches a device.  No GPU needed."""
import ctypes
import os
import struct
import subprocess

import pytest

import nullifier_log_cases as log_cases
import nullifier_retire_cases as retire_cases
import relay_window_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC]   # (field.h: #pragma unroll)
U64P = ctypes.POINTER(ctypes.c_uint64)
CP = ctypes.c_char_p
R = cases.R


@pytest.fixture(scope="module")
def L():
    so = os.path.join(HOST, "librelaywindowhost.so")
    src = os.path.join(HOST, "relaywindow.cpp")
    deps = [src, os.path.join(HOST, "nullifierretire.cpp"), os.path.join(HOST, "nullifierlog.cpp")] + \
        [os.path.join(CSRC, h) for h in ("relay.h", "nullifier_log.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.nr_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.nr_new.restype = ctypes.c_void_p
    lib.nr_free.argtypes = [ctypes.c_void_p]
    lib.nr_free.restype = None
    lib.nr_observe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, CP, U64P, CP, CP, U64P]
    lib.nr_retire.argtypes = [ctypes.c_void_p, ctypes.c_size_t, CP, U64P]
    lib.nr_info.argtypes = [ctypes.c_void_p, U64P]
    lib.nr_info.restype = None
    lib.nr_check_table.argtypes = [ctypes.c_void_p]
    lib.nr_check_table.restype = ctypes.c_int64
    lib.nr_seqs_ascend.argtypes = [ctypes.c_void_p]
    lib.rw_step.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t, CP, CP, CP, CP, ctypes.c_size_t,
                            CP, ctypes.c_size_t, U64P, CP, CP, CP, U64P]
    lib.rw_retain.argtypes = [ctypes.c_void_p, ctypes.c_size_t, CP, U64P]
    lib.rw_row.argtypes = [ctypes.c_void_p, ctypes.c_uint64, CP, U64P, U64P]
    lib.rw_row.restype = None
    lib.rw_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.rw_table.restype = None
    for name in ("rw_retain_refusal", "rw_epochs_refusal"):
        getattr(lib, name).argtypes = [CP, ctypes.c_size_t]
        getattr(lib, name).restype = CP
    return lib


def info(L, log):
    out = (ctypes.c_uint64 * 6)()
    L.nr_info(log, out)
    return list(out)


def rows_of(L, log):
    """[(share, tag, sequence number)] of the rows held"""
    out = []
    for row in range(info(L, log)[1]):
        share, tag, seq = ctypes.create_string_buffer(128), ctypes.c_uint64(), ctypes.c_uint64()
        L.rw_row(log, row, share, ctypes.byref(tag), ctypes.byref(seq))
        out.append((tuple(int.from_bytes(share.raw[32 * j:32 * j + 32], "little") for j in range(4)), tag.value, seq.value))
    return out


def table_of(L, log):
    out = (ctypes.c_uint32 * info(L, log)[2])()
    L.rw_table(log, out)
    return list(out)


def observe(L, log, shares, tags):
    n = len(shares)
    status, secrets, first = ctypes.create_string_buffer(n), ctypes.create_string_buffer(32 * n), (ctypes.c_uint64 * n)()
    tg = None if tags is None else (ctypes.c_uint64 * n)(*tags)
    assert L.nr_observe(log, n, log_cases.pack(shares), tg, status, secrets, first) == 0
    return status.raw, secrets.raw, list(first)


def retain(L, log, window):
    removed = ctypes.c_uint64()
    rc = L.rw_retain(log, len(window), cases.pack_frs(window), ctypes.byref(removed))
    return rc, removed.value


def retire(L, log, exts):
    removed = ctypes.c_uint64()
    assert L.nr_retire(log, len(exts), cases.pack_frs(exts), ctypes.byref(removed)) == 0
    return removed.value


def step(L, log, k, rows, ok, xs, roots, window, tags):
    n = len(rows)
    verdict, status = ctypes.create_string_buffer(max(n, 1)), ctypes.create_string_buffer(max(n, 1))
    secrets = ctypes.create_string_buffer(max(32 * n, 1))
    first = (ctypes.c_uint64 * max(n, 1))()
    tg = None if tags is None else (ctypes.c_uint64 * max(n, 1))(*tags)
    rc = L.rw_step(log, k, cases.n_values(k), n,
                   cases.pack_rows(rows), bytes(ok), cases.pack_frs(xs), cases.pack_frs(roots), len(roots),
                   cases.pack_frs(window), len(window), tg, verdict, status, secrets, first)
    assert rc == 0
    return (list(verdict.raw[:n]), list(status.raw[:n]),
            [int.from_bytes(secrets.raw[32 * i:32 * i + 32], "little") for i in range(n)], list(first[:n]))


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("chunk", [2000, 63])
def test_gate_with_a_window_matches_the_model(L, k, chunk):
    c = cases.messages(k)
    n = len(c["rows"])
    want = cases.model(c["rows"], c["ok"], c["xs"], c["roots"], c["tags"], k, {}, 0, c["window"])
    log = L.nr_new(4 * n, 17)
    try:
        got = ([], [], [], [])
        for o in range(0, n, chunk):
            part = step(L, log, k, c["rows"][o:o + chunk], c["ok"][o:o + chunk], c["xs"][o:o + chunk], c["roots"], c["window"],
                        c["tags"][o:o + chunk])
            got = tuple(a + b for a, b in zip(got, part))
        assert got == tuple(want[:4])
        assert cases.BAD_EPOCH in got[0] and cases.FOREIGN in got[1]
        assert [(s, t) for s, t, _q in rows_of(L, log)] == list(zip(want[4], want[5]))
        assert all(s[3] in c["window"] for s in want[4])          # everything the relay records lies in the window ...
        assert retain(L, log, c["window"]) == (0, 0)              # ... so retaining it removes nothing
        assert L.nr_check_table(log) == len(set(s[0] for s in want[4]))
    finally:
        L.nr_free(log)


@pytest.mark.parametrize("k", [1, 4])
def test_no_window_is_the_step_as_it_was(L, k):
    c = cases.messages(k)
    want = cases.relay_cases.model(c["rows"], c["ok"], c["xs"], c["roots"], c["tags"], k, {}, 0)
    log = L.nr_new(4 * len(c["rows"]), 17)
    try:
        got = step(L, log, k, c["rows"], c["ok"], c["xs"], c["roots"], (), c["tags"])
        assert got == tuple(want[:4]) and cases.BAD_EPOCH not in got[0]
    finally:
        L.nr_free(log)


@pytest.mark.parametrize("k", [1, 4])
def test_moving_the_window_between_two_steps(L, k):
    """a step under {e0, e1}, the window moved to {e1, e2} by a retain, a step under that: the second step answers as the
    model does over the survivors of the first, and sequence numbers go on where they were"""
    c = cases.messages(k)
    n, half = len(c["rows"]), len(c["rows"]) // 2
    e = c["exts"]
    cut = lambda name, a, b: c[name][a:b]
    log = L.nr_new(4 * n, 31)
    try:
        seen = {}
        first = cases.model(cut("rows", 0, half), cut("ok", 0, half), cut("xs", 0, half), c["roots"], None, k, seen, 0, e[:2])
        got = step(L, log, k, cut("rows", 0, half), cut("ok", 0, half), cut("xs", 0, half), c["roots"], e[:2], None)
        assert got == tuple(first[:4])
        kept = cases.retained(first[4], first[5], e[1:])
        assert retain(L, log, e[1:]) == (0, len(first[4]) - len(kept)) and 0 < len(kept) < len(first[4])
        assert rows_of(L, log) == kept
        seen = {}
        log_cases.model([s for s, _t, _q in kept], [t for _s, t, _q in kept], seen)
        second = cases.model(cut("rows", half, n), cut("ok", half, n), cut("xs", half, n), c["roots"], None, k, seen, len(first[4]),
                             e[1:])
        got = step(L, log, k, cut("rows", half, n), cut("ok", half, n), cut("xs", half, n), c["roots"], e[1:], None)
        assert got == tuple(second[:4])
        assert rows_of(L, log)[len(kept):] == [(s, t, t) for s, t in zip(second[4], second[5])]
        assert L.nr_seqs_ascend(log) == 1 and L.nr_check_table(log) == len(seen)
    finally:
        L.nr_free(log)


def test_retain_against_the_retire_flow(L):
    """the 4 096-share stream: retaining the second of its two external nullifiers after the first half must leave
    flow()["kept"] and then answer flow()["second"], which is what retiring the first one owes"""
    shares, tags, _ = log_cases.stream()
    flow = retire_cases.flow()
    half = retire_cases.HALF
    other = next(s[3] for s in shares if s[3] != flow["ext"])
    assert retire_cases.survivors(shares[:half], tags[:half], {s[3] for s in shares} - {other}) == list(flow["kept"])
    log = L.nr_new(len(shares), 5)
    try:
        assert observe(L, log, shares[:half], tags[:half]) == log_cases.flat(flow["first"])
        assert retain(L, log, [other]) == (0, half - len(flow["kept"]))
        assert rows_of(L, log) == list(flow["kept"])
        assert observe(L, log, shares[half:], tags[half:]) == log_cases.flat(flow["second"])
        assert L.nr_check_table(log) == flow["distinct"] == info(L, log)[3]
        assert info(L, log)[4] == len(shares)
    finally:
        L.nr_free(log)


@pytest.mark.parametrize("k_set", [6, 30, 64])
def test_retain_equals_retire_of_the_complement_record_for_record_and_slot_for_slot(L, k_set):
    shares, tags = cases.synthetic_log(1500, 70)
    # nullifiers that repeat under another external nullifier, so that "the first record" moves
    shares = list(shares) + [(s[0], s[1] + 1, s[2], 1000 + (i + 1) % 70) for i, s in enumerate(shares[:300])]
    tags = list(tags) + [7 * i for i in range(300)]
    window = [1000 + 69 - j for j in range(k_set)]
    if k_set == 64:
        window[5] = window[6]            # a duplicate in the set is not an error
    outside = sorted({s[3] for s in shares} - set(window))
    assert 1 <= len(outside) <= 64
    a, b = L.nr_new(len(shares) + 300, 77), L.nr_new(len(shares) + 300, 77)
    try:
        for log in (a, b):
            observe(L, log, shares, tags)
        gone = retain(L, a, window)
        assert gone == (0, retire(L, b, outside)) and 0 < gone[1] < len(shares)
        assert rows_of(L, a) == rows_of(L, b) == cases.retained(shares, tags, window)
        assert table_of(L, a) == table_of(L, b)
        assert info(L, a) == info(L, b)
        more = [(s[0], s[1] + 2, s[2] + 2, s[3]) for s in shares[::7]]
        assert observe(L, a, more, None) == observe(L, b, more, None)
    finally:
        L.nr_free(a)
        L.nr_free(b)


def test_the_removed_side_has_no_size_limit(L):
    """a log holding 200 distinct external nullifiers retains 3 of them in one call"""
    shares, tags = cases.synthetic_log(1000, 200)
    window = [1000 + 199, 1000, 1000 + 57]
    log = L.nr_new(1000, 9)
    try:
        observe(L, log, shares, tags)
        assert retain(L, log, window) == (0, 1000 - 15)
        assert rows_of(L, log) == cases.retained(shares, tags, window) and len(rows_of(L, log)) == 15
        assert L.nr_check_table(log) == 15 and L.nr_seqs_ascend(log) == 1
        assert info(L, log)[4] == 1000                       # sequence numbers are not reused
        assert retain(L, log, window) == (0, 0)
    finally:
        L.nr_free(log)


BIG = R.to_bytes(32, "little")
ONE = (1).to_bytes(32, "little")
RETAIN_REFUSALS = [   # (set, k), the text
    ((None, 1), "nullifier log: retain was given a null pointer for k > 0 external nullifiers"),
    ((None, 65), "nullifier log: retain was given a null pointer for k > 0 external nullifiers"),
    ((ONE, 0), "nullifier log: a retain of no external nullifiers would remove every record: use clear"),
    ((None, 0), "nullifier log: a retain of no external nullifiers would remove every record: use clear"),
    ((ONE * 65, 65), "nullifier log: retain takes at most 64 external nullifiers a call, not 65"),
    ((ONE * 2 + BIG + BIG, 4), "nullifier log: external nullifier 2 of the retain is not canonical (>= r)"),
    ((BIG, 1), "nullifier log: external nullifier 0 of the retain is not canonical (>= r)"),
    ((ONE * 64, 64), ""),
    ((ONE + ONE, 2), ""),
]
EPOCHS_REFUSALS = [
    ((None, 1), RETAIN_REFUSALS[0][1]),
    ((ONE * 65, 65), "relay: a window holds at most 64 external nullifiers (RLNAMD_RELAY_EPOCHS_MAX), not 65"),
    ((ONE + BIG, 2), "nullifier log: external nullifier 1 of the retain is not canonical (>= r)"),
    ((None, 0), ""),
    ((ONE, 0), ""),
    ((ONE * 64, 64), ""),
]


def test_refusal_texts_of_the_headers(L):
    for (ext, k), text in RETAIN_REFUSALS:
        assert L.rw_retain_refusal(ext, k).decode() == text, k
    for (ext, k), text in EPOCHS_REFUSALS:
        assert L.rw_epochs_refusal(ext, k).decode() == text, k


def test_refused_retains_leave_the_host_log_as_it_was(L):
    shares, tags = cases.synthetic_log(40, 3)
    log = L.nr_new(64, 9)
    try:
        observe(L, log, shares, tags)
        before = (info(L, log), rows_of(L, log), table_of(L, log))
        removed = ctypes.c_uint64()
        for (ext, k), text in RETAIN_REFUSALS:
            if text:
                assert L.rw_retain(log, k, ext, ctypes.byref(removed)) == 1 and removed.value == 0
        assert (info(L, log), rows_of(L, log), table_of(L, log)) == before
    finally:
        L.nr_free(log)


def test_the_c_abi_refuses_before_it_follows_a_handle():
    """the same texts through rlnamd_nullifier_log_retain and rlnamd_relay_set_epochs with no object behind the handle:
    what needs no object is refused first, and a null handle is an error of its own"""
    from zerokit_amd._native import last_error, lib
    removed = ctypes.c_uint64()
    for (ext, k), text in RETAIN_REFUSALS:
        assert lib().rlnamd_nullifier_log_retain(None, ext, k, ctypes.byref(removed)) != 0
        assert last_error() == (text or "rlnamd_nullifier_log_retain: null log"), k
    for (ext, k), text in EPOCHS_REFUSALS:
        assert lib().rlnamd_relay_set_epochs(None, ext, k, ctypes.byref(removed)) != 0
        assert last_error() == (text or "rlnamd_relay_set_epochs: null relay"), k
    out, kk = ctypes.create_string_buffer(32 * 64), ctypes.c_size_t()
    assert lib().rlnamd_relay_epochs(None, out, ctypes.byref(kk)) != 0 and last_error() == "rlnamd_relay_epochs: null pointer"


def test_the_drop_in_entries_refuse_before_they_follow_a_handle():
    from zerokit_amd._native import CFr, lib
    from zerokit_amd.public import _err

    def said(r):
        return bool(r.ok), (_err(r.err) if r.err.ptr else "")

    def cfrs(raw):
        return None if raw is None else (CFr * (len(raw) // 32)).from_buffer_copy(raw)

    removed = ctypes.c_size_t()
    dummy, null_handle = ctypes.c_void_p(64), ctypes.c_void_p(None)
    for (ext, k), text in RETAIN_REFUSALS:
        assert said(lib().ffi_nullifier_log_retain(None, cfrs(ext), k, ctypes.byref(removed))) == \
            (False, text or "rlnamd_nullifier_log_retain: null log"), k
    for name in ("ffi_relay_set_epochs", "ffi_rln_v3_relay_set_epochs"):
        F = getattr(lib(), name)
        for (ext, k), text in EPOCHS_REFUSALS:
            assert said(F(None, dummy, cfrs(ext), k, ctypes.byref(removed))) == (False, text or "relay set_epochs: null RLN object"), k
        assert said(F(ctypes.byref(null_handle), dummy, cfrs(ONE), 1, None)) == (False, "relay set_epochs: null RLN object")
        assert said(F(ctypes.byref(dummy), None, cfrs(ONE), 1, None)) == (False, "relay set_epochs: null log")


def test_python_names():
    from zerokit_amd import batch, public, public_v3
    assert batch.Relay.BAD_EPOCH == 4 and batch.Relay.EPOCHS_MAX == 64
    assert batch.Relay.INFO[7] == "bad_epoch"
    for owner, name in ((batch.NullifierLog, "retain"), (batch.Relay, "set_epochs"), (batch.Relay, "epochs"),
                        (public, "retain_external_nullifiers"), (public.RLN, "relay_set_epochs"),
                        (public_v3.RLNV3, "relay_set_epochs")):
        assert callable(getattr(owner, name))


def test_window_and_retain_under_asan_and_ubsan(L, tmp_path):
    """a stand-alone program of its own (tests/host/relaywindow_main.cpp), built with the sanitizers and run as a child
    process on the single and the multi cases"""
    exe = str(tmp_path / "relaywindow_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "relaywindow_main.cpp"), "-o", exe])
    for k in (1, 4):
        c = cases.messages(k)
        n = len(c["rows"])
        want = cases.model(c["rows"], c["ok"], c["xs"], c["roots"], c["tags"], k, {}, 0, c["window"])
        under_first = sum(1 for s in want[4] if s[3] == c["window"][0])
        path = str(tmp_path / ("case%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<8Q", k, cases.n_values(k), n, 64, len(c["window"]), 4 * n, 23, under_first))
            f.write(cases.pack_rows(c["rows"]) + bytes(c["ok"]) + cases.pack_frs(c["xs"]) + cases.pack_frs(c["roots"]) +
                    cases.pack_frs(c["window"]))
            f.write(struct.pack("<%dQ" % n, *c["tags"]))
            f.write(bytes(want[0]) + bytes(want[1]) + cases.pack_frs(want[2]) + struct.pack("<%dQ" % n, *want[3]))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "ok %d\n" % (4 * n), (r.stdout, r.stderr[-2000:])
