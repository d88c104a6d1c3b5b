"""Retiring epochs from the nullifier log on the device (rlnamd_nullifier_log_retire, ffi_nullifier_log_retire), judged
byte for byte by the flow of tests/nullifier_retire_cases.py: what a log owes after a retire is what the model of
tests/nullifier_log_cases.py says when it has seen only the survivors, with their tags, in their order."""
import ctypes as C
import random

import numpy as np
import pytest

import nullifier_log_cases as cases
import nullifier_retire_cases as rcases
from nullifier_log_cases import DUPLICATE, FOREIGN, NEW, R, SPAM

pytestmark = pytest.mark.gpu

N = 4096
HALF = rcases.HALF


def _log(capacity, seed=0):
    from zerokit_amd.batch import NullifierLog
    return NullifierLog(capacity, seed)


def _chunks(log, shares, tags, chunk):
    got = (b"", b"", [])
    for o in range(0, len(shares), chunk):
        part = log.observe_raw(cases.pack(shares[o:o + chunk]), tags[o:o + chunk])
        got = tuple(a + b for a, b in zip(got, part))
    return got


def _after(kept_shares, kept_tags, shares, tags):
    """the model's verdicts on `shares` in a log that holds the kept ones -> what observe_raw returns"""
    seen = {}
    cases.model(kept_shares, kept_tags, seen)
    return cases.flat(cases.model(shares, tags, seen))


# ------------------------------------------------------------------------------------------------ 1. model parity
@pytest.mark.parametrize("chunk", [1, 65, 257, 2048])
def test_parity_with_the_model(chunk):
    flow = rcases.flow()          # asserts first: 1 014 go, 1 034 stay, 726 verdicts differ from a log that kept them
    shares, tags, _ = cases.stream()
    log = _log(N, 5)
    assert _chunks(log, shares[:HALF], tags[:HALF], HALF) == cases.flat(flow["first"])
    assert log.retire([flow["ext"]]) == 1014
    assert log.info()[:4] == [N, 1034, 2 * N, len({k[0][0] for k in flow["kept"]})]
    got = _chunks(log, shares[HALF:], tags[HALF:], chunk)
    status, secrets, first = cases.flat(flow["second"])
    assert got[0] == status
    assert got[1] == secrets
    assert got[2] == first
    info = log.info()
    assert info[:4] == [N, 1034 + HALF, 2 * N, flow["distinct"]]
    assert info[6] == 0
    rinfo = log.retire_info()
    assert rinfo[:4] == [1, 1014, N, 1034 + HALF] and 1 <= rinfo[4] <= 2 * N and rinfo[5:] == [1, 0, 0]
    log.close()


# ------------------------------------------------------------------- 2. one nullifier under two external nullifiers
def test_the_first_surviving_record_becomes_the_first():
    a0, a1 = 9, 4
    share = lambda x, ext: (7, x, (a0 + x * a1) % R, ext)
    log = _log(16, 3)
    assert log.observe([share(11, 100), share(12, 200)], [50, 51]) == ([NEW, FOREIGN], [0, 0], [50, 50])
    assert log.retire([100]) == 1                        # the epoch of the first record
    status, secrets, first = log.observe([share(13, 200), share(12, 200), share(14, 100)], [52, 53, 54])
    assert status == [SPAM, DUPLICATE, FOREIGN]          # against the survivor under 200, which is the first now
    assert secrets == [a0, 0, 0]
    assert first == [51, 51, 51]
    assert log.info()[:4] == [16, 4, 32, 1]
    log.close()


# ------------------------------------------------------------------------------------------------ 3. default tags
def test_default_tags_and_get_by_sequence_number():
    from zerokit_amd._native import RLNError
    shares, _ = rcases.synthetic(310)
    log = _log(400, 3)
    assert log.observe(shares[:300])[2] == list(range(300))
    assert log.get(299) == (shares[299], 299)
    assert log.retire([1001]) == 100
    status, _, first = log.observe(shares[300:])
    assert status == [NEW] * 10 and first == list(range(300, 310))      # the counter was not lowered
    for seq in (0, 2, 3, 150, 299, 300, 309):
        assert log.get(seq) == (shares[seq], seq)
    for seq in (1, 4, 298):
        with pytest.raises(RLNError, match="record %d was retired" % seq):
            log.get(seq)
    with pytest.raises(RLNError, match="no record 310"):
        log.get(310)
    assert log.retire_info()[:4] == [1, 100, 310, 210]
    log.clear()                                            # clear resets the counter, as it did
    assert log.observe(shares[:3])[2] == [0, 1, 2] and log.get(1) == (shares[1], 1)
    assert log.retire_info()[:4] == [1, 100, 3, 3]
    log.close()


# ------------------------------------------------------------------- 4. sizes at which the passes can go wrong
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65536, 65537, 200003])
def test_sizes(n):
    shares, tags = rcases.synthetic(n)
    log = _log(n + 512, 7)
    status, _, _ = log.observe_raw(cases.pack(shares), tags)
    assert status == bytes(n)
    kept = [i for i in range(n) if i % 3 != 1]
    assert log.retire([1001]) == n - len(kept)
    info = log.info()
    assert info[:4] == [n + 512, len(kept), _slots(n + 512), len(kept)] and info[6] == 0
    assert log.retire_info()[:4] == [1, n - len(kept), n, len(kept)]
    for seq in sorted({kept[0], kept[-1], kept[len(kept) // 4], kept[len(kept) // 2], kept[3 * len(kept) // 4]}):
        assert log.get(seq) == (shares[seq], tags[seq]), seq
    rnd = random.Random(n)
    replays = [shares[rnd.randrange(n)] for _ in range(512)]
    retags = [9000000 + i for i in range(512)]
    want = _after([shares[i] for i in kept], [tags[i] for i in kept], replays, retags)
    assert log.observe_raw(cases.pack(replays), retags) == want
    if n > 2:
        assert {NEW, DUPLICATE} <= set(want[0])
    log.close()


def _slots(capacity):
    s = 16
    while s < 2 * capacity:
        s *= 2
    return s


# ------------------------------------------------------------------------------------ 5. the position pass alone
def _masks(n):
    rng = np.random.default_rng(1)
    run = np.zeros(n, np.uint8)
    run[n // 3:2 * n // 3 + 1] = 7
    alt = np.zeros(n, np.uint8)
    alt[::2] = 255
    return dict(all=np.full(n, 1, np.uint8), none=np.zeros(n, np.uint8), alternating=alt, run=run,
                random=(rng.integers(0, 2, n, dtype=np.uint8) * rng.integers(1, 256, n, dtype=np.uint8)).astype(np.uint8))


# 256-lane blocks: the levels change at 256, 65 536 and 2^24 items; 2^24 + 1 takes a fourth level
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 65535, 65536, 65537, 2 ** 24 + 1])
def test_positions_against_cumsum(n):
    from zerokit_amd._native import check, lib
    for name, keep in _masks(n).items():
        ones = (keep != 0).astype(np.uint32)
        want = np.cumsum(ones, dtype=np.uint32) - ones
        pos = np.full(n, 0xFFFFFFFF, np.uint32)
        kept = C.c_uint64(12345)
        check(lib().rlnamd_probe_log_positions(keep.ctypes.data, n, pos.ctypes.data, C.byref(kept)))
        assert kept.value == int(ones.sum(dtype=np.uint64)), name
        assert np.array_equal(pos, want), name
    kept = C.c_uint64(12345)
    check(lib().rlnamd_probe_log_positions(None, 0, None, C.byref(kept)))     # n = 0: no launch, nothing kept
    assert kept.value == 0


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_log_as_it_was():
    from zerokit_amd._native import lib
    shares, tags, _ = cases.stream()
    log, twin = _log(256, 9), _log(256, 9)
    for l in (log, twin):
        l.observe_raw(cases.pack(shares[:100]), tags[:100])
    h, ext = lib(), shares[0][3].to_bytes(32, "little")
    removed = C.c_uint64(777)
    assert h.rlnamd_nullifier_log_retire(log._h, None, 1, C.byref(removed)) != 0
    assert "null pointer" in h.rlnamd_last_error().decode()
    assert h.rlnamd_nullifier_log_retire(log._h, ext * 65, 65, C.byref(removed)) != 0
    assert "at most 64" in h.rlnamd_last_error().decode()
    assert h.rlnamd_nullifier_log_retire(log._h, ext + R.to_bytes(32, "little") + b"\xff" * 32, 3, C.byref(removed)) != 0
    assert "external nullifier 1 " in h.rlnamd_last_error().decode() and "not canonical" in h.rlnamd_last_error().decode()
    assert removed.value == 777
    assert log.info() == twin.info() and log.retire_info() == twin.retire_info()
    # k = 0 and an external nullifier nobody used: nothing is removed, and nothing observable changes
    assert log.retire([]) == 0 and log.retire([12345]) == 0 and log.retire([12345] * 64) == 0
    assert log.info() == twin.info()
    assert [log.get(i) for i in (0, 57, 99)] == [twin.get(i) for i in (0, 57, 99)]
    a = log.observe_raw(cases.pack(shares[100:256]), tags[100:256])
    assert a == twin.observe_raw(cases.pack(shares[100:256]), tags[100:256])
    assert a == tuple(p[n:] for p, n in zip(cases.flat(cases.model(shares[:256], tags[:256])), (100, 3200, 100)))
    assert log.info() == twin.info()
    assert log.retire_info()[:4] == [3, 0, 256, 256] and twin.retire_info()[:6] == [0, 0, 256, 256, 0, 0]
    log.close()
    twin.close()


# -------------------------------------------------------------------------------------------------------- 7. room
def test_a_retire_hands_the_room_back():
    from zerokit_amd._native import RLNError
    shares, tags = rcases.synthetic(1024, classes=2)
    log = _log(1024, 4)
    log.observe_raw(cases.pack(shares), tags)
    more = [(5000 + i, 1, 2, 1000) for i in range(600)]
    with pytest.raises(RLNError, match="do not fit"):
        log.observe(more[:1])
    removed = log.retire([1001])
    assert removed == 512 and log.info()[:4] == [1024, 512, 2048, 512]
    with pytest.raises(RLNError, match="do not fit"):
        log.observe(more[:removed + 1])
    assert log.observe(more[:removed]) == ([NEW] * removed, [0] * removed, list(range(1024, 1024 + removed)))
    with pytest.raises(RLNError, match="do not fit"):
        log.observe(more[removed:removed + 1])
    assert log.info()[:4] == [1024, 1024, 2048, 1024]
    # retiring everything leaves what clear leaves, but for the counter behind the default tags
    assert log.retire([1000, 1001]) == 1024
    assert log.info()[:4] == [1024, 0, 2048, 0]
    assert log.observe(more[:2]) == ([NEW, NEW], [0, 0], [1536, 1537])
    log.close()


# --------------------------------------------------------------------------------------------------------- 8. FFI
def _f(v):
    return int(v).to_bytes(32, "little")


def _vec(vals):
    return len(vals).to_bytes(8, "little") + b"".join(map(_f, vals))


def _v1(root, ext, x, ys, nulls, sel=None):
    if sel is None:
        return b"\x00" + _f(root) + _f(ext) + _f(x) + _f(ys) + _f(nulls)
    return b"\x01" + _f(root) + _f(ext) + _f(x) + _vec(ys) + _vec(nulls) + len(sel).to_bytes(8, "little") + bytes(sel)


def _v3(root, ext, x, ys, nulls, sel=None):
    if sel is None:
        return b"\x00" + _f(ys) + _f(root) + _f(nulls) + _f(x) + _f(ext)
    return b"\x01" + _vec(ys) + _f(root) + _vec(nulls) + _f(x) + _f(ext) + len(sel).to_bytes(8, "little") + bytes(sel)


def _shares_of(rows, tags):
    """-> (shares in slot order, their tags, the row each came from)"""
    shares, share_tags, owner = [], [], []
    for i, (root, ext, x, ys, nulls, sel) in enumerate(rows):
        slots = [(nulls, ys)] if sel is None else [(n, yy) for n, yy, s in zip(nulls, ys, sel) if s]
        for nul, yy in slots:
            shares.append((nul, x, yy, ext))
            share_tags.append(tags[i])
            owner.append(i)
    return shares, share_tags, owner


def _fold(verdicts, owner, n_rows):
    """the rule of the FFI layer: per proof the first of SPAM, FOREIGN, DUPLICATE, NEW among its shares"""
    out = []
    for i in range(n_rows):
        mine = [v for v, o in zip(verdicts, owner) if o == i]
        out.append(next(v for status in (SPAM, FOREIGN, DUPLICATE, NEW) for v in mine if v[0] == status))
    return out


@pytest.mark.parametrize("variant", ["v1", "v3"])
def test_ffi_retire_behind_observe_proof_values(variant):
    from zerokit_amd import public, public_v3
    rnd = random.Random(8)
    a0 = rnd.randrange(1, R)
    a1 = {nul: rnd.randrange(1, R) for nul in (42, 43, 600)}      # one line per message id, all through a0
    y = lambda nul, x: (a0 + x * a1[nul]) % R
    before = [
        (9, 77, 1111, [0, y(42, 1111), y(43, 1111), 0], [0, 42, 43, 0], [0, 1, 1, 0]),    # two slots under 77
        (9, 78, 4000, y(42, 4000), 42, None),                                            # 42 under 78: FOREIGN
        (9, 78, 5000, y(600, 5000), 600, None),                                          # new
    ]
    after = [
        (9, 78, 4500, y(42, 4500), 42, None),                                            # 42 again under 78
        (9, 78, 5000, [y(600, 5000), y(43, 5000), 0, 0], [600, 43, 0, 0], [1, 1, 0, 0]),  # 600 with its x, 43 anew
        (9, 77, 1111, [y(42, 1111), 0, 0, 0], [42, 0, 0, 0], [1, 0, 0, 0]),               # a late one under 77
    ]
    tags_before, tags_after = [100, 101, 102], [103, 104, 105]
    if variant == "v1":
        make = lambda r: public.RLNProofValues.from_bytes_le(_v1(*r))
        observe = public.observe_proof_values
    else:
        make = lambda r: public_v3.RLNProofValuesV3.from_bytes_le(_v3(*r))
        observe = public_v3.observe_proof_values
    s0, t0, o0 = _shares_of(before, tags_before)
    want0 = _fold(cases.model(s0, t0), o0, 3)
    assert [w[0] for w in want0] == [NEW, FOREIGN, NEW]
    kept = rcases.survivors(s0, t0, {77})
    assert len(kept) == 2
    s1, t1, o1 = _shares_of(after, tags_after)
    seen = {}
    cases.model([k[0] for k in kept], [k[1] for k in kept], seen)
    want1 = _fold(cases.model(s1, t1, seen), o1, 3)
    assert want1 == [(SPAM, a0, 101), (DUPLICATE, 0, 102), (FOREIGN, 0, 101)]
    log = _log(64, 3)
    status, secrets, first = observe(log, [make(r) for r in before], tags=tags_before)
    assert list(zip(status, secrets, first)) == want0
    assert public.retire_external_nullifiers(log, [77]) == 2
    assert log.info()[:4] == [64, 2, 128, 2]
    status, secrets, first = observe(log, [make(r) for r in after], tags=tags_after)
    assert list(zip(status, secrets, first)) == want1
    assert public.retire_external_nullifiers(log, []) == 0
    assert log.info()[1] == 6 and log.info()[6] == 0
    log.close()


# ------------------------------------------------------------------------------------- 9. the wipe is not disturbed
def test_a_retire_between_two_observes_does_not_disturb_the_wipe():
    flow = rcases.flow()
    shares, tags, _ = cases.stream()
    log = _log(N, 5)
    status, secrets, _ = log.observe_raw(cases.pack(shares[:HALF]), tags[:HALF])
    assert status.count(bytes([SPAM])) >= 50 and any(secrets) and log.info()[6] == 0
    assert log.retire([flow["ext"]]) == 1014
    assert log.info()[6] == 0
    status, secrets, _ = log.observe_raw(cases.pack(shares[HALF:HALF + 300]), tags[HALF:HALF + 300])   # a smaller call
    assert SPAM in status and any(secrets) and log.info()[6] == 0
    log.close()
