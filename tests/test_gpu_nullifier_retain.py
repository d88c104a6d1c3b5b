"""Retaining a window of epochs in the nullifier log on the device (rlnamd_nullifier_log_retain, ffi_nullifier_log_retain):
every record whose external nullifier is NOT in the set goes.  Judged by the model -- what a log owes afterwards is
what tests/nullifier_log_cases.py says when it has seen only the survivors (tests/relay_window_cases.retained) -- and by
a twin log with the same seed that retires the complement, which must end up equal in every record and in every counter that is a function of what the log holds
(_same_counters says which two are not)."""
import random

import pytest

import nullifier_log_cases as cases
import nullifier_retire_cases as rcases
import relay_window_cases as wcases
from nullifier_log_cases import DUPLICATE, NEW

pytestmark = pytest.mark.gpu

HALF = rcases.HALF


def _log(capacity, seed=0):
    from zerokit_amd.batch import NullifierLog
    return NullifierLog(capacity, seed)


def _after(kept, shares, tags):
    """the model's verdicts on `shares` in a log that holds kept = [(share, tag, seq)] -> what observe_raw returns"""
    seen = {}
    cases.model([k[0] for k in kept], [k[1] for k in kept], seen)
    return cases.flat(cases.model(shares, tags, seen))


def _records(log):
    from zerokit_amd._native import RLNError
    out = []
    for seq in range(log.retire_info()[2]):
        try:
            out.append(log.get(seq))
        except RLNError as e:
            out.append(str(e))
    return out


def _same_counters(a, b):
    """info and retire_info of twin logs, field by field.  Two fields are not functions of what a log holds: info[5],
    the longest probe walk so far, and retire_info[4], the longest walk of the last rebuild.  Which of two colliding
    keys takes the nearer slot is decided by the order in which lanes win their compare-and-swap, in the observe that
    filled BOTH logs as much as in the rebuild, so two runs of the same calls may differ in them (seen on the device:
    5 against 6).  They are held to their range -- at least one slot, at most the table -- and every other field to
    equality."""
    ia, ib, ra, rb = a.info(), b.info(), a.retire_info(), b.retire_info()
    assert ia[:5] + ia[6:] == ib[:5] + ib[6:] and ia[6] == 0
    assert ra[:4] + ra[5:] == rb[:4] + rb[5:]
    for walk in (ia[5], ib[5], ra[4], rb[4]):
        assert 1 <= walk <= ia[2]


def test_the_retire_flow_from_the_other_side():
    """the 4 096-share stream: retaining the second of its two external nullifiers leaves flow()["kept"] and then
    answers flow()["second"]"""
    flow = rcases.flow()
    shares, tags, _ = cases.stream()
    other = next(s[3] for s in shares if s[3] != flow["ext"])
    log = _log(len(shares), 5)
    try:
        assert log.observe_raw(cases.pack(shares[:HALF]), tags[:HALF]) == cases.flat(flow["first"])
        assert log.retain([other]) == HALF - len(flow["kept"])
        assert [log.get(q) for _s, _t, q in flow["kept"]] == [(s, t) for s, t, _q in flow["kept"]]
        assert log.observe_raw(cases.pack(shares[HALF:]), tags[HALF:]) == cases.flat(flow["second"])
        info = log.info()
        assert info[1] == len(flow["kept"]) + HALF and info[3] == flow["distinct"] and info[6] == 0
        assert log.retire_info()[:4] == [1, HALF - len(flow["kept"]), len(shares), info[1]] and log.retire_info()[5] == 1
    finally:
        log.close()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65537])
def test_sizes(n):
    """one lane, one workgroup and its two neighbours, the scan's second level: records under 5 external nullifiers,
    2 retained"""
    shares, tags = wcases.synthetic_log(n, 5)
    window = [1003, 1001]
    log = _log(n + 512, 7)
    try:
        assert log.observe_raw(cases.pack(shares), tags)[0] == bytes(n)
        kept = wcases.retained(shares, tags, window)
        assert log.retain(window) == n - len(kept)            # the room handed back
        info = log.info()
        assert info[:2] == [n + 512, len(kept)] and info[3] == len(kept) and info[6] == 0
        assert log.retire_info()[:4] == [1, n - len(kept), n, len(kept)]
        for j in sorted({0, len(kept) // 3, len(kept) // 2, len(kept) - 1} if kept else ()):
            assert log.get(kept[j][2]) == kept[j][:2]
        rnd = random.Random(n)
        replays = [shares[rnd.randrange(n)] for _ in range(512)]
        retags = [9000000 + i for i in range(512)]
        want = _after(kept, replays, retags)
        assert log.observe_raw(cases.pack(replays), retags) == want
        if n > 2:
            assert {NEW, DUPLICATE} <= set(want[0])
        assert log.info()[6] == 0                             # the result buffers are clean after the observe
        assert log.info()[1] == len(kept) + 512               # ... which had the room the retain handed back
    finally:
        log.close()


@pytest.mark.parametrize("k", [1, 32, 33, 64])
def test_set_sizes_with_the_only_match_last(k):
    """the set goes to LDS as k * 8 words over 256 lanes: 32 is the last set that takes one trip, 33 the first that
    takes two; the only element any record carries is the last of the set"""
    n = 777
    shares, tags = wcases.synthetic_log(n, 3)
    window = [5000 + j for j in range(k - 1)] + [1002]
    log = _log(n, 11)
    try:
        log.observe_raw(cases.pack(shares), tags)
        kept = wcases.retained(shares, tags, window)
        assert len(kept) == n // 3 and log.retain(window) == n - len(kept)
        assert [r for r in _records(log) if not isinstance(r, str)] == [kept_row[:2] for kept_row in kept]
        assert log.info()[1] == len(kept) and log.info()[3] == len(kept)
    finally:
        log.close()


@pytest.mark.parametrize("n,classes,k", [(3000, 70, 6), (3000, 70, 64), (65537, 9, 2)])
def test_retain_equals_retire_of_the_complement_on_twin_logs(n, classes, k):
    shares, tags = wcases.synthetic_log(n, classes)
    # nullifiers that come back under the next external nullifier, so that "the first record" moves
    again = [(s[0], s[1] + 1, s[2], 1000 + (i + 1) % classes) for i, s in enumerate(shares[:500])]
    shares, tags = list(shares) + again, list(tags) + [7 * i for i in range(len(again))]
    window = [1000 + classes - 1 - j for j in range(k)]
    if k == 64:
        window[5] = window[6]                                 # a duplicate in the set is not an error
    outside = sorted({s[3] for s in shares} - set(window))
    assert 1 <= len(outside) <= 64
    a, b = _log(len(shares) + 600, 77), _log(len(shares) + 600, 77)
    try:
        for log in (a, b):
            log.observe_raw(cases.pack(shares), tags)
        gone = a.retain(window)
        assert gone == b.retire(outside) == len(shares) - len(wcases.retained(shares, tags, window))
        _same_counters(a, b)
        assert a.retire_info()[:2] == [1, gone]
        if n < 10000:
            assert _records(a) == _records(b)
        else:
            for seq in (0, 1, 2, 4095, 4096, n - 1, n, len(shares) - 1):
                ra = rb = None
                try:
                    ra = a.get(seq)
                except Exception as e:   # retired: both must say so
                    ra = str(e)
                try:
                    rb = b.get(seq)
                except Exception as e:
                    rb = str(e)
                assert ra == rb
        more = [(s[0], s[1] + 2, s[2] + 2, s[3]) for s in shares[::max(1, len(shares) // 500)]]
        assert a.observe_raw(cases.pack(more), None) == b.observe_raw(cases.pack(more), None)
        _same_counters(a, b)
    finally:
        a.close()
        b.close()


def test_many_strangers_go_in_one_call():
    """the set has no size limit on the removed side: 200 distinct external nullifiers, 3 retained"""
    shares, tags = wcases.synthetic_log(1000, 200)
    window = [1199, 1000, 1057]
    log = _log(1000, 9)
    try:
        log.observe_raw(cases.pack(shares), tags)
        assert log.retain(window) == 1000 - 15
        assert [r for r in _records(log) if not isinstance(r, str)] == [r[:2] for r in wcases.retained(shares, tags, window)]
        assert log.retain(window) == 0 and log.retire_info()[:2] == [2, 985]
    finally:
        log.close()


def test_refusals_leave_the_log_as_it_was():
    from zerokit_amd._native import RLNError
    shares, tags = wcases.synthetic_log(300, 3)
    log = _log(512, 3)
    try:
        log.observe_raw(cases.pack(shares), tags)
        before = (log.info(), log.retire_info(), _records(log))
        for window, text in (([], "use clear"), ([1] * 65, "at most 64 external nullifiers a call, not 65"),
                             ([1001, 1002, cases.R], "external nullifier 2 of the retain is not canonical"),
                             (None, "null pointer for k > 0")):
            with pytest.raises(RLNError, match=text):
                if window is None:
                    _retain_raw(log, None, 2)
                else:
                    _retain_raw(log, b"".join(int(v).to_bytes(32, "little") for v in window), len(window))
        assert (log.info(), log.retire_info(), _records(log)) == before
        assert before[1][5] == 0 and log.retain([1000, 1001, 1002]) == 0    # a set every record matches: nothing moves
        assert log.retain([1001]) == 200 and log.retire_info()[:2] == [2, 200] and log.retire_info()[5] == 1
    finally:
        log.close()


def _retain_raw(log, raw, k):
    import ctypes as C
    from zerokit_amd._native import check, lib
    removed = C.c_uint64()
    check(lib().rlnamd_nullifier_log_retain(log._h, raw, k, C.byref(removed)))
    return removed.value


def test_the_drop_in_entry():
    from zerokit_amd import RLNError, public
    shares, tags = wcases.synthetic_log(30, 3)
    log = _log(64, 3)
    try:
        log.observe_raw(cases.pack(shares), tags)
        assert public.retain_external_nullifiers(log, [1002, 1000]) == 10
        assert log.info()[1] == 20 and log.retire_info()[:2] == [1, 10]
        with pytest.raises(RLNError, match="use clear"):
            public.retain_external_nullifiers(log, [])
        assert log.info()[1] == 20
    finally:
        log.close()
