"""The nullifier log on the device (rlnamd_nullifier_log_*, ffi_nullifier_log_observe and its V3 twin), judged byte for
byte by the model of tests/nullifier_log_cases.py: a dict from nullifier to the first share, shares taken in index
order, secrets from the oracle's compute_id_secret.  The shares are real line shares, so every SPAM secret is also the
member's a0."""
import ctypes as C
import random

import pytest

import nullifier_log_cases as cases
from nullifier_log_cases import DUPLICATE, FOREIGN, NEW, R, SKIPPED, SPAM

pytestmark = pytest.mark.gpu

N = 4096


def _log(capacity, seed=0):
    from zerokit_amd.batch import NullifierLog
    return NullifierLog(capacity, seed)


def _observe_chunks(log, chunk):
    shares, tags, _ = cases.stream()
    packed = cases.pack(shares)
    got = (b"", b"", [])
    for o in range(0, N, chunk):
        part = log.observe_raw(packed[128 * o:128 * (o + chunk)], tags[o:o + chunk])
        got = tuple(a + b for a, b in zip(got, part))
    return got


@pytest.fixture(scope="module")
def one_call():
    """the whole stream in a single call into a log with seed 5 -> (outputs, info after the call, a few records)"""
    log = _log(N, 5)
    got = _observe_chunks(log, N)
    info = log.info()
    records = {i: log.get(i) for i in (0, 1, 255, 256, 2047, N - 1)}
    log.close()
    return got, info, records


# ------------------------------------------------------------------------------------------------ 1. model parity
def test_model_parity(one_call):
    want = cases.expected()       # asserts first that the model meets each of the four statuses at least 50 times
    shares, tags, _ = cases.stream()
    assert shares[0][0] == shares[N - 1][0]     # one nullifier in the first and in the last workgroup
    got, info, records = one_call
    status, secrets, first = cases.flat(want)
    assert got[0] == status
    assert got[1] == secrets
    assert got[2] == first
    for i, rec in records.items():
        assert rec == (shares[i], tags[i]), i
    distinct = sum(1 for w in want if w[0] == NEW)
    assert info[:5] == [N, N, 2 * N, distinct, 1] and 1 <= info[5] <= 2 * N and info[7] == 5


# ------------------------------------------------------------------------------------------- 2. split invariance
@pytest.mark.parametrize("chunk", [1, 63, 64, 65, 257, 1000])
def test_split_invariance(one_call, chunk):
    log = _log(N, 5)
    assert _observe_chunks(log, chunk) == one_call[0]
    assert log.info()[:5] == one_call[1][:4] + [(N + chunk - 1) // chunk]
    log.close()


def test_the_seed_moves_slots_not_verdicts(one_call):
    shares, _, _ = cases.stream()
    a, b = _log(N, 5), _log(N, 6)
    assert [a.home_slot(s[0]) for s in shares[:64]] != [b.home_slot(s[0]) for s in shares[:64]]
    assert _observe_chunks(b, N) == one_call[0]
    drawn = _log(16)                 # seed 0: drawn at construction, reported by info
    assert drawn.info()[7] != 0
    for log in (a, b, drawn):
        log.close()


# ---------------------------------------------------------------------------------- 3. collisions and wrap-around
def test_collisions_and_wrap_around():
    rnd = random.Random(31)
    log = _log(16, 1)
    assert log.info()[2] == 32
    colliding, spread = [], {}
    while len(colliding) < 8 or len(spread) < 8:
        nul = rnd.randrange(1, R)
        h = log.home_slot(nul)
        if h == 31 and len(colliding) < 8:
            colliding.append(nul)
        elif h != 31 and h not in spread and len(spread) < 8:
            spread[h] = nul
    ext = 7
    lines = {nul: (rnd.randrange(1, R), rnd.randrange(1, R)) for nul in colliding}
    share = lambda nul, x: (nul, x, (lines[nul][0] + x * lines[nul][1]) % R, ext)
    first = [share(nul, 1000 + k) for k, nul in enumerate(colliding)]
    second = [share(nul, 2000 + k) for k, nul in enumerate(colliding)]
    # eight keys with home slot 31, the last slot: seven of them wrap around to slots 0 .. 6
    assert log.observe(first) == ([NEW] * 8, [0] * 8, list(range(8)))
    status, secrets, tags = log.observe(second)
    assert status == [SPAM] * 8
    assert secrets == [lines[nul][0] for nul in colliding]
    assert secrets == [w[1] for w in cases.model(first + second, range(16))[8:]]
    assert tags == list(range(8))
    assert log.info()[5] >= 8
    log.close()
    # eight keys with eight different home slots: nobody walks
    log = _log(16, 1)
    assert log.observe([(nul, 5, 6, ext) for nul in spread.values()])[0] == [NEW] * 8
    assert log.info()[5] == 1
    log.close()


# ----------------------------------------------------------------------------- 4. refusals leave the log as it was
def test_refusals_leave_the_log_as_it_was():
    from zerokit_amd._native import RLNError, lib
    shares, tags, _ = cases.stream()
    full = _log(64, 9)
    want = cases.flat(cases.model(shares[:64], tags[:64]))
    assert full.observe_raw(cases.pack(shares[:64]), tags[:64]) == want
    before = full.info()
    with pytest.raises(RLNError, match="do not fit"):
        full.observe(shares[64:65])
    assert full.info()[:6] == before[:6]
    assert full.observe([]) == ([], [], [])          # n = 0 succeeds, also in a full log
    assert full.info()[:6] == before[:6]
    full.close()

    log = _log(64, 9)
    assert log.observe_raw(cases.pack(shares[:10]), tags[:10]) == cases.flat(cases.model(shares[:10], tags[:10]))
    before = log.info()
    bad = list(shares[10:15])
    bad[3] = (bad[3][0], R, bad[3][2], bad[3][3])     # x = r
    with pytest.raises(RLNError, match="share 3 "):
        log.observe_raw(cases.pack(bad), tags[10:15])
    assert log.info()[:6] == before[:6]
    with pytest.raises(RLNError, match="do not fit"):
        log.observe_raw(cases.pack(shares[10:65]), tags[10:65])
    assert log.info()[:6] == before[:6]
    status = C.create_string_buffer(1)
    assert lib().rlnamd_nullifier_log_observe(log._h, 1, None, None, status, None, None) != 0
    assert "null pointer" in lib().rlnamd_last_error().decode()
    assert log.info()[:6] == before[:6]
    # a later valid call behaves as if the bad ones had never been made
    assert log.observe_raw(cases.pack(shares[10:64]), tags[10:64]) == tuple(p[n:] for p, n in zip(want, (10, 320, 10)))
    with pytest.raises(RLNError, match="no record 64"):
        log.get(64)
    log.close()
    for capacity in (0, 2 ** 31 + 1):
        with pytest.raises(RLNError, match="capacity"):
            _log(capacity)


# ----------------------------------------------------------------------------------------- 5. secrets do not stay
def test_secrets_do_not_stay(one_call):
    assert one_call[1][6] == 0               # after the call that recovered a thousand secrets
    shares, tags, _ = cases.stream()
    log = _log(N, 5)
    status, secrets, _ = log.observe_raw(cases.pack(shares), tags)
    assert status.count(bytes([SPAM])) >= 50 and any(secrets)
    assert log.info()[6] == 0
    log.clear()
    info = log.info()
    assert info[1] == 0 and info[3] == 0 and info[7] == 5
    # the stream's first 100 shares again: what a fresh log says, every nullifier's first sight NEW again
    again = log.observe_raw(cases.pack(shares[:100]), tags[:100])
    assert again == cases.flat(cases.model(shares[:100], tags[:100]))
    firsts = [i for i in range(100) if shares[i][0] not in {s[0] for s in shares[:i]}]
    assert len(firsts) > 50 and all(again[0][i] == NEW for i in firsts)
    assert SPAM in again[0] and log.info()[6] == 0      # also behind a call smaller than the one before
    log.close()


# ------------------------------------------------------------------------------------------------------- 6. FFI
def _f(v):
    return int(v).to_bytes(32, "little")


def _vec(vals):
    return len(vals).to_bytes(8, "little") + b"".join(map(_f, vals))


def _v1(root, ext, x, ys, nulls, sel=None):
    """RLNProofValues bytes: a single message (sel None: ys and nulls are the one y and nullifier) or the multi_bytes
    shape of tests/test_cabi_host.py"""
    if sel is None:
        return b"\x00" + _f(root) + _f(ext) + _f(x) + _f(ys) + _f(nulls)
    return b"\x01" + _f(root) + _f(ext) + _f(x) + _vec(ys) + _vec(nulls) + len(sel).to_bytes(8, "little") + bytes(sel)


def _v3(root, ext, x, ys, nulls, sel=None):
    if sel is None:
        return b"\x00" + _f(ys) + _f(root) + _f(nulls) + _f(x) + _f(ext)
    return b"\x01" + _vec(ys) + _f(root) + _vec(nulls) + _f(x) + _f(ext) + len(sel).to_bytes(8, "little") + bytes(sel)


def _ffi_case():
    """-> (rows of (root, ext, x, ys, nulls, sel), take, tags, the member's a0)"""
    rnd = random.Random(6)
    a0 = rnd.randrange(1, R)
    a1 = {nul: rnd.randrange(1, R) for nul in (42, 43, 99, 500, 600, 700)}    # one line per message id, all through a0
    y = lambda nul, x: (a0 + x * a1[nul]) % R
    rows = [
        (9, 77, 1111, [0, y(42, 1111), y(43, 1111), 0], [0, 42, 43, 0], [0, 1, 1, 0]),       # 0: two first sights
        (9, 77, 2222, [y(42, 2222), 0, 0, y(99, 2222)], [42, 0, 0, 99], [1, 0, 0, 1]),       # 1: 42 again, 99 new
        (9, 77, 3333, y(43, 3333), 43, None),                                               # 2: 43 in a single proof
        (9, 78, 4000, y(42, 4000), 42, None),                                               # 3: 42, another ext
        (9, 77, 4444, y(42, 4444), 42, None),                                               # 4: not taken
        (9, 77, 5555, y(500, 5555), 500, None),                                             # 5: new
        (9, 77, 5555, y(500, 5555), 500, None),                                             # 6: the same message again
        (9, 77, 6666, y(500, 6666), 500, None),                                             # 7: 500, another message
        (9, 77, 1111, [y(700, 1111), y(42, 1111), 0, 0], [700, 42, 0, 0], [1, 1, 0, 0]),     # 8: 700 new, 42 with its first x
    ]
    take = [True] * 9
    take[4] = False
    return rows, take, [100 + i for i in range(9)], a0


def _fold(rows, take, tags):
    """the rule of the FFI layer over the model: shares in slot order, the first of SPAM, FOREIGN, DUPLICATE, NEW"""
    shares, share_tags, owner = [], [], []
    for i, (root, ext, x, ys, nulls, sel) in enumerate(rows):
        if not take[i]:
            continue
        slots = [(nulls, ys)] if sel is None else [(n, yy) for n, yy, s in zip(nulls, ys, sel) if s]
        for nul, yy in slots:
            shares.append((nul, x, yy, ext))
            share_tags.append(tags[i])
            owner.append(i)
    verdicts = cases.model(shares, share_tags)
    out = [(SKIPPED, 0, 0)] * len(rows)
    for i in range(len(rows)):
        mine = [v for v, o in zip(verdicts, owner) if o == i]
        for status in (SPAM, FOREIGN, DUPLICATE, NEW):
            hit = [v for v in mine if v[0] == status]
            if hit:
                out[i] = hit[0]
                break
    return out, len(shares)


@pytest.mark.parametrize("variant", ["v1", "v3"])
def test_ffi_observe_proof_values(variant):
    from zerokit_amd import public, public_v3
    from zerokit_amd._native import RLNError
    rows, take, tags, a0 = _ffi_case()
    if variant == "v1":
        values = [public.RLNProofValues.from_bytes_le(_v1(*r)) for r in rows]
        observe = public.observe_proof_values
        recover = public.recover_id_secret
    else:
        values = [public_v3.RLNProofValuesV3.from_bytes_le(_v3(*r)) for r in rows]
        observe = public_v3.observe_proof_values
        recover = lambda a, b: a.recover_secret(b)
    want, n_shares = _fold(rows, take, tags)
    assert [w[0] for w in want] == [NEW, SPAM, SPAM, FOREIGN, SKIPPED, NEW, DUPLICATE, SPAM, DUPLICATE]
    assert [w[1] for w in want] == [0, a0, a0, 0, 0, 0, 0, a0, 0]
    assert [w[2] for w in want] == [100, 100, 100, 100, 0, 105, 105, 105, 100]
    log = _log(64, 3)
    status, secrets, first = observe(log, values, take=take, tags=tags)
    assert list(zip(status, secrets, first)) == want
    assert log.info()[1] == n_shares == 11           # the proof that was not taken left no record
    # against an earlier proof of the same variant, the secret is recover_id_secret's
    for i, f in ((1, 0), (7, 5)):
        assert secrets[i] == recover(values[f], values[i])
    # no take, no tags: every proof counts, a first tag is the sequence number of the first record with the nullifier
    log2 = _log(64, 3)
    status, secrets, first = observe(log2, values)
    want2, n2 = _fold(rows, [True] * 9, [None] * 9)
    assert status == [w[0] for w in want2] and status[4] == SPAM and secrets[4] == a0 and n2 == 12
    assert first[:4] == [0, 0, 1, 0] and first[5:8] == [7, 7, 7]
    # a call that does not fit is an error and leaves no record
    small = _log(4, 3)
    with pytest.raises(RLNError, match="do not fit"):
        observe(small, values)
    assert small.info()[1] == 0
    assert observe(small, []) == ([], [], [])
    for l in (log, log2, small):
        l.close()


# ----------------------------------------------------------------------------------------------- 7. real proofs
def test_real_proofs_verified_then_observed():
    """three members, each proving two signals under one external nullifier and one message id, member 0 once more with
    another message id: verified on the device, then observed with take = ok"""
    from oracle.pyref.poseidon import poseidon
    from zerokit_amd import public
    from zerokit_amd.batch import BatchProver, PoseidonTree
    rnd = random.Random(77)
    limit, leaves = 100, [3, 1 << 19, (1 << 20) - 1]
    a0 = [rnd.randrange(1, R) for _ in leaves]
    tree = PoseidonTree(20)
    tree.set_leaves([(leaf, poseidon([poseidon([s]), limit])) for leaf, s in zip(leaves, a0)])
    ext = rnd.randrange(1, R)
    who = [0, 1, 2, 0, 1, 2, 0]
    ws = [dict(identity_secret=a0[m], user_message_limit=limit, message_id=2 if i == 6 else 1, x=rnd.randrange(1, R),
               external_nullifier=ext) for i, m in enumerate(who)]
    rs = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in who]
    prover = BatchProver(max_batch=64, window_bits=8)
    out = prover.prove_members(tree, [leaves[m] for m in who], ws, rs)
    assert all(o["error"] == 0 for o in out)
    ok = prover.verify_many_gpu([o["proof"] for o in out], [o["public_inputs"] for o in out])
    assert ok == [True] * 7
    values = [public.RLNProofValues.from_bytes_le(
        _v1(o["values"]["root"], o["values"]["external_nullifier"], o["values"]["x"], o["values"]["y"],
            o["values"]["nullifier"])) for o in out]
    log = _log(16)
    status, secrets, first = public.observe_proof_values(log, values, take=ok, tags=list(range(50, 57)))
    assert status == [NEW, NEW, NEW, SPAM, SPAM, SPAM, NEW]
    assert secrets == [0, 0, 0] + a0 + [0]
    assert first == [50, 51, 52, 50, 51, 52, 56]
    log.close()
    prover.close()
    tree.close()
