"""The optimistic form of the device verifier (zerokit_amd/csrc/verify_agg.hip: rlnamd_verify_many_gpu_optimistic,
rlnamd_verify_gpu_aggregate, the "verify_optimistic" config key): the combined value against the host twin
rlnamd_verify_aggregate_with_zkey byte for byte, the verdicts against rlnamd_verify_many on host threads, and the
bookkeeping (accepted / fell back / cool-down) through the counters, not through timing."""
import ctypes as C
import json
import random
import statistics
import time

import pytest

import verify_cases as vc
from test_gpu_verify import chunk_size, host_verdicts, raw
from test_verify_agg_host import mixed_rows
from verify_cases import GT_ONE, le

pytestmark = pytest.mark.gpu
TOP = (1 << 128) - 1
PREPARE_REJECTS = {"input_eq_r", "input_max", "A_off_curve", "C_off_curve", "A_noncanonical_x", "B_outside_subgroup"}


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64)
    yield p
    p.close()


@pytest.fixture(autouse=True)
def _quiet(request):
    """every test starts outside a cool-down and with the default setting"""
    if "prover" in request.fixturenames:
        p = request.getfixturevalue("prover")
        p.verify_set_cooldown(0)
        p.verify_set_cooldown(16)
    yield


def rows_of(cases):
    return [(c[1], b"".join(raw(v) for v in c[2])) for c in cases]


def named_rejects(case):
    return dict((nm.split("/")[1], (pr, b"".join(raw(v) for v in pu))) for nm, pr, pu in vc.rejects(*case))


def join(rows):
    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)


def scalar_bytes(scalars):
    return b"".join(int(s).to_bytes(16, "little") for s in scalars)


def gpu_aggregate(p, rows, scalars, nv=5):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    pr, va = join(rows)
    gt, rej = C.create_string_buffer(384), C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1))
    check(lib().rlnamd_verify_gpu_aggregate(p._h, n, pr, va, nv, scalar_bytes(scalars), gt, rej))
    return gt.raw, rej.raw[:n]


def host_aggregate(zkey, rows, scalars, nv=5):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    pr, va = join(rows)
    gt, rej = C.create_string_buffer(384), C.create_string_buffer(max(n, 1))
    check(lib().rlnamd_verify_aggregate_with_zkey(zkey, len(zkey), n, pr, va, nv, scalar_bytes(scalars), gt, rej))
    return gt.raw, rej.raw[:n]


def optimistic(p, rows, scalars=None, nv=5):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    pr, va = join(rows)
    ok = C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1))
    check(lib().rlnamd_verify_many_gpu_optimistic(p._h, n, pr, va, nv, None if scalars is None else scalar_bytes(scalars),
                                                  ok))
    return ok.raw[:n]


def delta(p, fn):
    """(result of fn, change of the optimistic counters, change of the exact passes)"""
    s0, p0 = p.verify_optimistic_stats(), p.verify_gpu_passes()
    out = fn()
    s1, p1 = p.verify_optimistic_stats(), p.verify_gpu_passes()
    return out, {k: s1[k] - s0[k] for k in s0}, (p1[0] - p0[0], p1[1] - p0[1])


def fold_rows(base, n):
    """n rows from `base`: rows 64 g .. 64 g + 63 alternate between two of them, so that every slot meets an identical
    row in the first five steps of the fold and a different one in the last"""
    return [base[(i // 64 + (i & 1)) % len(base)] for i in range(n)]


def fold_scalars(n, seed):
    """seeded scalars: every third group of 64 has ONE scalar (identical rows under equal scalars: the doubling branch
    of the G1 fold), the first is 1 and the last 2^128 - 1"""
    rnd = random.Random(seed)
    sc = []
    for g in range(-(-n // 64)):
        same = rnd.randrange(1, 1 << 128)
        sc += [same if g % 3 == 0 else rnd.randrange(1, 1 << 128) for _ in range(64)]
    sc = sc[:n]
    sc[0] = 1
    if n > 1:
        sc[-1] = TOP
    return sc


def test_aggregate_value_equals_the_host_twin_depth20(prover):
    """1. rlnamd_verify_gpu_aggregate == rlnamd_verify_aggregate_with_zkey, value and reject flags, around one
    workgroup, at two and three fold levels and across a chunk boundary; all-valid rows give 1, and with damaged rows
    (a changed input, A and C swapped, A at infinity, an x off the curve) in between the value is not 1"""
    g = vc.golden_h20()
    base = rows_of(g)
    rj = named_rejects(g[2])
    damaged = [rj["input0"], rj["swapAC"], rj["A_infinity"], rj["A_off_curve"]]
    z = vc.zkey_bytes(20)
    for n in (1, 2, 63, 64, 65, 4096, 4097, chunk_size() + 1):
        rows, sc = fold_rows(base, n), fold_scalars(n, seed=n)
        got = gpu_aggregate(prover, rows, sc)
        assert got == (GT_ONE, bytes(n)), n
        if n <= 65 or n == 4097:
            assert got == host_aggregate(z, rows, sc), n
        for k, i in enumerate(range(n // 2, n, 97)):
            rows[i] = damaged[k % 4]
        got = gpu_aggregate(prover, rows, sc)
        want = host_aggregate(z, rows, sc)
        assert got[1] == want[1] and got[0] == want[0], n
        assert got[0] != GT_ONE, n


@pytest.mark.parametrize("depth,multi", [(10, False), (20, True)])
def test_aggregate_value_other_circuits(depth, multi):
    """1. on the other two shipped circuits (n_values differs): their golden proof, whole and with a changed input"""
    from zerokit_amd.batch import BatchProver
    golden = [(nm, pr, pu) for nm, d, m, pr, pu in vc.golden_other() if (d, m) == (depth, multi)][0]
    nv = len(golden[2])
    good = rows_of([golden])[0]
    bad = named_rejects(golden)["input%d" % (nv - 1)]
    z = vc.zkey_bytes(depth, multi)
    p = BatchProver(max_batch=64, depth=depth, multi=multi)
    try:
        assert p.num_public == nv and (nv > 5) == multi
        for n in (1, 2, 63, 64, 65):
            sc = fold_scalars(n, seed=100 + n)
            rows = [good] * n
            assert gpu_aggregate(p, rows, sc, nv) == (GT_ONE, bytes(n)), n
            rows[n // 2] = bad
            got = gpu_aggregate(p, rows, sc, nv)
            assert got == host_aggregate(z, rows, sc, nv), n
            assert got[0] != GT_ONE
    finally:
        p.close()


def test_all_valid_rows_take_no_exact_pass(prover):
    """2. 4 097 valid rows: all verdicts 1, one combined check accepted, no fallback, rlnamd_verify_gpu_passes unmoved"""
    rows = fold_rows(rows_of(vc.golden_h20()), 4097)
    ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
    assert ok == b"\x01" * 4097
    assert (d["combined"], d["accepted"], d["fell_back"], d["skipped_in_cooldown"], d["refused_proofs"]) == (1, 1, 0, 0, 0)
    assert passes == (0, 0)
    assert prover.verify_many_gpu_optimistic([vc.golden_h20()[0][1]] * 1100, [vc.golden_h20()[0][2]] * 1100) == [True] * 1100


@pytest.mark.parametrize("at,kind", [(0, "swapAC"), (2048, "input0"), (4096, "swapAC")])
def test_one_damaged_proof_falls_back_and_cools_down(prover, at, kind):
    """3. one row the pairing rejects among 4 097: the verdicts are the host's, the call falls back, the next `cooldown`
    calls skip the combined check and run exact passes, the call after them is combined again; with cool-down 0 every
    call is combined"""
    g = vc.golden_h20()
    rows = fold_rows(rows_of(g), 4097)
    rows[at] = named_rejects(g[1])[kind]
    want = bytearray(b"\x01" * 4097)
    want[at] = 0
    assert host_verdicts(prover, *join(rows[at:at + 1] + rows[5:8]), 5) == b"\x00\x01\x01\x01"
    prover.verify_set_cooldown(3)
    ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
    assert ok == bytes(want)
    assert (d["combined"], d["accepted"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 0, 1, 0) and passes == (1, 0)
    assert prover.verify_optimistic_stats()["cooldown_left"] == 3
    for _ in range(3):
        ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
        assert ok == bytes(want)
        assert (d["combined"], d["fell_back"], d["skipped_in_cooldown"]) == (0, 0, 1) and passes == (1, 0)
    ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
    assert ok == bytes(want) and (d["combined"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 1, 0)
    prover.verify_set_cooldown(0)
    for _ in range(2):
        ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
        assert ok == bytes(want) and (d["combined"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 1, 0)


def test_rows_that_prepare_rejects_are_named_without_a_fallback(prover):
    """4. every case of rejects() that the per-proof checks refuse, between valid rows: verdicts equal the host's, the
    counter counts them, the combined check accepts the rest (no fallback).  A, B and C at infinity are decided by the
    pairing: verdicts equal the host's, whichever path decides them"""
    g = vc.golden_h20()
    rows = fold_rows(rows_of(g), 1100)
    want = bytearray(b"\x01" * 1100)
    at = 7
    for case in g[:3]:
        rj = named_rejects(case)
        assert PREPARE_REJECTS <= set(rj)
        for name in sorted(PREPARE_REJECTS):
            rows[at] = rj[name]
            want[at] = 0
            at += 53
    refused = 3 * len(PREPARE_REJECTS)
    pr, va = join(rows)
    assert host_verdicts(prover, pr, va, 5) == bytes(want)
    _, rej = host_aggregate(vc.zkey_bytes(20), rows, [1] * 1100)
    assert rej == bytes(1 - v for v in want)      # it is the per-proof checks that refuse them
    ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
    assert ok == bytes(want)
    assert (d["combined"], d["accepted"], d["fell_back"], d["refused_proofs"]) == (1, 1, 0, refused) and passes == (0, 0)
    rj = named_rejects(g[4])
    for k, name in enumerate(("A_infinity", "B_infinity", "C_infinity")):
        rows[500 + k] = rj[name]
    pr, va = join(rows)
    host = host_verdicts(prover, pr, va, 5)
    assert host[500:503] == b"\x00\x00\x00"
    assert optimistic(prover, rows) == host


def test_cancelling_pair_needs_independent_scalars(prover):
    """5. two valid proofs with C_1 + T and C_2 - T (T the G1 generator): each is invalid, their product under EQUAL
    scalars is 1 -- the combined value with supplied scalars all 1 is 1 -- and under drawn scalars the check rejects
    and the exact pass names both, as the host does"""
    from oracle.pyref import arkzkey
    from oracle.pyref import bn254 as o
    g = vc.golden_h20()
    pair = []
    for case, t in ((g[0], o.G1_GEN), (g[1], o.G1.neg(o.G1_GEN))):
        A, B, Cp = arkzkey.proof_decompress(case[1])
        pair.append((arkzkey.proof_compress(A, B, o.G1.add(Cp, t)), b"".join(le(v) for v in case[2])))
    assert host_verdicts(prover, *join(pair), 5) == b"\x00\x00"
    assert gpu_aggregate(prover, pair, [1, 1]) == (GT_ONE, b"\x00\x00")
    assert gpu_aggregate(prover, pair, [1, 2])[0] != GT_ONE
    assert optimistic(prover, pair) == b"\x00\x00"
    rows = fold_rows(rows_of(g), 1100)
    rows[10], rows[700] = pair
    assert gpu_aggregate(prover, rows, [1] * 1100)[0] == GT_ONE
    want = bytearray(b"\x01" * 1100)
    want[10] = want[700] = 0
    prover.verify_set_cooldown(0)
    ok, d, _ = delta(prover, lambda: optimistic(prover, rows))
    assert ok == bytes(want) and (d["combined"], d["fell_back"]) == (1, 1)
    # the unsound choice, for contrast: equal supplied scalars accept the pair
    assert optimistic(prover, rows, scalars=[1] * 1100) == b"\x01" * 1100


def test_seeded_mix_against_the_host(prover):
    """6. 1 025 rows, a quarter of them byte_mutations' (seeded): verdicts equal the host's; at least 10 % rejected and
    at least 10 % accepted"""
    proofs, vals = mixed_rows(1025, seed=31)
    host = host_verdicts(prover, proofs, vals, 5)
    assert sum(host) >= 103 and 1025 - sum(host) >= 103
    rows = [(proofs[128 * i:128 * i + 128], vals[160 * i:160 * i + 160]) for i in range(1025)]
    prover.verify_set_cooldown(0)
    ok, d, _ = delta(prover, lambda: optimistic(prover, rows))
    assert ok == host and d["combined"] == 1


def test_drop_in_boundary(tmp_path):
    """7. an object with "verify_optimistic": true and one without give the same ok for 1 025 proofs with three damaged
    ones through ffi_verify_rln_proofs_batch and ffi_verify_rln_signals_batch; "verify_lanes": 8 keeps teams and never
    aggregates; a bad cool-down value is a configuration error"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.public import RLN, RLNProof, RLNWitnessInput

    def obj(**cfg):
        path = tmp_path / ("cfg%d.json" % len(list(tmp_path.iterdir())))
        path.write_text(json.dumps(dict(cfg, verify_gpu_min=4, hash_gpu_min=0)))
        return RLN(20, tree_config=str(path))
    opt, plain = obj(verify_optimistic=True, verify_optimistic_cooldown=0), obj()
    teams = obj(verify_optimistic=True, verify_lanes=8)
    secret = hashers.hash_to_field_le(b"optimistic-member")
    for o in (opt, plain, teams):
        o.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = opt.get_merkle_proof(3)
    signals = [b"relay message %d" % i for i in range(6)]
    xs = [hashers.hash_to_field_le(s) for s in signals]
    ws = [RLNWitnessInput(secret, 100, i, path[0], path[1], xs[i], 4242) for i in range(6)]
    good = opt.generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(6)])
    b0, b1 = good[0].to_bytes_le(), good[1].to_bytes_le()
    forged = RLNProof.from_bytes_le(b0[:1] + b1[1:129] + b0[129:])   # proof 1's points under proof 0's values
    n = 1025
    proofs, sig, x = [good[i % 6] for i in range(n)], [signals[i % 6] for i in range(n)], [xs[i % 6] for i in range(n)]
    want = [True] * n
    for i in (0, 511, 1024):
        proofs[i], sig[i], x[i], want[i] = forged, signals[0], xs[0], False
    sig[77] = b"another message"
    x[77] = hashers.hash_to_field_le(sig[77])
    want[77] = False                                                  # a wrong signal: the pairing is not what fails
    assert plain.verify_rln_proofs_batch(proofs, x) == want
    for call in (lambda o: o.verify_rln_proofs_batch(proofs, x), lambda o: o.verify_rln_signals_batch(proofs, sig)):
        s0 = opt.verify_stats()
        assert call(opt) == want
        s1 = opt.verify_stats()
        assert (s1["combined"] - s0["combined"], s1["fell_back"] - s0["fell_back"]) == (1, 1)
        assert call(plain) == want
        s0 = teams.verify_stats()
        assert call(teams) == want
        s1 = teams.verify_stats()
        assert s1["combined"] == s0["combined"] and s1["skipped_in_cooldown"] == s0["skipped_in_cooldown"]
        assert s1["team_passes"] > s0["team_passes"] and s1["lane_passes"] == s0["lane_passes"]
    # all valid: accepted, no exact pass
    s0 = opt.verify_stats()
    assert opt.verify_rln_proofs_batch([good[i % 6] for i in range(n)], [xs[i % 6] for i in range(n)]) == [True] * n
    s1 = opt.verify_stats()
    assert s1["accepted"] - s0["accepted"] == 1 and s1["lane_passes"] == s0["lane_passes"]
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"verify_optimistic_cooldown": -2}))
    with pytest.raises(RLNError, match="verify_optimistic_cooldown"):
        RLN(20, tree_config=str(bad))


def test_call_level_errors(prover):
    """8. n = 0 succeeds; null pointers with n > 0, a wrong n_values and a zero supplied scalar are errors, each with
    its own text, and leave the verifier working"""
    from zerokit_amd import lib
    L = lib()
    rows = fold_rows(rows_of(vc.golden_h20()), 1100)
    pr, va = join(rows)
    ok = C.create_string_buffer(1100)
    gt = C.create_string_buffer(384)
    assert L.rlnamd_verify_many_gpu_optimistic(prover._h, 0, None, None, 5, None, None) == 0
    assert L.rlnamd_verify_gpu_aggregate(prover._h, 0, None, None, 5, None, gt, None) == 0 and gt.raw == GT_ONE
    assert prover.verify_many_gpu_optimistic([], []) == []

    def text(rc):
        assert rc != 0
        return L.rlnamd_last_error().decode()
    t_null = text(L.rlnamd_verify_many_gpu_optimistic(prover._h, 1100, None, va, 5, None, ok))
    assert "null" in text(L.rlnamd_verify_many_gpu_optimistic(prover._h, 1100, pr, va, 5, None, None))
    t_nv = text(L.rlnamd_verify_many_gpu_optimistic(prover._h, 1100, pr, va, 4, None, ok))
    sc = bytearray(scalar_bytes([3] * 1100))
    sc[16 * 1099:] = bytes(16)
    t_zero = text(L.rlnamd_verify_many_gpu_optimistic(prover._h, 1100, pr, va, 5, bytes(sc), ok))
    assert "null" in t_null and "n_values" in t_nv and "MalformedVerifyingKey" in t_nv and "scalar is zero" in t_zero
    assert len({t_null, t_nv, t_zero}) == 3
    assert "scalar is zero" in text(L.rlnamd_verify_gpu_aggregate(prover._h, 1100, pr, va, 5, bytes(sc), gt, ok))
    assert "n_values" in text(L.rlnamd_verify_gpu_aggregate(prover._h, 1100, pr, va, 6, None, gt, ok))
    assert optimistic(prover, rows) == b"\x01" * 1100


def test_optimistic_beats_the_exact_pass_at_8192(prover):
    """9. a guard, not a benchmark: at n = 8 192, all valid, the median of 5 optimistic calls is below the median of 5
    exact lane-per-proof calls, alternated in one process.  That is the feature's purpose: no margin."""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    rows = fold_rows(rows_of(vc.golden_h20()), 8192)
    pr, va = join(rows)
    ok = C.create_string_buffer(8192)

    def exact():
        check(lib().rlnamd_verify_many_gpu_ex(prover._h, 8192, pr, va, 5, 1, ok, None))

    def opt():
        check(lib().rlnamd_verify_many_gpu_optimistic(prover._h, 8192, pr, va, 5, None, ok))
    exact()
    opt()                       # warm-up, and the buffers at their size
    before = prover.verify_optimistic_stats()
    t_opt, t_exact = [], []
    for _ in range(5):
        for fn, ts in ((opt, t_opt), (exact, t_exact)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            assert ok.raw == b"\x01" * 8192
    after = prover.verify_optimistic_stats()
    assert after["accepted"] - before["accepted"] == 5 and after["fell_back"] == before["fell_back"]
    a, b = statistics.median(t_opt), statistics.median(t_exact)
    print("n = 8192: optimistic %.1f ms (%.0f /s), exact lane-per-proof %.1f ms (%.0f /s)"
          % (a * 1e3, 8192 / a, b * 1e3, 8192 / b))
    assert a < b
