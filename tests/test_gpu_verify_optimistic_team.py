"""The optimistic form of the device verifier with a team of 8 lanes per proof (zerokit_amd/csrc/verify_agg_team.hip:
rlnamd_verify_many_gpu_optimistic_ex, rlnamd_verify_gpu_aggregate_ex, the "verify_optimistic_teams" config key): the
combined value against the host twin rlnamd_verify_aggregate_with_zkey byte for byte, the verdicts against
rlnamd_verify_many on host threads, and the bookkeeping through the counters, not through timing."""
import ctypes as C
import json
import statistics
import time

import pytest

import verify_cases as vc
from test_gpu_verify import host_verdicts
from test_gpu_verify_optimistic import (PREPARE_REJECTS, delta, fold_rows, fold_scalars, gpu_aggregate, host_aggregate, join,
                                        named_rejects, rows_of, scalar_bytes)
from test_verify_agg_host import mixed_rows
from verify_cases import GT_ONE, le

pytestmark = pytest.mark.gpu
TEAM_CHUNK = 8192


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


def aggregate_ex(p, rows, scalars, lanes=8, nv=5):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    pr, va = join(rows)
    gt, rej = C.create_string_buffer(384), C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1))
    check(lib().rlnamd_verify_gpu_aggregate_ex(p._h, n, pr, va, nv, scalar_bytes(scalars), lanes, gt, rej))
    return gt.raw, rej.raw[:n]


def optimistic_ex(p, rows, scalars=None, lanes=8, nv=5):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(rows)
    pr, va = join(rows)
    ok = C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1))
    check(lib().rlnamd_verify_many_gpu_optimistic_ex(p._h, n, pr, va, nv, None if scalars is None else scalar_bytes(scalars),
                                                     lanes, ok))
    return ok.raw[:n]


def damage(rows, n):
    g = vc.golden_h20()
    rj = named_rejects(g[2])
    damaged = [rj["input0"], rj["swapAC"], rj["A_infinity"], rj["A_off_curve"]]
    for k, i in enumerate(range(n // 2, n, 97)):
        rows[i] = damaged[k % 4]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 513, 4097])
def test_aggregate_value_equals_the_host_twin_depth20(prover, n):
    """1. rlnamd_verify_gpu_aggregate_ex(lanes = 8) == rlnamd_verify_aggregate_with_zkey, value and reject flags, around
    one wave of teams and one workgroup of the fold, at one, two and three fold levels; all-valid rows give 1, and with
    damaged rows in between the value is the twin's and not 1"""
    z = vc.zkey_bytes(20)
    rows, sc = fold_rows(rows_of(vc.golden_h20()), n), fold_scalars(n, seed=n)
    got = aggregate_ex(prover, rows, sc)
    assert got == (GT_ONE, bytes(n))
    assert got == host_aggregate(z, rows, sc)
    damage(rows, n)
    got = aggregate_ex(prover, rows, sc)
    want = host_aggregate(z, rows, sc)
    assert got[1] == want[1] and got[0] == want[0]
    assert got[0] != GT_ONE


def test_aggregate_value_across_a_team_chunk(prover):
    """1. at 8 193 proofs (two team chunks, the second of one proof) the product of the chunk values equals the lane
    form's value (rlnamd_verify_gpu_aggregate), which the lane form's tests hold against the twin"""
    n = TEAM_CHUNK + 1
    rows, sc = fold_rows(rows_of(vc.golden_h20()), n), fold_scalars(n, seed=n)
    got = aggregate_ex(prover, rows, sc)
    assert got == (GT_ONE, bytes(n)) and got == gpu_aggregate(prover, rows, sc)
    damage(rows, n)
    rows[n - 1] = named_rejects(vc.golden_h20()[2])["swapAC"]
    got = aggregate_ex(prover, rows, sc)
    assert got == gpu_aggregate(prover, rows, sc)
    assert got[0] != GT_ONE and sum(got[1]) > 0


@pytest.mark.parametrize("depth,multi", [(10, False), (20, True)])
def test_aggregate_value_other_circuits(depth, multi):
    """2. the other two shipped circuits (the multi-message-id one has more than 8 inputs: two rounds of lanes): their
    golden proof, whole and with a changed input"""
    from zerokit_amd.batch import BatchProver
    golden = [(nm, pr, pu) for nm, d, m, pr, pu in vc.golden_other() if (d, m) == (depth, multi)][0]
    nv = len(golden[2])
    good = rows_of([golden])[0]
    bad = named_rejects(golden)["input%d" % (nv - 1)]
    z = vc.zkey_bytes(depth, multi)
    p = BatchProver(max_batch=64, depth=depth, multi=multi)
    try:
        assert p.num_public == nv and (nv > 8) == multi
        for n in (1, 9, 65):
            sc = fold_scalars(n, seed=100 + n)
            rows = [good] * n
            assert aggregate_ex(p, rows, sc, nv=nv) == (GT_ONE, bytes(n)), n
            rows[n // 2] = bad
            got = aggregate_ex(p, rows, sc, nv=nv)
            assert got == host_aggregate(z, rows, sc, nv), n
            assert got[0] != GT_ONE
    finally:
        p.close()


def test_all_valid_rows_take_no_exact_pass(prover):
    """3. 1 000 valid rows in team form: all verdicts 1, one combined check in team form accepted, no fallback,
    rlnamd_verify_gpu_passes unmoved"""
    rows = fold_rows(rows_of(vc.golden_h20()), 1000)
    ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows))
    assert ok == b"\x01" * 1000
    assert (d["combined"], d["combined_team"], d["accepted"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 1, 1, 0, 0)
    assert passes == (0, 0)
    g = vc.golden_h20()
    assert prover.verify_many_gpu_optimistic([g[0][1]] * 20, [g[0][2]] * 20, lanes=8) == [True] * 20
    assert prover.verify_gpu_aggregate([g[0][1]] * 3, [g[0][2]] * 3, scalars=[1, 2, 3], lanes=8) == (GT_ONE, [False] * 3)


@pytest.mark.parametrize("at,kind", [(0, "swapAC"), (511, "input0"), (999, "swapAC")])
def test_one_damaged_proof_falls_back_and_cools_down(prover, at, kind):
    """4. one row the pairing rejects among 1 000: the verdicts are the host's, the call falls back to exactly one exact
    team pass, the next `cooldown` calls skip the combined check, the call after them is combined again"""
    g = vc.golden_h20()
    rows = fold_rows(rows_of(g), 1000)
    rows[at] = named_rejects(g[1])[kind]
    want = bytearray(b"\x01" * 1000)
    want[at] = 0
    assert host_verdicts(prover, *join(rows), 5) == bytes(want)
    prover.verify_set_cooldown(2)
    ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows))
    assert ok == bytes(want)
    assert (d["combined"], d["combined_team"], d["accepted"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 1, 0, 1, 0)
    assert passes == (0, 1)
    assert prover.verify_optimistic_stats()["cooldown_left"] == 2
    for _ in range(2):
        ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows))
        assert ok == bytes(want)
        assert (d["combined"], d["fell_back"], d["skipped_in_cooldown"]) == (0, 0, 1) and passes == (0, 1)
    ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows))
    assert ok == bytes(want) and (d["combined"], d["combined_team"], d["fell_back"], d["skipped_in_cooldown"]) == (1, 1, 1, 0)


def test_rows_that_prepare_rejects_are_named_without_a_fallback(prover):
    """5. every case of rejects() that the per-proof checks refuse, between valid rows: verdicts equal the host's, the
    counter counts them, the combined check accepts the rest (no fallback)"""
    g = vc.golden_h20()
    rows = fold_rows(rows_of(g), 600)
    want = bytearray(b"\x01" * 600)
    at = 7
    for case in g[:3]:
        rj = named_rejects(case)
        assert PREPARE_REJECTS <= set(rj)
        for name in sorted(PREPARE_REJECTS):
            rows[at] = rj[name]
            want[at] = 0
            at += 31
    refused = 3 * len(PREPARE_REJECTS)
    assert host_verdicts(prover, *join(rows), 5) == bytes(want)
    _, rej = host_aggregate(vc.zkey_bytes(20), rows, [1] * 600)
    assert rej == bytes(1 - v for v in want)      # it is the per-proof checks that refuse them
    ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows))
    assert ok == bytes(want)
    assert (d["combined"], d["combined_team"], d["accepted"], d["fell_back"], d["refused_proofs"]) == (1, 1, 1, 0, refused)
    assert passes == (0, 0)


def test_cancelling_pair_needs_independent_scalars(prover):
    """6. two valid proofs with C_1 + T and C_2 - T (T the G1 generator): each is invalid, their product under EQUAL
    scalars is 1 -- the combined value in team form with supplied scalars [1, 1] is 1, with [1, 2] it is not -- and under
    drawn scalars both are named"""
    from oracle.pyref import arkzkey
    from oracle.pyref import bn254 as o
    g = vc.golden_h20()
    pair = []
    for case, t in ((g[0], o.G1_GEN), (g[1], o.G1.neg(o.G1_GEN))):
        A, B, Cp = arkzkey.proof_decompress(case[1])
        pair.append((arkzkey.proof_compress(A, B, o.G1.add(Cp, t)), b"".join(le(v) for v in case[2])))
    assert host_verdicts(prover, *join(pair), 5) == b"\x00\x00"
    assert aggregate_ex(prover, pair, [1, 1]) == (GT_ONE, b"\x00\x00")
    assert aggregate_ex(prover, pair, [1, 2])[0] != GT_ONE
    ok, d, passes = delta(prover, lambda: optimistic_ex(prover, pair))
    assert ok == b"\x00\x00" and (d["combined_team"], d["fell_back"]) == (1, 1) and passes == (0, 1)


def test_seeded_mix_against_the_host(prover):
    """7. 1 024 rows, a quarter of them byte_mutations' (seeded): verdicts equal the host's; at least 10 % rejected and
    at least 10 % accepted, by the host's verdicts"""
    proofs, vals = mixed_rows(1024, seed=31)
    host = host_verdicts(prover, proofs, vals, 5)
    assert sum(host) >= 103 and 1024 - sum(host) >= 103
    rows = [(proofs[128 * i:128 * i + 128], vals[160 * i:160 * i + 160]) for i in range(1024)]
    prover.verify_set_cooldown(0)
    ok, d, _ = delta(prover, lambda: optimistic_ex(prover, rows))
    assert ok == host and (d["combined"], d["combined_team"]) == (1, 1)


def test_lanes_0_chooses_by_the_size_of_the_call(prover):
    """8. through _ex, lanes = 0: 1 024 proofs take the combined check in team form, 1 025 with a lane per proof; the
    old rlnamd_verify_many_gpu_optimistic at n = 1 000 still runs an exact team pass and no combined check"""
    from test_gpu_verify_optimistic import optimistic
    base = rows_of(vc.golden_h20())
    for n, team in ((1024, 1), (1025, 0)):
        rows = fold_rows(base, n)
        ok, d, passes = delta(prover, lambda: optimistic_ex(prover, rows, lanes=0))
        assert ok == b"\x01" * n
        assert (d["combined"], d["combined_team"], d["accepted"]) == (1, team, 1) and passes == (0, 0), n
    rows = fold_rows(base, 1000)
    ok, d, passes = delta(prover, lambda: optimistic(prover, rows))
    assert ok == b"\x01" * 1000
    assert (d["combined"], d["combined_team"], d["skipped_in_cooldown"]) == (0, 0, 0) and passes == (0, 1)


def test_drop_in_boundary(tmp_path):
    """9. objects with verify_gpu_min = 4: {"verify_optimistic", "verify_optimistic_teams"} and a plain object give the
    same ok for 600 proofs with three forged ones through ffi_verify_rln_proofs_batch and ffi_verify_rln_signals_batch,
    and combined_team rises; 600 valid proofs are accepted with no team pass; "verify_optimistic_teams" alone is a
    configuration error that names both keys"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.public import RLN, RLNProof, RLNWitnessInput

    def obj(**cfg):
        path = tmp_path / ("cfg%d.json" % len(list(tmp_path.iterdir())))
        path.write_text(json.dumps(dict(cfg, verify_gpu_min=4, hash_gpu_min=0)))
        return RLN(20, tree_config=str(path))
    opt = obj(verify_optimistic=True, verify_optimistic_teams=True, verify_optimistic_cooldown=0)
    plain = obj()
    secret = hashers.hash_to_field_le(b"optimistic-team-member")
    for o in (opt, plain):
        o.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = opt.get_merkle_proof(3)
    signals = [b"relay message %d" % i for i in range(6)]
    xs = [hashers.hash_to_field_le(s) for s in signals]
    ws = [RLNWitnessInput(secret, 100, i, path[0], path[1], xs[i], 4242) for i in range(6)]
    good = opt.generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(6)])
    b0, b1 = good[0].to_bytes_le(), good[1].to_bytes_le()
    forged = RLNProof.from_bytes_le(b0[:1] + b1[1:129] + b0[129:])   # proof 1's points under proof 0's values
    n = 600
    proofs, sig, x = [good[i % 6] for i in range(n)], [signals[i % 6] for i in range(n)], [xs[i % 6] for i in range(n)]
    want = [True] * n
    for i in (0, 299, 599):
        proofs[i], sig[i], x[i], want[i] = forged, signals[0], xs[0], False
    assert plain.verify_rln_proofs_batch(proofs, x) == want
    for call in (lambda o: o.verify_rln_proofs_batch(proofs, x), lambda o: o.verify_rln_signals_batch(proofs, sig)):
        s0 = opt.verify_stats()
        assert call(opt) == want
        s1 = opt.verify_stats()
        assert (s1["combined"] - s0["combined"], s1["combined_team"] - s0["combined_team"],
                s1["fell_back"] - s0["fell_back"], s1["team_passes"] - s0["team_passes"]) == (1, 1, 1, 1)
        assert call(plain) == want
    s0 = opt.verify_stats()
    assert opt.verify_rln_proofs_batch([good[i % 6] for i in range(n)], [xs[i % 6] for i in range(n)]) == [True] * n
    s1 = opt.verify_stats()
    assert s1["accepted"] - s0["accepted"] == 1 and s1["combined_team"] - s0["combined_team"] == 1
    assert s1["team_passes"] == s0["team_passes"] and s1["lane_passes"] == s0["lane_passes"]
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"verify_optimistic_teams": True}))
    with pytest.raises(RLNError, match="verify_optimistic_teams.*\"verify_optimistic\""):
        RLN(20, tree_config=str(bad))


def test_call_level_errors(prover):
    """10. lanes = 3, a zero supplied scalar and a null pointer with n > 0 are errors, each with its own text, and leave
    the verifier working"""
    from zerokit_amd import lib
    L = lib()
    rows = fold_rows(rows_of(vc.golden_h20()), 100)
    pr, va = join(rows)
    ok = C.create_string_buffer(100)
    gt = C.create_string_buffer(384)
    assert L.rlnamd_verify_many_gpu_optimistic_ex(prover._h, 0, None, None, 5, None, 8, None) == 0
    assert L.rlnamd_verify_gpu_aggregate_ex(prover._h, 0, None, None, 5, None, 8, gt, None) == 0 and gt.raw == GT_ONE

    def text(rc):
        assert rc != 0
        return L.rlnamd_last_error().decode()
    t_lanes = text(L.rlnamd_verify_many_gpu_optimistic_ex(prover._h, 100, pr, va, 5, None, 3, ok))
    t_null = text(L.rlnamd_verify_many_gpu_optimistic_ex(prover._h, 100, None, va, 5, None, 8, ok))
    sc = bytearray(scalar_bytes([3] * 100))
    sc[16 * 99:] = bytes(16)
    t_zero = text(L.rlnamd_verify_many_gpu_optimistic_ex(prover._h, 100, pr, va, 5, bytes(sc), 8, ok))
    assert "lanes" in t_lanes and "null" in t_null and "scalar is zero" in t_zero
    assert len({t_lanes, t_null, t_zero}) == 3
    assert "lanes" in text(L.rlnamd_verify_gpu_aggregate_ex(prover._h, 100, pr, va, 5, None, 0, gt, ok))
    assert "scalar is zero" in text(L.rlnamd_verify_gpu_aggregate_ex(prover._h, 100, pr, va, 5, bytes(sc), 8, gt, ok))
    assert "null" in text(L.rlnamd_verify_gpu_aggregate_ex(prover._h, 100, pr, None, 5, None, 8, gt, ok))
    assert optimistic_ex(prover, rows) == b"\x01" * 100


def test_optimistic_team_beats_the_exact_team_pass_at_1024(prover):
    """11. a guard, not a benchmark: at n = 1 024, all valid, the median of 5 optimistic calls in team form is below the
    median of 5 exact team calls, alternated in one process.  That is the feature's purpose: no margin."""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = 1024
    rows = fold_rows(rows_of(vc.golden_h20()), n)
    pr, va = join(rows)
    ok = C.create_string_buffer(n)

    def exact():
        check(lib().rlnamd_verify_many_gpu_ex(prover._h, n, pr, va, 5, 8, ok, None))

    def opt():
        check(lib().rlnamd_verify_many_gpu_optimistic_ex(prover._h, n, pr, va, 5, None, 8, ok))
    exact()
    opt()                       # warm-up, and the buffers at their size
    before = prover.verify_optimistic_stats()
    t_opt, t_exact = [], []
    for _ in range(5):
        for fn, ts in ((opt, t_opt), (exact, t_exact)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            assert ok.raw == b"\x01" * n
    after = prover.verify_optimistic_stats()
    assert after["combined_team"] - before["combined_team"] == 5 and after["fell_back"] == before["fell_back"]
    a, b = statistics.median(t_opt), statistics.median(t_exact)
    print("n = 1024: optimistic team %.2f ms (%.0f /s), exact team %.2f ms (%.0f /s)"
          % (a * 1e3, n / a, b * 1e3, n / b))
    assert a < b
