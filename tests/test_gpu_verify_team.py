"""Groth16 verification on the device with a team of 8 lanes per proof (zerokit_amd/csrc/verify_team.hip:
rlnamd_verify_many_gpu_ex with lanes = 8) against the host verifier, which is the yardstick: every verdict is compared
with rlnamd_verify_many (host threads), every GT row with the host build's vmh_host_verify, never with the team path
itself; in addition lanes = 8 and lanes = 1 give the same bytes."""
import ctypes as C
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

import pytest

import verify_cases as vc
from verify_cases import GT_ONE, R, ROOT, le

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 64


def chunk_size():
    src = open(os.path.join(ROOT, "zerokit_amd", "csrc", "verify.h")).read()
    return int(re.search(r"CHUNK = (\d+);", src).group(1))


def host_verdicts(p, proofs, vals, nv, threads=16):
    """rlnamd_verify_many on raw bytes (proofs n x 128, vals n x nv x 32) -> bytes of 0 / 1"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(proofs) // 128
    assert len(proofs) == 128 * n and len(vals) == 32 * nv * n
    ok = C.create_string_buffer(max(n, 1))
    check(lib().rlnamd_verify_many(p._h, n, proofs, vals, nv, threads, ok))
    return ok.raw[:n]


def case_rows(golden):
    """golden cases and their hand-made rejects as (names, proofs bytes, vals bytes)"""
    rows = []
    for name, proof, pub in golden:
        rows.append((name, proof, pub))
        rows += vc.rejects(name, proof, pub)
    raw = lambda x: (int(x) % (1 << 256)).to_bytes(32, "little")   # noqa: E731
    return ([r[0] for r in rows], b"".join(r[1] for r in rows), b"".join(raw(v) for r in rows for v in r[2]))


def host_gt_lib(depth=20, multi=False):
    """the CPU build of the host verifier (tests/host/verifymath.cpp: vmh_host_verify is capi.cpp's verify_common)"""
    so = os.path.join(ROOT, "tests", "host", "libverifymath.so")
    src = os.path.join(ROOT, "tests", "host", "verifymath.cpp")
    csrc = os.path.join(ROOT, "zerokit_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("field.h", "curve.h", "pairing.h", "zkey.cpp", "zkey.h", "common.h",
                                                    "verify_math.h", "verify_key.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", csrc, src, "-o", so])
    lib = C.CDLL(so)
    z = vc.zkey_bytes(depth, multi)
    assert lib.vmh_load_zkey(z, len(z)) == 0
    return lib


def mixed_rows(gen, count, seed):
    """`count` rows from the generated proofs: a third untouched, a third with one flipped byte at a random offset of
    the proof, a third with one public input replaced (the rows of test_gpu_verify.py's mix for the same seed)"""
    rnd = random.Random(seed)
    n = len(gen["proofs"]) // 128
    ps, vs = [], []
    for _ in range(count):
        i = rnd.randrange(n)
        proof = bytearray(gen["proofs"][128 * i:128 * i + 128])
        val = bytearray(gen["values"][160 * i:160 * i + 160])
        kind = rnd.randrange(3)
        if kind == 1:
            proof[rnd.randrange(128)] ^= 1 << rnd.randrange(8)
        elif kind == 2:
            k = rnd.randrange(5)
            val[32 * k:32 * k + 32] = le(rnd.randrange(R))
        ps.append(bytes(proof))
        vs.append(bytes(val))
    return b"".join(ps), b"".join(vs)


def team_max():
    src = open(os.path.join(ROOT, "zerokit_amd", "csrc", "verify.h")).read()
    return int(re.search(r"TEAM_MAX = (\d+);", src).group(1))


def gpu_ex(p, proofs, vals, nv, lanes, want_ok=True, want_gt=False):
    """rlnamd_verify_many_gpu_ex on raw bytes -> (verdict bytes or None, GT bytes or None); both buffers are PAD rows
    longer than n, filled with a sentinel, and must be untouched beyond row n - 1"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(proofs) // 128
    assert len(proofs) == 128 * n and len(vals) == 32 * nv * n
    ok = C.create_string_buffer(bytes([SENTINEL]) * (n + PAD), n + PAD) if want_ok else None
    gt = C.create_string_buffer(bytes([SENTINEL]) * (384 * (n + PAD)), 384 * (n + PAD)) if want_gt else None
    check(lib().rlnamd_verify_many_gpu_ex(p._h, n, proofs, vals, nv, lanes, ok, gt))
    if ok is not None:
        assert ok.raw[n:] == bytes([SENTINEL]) * PAD, "verdicts written beyond row n - 1"
    if gt is not None:
        assert gt.raw[384 * n:] == bytes([SENTINEL]) * (384 * PAD), "GT rows written beyond row n - 1"
    return (ok.raw[:n] if ok is not None else None), (gt.raw[:384 * n] if gt is not None else None)


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=1024)
    yield p
    p.close()


@pytest.fixture(scope="module")
def generated(prover):
    """1 024 proofs of the bench workload's witnesses made on the device"""
    from zerokit_amd import workload
    ws, rs = workload.config2_range(0, 1024)
    inp, rsb = prover.pack_inputs(ws), prover.pack_rs(rs)
    t, n = prover.submit(inp, rsb)
    proofs, values, errs = prover.collect_raw(t, n)
    assert not any(errs)
    return dict(inputs=inp, rs=rsb, proofs=proofs, values=values)


def _check_against_host(p, names, proofs, vals, nv, hv):
    """verdicts and GT rows of lanes = 8 against the host; the same bytes from lanes = 1"""
    n = len(names)
    host = host_verdicts(p, proofs, vals, nv)
    ok8, gt8 = gpu_ex(p, proofs, vals, nv, 8, want_gt=True)
    assert list(ok8) == list(host), [nm for nm, a, b in zip(names, ok8, host) if a != b]
    by_pairing = before = 0
    for i, nm in enumerate(names):
        want = C.create_string_buffer(384)
        assert hv.vmh_host_verify(proofs[128 * i:128 * i + 128], vals[32 * nv * i:32 * nv * (i + 1)], nv, want) == host[i], nm
        row = gt8[384 * i:384 * i + 384]
        assert row == want.raw, nm
        if host[i]:
            assert row == GT_ONE, nm
        by_pairing += (not host[i]) and row != bytes(384)
        before += (not host[i]) and row == bytes(384)
    ok1, gt1 = gpu_ex(p, proofs, vals, nv, 1, want_gt=True)
    assert ok1 == ok8 and gt1 == gt8
    return host, by_pairing, before


def test_golden_proofs_and_hand_made_rejects_in_team_form(prover):
    """the golden cases of the depth-20 circuit and their hand-made rejects, accepted and rejected proofs side by side in
    a wave: verdicts element for element, GT rows (1 for accepted, the host's value where the pairing ran, zeros where it
    did not)"""
    names, proofs, vals = case_rows(vc.golden_h20())
    host, by_pairing, before = _check_against_host(prover, names, proofs, vals, 5, host_gt_lib())
    assert sum(host) == 6 and len(names) == 6 * 16
    assert by_pairing >= 6 * 6 and before >= 6
    # only verdicts, only GT rows, neither
    ok8, none = gpu_ex(prover, proofs, vals, 5, 8)
    assert ok8 == host and none is None
    none, gt8 = gpu_ex(prover, proofs, vals, 5, 8, want_ok=False, want_gt=True)
    assert none is None and gt8[:384] == GT_ONE
    assert gpu_ex(prover, proofs, vals, 5, 8, want_ok=False) == (None, None)
    # the Python wrappers
    g = vc.golden_h20()
    assert prover.verify_many_gpu([c[1] for c in g], [c[2] for c in g], lanes=8) == [True] * 6
    assert prover.verify_many_gpu_gt([g[0][1]], [g[0][2]], lanes=8) == [GT_ONE]
    bad = [list(c[2]) for c in g]
    bad[2][0] ^= 1
    assert prover.verify_many_gpu([c[1] for c in g], bad, lanes=8) == [True, True, False, True, True, True]
    assert prover.verify_many_gpu([], [], lanes=8) == []


@pytest.mark.parametrize("depth,multi", [(10, False), (20, True)])
def test_other_circuits_in_team_form(depth, multi):
    """the golden proof and the hand-made rejects of the depth-10 and of the multi-message-id circuit (more than eight
    public inputs: two rounds of a lane per input)"""
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, depth=depth, multi=multi)
    try:
        golden = [(nm, pr, pu) for nm, d, m, pr, pu in vc.golden_other() if (d, m) == (depth, multi)]
        nv = len(golden[0][2])
        assert nv == p.num_public and (nv > 5) == multi
        names, gp, gv = case_rows(golden)
        host, by_pairing, before = _check_against_host(p, names, gp, gv, nv, host_gt_lib(depth, multi))
        assert sum(host) == 1 and by_pairing >= nv and before >= 1
    finally:
        p.close()


def test_generated_proofs_and_a_seeded_mix_in_team_form(prover, generated):
    """1 024 proofs made on the device all pass; 2 048 rows mixed from them get the host path's verdicts (both verdicts
    occur at least 256 times)"""
    assert gpu_ex(prover, generated["proofs"], generated["values"], 5, 8)[0] == b"\x01" * 1024
    proofs, vals = mixed_rows(generated, 2048, seed=77)
    host = host_verdicts(prover, proofs, vals, 5)
    assert gpu_ex(prover, proofs, vals, 5, 8)[0] == host
    assert gpu_ex(prover, proofs, vals, 5, 1)[0] == host
    assert sum(host) >= 256 and 2048 - sum(host) >= 256


def test_any_n_in_team_form(prover):
    """n = 0, 1, 7, 8, 9, 63, 64, 65, 8 191, 8 192, 8 193 and two chunks with a ragged tail: rows tiled from the golden
    cases and their rejects at a shifting offset, each verdict the host's for that row; verdict and GT buffers are 64
    rows longer than n and untouched beyond row n - 1 (gpu_ex asserts it)"""
    names, proofs, vals = case_rows(vc.golden_h20())
    m = len(names)
    host = host_verdicts(prover, proofs, vals, 5)
    hv = host_gt_lib()
    gts = []
    for i in range(m):
        want = C.create_string_buffer(384)
        hv.vmh_host_verify(proofs[128 * i:128 * i + 128], vals[160 * i:160 * i + 160], 5, want)
        gts.append(want.raw)
    assert gpu_ex(prover, b"", b"", 5, 8, want_gt=True) == (b"", b"")
    before = prover.verify_gpu_passes()
    chunks = 0
    for n in (1, 7, 8, 9, 63, 64, 65, 8191, 8192, 8193, 2 * 8192 + 1237):
        off = n % 7   # not always the same row first
        reps = (off + n) // m + 1
        pr = (proofs * reps)[128 * off:128 * (off + n)]
        va = (vals * reps)[160 * off:160 * (off + n)]
        want = (host * reps)[off:off + n]
        ok, gt = gpu_ex(prover, pr, va, 5, 8, want_gt=True)
        assert ok == want, n
        assert gt == b"".join((gts * reps)[off:off + n]), n
        chunks += -(-n // 8192)
    after = prover.verify_gpu_passes()
    assert after[1] - before[1] == chunks and after[0] == before[0]


_CHILD = r"""
import os, sys, json
sys.path.insert(0, os.environ["RLN_ROOT"])
sys.path.insert(0, os.path.join(os.environ["RLN_ROOT"], "tests"))
import verify_cases as vc
from zerokit_amd.batch import BatchProver
p = BatchProver(max_batch=64)
g = vc.golden_h20()
proofs, pub = [c[1] for c in g] * 3, [c[2] for c in g] * 3
out = []
for lanes in (0, 1, 8):
    before = p.verify_gpu_passes()
    assert p.verify_many_gpu(proofs, pub, lanes=lanes) == [True] * 18
    after = p.verify_gpu_passes()
    out.append([after[0] - before[0], after[1] - before[1]])
print("RESULT " + json.dumps({"passes": out, "describe": p.describe()}))
p.close()
"""


def _child(forced):
    env = dict(os.environ, RLN_ROOT=ROOT)
    env.pop("RLNAMD_VERIFY_LANES", None)
    if forced is not None:
        env["RLNAMD_VERIFY_LANES"] = str(forced)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_the_shape_follows_n_unless_it_is_named_or_forced(prover, generated):
    """lanes = 0 takes teams at n <= verify_team_max and a lane per proof above it, seen through
    rlnamd_verify_gpu_passes and not through timing; RLNAMD_VERIFY_LANES = 8 / 1 forces the shape of lanes = 0 (read
    once at construction: child processes) and leaves a named shape alone; lanes = 3 is an error, not a crash"""
    from zerokit_amd import RLNError, lib
    assert "RLNAMD_VERIFY_LANES" not in os.environ
    tm = team_max()
    assert tm <= chunk_size()
    assert "verify_lanes=0" in prover.describe().split()

    def passes_of(n, lanes):
        reps = -(-n // 1024)
        pr, va = (generated["proofs"] * reps)[:128 * n], (generated["values"] * reps)[:160 * n]
        before = prover.verify_gpu_passes()
        ok, _ = gpu_ex(prover, pr, va, 5, lanes)
        assert ok == b"\x01" * n
        after = prover.verify_gpu_passes()
        return after[0] - before[0], after[1] - before[1]

    if tm > 0:
        assert passes_of(min(tm, 64), 0) == (0, 1)
        assert passes_of(tm, 0) == (0, -(-tm // 8192))
    assert passes_of(tm + 1, 0) == (1, 0)
    assert passes_of(64, 1) == (1, 0)
    assert passes_of(64, 8) == (0, 1)
    # the entry points that keep their signatures leave the choice to the verifier
    from zerokit_amd._native import check
    before = prover.verify_gpu_passes()
    ok = C.create_string_buffer(64)
    check(lib().rlnamd_verify_many_gpu(prover._h, 64, generated["proofs"][:128 * 64], generated["values"][:160 * 64], 5, ok))
    assert ok.raw == b"\x01" * 64
    after = prover.verify_gpu_passes()
    assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if tm >= 64 else (1, 0))
    # any other lane count is an error return
    g = vc.golden_h20()
    for bad in (3, -1, 64):
        ok = C.create_string_buffer(b"\x07", 1)
        rc = lib().rlnamd_verify_many_gpu_ex(prover._h, 1, g[0][1], b"".join(le(v) for v in g[0][2]), 5, bad, ok, None)
        assert rc != 0 and ok.raw == b"\x07"
    with pytest.raises(RLNError):
        prover.verify_many_gpu([g[0][1]], [g[0][2]], lanes=3)
    # forced shapes
    free = _child(None)
    assert free["passes"] == [[0, 1] if tm >= 18 else [1, 0], [1, 0], [0, 1]]
    f8 = _child(8)
    assert f8["passes"] == [[0, 1], [1, 0], [0, 1]] and "verify_lanes=8" in f8["describe"].split()
    f1 = _child(1)
    assert f1["passes"] == [[1, 0], [1, 0], [0, 1]] and "verify_lanes=1" in f1["describe"].split()


def test_ffi_verify_rln_proofs_batch_with_verify_lanes(tmp_path):
    """an FFI object with {"verify_gpu_min": 4, "verify_lanes": 8}: ffi_verify_rln_proofs_batch == a loop over
    verify_rln_proof / verify_with_roots for eight proofs (one whose pairing fails, one made at an older root, one wrong
    signal) and four root lists; an out-of-range "verify_lanes" is a configuration error"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.public import RLN, RLNProof, RLNWitnessInput
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"verify_gpu_min": 4, "verify_lanes": 8}))
    dev_obj, host_obj = RLN(20, tree_config=str(cfgp)), RLN(20)
    secrets = [hashers.hash_to_field_le(b"batch-verify-member-%d" % k) for k in range(3)]
    for obj in (dev_obj, host_obj):
        obj.set_leaf(5, hashers.poseidon_hash_pair(hashers.poseidon_hash([secrets[0]]), 100))
    old_path = dev_obj.get_merkle_proof(5)
    old = dev_obj.generate_rln_proof_with_rs(RLNWitnessInput(secrets[0], 100, 1, old_path[0], old_path[1], 900, 4242), 3, 4)
    old_root = old.values.root
    for obj in (dev_obj, host_obj):
        for k in (1, 2):
            obj.set_leaf(5 + k, hashers.poseidon_hash_pair(hashers.poseidon_hash([secrets[k]]), 100))
    paths = [dev_obj.get_merkle_proof(5 + k) for k in range(3)]
    ws = [RLNWitnessInput(secrets[i % 3], 100, i, paths[i % 3][0], paths[i % 3][1], 1000 + i, 4242) for i in range(6)]
    good = dev_obj.generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(6)])
    b0, b1 = good[0].to_bytes_le(), good[1].to_bytes_le()
    forged = RLNProof.from_bytes_le(b0[:1] + b1[1:129] + b0[129:])   # proof 1's points under proof 0's values
    proofs = good + [forged, old]
    xs = [1000 + i for i in range(6)] + [1000, 900]
    xs[3] = 77                                                       # one wrong signal
    now_root = good[0].values.root
    assert now_root != old_root

    def loop(obj, roots):
        out = []
        for pr, x in zip(proofs, xs):
            try:
                out.append(obj.verify_rln_proof(pr, x) if roots is None else obj.verify_with_roots(pr, x, roots))
            except RLNError as e:
                assert "Verification error" in str(e)
                out.append(False)
        return out

    expect = {None: [1, 1, 1, 0, 1, 1, 0, 0], "match": [1, 1, 1, 0, 1, 1, 0, 1], "other": [0] * 8,
              "empty": [1, 1, 1, 0, 1, 1, 0, 1]}
    for key, roots in ((None, None), ("match", [old_root, now_root]), ("other", [12345]), ("empty", [])):
        want = loop(host_obj, roots)
        assert want == [bool(v) for v in expect[key]], key
        assert dev_obj.verify_rln_proofs_batch(proofs, xs, roots) == want, key        # 8 >= 4: the device, in teams
        assert dev_obj.verify_rln_proofs_batch(proofs[:3], xs[:3], roots) == want[:3], key   # 3 < 4: host threads
    cfgp.write_text(json.dumps({"verify_lanes": 3}))
    with pytest.raises(RLNError, match="verify_lanes"):
        RLN(20, tree_config=str(cfgp))


def test_team_verification_beside_proving(prover, generated):
    """a 1 024-proof batch is submitted, 64 rows are verified in team form before it is collected: the verdicts are
    right and the proofs are byte-identical to a quiet run"""
    names, proofs, vals = case_rows(vc.golden_h20())
    proofs, vals = proofs[:128 * 64], vals[:160 * 64]
    host = host_verdicts(prover, proofs, vals, 5)
    t, n = prover.submit(generated["inputs"], generated["rs"])
    assert gpu_ex(prover, proofs, vals, 5, 8)[0] == host
    got, values, errs = prover.collect_raw(t, n)
    assert got == generated["proofs"] and values == generated["values"] and not any(errs)


def test_teams_beat_a_lane_per_proof_at_1024(prover, generated):
    """a guard, not a benchmark, and only where the verifier would choose teams by itself: at n = 1 024, after a
    warm-up call of each shape, the median of 5 calls with lanes = 8 is below the median of 5 calls with lanes = 1 (the
    lane-per-proof kernels are the ones shipped before teams existed), each call ending in its own synchronise"""
    if team_max() == 0:
        return
    proofs, vals = generated["proofs"], generated["values"]
    med = {}
    for lanes in (8, 1):
        assert gpu_ex(prover, proofs, vals, 5, lanes)[0] == b"\x01" * 1024
    for lanes in (8, 1):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ok, _ = gpu_ex(prover, proofs, vals, 5, lanes)
            ts.append(time.perf_counter() - t0)
            assert ok == b"\x01" * 1024
        med[lanes] = statistics.median(ts)
    print("n = 1024: lanes = 8 %.2f ms, lanes = 1 %.2f ms" % (med[8] * 1e3, med[1] * 1e3))
    assert med[8] < med[1]
