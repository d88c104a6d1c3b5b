"""Groth16 verification on the device (zerokit_amd/csrc/verify.hip: rlnamd_verify_many_gpu, ffi_verify_rln_proofs_batch)
against the host verifier, which is the yardstick: the same verdict for every input, the same pairing value where the
pairing runs."""
import ctypes as C
import json
import os
import random
import re
import statistics
import threading
import time

import pytest

import verify_cases as vc
from verify_cases import GT_ONE, R, ROOT, le

pytestmark = pytest.mark.gpu


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


def gpu_verdicts(p, proofs, vals, nv):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(proofs) // 128
    assert len(proofs) == 128 * n and len(vals) == 32 * nv * n
    ok = C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1))
    check(lib().rlnamd_verify_many_gpu(p._h, n, proofs, vals, nv, ok))
    return ok.raw[:n]


def gpu_gt(p, proofs, vals, nv):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    n = len(proofs) // 128
    gt = C.create_string_buffer(384 * n)
    check(lib().rlnamd_verify_many_gpu_gt(p._h, n, proofs, vals, nv, gt))
    return [gt.raw[384 * i:384 * (i + 1)] for i in range(n)]


def raw(x):
    return (int(x) % (1 << 256)).to_bytes(32, "little")


def case_rows(golden):
    """golden cases and their hand-made rejects as (names, proofs bytes, vals bytes)"""
    rows = []
    for name, proof, pub in golden:
        rows.append((name, proof, pub))
        rows += vc.rejects(name, proof, pub)
    return ([r[0] for r in rows], b"".join(r[1] for r in rows), b"".join(raw(v) for r in rows for v in r[2]))


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=1024)
    yield p
    p.close()


@pytest.fixture(scope="module")
def generated(prover):
    """1 024 proofs of the bench workload's witnesses made on the device -> (proofs, public inputs, raw collect bytes)"""
    from zerokit_amd import workload
    ws, rs = workload.config2_range(0, 1024)
    inp, rsb = prover.pack_inputs(ws), prover.pack_rs(rs)
    t, n = prover.submit(inp, rsb)
    proofs, values, errs = prover.collect_raw(t, n)
    assert not any(errs)
    return dict(inputs=inp, rs=rsb, proofs=proofs, values=values)


def host_gt_lib(depth=20, multi=False):
    from test_verify_math_host import _build
    lib = _build()
    z = vc.zkey_bytes(depth, multi)
    assert lib.vmh_load_zkey(z, len(z)) == 0
    return lib


def test_golden_proofs_and_hand_made_rejects_equal_the_host(prover):
    """verdicts equal rlnamd_verify_many's element for element; the GT rows of accepted proofs are the encoding of 1,
    those of proofs rejected by the pairing equal the host build's value, those rejected before it are zero"""
    names, proofs, vals = case_rows(vc.golden_h20())
    n = len(names)
    host = host_verdicts(prover, proofs, vals, 5)
    dev = gpu_verdicts(prover, proofs, vals, 5)
    assert list(dev) == list(host), [nm for nm, a, b in zip(names, dev, host) if a != b]
    assert sum(host) == 6 and n == 6 * 16
    gts = gpu_gt(prover, proofs, vals, 5)
    hv = host_gt_lib()
    by_pairing = 0
    for i, nm in enumerate(names):
        want = C.create_string_buffer(384)
        assert hv.vmh_host_verify(proofs[128 * i:128 * i + 128], vals[160 * i:160 * i + 160], 5, want) == host[i], nm
        assert gts[i] == want.raw, nm
        if host[i]:
            assert gts[i] == GT_ONE, nm
        by_pairing += (not host[i]) and gts[i] != bytes(384)
    assert by_pairing >= 6 * 6
    # the Python wrappers
    g = vc.golden_h20()
    assert prover.verify_many_gpu([c[1] for c in g], [c[2] for c in g]) == [True] * 6
    assert prover.verify_many_gpu_gt([g[0][1]], [g[0][2]]) == [GT_ONE]
    bad = [list(c[2]) for c in g]
    bad[2][0] ^= 1
    assert prover.verify_many_gpu([c[1] for c in g], bad) == [True, True, False, True, True, True]
    assert prover.verify_many_gpu([], []) == []
    from zerokit_amd import RLNError
    with pytest.raises(RLNError, match="MalformedVerifyingKey"):
        prover.verify_many_gpu([g[0][1]], [g[0][2][:4]])


def mixed_rows(gen, count, seed):
    """`count` rows from the generated proofs: a third untouched, a third with one flipped byte at a random offset of
    the proof, a third with one public input replaced"""
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


def test_generated_proofs_and_a_seeded_mix_of_damaged_ones(prover, generated):
    """1 024 proofs made on the device all pass; 2 048 rows mixed from them (untouched / one flipped proof byte / one
    replaced public input) get the host path's verdicts, and both verdicts occur at least 256 times"""
    assert gpu_verdicts(prover, generated["proofs"], generated["values"], 5) == b"\x01" * 1024
    proofs, vals = mixed_rows(generated, 2048, seed=77)
    host = host_verdicts(prover, proofs, vals, 5)
    dev = gpu_verdicts(prover, proofs, vals, 5)
    assert dev == host
    assert sum(host) >= 256 and 2048 - sum(host) >= 256


@pytest.mark.parametrize("depth,multi", [(10, False), (20, True)])
def test_other_circuits(depth, multi):
    """64 generated proofs of the depth-10 and the multi-message-id circuit (more than 5 public inputs: the count comes
    from the key), whole and damaged, and their golden proof with its hand-made rejects"""
    from zerokit_amd import workload
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=64, depth=depth, multi=multi)
    try:
        named, rs = workload.circuit_range(1000, 64, depth, multi)
        k = p.upload(p.pack_named_inputs(named), rs)
        p.run(k)
        out, pub = p.download(k), p.download_public(k)
        nv = len(pub[0])
        assert nv == p.num_public and (nv > 5) == multi
        proofs = b"".join(o["proof"] for o in out)
        vals = b"".join(le(v) for row in pub for v in row)
        assert gpu_verdicts(p, proofs, vals, nv) == b"\x01" * 64
        rnd = random.Random(depth)
        pb, vb = bytearray(proofs), bytearray(vals)
        for i in range(0, 64, 2):
            if i % 4:
                pb[128 * i + rnd.randrange(128)] ^= 1 << rnd.randrange(8)
            else:
                j = rnd.randrange(nv)
                vb[32 * (nv * i + j):32 * (nv * i + j + 1)] = le(rnd.randrange(R))
        host = host_verdicts(p, bytes(pb), bytes(vb), nv)
        assert gpu_verdicts(p, bytes(pb), bytes(vb), nv) == host
        assert sum(host) == 32
        golden = [(nm, pr, pu) for nm, d, m, pr, pu in vc.golden_other() if (d, m) == (depth, multi)]
        names, gp, gv = case_rows(golden)
        host = host_verdicts(p, gp, gv, nv)
        assert list(gpu_verdicts(p, gp, gv, nv)) == list(host), names
        assert sum(host) == 1
        hv = host_gt_lib(depth, multi)
        for i, gt in enumerate(gpu_gt(p, gp, gv, nv)):
            want = C.create_string_buffer(384)
            hv.vmh_host_verify(gp[128 * i:128 * i + 128], gv[32 * nv * i:32 * nv * (i + 1)], nv, want)
            assert gt == want.raw, names[i]
    finally:
        p.close()


def test_any_n_runs_as_chunks(prover):
    """n = 0, 1, 63, 64, 65, one more than the chunk, three chunks and a ragged tail: rows tiled from the golden cases
    and their rejects, each verdict equal to the host's for that row"""
    names, proofs, vals = case_rows(vc.golden_h20())
    m = len(names)
    host = host_verdicts(prover, proofs, vals, 5)
    ch = chunk_size()
    assert gpu_verdicts(prover, b"", b"", 5) == b""
    for n in (1, 63, 64, 65, ch + 1, 3 * ch + 1237):
        off = n % 7   # not always the same row first
        reps = (off + n) // m + 1
        pr = (proofs * reps)[128 * off:128 * (off + n)]
        va = (vals * reps)[160 * off:160 * (off + n)]
        want = (host * reps)[off:off + n]
        assert gpu_verdicts(prover, pr, va, 5) == want, n


def test_verification_does_not_wait_for_or_disturb_proving(prover, generated):
    """(a) a 1 024-proof batch is submitted, 64 rows are verified on the device from the same thread before it is
    collected; (b) one thread streams proving batches while another verifies.  The verdicts are right and the proofs
    are byte-identical to a quiet run both times."""
    names, proofs, vals = case_rows(vc.golden_h20())
    proofs, vals = proofs[:128 * 64], vals[:160 * 64]
    host = host_verdicts(prover, proofs, vals, 5)
    t, n = prover.submit(generated["inputs"], generated["rs"])
    assert gpu_verdicts(prover, proofs, vals, 5) == host
    got, values, errs = prover.collect_raw(t, n)
    assert got == generated["proofs"] and values == generated["values"] and not any(errs)

    result, stop = {}, threading.Event()

    def prove():
        try:
            outs = []
            for _ in range(6):
                t, n = prover.submit(generated["inputs"], generated["rs"])
                outs.append(prover.collect_raw(t, n)[0])
            result["proofs"] = outs
        except Exception as e:  # noqa: BLE001
            result["error"] = e
        finally:
            stop.set()

    th = threading.Thread(target=prove)
    th.start()
    rounds = 0
    try:
        while not stop.is_set() or rounds == 0:
            assert gpu_verdicts(prover, proofs, vals, 5) == host
            rounds += 1
    finally:
        th.join()
    assert "error" not in result, result.get("error")
    assert all(o == generated["proofs"] for o in result["proofs"]) and rounds >= 1


def test_ffi_verify_rln_proofs_batch(tmp_path):
    """ffi_verify_rln_proofs_batch == a loop over verify_rln_proof / verify_with_roots (False where the loop raises),
    on the host branch and on the device branch ("verify_gpu_min"), for roots = None, a matching list, a non-matching
    list and an empty list, with a proof whose pairing fails, a proof made at an older root and one wrong signal"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.public import RLN, RLNProof, RLNWitnessInput
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"verify_gpu_min": 4}))
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
        assert host_obj.verify_rln_proofs_batch(proofs, xs, roots) == want, key       # 8 < 512: host threads
        assert dev_obj.verify_rln_proofs_batch(proofs, xs, roots) == want, key        # 8 >= 4: the device
        assert dev_obj.verify_rln_proofs_batch(proofs[:3], xs[:3], roots) == want[:3], key   # 3 < 4: host threads
    assert dev_obj.verify_rln_proofs_batch([], []) == []
    with pytest.raises(RLNError):
        dev_obj.verify_rln_proofs_batch(proofs, xs[:2])


def test_device_beats_sixteen_host_threads_at_8192(prover, generated):
    """a guard, not a benchmark: at n = 8 192 (the generated proofs tiled eight times) the median of 5 device calls is
    faster than the median of 5 rlnamd_verify_many(threads = 16) calls on the same inputs"""
    proofs, vals = generated["proofs"] * 8, generated["values"] * 8
    assert gpu_verdicts(prover, proofs, vals, 5) == b"\x01" * 8192   # warm-up, and the buffers at their size
    dev, host = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        ok = gpu_verdicts(prover, proofs, vals, 5)
        dev.append(time.perf_counter() - t0)
        assert ok == b"\x01" * 8192
    for _ in range(5):
        t0 = time.perf_counter()
        ok = host_verdicts(prover, proofs, vals, 5, threads=16)
        host.append(time.perf_counter() - t0)
        assert ok == b"\x01" * 8192
    d, h = statistics.median(dev), statistics.median(host)
    print("n = 8192: device %.1f ms (%.0f /s), 16 host threads %.1f ms (%.0f /s)" % (d * 1e3, 8192 / d, h * 1e3, 8192 / h))
    assert d < h
