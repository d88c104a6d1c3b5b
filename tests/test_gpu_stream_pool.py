"""GPU tests of the round-3 paths, all through the C ABI (include/rln_amd.h):

  * streamed batches (rlnamd_prover_submit / _collect): SURVEY 8(d)'s timed region, a fresh witness batch per call as
    in /root/reference/rln/src/protocol/proof.rs:753-777;
  * BASELINE config 2 at full size on the BENCH table schedule and config 4's 8 192-proof shard through the streaming
    API (skipped only when the device cannot hold the 228 GiB tables);
  * rlnamd_pool (native multi-GPU dispatcher) against a single prover, including two replicas sharing one device;
  * the RCCL path of config 5 in C (rlnamd_comm_*, rlnamd_msm_run_sharded) and the torch.distributed harness with the
    REAL device objects in two processes sharing the device (backend gloo).
Bit-exact everywhere: no tolerances."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_SCHEDULE = 7150114        # bench.py's comb schedule: G1 15 + 8 x 14 bits, G2 7 x 16 + 15 bits, 228 GiB


def _oracle(ws, rs):
    from oracle.c import binding as ob
    _, proofs, pub = ob.Circuit(20).prove_many(ws, rs)
    return proofs, pub


def _split(proofs, values, n):
    return ([proofs[128 * i:128 * i + 128] for i in range(n)],
            [[int.from_bytes(values[160 * i + 32 * k:160 * i + 32 * k + 32], "little") for k in range(5)]
             for i in range(n)])


@pytest.fixture(scope="module")
def prover():
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=256)
    yield p
    p.close()


def test_three_distinct_batches_back_to_back_without_sync(prover):
    """three DIFFERENT batches of different sizes enqueued back to back (no sync, no collect in between) come out
    bit-identical to oracle/c; then a fourth batch reuses the first slot after a wrap"""
    from zerokit_amd import workload
    sizes = [(0, 200), (200, 130), (330, 70)]
    packed = [workload.config2_packed(prover.slots, prover.inputs_size, f, n) for f, n in sizes]
    tickets = [prover.submit(inp, rsb) for inp, rsb in packed]
    assert [t for t, _ in tickets] == sorted(t for t, _ in tickets) and all(t > 0 for t, _ in tickets)
    got = [prover.collect(t, n) for t, n in reversed(tickets)][::-1]   # collecting out of order is allowed
    ws, rs = workload.config2_range(0, 400)
    ref_proofs, ref_pub = _oracle(ws, rs)
    for (f, n), out in zip(sizes, got):
        assert all(o["error"] == 0 for o in out)
        assert [o["proof"] for o in out] == ref_proofs[f:f + n]
        assert [o["public_inputs"] for o in out] == ref_pub[f:f + n]
    # wrap: more submits than slots; the expired ticket is refused, the live ones still match
    nslots = prover.n_slots()
    small = workload.config2_packed(prover.slots, prover.inputs_size, 0, 64)
    ts = [prover.submit(*small)[0] for _ in range(nslots + 1)]
    from zerokit_amd._native import RLNError
    with pytest.raises(RLNError, match="expired"):
        prover.collect(ts[0], 64)
    out = prover.collect(ts[-1], 64)
    assert [o["proof"] for o in out] == ref_proofs[:64]


def test_prove_stream_ragged_sizes_match_resident_path(prover):
    """rlnamd_prover_prove_stream over n that is not a multiple of the capacity (256): 256 + 256 + 88, and the empty
    job; the same bytes as upload + run + download of the same witnesses"""
    from zerokit_amd import workload
    n = 600
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 1000, n)
    proofs, values, errs = prover.prove_stream_raw(inp, rsb)
    assert not any(errs) and len(errs) == n
    ws, rs = workload.config2_range(1000, n)
    for lo in (0, 256, 512):
        cnt = min(256, n - lo)
        ref = prover.prove(ws[lo:lo + cnt], rs[lo:lo + cnt])
        assert [r["proof"] for r in ref] == [proofs[128 * i:128 * i + 128] for i in range(lo, lo + cnt)]
        assert b"".join(v.to_bytes(32, "little") for r in ref for v in r["public_inputs"]) == \
            values[160 * lo:160 * (lo + cnt)]
    assert prover.prove_stream_raw(b"", b"") == (b"", b"", [])


def test_streamed_partial_and_finish_match_full(prover):
    """PROVE_PARTIAL and PROVE_FINISH through submit / collect: partial + finish == full proof for the same (r, s)"""
    from zerokit_amd import workload
    n = 70
    ws, rs = workload.config2_range(5000, n)
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 5000, n)
    zero = dict(message_id=0, x=0, external_nullifier=0)
    pinp = prover.pack_inputs([dict(w, **zero) for w in ws])
    t, _ = prover.submit(pinp, prover.pack_rs([(0, 0)] * n), mode=1)
    partials = prover.collect_partial(t, n)
    assert partials == prover.prove_partial([{k: w[k] for k in ("identity_secret", "user_message_limit",
                                                                  "path_elements", "identity_path_index")} for w in ws])
    t2, _ = prover.submit(inp, rsb, mode=2, partials=partials)
    t3, _ = prover.submit(inp, rsb)
    fin, full = prover.collect(t2, n), prover.collect(t3, n)
    assert [o["proof"] for o in fin] == [o["proof"] for o in full]
    assert [o["public_inputs"] for o in fin] == [o["public_inputs"] for o in full]


def test_big_batch_partial_and_finish_match_full_and_oracle(prover):
    """the THROUGHPUT shapes of the three modes (200 proofs: lanes = proofs walks, pair chunks in every mode's plan):
    partial + finish == full, and the full proofs equal oracle/c on a sample"""
    from zerokit_amd import workload
    n = 200
    ws, rs = workload.config2_range(9000, n)
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 9000, n)
    zero = dict(message_id=0, x=0, external_nullifier=0)
    pinp = prover.pack_inputs([dict(w, **zero) for w in ws])
    t, _ = prover.submit(pinp, prover.pack_rs([(0, 0)] * n), mode=1)
    partials = prover.collect_partial(t, n)
    t2, _ = prover.submit(inp, rsb, mode=2, partials=partials)
    t3, _ = prover.submit(inp, rsb)
    fin, full = prover.collect(t2, n), prover.collect(t3, n)
    assert all(o["error"] == 0 for o in fin + full)
    assert [o["proof"] for o in fin] == [o["proof"] for o in full]
    assert [o["public_inputs"] for o in fin] == [o["public_inputs"] for o in full]
    idx = [0, 63, 64, 127, 128, 199]
    ref_proofs, ref_pub = _oracle([ws[i] for i in idx], [rs[i] for i in idx])
    assert [full[i]["proof"] for i in idx] == ref_proofs
    assert [full[i]["public_inputs"] for i in idx] == ref_pub


# ---------------------------------------------------------------------------------------------------- pool
def test_secrets_are_wiped_behind_collect_and_on_request(prover):
    """the reference zeroises the identity secret and the witness calculator's inputs (rln/src/utils.rs:440-527,
    rln/src/circuit/iden3calc.rs:45-56).  Here: after collect the slot's witness values read back as zeros and its
    public signals are refused; the resident path keeps its witness for the parity taps until wipe(), then reads zeros;
    proofs made after a wipe are unchanged"""
    import ctypes as C
    from zerokit_amd import lib, workload
    from zerokit_amd._native import RLNError, check
    ws, rs = workload.config2_range(300, 5)
    ref = prover.prove(ws, rs)
    w0 = prover.fetch_witness(0)
    assert any(w0) and w0[0] == 1
    # the window digits re-encode every witness scalar (and r, s) without loss; a | b | c and the walks' partial sums are
    # images of the witness: all present before the wipe, all zero behind it
    left = prover.residue()
    assert left["digits_g1"] and left["digits_g2"] and left["abc"] and left["partial_g1"] and left["partial_g2"]
    prover.wipe()
    assert not any(prover.fetch_witness(0)) and not any(prover.fetch_witness(4))
    inp, rsb = prover.pack_inputs(ws), prover.pack_rs(rs)
    t, n = prover.submit(inp, rsb)
    got = prover.collect(t, n)
    assert [g["proof"] for g in got] == [r["proof"] for r in ref]
    assert not any(prover.fetch_witness(0))                     # the streamed batch's slot is the last run: wiped by collect
    out = C.create_string_buffer(32 * 5 * 5)
    assert lib().rlnamd_prover_collect_public(prover._h, t, 5, out) != 0
    assert "wiped" in lib().rlnamd_last_error().decode()
    # collect_public BEFORE collect is the supported order
    t, n = prover.submit(inp, rsb)
    check(lib().rlnamd_prover_collect_public(prover._h, t, 5, out))
    pub0 = [int.from_bytes(out.raw[32 * k:32 * k + 32], "little") for k in range(5)]
    assert pub0 == ref[0]["public_inputs"]
    prover.collect(t, n)
    assert prover.prove(ws, rs) == ref                          # nothing the next batch needs was wiped
    assert any(prover.fetch_witness(0))


def test_nothing_derived_from_the_witness_outlives_a_collected_batch():
    """the signed window digits are a lossless re-encoding of every witness scalar (identity secret, r, s),
    a | b | c and the walks' partial sums are images of the witness.  On a prover of its own (so that no earlier
    resident run left anything): behind every collect -- throughput shape (200 proofs, digit stride = capacity), small
    shapes (70: lanes = proofs short chunks; 20; 3: one row per lane, compact digit rows) -- every 16-byte word of the
    slot's digit rows, a | b | c, partial sums and staged inputs is zero; the bytes returned stay those of the oracle"""
    from zerokit_amd import workload
    from zerokit_amd.batch import BatchProver
    p = BatchProver(max_batch=256)
    try:
        ws, rs = workload.config2_range(0, 423)
        ref_proofs, _ = _oracle(ws, rs)
        for first, n in ((0, 200), (200, 70), (270, 20), (290, 3), (293, 130)):
            inp, rsb = workload.config2_packed(p.slots, p.inputs_size, first, n)
            t, k = p.submit(inp, rsb)
            got = p.collect(t, k)
            left = p.residue()
            assert not any(left.values()), (n, left)
            assert [g["proof"] for g in got] == ref_proofs[first:first + n], n
        # a resident run keeps everything for the parity taps until it is wiped
        ws, rs = workload.config2_range(300, 5)
        p.prove(ws, rs)
        left = p.residue()
        assert left["digits_g1"] and left["digits_g2"] and left["abc"] and left["partial_g1"] and left["partial_g2"]
        p.wipe()
        assert not any(p.residue().values()), p.residue()
    finally:
        p.close()


def test_pool_of_one_and_two_replicas_on_one_device_equal_single_prover(prover):
    """rlnamd_pool: a pool of one replica and a pool of two replicas sharing device 0 return, index for index, the
    bytes of a single prover (ragged n = 301: shards of 128 + 173 proofs, chunks of 128)"""
    from zerokit_amd import workload
    from zerokit_amd.batch import ProverPool
    n = 301
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 3000, n)
    ref = prover.prove_stream_raw(inp, rsb)
    for devices in ([0], [0, 0]):
        pool = ProverPool(devices=devices, max_batch=128)
        assert pool.size == len(devices) and pool.devices == devices
        got = pool.prove_raw(inp, rsb)
        got2 = pool.prove_raw(inp, rsb)            # a second job on the same replicas
        assert got == ref and got2 == ref
        assert pool.prove_raw(b"", b"") == (b"", b"", [])
        gp, gv = _split(got[0], got[1], n)
        assert all(pool.verify_many(gp[:8], gv[:8]))
        pool.close()
    from zerokit_amd._native import RLNError
    with pytest.raises(RLNError, match="does not exist"):
        ProverPool(devices=[0, 63], max_batch=64)


def test_pool_dynamic_assignment_is_index_identical_and_a_failed_replica_does_not_take_the_pool_down(prover):
    """VERDICT r4 item 7.  (a) chunk-granular dynamic assignment -- a cursor shared by the replicas over chunks of
    max_batch proofs -- returns, index for index, the bytes of the static contiguous shards and of a single prover
    (ragged n = 1 000 over two replicas with 128-proof chunks: 7 full chunks + 104), and every proof is made exactly
    once; (b) a replica that throws in the middle of a job (test hook): the call returns an error naming the device, the
    other replica finishes, nothing of the failed replica's batches stays behind unwiped, and the next job on the same
    pool -- static or dynamic -- is complete and correct."""
    from zerokit_amd import workload
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import ProverPool
    n = 1000
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 9000, n)
    ref = prover.prove_stream_raw(inp, rsb)
    pool = ProverPool(devices=[0, 0], max_batch=128)
    try:
        static = pool.prove_raw(inp, rsb)
        assert static == ref and sum(pool.last_proofs()) == n and pool.last_proofs() == [512, 488]
        pool.set_dynamic(True)
        for _ in range(2):
            dyn = pool.prove_raw(inp, rsb)
            took = pool.last_proofs()
            assert dyn == ref, "dynamic assignment changed a byte"
            assert sum(took) == n and all(took), took
        small = pool.prove_raw(inp[:5 * prover.inputs_size * 32], rsb[:5 * 64])     # fewer chunks than replicas
        assert small[0] == ref[0][:5 * 128] and sum(pool.last_proofs()) == 5
        # (b) the fault: replica 1 throws when it is handed its second next chunk
        for dynamic in (True, False):
            pool.set_dynamic(dynamic)
            pool.inject_fault(1, after_chunks=1)
            with pytest.raises(RLNError, match="injected fault"):
                pool.prove_raw(inp, rsb)
            assert pool.last_proofs()[0] > 0                      # the healthy replica went on
            again = pool.prove_raw(inp, rsb)                      # the pool is usable, the hook was one shot
            assert again == ref and sum(pool.last_proofs()) == n
    finally:
        pool.close()
    # eight replicas (one device), 64-proof chunks: 16 chunks drawn from the shared cursor by eight workers at once; a
    # replica failing on its first chunk while seven others keep drawing
    pool = ProverPool(devices=[0] * 8, max_batch=64, window_bits=8)
    try:
        pool.set_dynamic(True)
        dyn = pool.prove_raw(inp, rsb)
        assert dyn == ref and sum(pool.last_proofs()) == n and sum(1 for k in pool.last_proofs() if k) >= 4
        pool.inject_fault(5, after_chunks=0)
        with pytest.raises(RLNError, match="injected fault"):
            pool.prove_raw(inp, rsb)
        assert pool.prove_raw(inp, rsb) == ref
        pool.set_dynamic(False)
        assert pool.prove_raw(inp, rsb) == ref and pool.last_proofs() == [128] * 7 + [104]
    finally:
        pool.close()


def test_pool_failover_reproves_a_failed_replicas_chunks_on_the_others(prover):
    """rlnamd_pool_set_failover: a replica that throws in the middle of a job (test hook) no longer fails the job --
    everything it had been handed, and what it had not reached of its static shard, is proved again by the replicas that
    finished, the result is byte-identical to a single prover's, the failed replica is quarantined (later jobs are cut
    among the others) until revive().  Static and dynamic assignment, two and eight replicas; with every replica
    quarantined, and with the rounds spent, the job fails with the first error."""
    from zerokit_amd import workload
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import ProverPool
    n = 1000
    inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, 9000, n)
    ref = prover.prove_stream_raw(inp, rsb)
    pool = ProverPool(devices=[0, 0], max_batch=128)
    try:
        pool.set_failover(1)
        for dynamic in (False, True):
            pool.set_dynamic(dynamic)
            pool.inject_fault(1, after_chunks=1)        # replica 1: one chunk in flight, fails when it asks for the next
            got = pool.prove_raw(inp, rsb)
            assert got == ref, "failover changed a byte"
            assert pool.health()[1][0] and not pool.health()[0][0]
            took = pool.last_proofs()
            assert took[1] == 0 and took[0] >= n, took   # replica 0 made its own chunks and replica 1's again
            got = pool.prove_raw(inp, rsb)              # quarantined: the whole job on replica 0
            assert got == ref and pool.last_proofs() == [n, 0]
            pool.revive(1)
            assert pool.prove_raw(inp, rsb) == ref and all(pool.last_proofs())
        assert [f for _, f in pool.health()] == [0, 2]
        # the survivor fails as well: nobody left
        pool.set_dynamic(False)
        pool.inject_fault(0, after_chunks=0)
        pool.prove_raw(inp, rsb)                        # replica 0 quarantined, replica 1 takes over
        assert [q for q, _ in pool.health()] == [True, False]
        pool.inject_fault(1, after_chunks=2)
        with pytest.raises(RLNError, match="no replica left"):
            pool.prove_raw(inp, rsb)
        with pytest.raises(RLNError, match="every replica is quarantined"):
            pool.prove_raw(inp, rsb)
        pool.revive(0)
        pool.revive(1)
        assert pool.prove_raw(inp, rsb) == ref
        # probation (what an FFI object's pool runs with: its callers cannot call revive): a quarantined replica sits
        # out two jobs and is handed work again by itself; with nobody left everybody is tried again at once
        pool.set_probation(2)
        pool.inject_fault(1, after_chunks=1)
        assert pool.prove_raw(inp, rsb) == ref and pool.health()[1][0]
        for _ in range(2):
            assert pool.prove_raw(inp, rsb) == ref and pool.last_proofs() == [n, 0]
        assert pool.prove_raw(inp, rsb) == ref and all(pool.last_proofs()) and not pool.health()[1][0]
        pool.inject_fault(0, after_chunks=0)
        assert pool.prove_raw(inp, rsb) == ref and pool.health()[0][0]
        pool.inject_fault(1, after_chunks=0)
        with pytest.raises(RLNError, match="no replica left"):
            pool.prove_raw(inp, rsb)
        assert [q for q, _ in pool.health()] == [True, True]
        assert pool.prove_raw(inp, rsb) == ref and all(pool.last_proofs())   # both back at once
    finally:
        pool.close()
    pool = ProverPool(devices=[0] * 8, max_batch=64, window_bits=8)
    try:
        pool.set_failover(2)
        pool.set_dynamic(True)
        pool.inject_fault(5, after_chunks=0)
        assert pool.prove_raw(inp, rsb) == ref
        assert [q for q, _ in pool.health()] == [k == 5 for k in range(8)]
        pool.set_dynamic(False)
        pool.inject_fault(2, after_chunks=1)            # static: seven shards, the third one fails after one chunk
        assert pool.prove_raw(inp, rsb) == ref
        assert [q for q, _ in pool.health()] == [k in (2, 5) for k in range(8)]
        assert pool.prove_raw(inp, rsb) == ref and sum(pool.last_proofs()) == n
    finally:
        pool.close()


# ---------------------------------------------------------------------------------------------------- RCCL in C
def test_msm_run_sharded_single_rank_communicator_vs_closed_form():
    """config 5 through the C ABI only: RCCL communicator of one rank (rlnamd_comm_init_rank), 2^18 generated points,
    local Pippenger + ncclAllGather + fold == the oracle's (sum k_i s_i) G; and the one-process multi-device entry with
    one device"""
    import ctypes as C
    from oracle.c import binding as ob
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import Comm, MsmG1
    n = 1 << 18
    comm = Comm.init_rank(Comm.unique_id(), 1, 0)
    assert comm.ranks() == 1
    m = MsmG1(n)
    m.generate(0xC0FFEE, 0, n)
    res, ms = m.run_sharded(comm)
    assert res == ob.msm_expected(0xC0FFEE, 0, n)
    assert set(ms) == {"sort_ms", "buckets_ms", "all_gather_ms", "combine_ms"} and ms["buckets_ms"] > 0
    # same object, host-gather path: identical point
    blob, _ = m.run_windows()
    assert m.combine([blob]) == res
    m.close()
    comm.close()
    out = C.create_string_buffer(64)
    ms5 = (C.c_float * 5)()
    devs = (C.c_int * 1)(0)
    check(lib().rlnamd_msm_generated_multi(devs, 1, 0xC0FFEE, n, 0, 2, out, ms5))
    assert (int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")) == res


# ------------------------------------------------------------------------------- two processes, one device
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_WORKER = r"""
import json, os, sys
sys.path.insert(0, os.environ["RLN_ROOT"])
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
from zerokit_amd import workload
from zerokit_amd.batch import BatchProver, MsmG1
from zerokit_amd.distributed import msm_sharded, prove_sharded, shard_bounds
n_total = 1 << 18
lo, hi = shard_bounds(n_total, world)[rank]
m = MsmG1(hi - lo)
res, _ = msm_sharded(m, 0xC0FFEE, n_total)            # the REAL device MSM on this rank's slice + all_gather + fold
m.close()
p = BatchProver(max_batch=64)
dist.barrier()                                        # both ranks (and the test's own process) hold a prover on the device now
import time
time.sleep(0.06)                                      # (the neighbour probe is taken at most every 50 ms)
shared = p.device_shared()
ws, rs = workload.config2_range(0, 37)                # ragged: shards of 19 and 18
out = prove_sharded(p.prove, ws, rs)                  # the REAL device prover as prove_fn
p.close()
if rank == 0:
    print("RESULT " + json.dumps({"msm": [str(res[0]), str(res[1])], "proofs": [o["proof"].hex() for o in out],
                                  "pub": [[str(v) for v in o["public_inputs"]] for o in out], "shared": shared}))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_processes_sharing_the_device_msm_sharded_and_prove_sharded(prover):
    """zerokit_amd.distributed with the product objects under world size 2: two processes share the one GPU
    (backend gloo); msm_sharded(MsmG1) at 2^18 equals the closed form, prove_sharded(BatchProver.prove) equals a
    single-process run; and every process SEES the others' provers on its device (rlnamd_prover_device_shared, bit 1)"""
    import json
    import time
    from zerokit_amd import workload
    from zerokit_amd.batch import MsmG1
    time.sleep(0.06)
    assert prover.device_shared() & 2 == 0          # no other PROCESS proves on this device yet (round 6: the neighbour probe)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   RLN_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-c", _WORKER], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    line = next(l for l in outs[0][0].splitlines() if l.startswith("RESULT "))
    got = json.loads(line[7:])
    from oracle.c import binding as ob
    exp = ob.msm_expected(0xC0FFEE, 0, 1 << 18)
    assert (int(got["msm"][0]), int(got["msm"][1])) == exp
    assert got["shared"] & 2, "a prover in another process on the same device was not seen"
    ws, rs = workload.config2_range(0, 37)
    ref = prover.prove(ws, rs)
    assert got["proofs"] == [o["proof"].hex() for o in ref]
    assert got["pub"] == [[str(v) for v in o["public_inputs"]] for o in ref]


# ------------------------------------------------------------------------------- eight-way readiness on one device
def test_config4_full_65536_over_eight_replicas_on_one_device_boundaries_vs_c_oracle():
    """BASELINE config 4 at its FULL size through the multi-GPU code path: 65 536 proofs over EIGHT prover replicas
    (rlnamd_pool with the one device listed eight times: eight host threads, eight sets of tables and workspaces, c = 8
    tables so that they fit beside each other), contiguous shards of 8 192.  No error flag, no two proofs equal, every
    shard boundary (last index of shard k, first of shard k + 1) and the ends byte-equal to oracle/c, a sample verified"""
    from zerokit_amd import workload
    from zerokit_amd.batch import ProverPool
    n, shard = 65536, 8192
    from zerokit_amd.batch import BatchProver
    probe = BatchProver(max_batch=64, window_bits=8)       # the input slots come from the graph; any prover knows them
    slots = dict(probe.slots)
    probe.close()
    pool = ProverPool(devices=[0] * 8, max_batch=1024, window_bits=8)
    try:
        assert pool.size == 8
        inputs, rsb = workload.config2_packed(slots, pool.inputs_size, 0, n)
        proofs, values, errs = pool.prove_raw(inputs, rsb)
        assert not any(errs)
        ms = pool.last_ms()
        assert len(ms) == 8 and all(m > 0 for m in ms)
        got_proofs, got_pub = _split(proofs, values, n)
        assert len(set(got_proofs)) == n
        idx = sorted({0, n - 1} | {k * shard - 1 for k in range(1, 8)} | {k * shard for k in range(1, 8)} |
                     {k * shard + 1023 for k in range(8)} | {k * shard + 1024 for k in range(8)})
        ws, rs = [], []
        for i in idx:
            w, r = workload.config2_range(i, 1)
            ws += w
            rs += r
        ref_proofs, ref_pub = _oracle(ws, rs)
        assert [got_proofs[i] for i in idx] == ref_proofs
        assert [got_pub[i] for i in idx] == ref_pub
        sample = list(range(0, n, 1009))
        assert all(pool.verify_many([got_proofs[i] for i in sample], [got_pub[i] for i in sample]))
    finally:
        pool.close()


def test_bench_under_torchrun_with_four_ranks_on_one_device():
    """`bench.py --gpus 4` the way the driver launches a multi-GPU run (python -m torch.distributed.run, one process per
    rank), on a box with ONE device: every rank is pinned to device 0 (RLNAMD_BENCH_DEVICE) with gloo in place of RCCL,
    which refuses two ranks on one device, and small tables so that the provers fit.  Four ranks, so that together with
    this process no more than five processes hold the device.  rc 0, exactly one JSON line on stdout, n_gpus 4,
    config 4 (4 x 8 192 proofs per step), verified"""
    import json
    port = _free_port()
    env = dict(os.environ, RLNAMD_BENCH_DEVICE="0", RLNAMD_BENCH_BACKEND="gloo", RLNAMD_WINDOW_BITS="8",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0",
           "--no-side-configs"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["steps"] == 1 and d["unit"] == "proofs/s" and d["scaling"] == "weak"
    assert d["config"]["verified"] is True and d["config"]["batch_per_gpu"] == 8192
    assert abs(d["value"] - 4 * 8192 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    # (under the real backend a line is only printed when RCCL had --gpus ranks; this run says it had none)
    assert d["rccl_ranks"] is None and "test hook" in d["rccl_ranks_source"]


def _bench(args, env_extra, timeout=900):
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_side_workloads_and_the_one_process_pool_mode_each_print_one_checked_line():
    """the other ways bench.py is run, each to ONE JSON line whose `correct` / `verified` flag is the oracle's or the host
    verifier's: plain `--gpus 2` (one process driving an rlnamd_pool; two replicas on this device through the test hook,
    small tables), `--workload msm` (config 5 at 2^16 with the shard timing), `--workload merkle` (config 3), and the
    default line's new objects on small tables (both walks under `roofline.kernels`, `whole_step`, `init_ms`)"""
    d = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"RLNAMD_BENCH_POOL_DEVICES": "0,0", "RLNAMD_WINDOW_BITS": "8"})
    assert d["n_gpus"] == 2 and d["config"]["verified"] is True and d["config"]["batch_per_gpu"] == 8192
    assert abs(d["value"] - 2 * 8192 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3 and len(d["replica_ms_last_step"]) == 2
    d = _bench(["--workload", "msm", "--steps", "2"], {"RLNAMD_MSM_LOG2": "16"})
    assert d["correct"] is True and d["rccl_ranks"] == 1 and d["shard_2^13"]["correct"] is True
    assert d["shard_2^13"]["points"] == 1 << 13 and d["stage_ms_rank0"]["combine_ms"] < 1.0      # the fold on the host
    assert d["g2_2^14"]["correct"] is True and d["g2_2^14"]["points"] == 1 << 14                  # the same MSM on the twist
    d = _bench(["--workload", "merkle", "--steps", "1"], {})
    assert d["correct"] is True and d["paths_failed_device_verification"] == 0
    assert d["updates_ffi"]["single_update_plus_root_ms_median"] < 1.5                              # the host chain (3 ms on the device)
    # round 6: the default line also carries the steady-state leg and the finish-from-partial object (small tables,
    # 256 per batch here)
    d = _bench(["--steps", "3", "--warmup", "1", "--batch", "256", "--side", "finish,latency", "--sustained-seconds", "1.5",
                "--cpu-seconds", "1"], {"RLNAMD_WINDOW_BITS": "8"})
    assert d["config"]["verified"] is True and set(d["config"]["init_ms"]) == {"parse", "table_alloc", "table_build", "rest"}
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and r["peaks"]["mad_slot_peak_Ginst_per_s"] == 614.4
    # (the issue-cycle view belongs to the bench schedule and batch: on other tables the line says it was left out)
    assert r["kernels"] is None and "issue_view_omitted" in r
    # finished proofs byte-identical to the full ones, partial points and the finished proof of witness 0 judged by
    # oracle/c, the CPU port's full / partial / finish beside them; then `--workload finish` by itself
    su, f = d["sustained"], d["finish"]
    assert su["seconds"] >= 1.5 and su["same_bytes_as_the_timed_region"] is True and 0.5 < su["ratio_to_value"] < 1.5
    assert su["batches"] * 256 / su["seconds"] == pytest.approx(su["proofs_per_s"], rel=2e-2) and len(su["proofs_per_s_by_quarter"]) >= 3
    assert f["correct"] is True and f["byte_identical_to_the_full_proofs"] is True and f["single_call_byte_identical"] is True
    assert f["proofs_per_s"] > f["full_proofs_per_s"] and f["single_call_took_the_cone"] is True
    assert 0 < f["single_call_ms_median"] < f["single_call_whole_graph_ms_median"]
    assert f["witness_program_steps"]["cone"] * 8 < f["witness_program_steps"]["full"]
    cb = f["cpu_baseline"]
    assert cb["gpu_partial_points_equal_oracle"] is True and cb["gpu_finish_equals_oracle_finish"] is True
    assert cb["finish_equals_full"] is True and cb["single_thread_ms"]["finish"] < cb["single_thread_ms"]["full"]
    d = _bench(["--workload", "finish", "--steps", "3", "--warmup", "1", "--batch", "256"], {"RLNAMD_WINDOW_BITS": "8"})
    assert d["config"]["verified"] is True and "finish_rln_proof" in d["metric"]


# ------------------------------------------------------------------- full sizes on the bench schedule (last: 228 GiB)
@pytest.fixture(scope="module")
def bench_prover():
    from zerokit_amd._native import RLNError
    from zerokit_amd.batch import BatchProver
    try:
        p = BatchProver(max_batch=1024, window_bits=BENCH_SCHEDULE)
    except RLNError as e:
        if "out of memory" in str(e).lower() or "hipErrorOutOfMemory" in str(e):
            pytest.skip("the device cannot hold the 228 GiB bench tables: %s" % e)
        raise
    yield p
    p.close()


def test_config2_full_size_on_the_bench_schedule_vs_c_oracle(bench_prover):
    """BASELINE config 2 exactly as bench.py runs it: 1 024 proofs on the 228 GiB GLV comb schedule (16-bit digits at
    the int16 edge), streamed; every proof and every public value bit-identical to oracle/c"""
    from zerokit_amd import workload
    p = bench_prover
    assert int(p.info.windows) == 18 and int(p.info.windows_g2) == 16 and int(p.info.glv) == 1
    n = 1024
    proofs, values, errs = p.prove_stream_raw(*workload.config2_packed(p.slots, p.inputs_size, 0, n))
    assert not any(errs)
    from conftest import oracle_config2
    ws, rs, ref_proofs, ref_pub = oracle_config2(0, n)
    got_proofs, got_pub = _split(proofs, values, n)
    assert got_proofs == ref_proofs
    assert got_pub == ref_pub


def test_config4_shard_8192_streamed_all_verified_sampled_vs_c_oracle(bench_prover):
    """BASELINE config 4's per-GPU shard: witnesses 8 192 .. 16 384 of the 65 536-index stream (the shard of GPU 1)
    through the streaming API on the bench schedule; all 8 192 verify (rlnamd_verify_many), 96 sampled indices are
    byte-equal to oracle/c, and no two proofs coincide"""
    from zerokit_amd import workload
    p = bench_prover
    first, n = 8192, 8192
    proofs, values, errs = p.prove_stream_raw(*workload.config2_packed(p.slots, p.inputs_size, first, n))
    assert not any(errs)
    got_proofs, got_pub = _split(proofs, values, n)
    assert all(p.verify_many(got_proofs, got_pub))
    assert len(set(got_proofs)) == n
    idx = sorted(set(list(range(0, n, 89)) + [1023, 1024, 8191]))
    assert len(idx) >= 64
    ws, rs = workload.config2_range(first, n)
    ref_proofs, ref_pub = _oracle([ws[i] for i in idx], [rs[i] for i in idx])
    assert [got_proofs[i] for i in idx] == ref_proofs
    assert [got_pub[i] for i in idx] == ref_pub
