"""The shared rows of the throughput plan on the device (prover_plan.h: G1Rows::shared): a big batch walks a proving-key
row that the A and B1 queries share once and k_glv_fold uses its sum twice.  Smallest tables (window_bits = 8), capacity
192, batches of 129 proofs -- the smallest that take the throughput plan (lanechunk_max = 128).  Everything is compared
byte for byte: RLNAMD_SHARED_ROWS=1 against =0 and against oracle/c on the three shipped circuits; on depth 20 also
partial then finish against the full proofs in both stream shapes, and the 129 adversarial witnesses of
tests/witness_edge_cases.py (all zero, C at infinity, edge GLV halves: the inputs under which a shared sum is the point at
infinity or meets the rest of A or B1 in a doubling or a cancellation) against oracle_prove_witness.

Per circuit and switch one prover and one batch, computed once and shared by the tests of the module."""
import os

import pytest

import shared_rows_cases as cases
import witness_edge_cases as wec

pytestmark = pytest.mark.gpu

N = 129
CAP = 192
WB = 8
CIRCUITS = [(20, False), (10, False), (20, True)]


def _tuning(text):
    return {k: v for k, v in (kv.split("=", 1) for kv in text.split() if "=" in kv)}


def _prover(shared, depth=20, multi=False, shape=None):
    from zerokit_amd.batch import BatchProver
    env = {"RLNAMD_SHARED_ROWS": str(shared)}
    if shape:
        env["RLNAMD_STREAM_SHAPE"] = shape
    saved = {k: os.environ.get(k) for k in ("RLNAMD_SHARED_ROWS", "RLNAMD_STREAM_SHAPE")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)                      # (read once, when the prover is built)
    try:
        p = BatchProver(max_batch=CAP, window_bits=WB, depth=depth, multi=multi)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    t = _tuning(p.describe())
    assert t["shared_rows"] == str(shared) and int(t["lanechunk"]) == N - 1, p.describe()
    if shape:
        assert t["stream_shape"] == shape
    return p


def _full(p, inp, rsb):
    """one streamed full batch -> (results, residue behind the wiping collect)"""
    out = p.collect(*p.submit(inp, rsb))
    return out, p.residue()


class _Run:
    """a circuit's batch of N under both settings of the switch"""

    def __init__(self, depth, multi):
        from zerokit_amd import workload
        self.depth, self.multi = depth, multi
        self.sub = cases.circuit_dir(depth, multi)
        self.named, self.rs = workload.circuit_range(7000, N, depth, multi)
        self.out, self.residue, self.g1_rows, self.provers = {}, {}, {}, {}
        for shared in (1, 0):
            p = _prover(shared, depth, multi)
            self.inp, self.rsb = p.pack_named_inputs(self.named), p.pack_rs(self.rs)
            self.out[shared], self.residue[shared] = _full(p, self.inp, self.rsb)
            self.g1_rows[shared] = int(p.info.g1_rows)
            self.windows = int(p.info.windows)
            if shared == 1 and depth == 20 and not multi:
                self.provers[1] = p             # (depth 20 goes on: the adversarial witnesses)
            else:
                p.close()


_made = {}


@pytest.fixture(scope="module", params=CIRCUITS, ids=["depth20", "depth10", "depth20_multi"])
def run(request):
    if request.param not in _made:
        _made[request.param] = _Run(*request.param)
    return _made[request.param]


@pytest.fixture(scope="module")
def run20():
    if CIRCUITS[0] not in _made:
        _made[CIRCUITS[0]] = _Run(*CIRCUITS[0])
    return _made[CIRCUITS[0]]


@pytest.fixture(scope="module", autouse=True)
def _close_provers():
    yield
    for r in _made.values():
        for p in r.provers.values():
            p.close()
    _made.clear()


def test_a_full_batch_is_the_same_bytes_with_and_without_the_shared_rows(run):
    on, off = run.out[1], run.out[0]
    assert len(on) == len(off) == N
    assert [o["error"] for o in on] == [0] * N == [o["error"] for o in off]
    assert [o["proof"] for o in on] == [o["proof"] for o in off]
    assert [o["public_inputs"] for o in on] == [o["public_inputs"] for o in off]
    assert len({o["proof"] for o in on}) == N
    for shared in (1, 0):
        assert not any(run.residue[shared].values()), (run.sub, shared, run.residue[shared])


def test_proofs_0_64_and_128_equal_the_c_oracle(run):
    from oracle.c import binding as ob
    o = ob.Circuit(run.depth, run.multi)
    for i in (0, 64, 128):
        ref = o.prove_packed(o.pack_named(run.named[i]), *run.rs[i])
        assert run.out[1][i]["proof"] == ref["proof"], (run.sub, i)


def test_g1_rows_counts_the_rows_the_plan_walks(run):
    """table rows minus the dropped B1 rows with the switch on, every table row with it off (bench.py prices the G1 walk
    by info.g1_rows x info.windows x batch)"""
    k = cases.key_facts(run.sub)
    shared = len(k["eq"]) + len(k["opp"])
    assert (len(k["eq"]), len(k["opp"])) == cases.COUNTS[run.sub]
    assert run.g1_rows[0] == k["table_rows"] and run.g1_rows[1] == k["table_rows"] - shared, (run.sub, run.g1_rows, k["table_rows"], shared)
    print("%s: %d table rows, %d walked; %d fewer lane additions per proof" % (run.sub, run.g1_rows[0], run.g1_rows[1], shared * run.windows))


@pytest.mark.parametrize("shape", ["wide", "compact"])
def test_depth_20_in_both_stream_shapes_full_and_partial_then_finish(run20, shape):
    """the full batch, then partial and finish of the same witnesses: all the bytes of the three-segment plan"""
    want = run20.out[0]
    p = _prover(1, shape=shape)
    try:
        out, residue = _full(p, run20.inp, run20.rsb)
        assert out == want and not any(residue.values()), (shape, residue)
        part = [dict(w, messageId=[0], x=[0], externalNullifier=[0]) for w in run20.named]
        partials = p.collect_partial(*p.submit(p.pack_named_inputs(part), bytes(64 * N), 1))
        assert len(set(partials)) == N and not any(p.residue().values())
        fin = p.collect(*p.submit(run20.inp, run20.rsb, 2, partials))
        assert fin == want, shape
        assert not any(p.residue().values()), (shape, p.residue())
    finally:
        p.close()


def test_depth_20_partial_proofs_are_the_same_bytes_without_the_shared_rows(run20):
    """the 320-byte partial proofs themselves (pi_a and rho hold S+ and S- of the known rows)"""
    part = [dict(w, messageId=[0], x=[0], externalNullifier=[0]) for w in run20.named]
    got = {}
    for shared in (1, 0):
        p = run20.provers[1] if shared else _prover(0)
        try:
            got[shared] = p.collect_partial(*p.submit(p.pack_named_inputs(part), bytes(64 * N), 1))
        finally:
            if not shared:
                p.close()
    assert got[1] == got[0] and len(set(got[1])) == N


def test_depth_20_adversarial_witnesses_equal_the_oracle(run20):
    """tests/witness_edge_cases.py's 129 witnesses, built for this prover's window schedule, as one big batch through
    prove_with_witness against oracle/c's oracle_prove_witness"""
    from oracle.c import binding as ob
    from zerokit_amd import workload
    p = run20.provers[1]
    wb = int(_tuning(p.describe())["window_bits"])
    assert wb == WB
    o = ob.Circuit(20, False)
    named, hrs = workload.circuit_range(5000, 96, 20, False)
    packed = [o.pack_named(w) for w in named]
    honest = [o.witness_packed(b) for b in packed]
    W, RS, labels, counts = wec.build(int(p.info.num_signals), p.num_public, wb, honest, hrs)
    wec.check_counts(counts)
    assert len(W) == N == wec.N_WITNESSES
    _, ref, _ = o.prove_many_witness(W, RS, threads=min(16, ob.usable_cores()))
    assert ref[0][96:] == bytes(31) + b"\x40"                    # all zero, r = s = 0: C is the point at infinity
    inputs = b"".join(packed[i % len(packed)] for i in range(N))
    blob = b"".join(v.to_bytes(32, "little") for w in W for v in w)
    out = p.prove_with_witness(inputs, [tuple(v % wec.R for v in rs) for rs in RS], blob)
    assert [x["error"] for x in out] == [0] * N
    bad = [(i, labels[i]) for i in range(N) if out[i]["proof"] != ref[i]]
    assert not bad, "proofs differ from the oracle's at (witness, category) %s" % bad[:8]
    p.wipe()
    assert not any(p.residue().values()), p.residue()
