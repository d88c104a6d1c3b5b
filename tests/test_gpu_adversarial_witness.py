"""The device against the oracle over adversarial witnesses (tests/witness_edge_cases.py): scalars 0, 1, r - 1, lambda, a
GLV half of 0, halves at the split's bound, window values of exactly 2^(c-1) on either schedule, carries through every
window, w_0 != 1, values >= r, a proof whose C is the point at infinity -- none of which an honest RLN witness holds.  They
enter through BatchProver.prove_with_witness (rlnamd_prover_upload_witness, k_scatter_witness); the reference is oracle/c's
oracle_prove_witness, pinned to the Python oracle in tests/test_oracle_c.py.  Everything is compared exactly.

Per shipped circuit one prover (default tables, max_batch 192) and one run of the oracle over the 129 witnesses, shared by
the tests of the module.  Batch sizes: 1, tiny_max, lanechunk_walk_max, ntt_lg_max, ntt_lg_max + 1, lanechunk_max + 1 --
read from rlnamd_prover_describe -- i.e. the lone shape, the tiny shape, lanes = chunks at its bound, the LDS transforms at
theirs, the passes, and the big batch with its lone lane in the third group.  Each size walks its own rotation of the 129 in
consecutive batches, so every witness is proved at every size, in lane 0 and in a last lane (size 1); the 129-proof batch is
run once more per witness of LONE_LANE with that witness in lane 128.  After every batch: rlnamd_prover_wipe, then
rlnamd_prover_residue all zero (the uploaded witness is counted in its field 5)."""
import time

import pytest

import witness_edge_cases as wec

pytestmark = pytest.mark.gpu

R = wec.R
N = wec.N_WITNESSES
CIRCUITS = [(20, False), (10, False), (20, True)]
LONE_LANE = ("zero_rs_zero", "tie_pos_g1", "tie_neg_g1", "tie_pos_g2", "tie_neg_g2")
UNSATISFYING = ("all_one", "all_r_minus_1", "single_at_1", "w0_0", "w0_2", "w0_r_minus_1", "ripple")


def _tuning(text):
    return {k: v for k, v in (kv.split("=", 1) for kv in text.split() if "=" in kv)}


class _Circuit:
    def __init__(self, depth, multi):
        from oracle.c import binding as ob
        from zerokit_amd import workload
        from zerokit_amd.batch import BatchProver
        self.depth, self.multi = depth, multi
        self.name = "tree_depth_%d%s" % (depth, "_multi" if multi else "")
        t0 = time.perf_counter()
        self.p = p = BatchProver(max_batch=192, depth=depth, multi=multi)
        self.t_prover = time.perf_counter() - t0
        self.tune = _tuning(p.describe())
        wb = int(self.tune["window_bits"])
        cw1, cw2 = wec.schedules(wb)
        # the schedules the witnesses are built for are the prover's
        assert (int(p.info.window_bits), int(p.info.windows)) == (min(cw1), 2 * len(cw1)), (wb, cw1)
        assert (int(p.info.window_bits_g2), int(p.info.windows_g2)) == (min(cw2), 2 * len(cw2)), (wb, cw2)
        self.ns, self.n = int(p.info.num_signals), int(p.info.domain_size)
        t0 = time.perf_counter()
        o = ob.Circuit(depth, multi)
        assert (o.n_signals, o.domain, o.n_public) == (self.ns, self.n, p.num_public)
        named, hrs = workload.circuit_range(5000, 96, depth, multi)
        self.packed = [o.pack_named(w) for w in named]
        assert p.pack_named_inputs(named[:2]) == self.packed[0] + self.packed[1]
        honest = [o.witness_packed(b) for b in self.packed]
        self.W, self.RS, self.labels, self.counts = wec.build(self.ns, p.num_public, wb, honest, hrs)
        self.blob = [b"".join(v.to_bytes(32, "little") for v in w) for w in self.W]
        self.honest_pub = {i: [v % R for v in self.W[i][1:1 + p.num_public]] for i in range(N)}
        secs, self.ref, self.ref_h = o.prove_many_witness(self.W, self.RS, threads=min(16, ob.usable_cores()), want_h=True)
        self.t_oracle = time.perf_counter() - t0
        self.edges = set(wec.edge_indices(self.labels))
        self.proved = {}          # size -> [proof bytes per witness]
        print("%s: prover %.1f s; oracle %.1f s for %d witnesses (%.2f s of proving on its threads); window_bits %d"
              % (self.name, self.t_prover, self.t_oracle, N, secs, wb))

    def sizes(self):
        t = self.tune
        s = [1, int(t["tiny"]), int(t["lanechunk_walk"]), int(t["ntt_lg_max"]), int(t["ntt_lg_max"]) + 1, int(t["lanechunk"]) + 1]
        assert s == sorted(set(s)) and s[-1] == N <= int(self.p.info.capacity), s
        return s

    def run(self, idx, check_h=True):
        """one batch of the witnesses idx through prove_with_witness: error 0, the oracle's bytes, the oracle's h for the
        edge witnesses, and nothing left behind the wipe (a resident run keeps its data until rlnamd_prover_wipe, which
        covers the LAST run: every run is wiped, as ffi_generate_rln_proof_with_witness does) -> the proofs"""
        p = self.p
        inputs = b"".join(self.packed[i % len(self.packed)] for i in idx)
        out = p.prove_with_witness(inputs, [tuple(v % R for v in self.RS[i]) for i in idx], b"".join(self.blob[i] for i in idx))
        assert [o["error"] for o in out] == [0] * len(idx)
        bad = [(lane, i, self.labels[i]) for lane, i in enumerate(idx) if out[lane]["proof"] != self.ref[i]]
        assert not bad, "%s, batch of %d: proofs differ from the oracle's at (lane, witness, category) %s" % (self.name, len(idx), bad[:8])
        if check_h:
            import ctypes as C
            from zerokit_amd import lib
            from zerokit_amd._native import check
            buf = C.create_string_buffer(32 * self.n)
            for lane, i in enumerate(idx):
                if i in self.edges:
                    check(lib().rlnamd_prover_fetch_h(p._h, lane, buf))
                    assert buf.raw == self.ref_h[i], (self.name, len(idx), lane, self.labels[i])
        p.wipe()
        res = p.residue()
        assert not any(res.values()), (self.name, len(idx), res)     # the uploaded witness included (field "inputs")
        return [o["proof"] for o in out]


_made = {}


@pytest.fixture(scope="module", params=CIRCUITS, ids=["depth20", "depth10", "depth20_multi"])
def circuit(request):
    if request.param not in _made:
        _made[request.param] = _Circuit(*request.param)
    return _made[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_provers():
    yield
    for c in _made.values():
        c.p.close()
    _made.clear()


def test_the_witnesses_hold_every_category(circuit):
    print(circuit.name, circuit.counts)
    wec.check_counts(circuit.counts)
    assert circuit.ref[0][96:] == bytes(31) + b"\x40"            # all zero, r = s = 0: C is the point at infinity
    assert not any(circuit.ref_h[0])


@pytest.mark.parametrize("which", range(6), ids=["lone", "tiny", "lanes_chunks", "lds_ntt_bound", "passes", "big"])
def test_every_witness_at_this_batch_size_equals_the_oracle(circuit, which):
    c = circuit
    k = c.sizes()[which]
    t0 = time.perf_counter()
    hinted0 = c.p.hint_stats()["hinted_batches"]
    rot = 29 * (which + 1) % N                                   # a rotation of its own per size
    order = [(rot + j) % N for j in range(N)]
    runs = 0
    for b in range(0, N, k):
        idx = order[b:b + k]
        idx += order[:k - len(idx)]                              # the last batch wraps, so that it has the size too
        c.run(idx)
        runs += 1
    if k == N:
        for lb in LONE_LANE:                                     # ... and in the lone lane of the third group
            i = c.labels.index(lb)
            c.run([(i + 1 + j) % N for j in range(N)])
            runs += 1
    print("%s: %d batches of %d in %.2f s; a resident run takes no hinted segments (hinted batches %d -> %d), the other shapes "
          "are submit's: %s" % (c.name, runs, k, time.perf_counter() - t0, hinted0, c.p.hint_stats()["hinted_batches"],
                                " ".join("%s=%s" % (n, c.tune[n]) for n in ("tiny", "lanechunk_walk", "ntt_lg_max", "lanechunk", "lone"))))


def test_w0_follows_the_reference_and_only_honest_witnesses_verify(circuit):
    """the constant row (query[0], alpha, beta) is walked under the scalar one whatever w_0 is, the mat-vec reads w_0 as
    given (ark-groth16's create_proof_with_reduction_and_matrices): the oracle's bytes for w_0 in {0, 2, r - 1}, which differ
    from the bytes of the same witness with w_0 = 1.  Unsatisfying witnesses give proofs that do not verify; an honest
    witness proved through this path does."""
    c = circuit
    idx = [c.labels.index(lb) for lb in UNSATISFYING] + [i for i, lb in enumerate(c.labels) if lb == "honest"][:3]
    proofs = c.run(idx)
    for lane, i in enumerate(idx):
        ok = c.p.verify_public(proofs[lane], c.honest_pub[i])
        assert ok == (c.labels[i] == "honest"), (c.name, c.labels[i])
    for lb in ("w0_0", "w0_2", "w0_r_minus_1"):
        i = c.labels.index(lb)
        same_but_w0 = [j for j in range(N) if c.labels[j] == "honest" and c.W[j][1:] == c.W[i][1:]]
        assert same_but_w0 and all(c.ref[j][:96] == c.ref[i][:96] and c.ref[j] != c.ref[i] for j in same_but_w0
                                   if c.RS[j] == c.RS[i])        # A and B do not depend on w_0; C does, through h
