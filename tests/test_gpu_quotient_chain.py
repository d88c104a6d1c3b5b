"""The quotient chain and the partial sums of a BIG batch (lanes = proofs: k_matvec, the k_ntt_pass / k_ntt_turn launches of
ntt_pass_list, the quotient formed inside k_recode, k_sum_ranges) at the smallest size that takes
those shapes: 129 proofs -- above lanechunk_max = 128 and ntt_lg_max = 96 -- which is three lane groups, the last with one
live lane.  Default tables, max_batch 192, every shipped circuit.  Bit-exact everywhere (integer arithmetic).

Turn widths: a circuit's domain has 2^logn points and the turn takes ((logn - 1) mod 3) + 1 levels; each test prints the
logn and the width it ran.  A width that no shipped circuit reaches runs on the device in the transform probe
(tests/test_gpu_transform_probe.py: the same launches at logn 1 .. 14, against Python integers) and in the host replay of
the index formulas (tests/test_ntt_plan_host.py) -- test_the_turn_widths_the_shipped_circuits_reach says which."""
import ctypes as C
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 129
CIRCUITS = [(20, False), (10, False), (20, True)]
H_LANES = (0, 63, 64, 128)   # both ends of the first group, the first lane of the second, the lone lane of the third


def _config2_reference(n):
    """oracle/c's proofs of the first n config-2 witnesses, from the session's 1 024 where another file has made them"""
    import conftest
    key = (0, 1024) if (0, 1024) in conftest._CONFIG2_ORACLE else (0, n)
    ws, rs, proofs, pub = conftest.oracle_config2(*key)
    return ws[:n], rs[:n], proofs[:n], pub[:n]


class _Circuit:
    """one prover per circuit and the 129 witnesses with oracle/c's proofs, shared by the tests below"""

    def __init__(self, depth, multi):
        from oracle.c import binding as ob
        from zerokit_amd import workload
        from zerokit_amd.batch import BatchProver
        self.depth, self.multi = depth, multi
        self.p = BatchProver(max_batch=192, depth=depth, multi=multi)
        p = self.p
        if depth == 20 and not multi:
            ws, self.rs, self.ref_proofs, self.ref_pub = _config2_reference(N)
            self.inp = p.pack_inputs(ws)
        else:
            o = ob.Circuit(depth, multi)
            named, self.rs = workload.circuit_range(1000, N, depth, multi)
            self.inp = p.pack_named_inputs(named)
            _, self.ref_proofs, pub = o.prove_many_packed(self.inp, p.pack_rs(self.rs))
            self.ref_pub = pub
        self.per = p.inputs_size * 32
        self.logn = int(p.info.domain_size).bit_length() - 1
        assert 1 << self.logn == int(p.info.domain_size)
        self.turn = (self.logn - 1) % 3 + 1
        self.full = None

    def run(self, idx, mode=0):
        p = self.p
        k = p.upload(b"".join(self.inp[i * self.per:(i + 1) * self.per] for i in idx), [self.rs[i] for i in idx])
        from zerokit_amd import lib
        from zerokit_amd._native import check
        check(lib().rlnamd_prover_run_mode(p._h, k, mode))
        return k

    def full_proofs(self):
        if self.full is None:
            k = self.run(range(N))
            self.full = (self.p.download(k), self.p.download_public(k))
        return self.full

    def say(self):
        print("tree_depth_%d%s: logn %d, turn width %d, launches %d" %
              (self.depth, "_multi" if self.multi else "", self.logn, self.turn, 2 * ((self.logn - self.turn) // 3) + 1))


_made = {}


@pytest.fixture(scope="module", params=CIRCUITS, ids=["depth20", "depth10", "depth20_multi"])
def circuit(request):
    key = request.param
    if key not in _made:
        _made[key] = _Circuit(*key)
    c = _made[key]
    c.say()
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_provers():
    yield
    for c in _made.values():
        c.p.close()
    _made.clear()


def test_all_129_proofs_and_public_values_equal_the_c_oracle(circuit):
    out, pub = circuit.full_proofs()
    assert [o["error"] for o in out] == [0] * N
    assert [o["proof"] for o in out] == circuit.ref_proofs
    assert pub == circuit.ref_pub
    if not circuit.multi:
        assert [o["public_inputs"] for o in out] == circuit.ref_pub


def test_h_of_four_lanes_equals_the_h_of_a_small_batch(circuit):
    """fetch_h(0 / 63 / 64 / 128) of the 129-proof batch against the same witnesses proved four at a time: that batch
    takes k_ntt_edge / k_ntt_mid (domains of 2^9 points and more) and forms h in the lanes = scalars recode"""
    p = circuit.p
    k = circuit.run(H_LANES)
    assert [o["error"] for o in p.download(k)] == [0] * len(H_LANES)
    small = [p.fetch_h(j) for j in range(len(H_LANES))]
    assert len({tuple(h) for h in small}) == len(H_LANES) and all(any(h) for h in small)
    k = circuit.run(range(N))
    assert [o["error"] for o in p.download(k)] == [0] * N
    for j, i in enumerate(H_LANES):
        assert p.fetch_h(i) == small[j], (circuit.depth, circuit.multi, i)
    if circuit.logn < 9:
        print("logn %d < 9: the small batch took the passes as well (no LDS kernels below 512 points)" % circuit.logn)


def test_partial_then_finish_of_129_gives_the_bytes_of_the_full_proofs(circuit):
    """the partial sums of a partial run (the rows of the known signals) and of a finish (the rest, the h rows among them)
    through k_sum_ranges, folded with the partial points: the full proofs' bytes"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    p = circuit.p
    out, _ = circuit.full_proofs()
    k = circuit.run(range(N), mode=1)
    buf = C.create_string_buffer(320 * k)
    check(lib().rlnamd_prover_download_partial(p._h, k, buf))
    parts = [buf.raw[320 * i:320 * (i + 1)] for i in range(k)]
    assert len(set(parts)) > 1
    p.upload(circuit.inp, circuit.rs)
    p.upload_partial(parts)
    check(lib().rlnamd_prover_run_mode(p._h, N, 2))
    fin = p.download(N)
    assert [o["error"] for o in fin] == [0] * N
    assert [o["proof"] for o in fin] == [o["proof"] for o in out] == circuit.ref_proofs


def test_h_of_the_golden_cases_in_a_big_batch_equals_the_golden_digest():
    """depth 20: the golden witnesses at the head of a 129-proof batch and one of them again in lane 128"""
    import hashlib
    from zerokit_amd.batch import BatchProver
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["cases"]
    assert 0 < len(cases) < 64

    def w(c):
        t = c["witness"]
        return dict(identity_secret=int(t["identity_secret"]), user_message_limit=int(t["user_message_limit"]),
                    message_id=int(t["message_id"]), path_elements=[int(v) for v in t["path_elements"]],
                    identity_path_index=[int(v) for v in t["identity_path_index"]], x=int(t["x"]),
                    external_nullifier=int(t["external_nullifier"]))

    ws0, rs0, _, _ = _config2_reference(N)
    where = list(range(len(cases))) + [N - 1]
    ws, rs = list(ws0), list(rs0)
    for i, c in zip(where, cases + [cases[0]]):
        ws[i], rs[i] = w(c), (int(c["r"]), int(c["s"]))
    made = (20, False) not in _made
    p = BatchProver(max_batch=192) if made else _made[(20, False)].p
    try:
        out = p.prove(ws, rs)
        assert [o["error"] for o in out] == [0] * N
        for i, c in zip(where, cases + [cases[0]]):
            h = p.fetch_h(i)
            assert hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in h)).hexdigest() == c["h_sha256"], (i, c["name"])
            assert out[i]["proof"].hex() == c["proof_compressed"], (i, c["name"])
    finally:
        if made:
            p.close()


def test_the_turn_widths_the_shipped_circuits_reach():
    """which widths the tests above ran on the device inside whole proofs; the probe runs every width on the device
    (tests/test_gpu_transform_probe.py), the host replay every index formula (tests/test_ntt_plan_host.py)"""
    from zerokit_amd.batch import BatchProver
    seen = {}
    for depth, multi in CIRCUITS:
        c = _made.get((depth, multi))
        p = c.p if c else BatchProver(max_batch=64, depth=depth, multi=multi)
        logn = int(p.info.domain_size).bit_length() - 1
        seen[(depth, multi)] = (logn, (logn - 1) % 3 + 1)
        if not c:
            p.close()
    widths = {w for _, w in seen.values()}
    print("logn and turn width per circuit:", seen, "-- widths no shipped circuit reaches (run on the device by the transform probe):", sorted({1, 2, 3} - widths))
    assert seen[(20, False)] == (13, 1)     # the headline circuit: 3, 3, 3, 3 | turn(1) | 3, 3, 3, 3
    assert widths <= {1, 2, 3}
