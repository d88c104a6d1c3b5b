"""A batch whose hints do not check is run again over the whole graph (Prover::settle_hints) -- here with every workspace
slot in flight, which is how prove_many and ffi_finish_rln_proofs_batch drive the prover and how any C caller may.  The
re-run must not read a staging buffer that a wipe clears under it, must not displace another uncollected ticket, and
must leave nothing behind (rlnamd_prover_residue_slot, every slot).  "Foreign" hints are rlnamd_prover_hints_for of
OTHER golden cases' inputs (asserted to differ); the RLNAMD_HINT_FAULT hook corrupts the hints hashed inside submit.
Every proof and every public input is compared with the golden bytes; the counters of rlnamd_prover_hint_stats say that
every batch was hinted and exactly the foreign ones were run again.  One prover per environment, smallest tables."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 8, 24)


def _w(case):
    w = case["witness"]
    return dict(identity_secret=int(w["identity_secret"]), user_message_limit=int(w["user_message_limit"]),
                message_id=int(w["message_id"]), path_elements=[int(t) for t in w["path_elements"]],
                identity_path_index=[int(t) for t in w["identity_path_index"]], x=int(w["x"]),
                external_nullifier=int(w["external_nullifier"]))


class _Rig:
    def __init__(self, env):
        from zerokit_amd.batch import BatchProver
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)                      # (read once, when the prover is built)
        try:
            self.p = p = BatchProver(max_batch=64, window_bits=8)
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        self.cases = json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["cases"]
        self.nc = len(self.cases)
        self.inp = [p.pack_inputs([_w(c)]) for c in self.cases]
        self.rs = [p.pack_rs([(int(c["r"]), int(c["s"]))]) for c in self.cases]
        self.hints = [p.hints_for(b)[0] for b in self.inp]
        # the case whose hints stand in for case i's: the next one -- no two neighbours share a member (two of the golden
        # cases do: the same witness under another r)
        for i in range(self.nc):
            assert bytes(self.hints[i]) != bytes(self.hints[(i + 1) % self.nc]), i

    def submit(self, idx, foreign=False, hinted=True):
        p = self.p
        inp, rsb = b"".join(self.inp[i] for i in idx), b"".join(self.rs[i] for i in idx)
        if not hinted:
            return p.submit(inp, rsb) + (idx,)
        return p.submit_hinted(inp, rsb, [self.hints[(i + 1) % self.nc if foreign else i] for i in idx]) + (idx,)

    def collect(self, pending):
        t, n, idx = pending
        for lane, (o, i) in enumerate(zip(self.p.collect(t, n), idx)):
            c = self.cases[i]
            assert o["error"] == 0 and o["proof"].hex() == c["proof_compressed"], (len(idx), lane, c["name"])
            assert [str(v) for v in o["public_inputs"]] == c["public_inputs"], (len(idx), lane, c["name"])

    def clean(self):
        for k in range(self.p.n_slots()):
            res = self.p.residue_slot(k)
            assert set(res.values()) == {0}, (k, res)


_made = {}


def _rig(**env):
    key = tuple(sorted(env.items()))
    if key not in _made:
        _made[key] = _Rig(env)
    return _made[key]


@pytest.fixture(scope="module", autouse=True)
def _close_provers():
    yield
    for r in _made.values():
        r.p.close()
    _made.clear()


def _idx(b, n, nc):
    return [(b + j) % nc for j in range(n)]


def _in_order(r):
    """3 S batches of 1, 2, 8, 24, ... proofs through submit_hinted, every second one with foreign hints, S pending at any
    time: the oldest is collected, then the next submitted -- the slot the re-run used to take is the batch's own"""
    p, S = r.p, r.p.n_slots()
    st0 = p.hint_stats()
    flight, foreign = [], 0
    for b in range(3 * S):
        if len(flight) == S:
            r.collect(flight.pop(0))
        f = b % 2 == 1
        foreign += f
        flight.append(r.submit(_idx(b, SIZES[b % len(SIZES)], r.nc), foreign=f))
    while flight:
        r.collect(flight.pop(0))
    st = p.hint_stats()
    assert st["hinted_batches"] - st0["hinted_batches"] == 3 * S, (st0, st)
    assert st["fallbacks"] - st0["fallbacks"] == foreign, (st0, st, foreign)
    r.clean()


def test_reruns_in_order_with_every_slot_in_flight():
    r = _rig()
    assert r.p.n_slots() >= 2
    _in_order(r)


def test_reruns_in_order_on_the_tightest_ring():
    r = _rig(RLNAMD_SLOTS="2")
    assert r.p.n_slots() == 2
    _in_order(r)


@pytest.mark.parametrize("where", ["middle", "first"])
def test_reruns_out_of_order_displace_no_other_ticket(where):
    """S batches pending.  middle: the foreign one in the middle, collected first, then the newest, then the rest.  first:
    the foreign one submitted first and collected last (behind the newest ... the second)."""
    r = _rig()
    p, S = r.p, r.p.n_slots()
    st0 = p.hint_stats()
    at = S // 2 if where == "middle" else 0
    flight = [r.submit(_idx(b + 1, SIZES[b % len(SIZES)], r.nc), foreign=(b == at)) for b in range(S)]
    if where == "middle":
        order = [at, S - 1] + [b for b in range(S) if b not in (at, S - 1)]
    else:
        order = list(range(S - 1, -1, -1))
    assert sorted(order) == list(range(S)) and len(set(t for t, _, _ in flight)) == S
    for b in order:
        r.collect(flight[b])
    st = p.hint_stats()
    assert st["hinted_batches"] - st0["hinted_batches"] == S and st["fallbacks"] - st0["fallbacks"] == 1, (st0, st)
    r.clean()


def test_hints_hashed_inside_the_call_are_rerun_with_every_slot_in_flight():
    """RLNAMD_HINT_FAULT = 9 corrupts a hint of the first proof of every hinted batch: plain submits of 1 and 2 proofs, S
    pending, every batch run again"""
    r = _rig(RLNAMD_HINT_FAULT="9")
    p, S = r.p, r.p.n_slots()
    st0 = p.hint_stats()
    flight, batches = [], 2 * S + 1
    for b in range(batches):
        if len(flight) == S:
            r.collect(flight.pop(0))
        flight.append(r.submit(_idx(b, 1 + b % 2, r.nc), hinted=False))
    while flight:
        r.collect(flight.pop(0))
    st = p.hint_stats()
    assert st["hinted_batches"] - st0["hinted_batches"] == batches and st["fallbacks"] - st0["fallbacks"] == batches, (st0, st)
    r.clean()


def test_a_rerun_finish_batch_still_sees_its_partial_points():
    """finish mode: the partial points are staged in the third region of the slot's pinned buffer; S one-proof finish
    batches pending, every one hinted inside submit, corrupted by the hook and run again"""
    r = _rig(RLNAMD_HINT_FAULT="9")
    p, S = r.p, r.p.n_slots()
    fx = {c["name"]: bytes.fromhex(c["partial320"]) for c in
          json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_partial.json")))["cases"]}
    have = [i for i, c in enumerate(r.cases) if c["name"] in fx]
    assert len(have) >= 2
    st0 = p.hint_stats()
    flight = []
    for b in range(S):
        i = have[b % len(have)]
        flight.append(p.submit(r.inp[i], r.rs[i], 2, [fx[r.cases[i]["name"]]]) + ([i],))
    for f in flight:
        r.collect(f)
    st = p.hint_stats()
    assert st["hinted_batches"] - st0["hinted_batches"] == S and st["fallbacks"] - st0["fallbacks"] == S, (st0, st)
    r.clean()
