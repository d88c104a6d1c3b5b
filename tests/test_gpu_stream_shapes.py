"""The two stream shapes of a big batch (prover_plan.h: stream_plan) on the device: `wide`, the map of eight streams, and
`compact`, the same launches on four with the public values read off the witness.  Smallest tables (window_bits = 8),
capacity 192, batches of 129 and 192 proofs -- the smallest that take the throughput path.  Bit-exact everywhere."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CAP = 192


def _prover(shape):
    from zerokit_amd.batch import BatchProver
    os.environ["RLNAMD_STREAM_SHAPE"] = shape      # (read once, when the prover is built)
    try:
        return BatchProver(max_batch=CAP, window_bits=8)
    finally:
        del os.environ["RLNAMD_STREAM_SHAPE"]


@pytest.fixture(scope="module")
def compact():
    p = _prover("compact")
    yield p
    p.close()


@pytest.fixture(scope="module")
def wide():
    p = _prover("wide")
    yield p
    p.close()


@pytest.fixture(scope="module")
def pool():
    """CAP + 8 distinct witnesses with their (r, s): batch j of a stream is the window [j, j + n) of them"""
    from oracle.pyref import workload
    return workload.config2_witnesses(CAP + 8, seed=20260)


def _batches(p, pool, count):
    """(n, inputs, rs) of `count` batches, 129 and 192 proofs in turn.  Two witnesses the circuit's interpreter refuses (an
    input that is not canonical): x = r in the middle of batch 3, and identityPathIndex[7] = r in the middle of batch 5 --
    the second sits on a multiplexer of the circuit, where k_proof_values selects on "index != 0" instead"""
    ws, rs = pool
    out = []
    for j in range(count):
        n = 129 if j % 2 == 0 else CAP
        inp = bytearray(p.pack_inputs(ws[j:j + n]))
        if j == 3:
            off = (n // 2) * p.inputs_size + p.slots["x"][0]
            inp[32 * off:32 * off + 32] = R.to_bytes(32, "little")
        if j == 5:
            off = (n // 2) * p.inputs_size + p.slots["identityPathIndex"][0] + 7
            inp[32 * off:32 * off + 32] = R.to_bytes(32, "little")
        out.append((n, bytes(inp), p.pack_rs(rs[j:j + n])))
    return out


def _stream(p, batches):
    """every slot in flight: the oldest batch is collected when the next one needs its slot -> results in order"""
    nslot, inflight, res = p.n_slots(), [], []
    for n, inp, rsb in batches:
        if len(inflight) == nslot:
            res.append(p.collect(*inflight.pop(0)))
        inflight.append(p.submit(inp, rsb))
    while inflight:
        res.append(p.collect(*inflight.pop(0)))
    return res


@pytest.fixture(scope="module")
def streams(compact, wide, pool):
    """nslot + 3 batches through both shapes, computed once and left unchanged"""
    count = compact.n_slots() + 3
    return {"compact": _stream(compact, _batches(compact, pool, count)), "wide": _stream(wide, _batches(wide, pool, count))}


def test_full_proofs_are_the_same_in_both_shapes_and_equal_the_c_oracle(compact, wide, pool, streams):
    from oracle.c import binding as ob
    assert "stream_shape=compact" in compact.describe().split() and "stream_shape=wide" in wide.describe().split()
    assert compact.n_slots() == wide.n_slots() and len(streams["compact"]) == compact.n_slots() + 3
    ws, rs = pool
    c = ob.Circuit(20)
    for j, (a, b) in enumerate(zip(streams["compact"], streams["wide"])):
        n = len(a)
        assert n == len(b) == (129 if j % 2 == 0 else CAP)
        bad = n // 2 if j in (3, 5) else None
        keep = [i for i in range(n) if i != bad]
        assert [a[i]["proof"] for i in keep] == [b[i]["proof"] for i in keep], j
        assert [a[i]["public_inputs"] for i in keep] == [b[i]["public_inputs"] for i in keep], j
        assert [o["error"] for o in a] == [o["error"] for o in b], j
        assert [i for i, o in enumerate(a) if o["error"] != 0] == ([bad] if bad is not None else []), j
        if bad is not None:      # the refused proof itself: what the two shapes hand out for it (its error code is equal above)
            print("batch %d refused proof %d: error %d, proof bytes %s, values %s in both shapes" % (
                j, bad, a[bad]["error"], "equal" if a[bad]["proof"] == b[bad]["proof"] else "DIFFERENT",
                "equal" if a[bad]["public_inputs"] == b[bad]["public_inputs"] else "DIFFERENT"))
        for i in (0, n - 1) + ((bad - 1, bad + 1) if bad is not None else ()):
            ref = c.prove(ws[j + i], *rs[j + i])
            assert a[i]["proof"] == ref["proof"] and a[i]["public_inputs"] == ref["public_inputs"], (j, i)
    assert len({o["proof"] for res in streams["compact"] for o in res}) > CAP    # the batches really differ


def test_collects_newest_first_give_the_same_bytes(compact, pool, streams):
    nslot = compact.n_slots()
    tickets = [compact.submit(inp, rsb) for n, inp, rsb in _batches(compact, pool, nslot)]
    got = {}
    for j in reversed(range(nslot)):
        got[j] = compact.collect(*tickets[j])
    for j in range(nslot):
        assert got[j] == streams["compact"][j], j


def test_partial_then_finish_equals_the_full_proofs(compact, pool, streams):
    """two partial batches and two finish batches of 129 back to back (the second of each pair is not alone on the device)"""
    ws, rs = pool
    n = 129
    part_w = [dict(w, message_id=0, x=0, external_nullifier=0) for w in ws[:n]]
    pinp = compact.pack_inputs(part_w)
    tp = [compact.submit(pinp, bytes(64 * n), 1) for _ in range(2)]
    partials = [compact.collect_partial(t, k) for t, k in tp]
    assert partials[0] == partials[1] and len(set(partials[0])) == n
    inp, rsb = compact.pack_inputs(ws[:n]), compact.pack_rs(rs[:n])
    tf = [compact.submit(inp, rsb, 2, partials[k]) for k in range(2)]
    for t, k in tf:
        assert compact.collect(t, k) == streams["compact"][0]


def test_small_batches_between_big_ones_keep_their_shapes(compact, wide, pool, streams):
    """five proofs and one proof per call between 129-proof batches: golden bytes, and the small batches are still
    interpreted as segments behind hints (they take the lone shapes behind a batch in flight), in both shapes alike"""
    ws, rs = pool
    seen = {}
    for name, p in (("compact", compact), ("wide", wide)):
        big = _batches(p, pool, 1)[0]
        before = p.hint_stats()
        ts = [p.submit(big[1], big[2]),
              p.submit(p.pack_inputs(ws[:5]), p.pack_rs(rs[:5])),
              p.submit(big[1], big[2]),
              p.submit(p.pack_inputs(ws[7:8]), p.pack_rs(rs[7:8])),
              p.submit(big[1], big[2])]
        out = [p.collect(*t) for t in ts]
        after = p.hint_stats()
        full = streams[name][0]
        assert out[0] == full and out[2] == full and out[4] == full, name
        assert [o["proof"] for o in out[1]] == [o["proof"] for o in full[:5]], name
        assert [o["public_inputs"] for o in out[1]] == [o["public_inputs"] for o in full[:5]], name
        assert out[3][0]["proof"] == full[7]["proof"] and out[3][0]["public_inputs"] == full[7]["public_inputs"], name
        assert all(o["error"] == 0 for res in out for o in res), name
        seen[name] = {k: after[k] - before[k] for k in ("hinted_batches", "fallbacks")}
        assert seen[name] == {"hinted_batches": 2, "fallbacks": 0}, (name, seen)
        assert "lanechunk=128" in p.describe().split() and "lone=-1" in p.describe().split()
    assert seen["compact"] == seen["wide"]


def test_no_residue_in_any_slot_after_a_wiping_collect(compact, pool):
    big = _batches(compact, pool, 2)
    for k in range(compact.n_slots()):      # consecutive batches take consecutive slots; residue() reads the last batch's
        n, inp, rsb = big[k % 2]
        compact.collect(*compact.submit(inp, rsb))
        assert set(compact.residue().values()) == {0}, (k, compact.residue())
    tickets = [compact.submit(inp, rsb) for n, inp, rsb in big]      # ... and with another batch in flight behind it
    compact.collect(*tickets[1])
    assert set(compact.residue().values()) == {0}, compact.residue()
    compact.collect(*tickets[0])


_CHILD = r"""
import os, sys, json
sys.path.insert(0, os.environ["RLN_ROOT"])
from zerokit_amd.batch import BatchProver
p = BatchProver(max_batch=64, window_bits=8)
print("RESULT " + json.dumps({"describe": p.describe()}))
p.close()
"""


@pytest.mark.parametrize("queues,want", [("8", "wide"), ("4", "compact"), (None, "compact")])
def test_the_shape_follows_the_queue_count_of_the_process(queues, want):
    """a fresh child process per prover, RLNAMD_STREAM_SHAPE unset"""
    env = dict(os.environ, RLN_ROOT=ROOT)
    env.pop("RLNAMD_STREAM_SHAPE", None)
    env.pop("GPU_MAX_HW_QUEUES", None)
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    desc = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])["describe"].split()
    assert "stream_shape=" + want in desc and "hw_queues=" + (queues or "4") in desc, desc
