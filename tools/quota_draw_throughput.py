#!/usr/bin/env python3
"""Quota-ledger throughput: rlnamd_quota_draw by itself, and proving with drawn ids against proving with ids the host
supplies.

    python tools/quota_draw_throughput.py [--calls 9] [--out FILE] [--counts] [--store DIR [--store-mem DIR]]

prints ONE JSON line.  Torch-free (ctypes).  Each of the two steps runs in a child process of its own under a time
limit; a step that fails or runs out of time ends the run there.

  draw    a draw of 1 024, 8 192 and 65 536 requests on a depth-20 ledger with two open external nullifiers, in two
          shapes: every request a member of its own, and every request the SAME member.  The limit is 2^32 - 1, so every
          request is granted and the counters rise from call to call.  Leaf indices, external nullifiers and limits in,
          ids and statuses out, the copies inside the timed region.  The two shapes take turns in one process; median
          and min-max of `calls` calls after 2 warm-up calls each.  "one_member_over_distinct" is the ratio of the
          medians: the draw's passes do not depend on how often members repeat, so it is expected near 1.
  prove   rlnamd_prover_prove_stream_members_drawn against rlnamd_prover_prove_stream_members with the ids in the
          inputs, 1 024 and 8 192 proofs for distinct members through a prover of capacity 1 024; the two take turns in
          one process, median of `calls` calls after 1 warm-up call each.  "draw_share_1024" is the median of a
          1 024-request draw (step draw, distinct) over the median of the drawn 1 024-proof call.

--store DIR measures the durable ledger (rlnamd_quota_open) with its store in a fresh directory under DIR, which should be
on the machine's local disk; --store-mem DIR2 adds a second durable ledger under DIR2, meant for a memory file system,
where an fdatasync costs next to nothing.  With them
  draw    runs the same calls on a plain ledger, on the ledger under DIR ("store") and on the one under DIR2
          ("store_mem"), the three taking turns in one process.  Per size and shape: "store_mem" - "plain" is what the
          delta costs (three kernels, the scan, two copies back and the append), "store" - "store_mem" what the sync to
          the disk costs.  The durable ledgers are opened with a journal threshold that is never reached, so no call
          compacts behind itself.  The plain series is what the tool measures without --store.
  prove   adds "drawn_store": the drawn call on the ledger under DIR, in turn with the other two.
  store   (only with --store) a depth-20 ledger with all 2^20 counters of one slot non-zero: rlnamd_quota_compact and a
          reopen (rlnamd_quota_free, which finds nothing to compact, then rlnamd_quota_open), median of `calls` each.

--counts measures the draw by count (rlnamd_quota_draw_counts) instead, by the same method:
  draw_counts   the plain draw and the draw by count, counts 1 .. 4 in turn, each in both shapes: four series that take
                turns in one process on one ledger.  "counts_over_draw" is the ratio of the medians per shape -- the
                extra is one gather and one scan over n words -- and "one_member_over_distinct" is given for both.
  prove_counts  on a multi-message-id prover of capacity 1 024, 1 024 proofs for distinct members:
                rlnamd_prover_prove_stream_members with ids and selectors in the inputs (its 160-byte values stay zero
                on this circuit), rlnamd_prover_prove_stream_members_public with the same inputs (every public value
                read back, as the drawn call reads them) and rlnamd_prover_prove_stream_members_drawn_counts.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRAW_SIZES = (1024, 8192, 65536)
PROVE_SIZES = (1024, 8192)
DEPTH = 20
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
EA, EB = 1001, 1002
STEP_LIMIT_S = {"draw": 120, "prove": 420, "draw_counts": 180, "prove_counts": 420, "store": 300}
STORE = {"store": None, "store_mem": None}      # --store, --store-mem


def durable_ledgers():
    """{name: a QuotaLedger opened on a fresh directory under --store / --store-mem}"""
    from zerokit_amd.batch import QuotaLedger
    out = {}
    for name, root in STORE.items():
        if root:
            os.makedirs(root, exist_ok=True)
            # (no automatic compaction inside the timed calls: step "store" times a compaction by itself)
            q = QuotaLedger.open(tempfile.mkdtemp(prefix="quota_", dir=root), DEPTH, 4, 1 << 40)
            q.set_epochs([EA, EB])
            out[name] = q
    return out


def row(n, ts):
    med = statistics.median(ts)
    return {"n": n, "calls": len(ts), "median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3), "per_s": round(n / med, 1)}


def need_device():
    from zerokit_amd import lib
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("quota_draw_throughput: no HIP device (there is no CPU fallback)")


def step_draw(calls):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import QuotaLedger
    need_device()
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    durable = durable_ledgers()
    rnd = random.Random(20261020)
    rows = []
    for n in DRAW_SIZES:
        ext = b"".join((EA if i & 1 else EB).to_bytes(32, "little") for i in range(n))
        limits = (C.c_uint32 * n)(*([0xFFFFFFFF] * n))
        ids, status = (C.c_uint32 * n)(), C.create_string_buffer(n)
        shapes = {"distinct": (C.c_uint64 * n)(*rnd.sample(range(1 << DEPTH), n)), "one_member": (C.c_uint64 * n)(*([12345] * n))}
        series = [(name, q, leaf) for name, leaf in shapes.items()]
        series += [(kind + "_" + name, d, leaf) for name, leaf in shapes.items() for kind, d in durable.items()]
        ts = {name: [] for name, _, _ in series}
        for c in range(2 + calls):
            for name, ledger, leaf in series:
                t0 = time.perf_counter()
                check(lib().rlnamd_quota_draw(ledger._h, n, leaf, ext, limits, ids, status))
                t1 = time.perf_counter()
                assert status.raw == b"\0" * n
                if c >= 2:
                    ts[name].append(t1 - t0)
        r = {name: row(n, t) for name, t in ts.items()}
        r["one_member_over_distinct"] = round(r["one_member"]["median_ms"] / r["distinct"]["median_ms"], 3)
        for shape in shapes:
            if "store_mem" in durable:
                r["delta_ms_" + shape] = round(r["store_mem_" + shape]["median_ms"] - r[shape]["median_ms"], 3)
            if "store" in durable and "store_mem" in durable:
                r["disk_sync_ms_" + shape] = round(r["store_" + shape]["median_ms"] - r["store_mem_" + shape]["median_ms"], 3)
        r["plan"] = list(QuotaLedger.plan(n, DEPTH))
        rows.append(r)
    out = {"depth": DEPTH, "rows": rows, "residue": q.info()["residue"]}
    q.close()
    for kind, d in durable.items():
        out[kind + "_info"] = d.store_info()
        out[kind + "_residue"] = d.info()["residue"]
        d.close()
    return out


def step_prove(calls):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import BatchProver, PoseidonTree, QuotaLedger
    need_device()
    p = BatchProver(max_batch=1024)
    tree = PoseidonTree(DEPTH)
    tree.fill_sequential(0, max(PROVE_SIZES), 1)
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    qs = durable_ledgers().get("store")
    rnd = random.Random(7)
    rows = []
    for n in PROVE_SIZES:
        ws = [dict(identity_secret=rnd.randrange(1, R), user_message_limit=1 << 20, message_id=i % 1000, x=rnd.randrange(R),
                   external_nullifier=EA if i & 1 else EB) for i in range(n)]
        inputs = p.pack_member_inputs(ws)
        rsb = p.pack_rs([(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)])
        idx = (C.c_uint64 * n)(*range(n))
        proofs, values = C.create_string_buffer(128 * n), C.create_string_buffer(160 * n)
        errs, status = (C.c_uint32 * n)(), C.create_string_buffer(n)

        def host_ids():
            check(lib().rlnamd_prover_prove_stream_members(p._h, tree._h, n, idx, inputs, rsb, proofs, values, errs))

        def drawn():
            check(lib().rlnamd_prover_prove_stream_members_drawn(p._h, tree._h, q._h, n, idx, inputs, rsb, status, proofs, values, errs))

        def drawn_store():
            check(lib().rlnamd_prover_prove_stream_members_drawn(p._h, tree._h, qs._h, n, idx, inputs, rsb, status, proofs, values, errs))
        fns = (("host_ids", host_ids), ("drawn", drawn)) + ((("drawn_store", drawn_store),) if qs else ())
        ts = {name: [] for name, _ in fns}
        for c in range(1 + calls):
            for name, fn in fns:
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                assert not any(errs)
                if c >= 1:
                    ts[name].append(t1 - t0)
        assert status.raw == b"\0" * n
        r = {name: row(n, t) for name, t in ts.items()}
        r["drawn_over_host_ids"] = round(r["drawn"]["median_ms"] / r["host_ids"]["median_ms"], 4)
        if qs:
            r["drawn_store_over_drawn"] = round(r["drawn_store"]["median_ms"] / r["drawn"]["median_ms"], 4)
        rows.append(r)
    out = {"capacity": 1024, "rows": rows, "ledger_residue": q.info()["residue"]}
    if qs:
        out["store_info"], out["store_residue"] = qs.store_info(), qs.info()["residue"]
        qs.close()
    q.close()
    tree.close()
    p.close()
    return out


def step_draw_counts(calls):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import QuotaLedger
    need_device()
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    rnd = random.Random(20261021)
    rows = []
    for n in DRAW_SIZES:
        ext = b"".join((EA if i & 1 else EB).to_bytes(32, "little") for i in range(n))
        limits = (C.c_uint32 * n)(*([0xFFFFFFFF] * n))
        counts = bytes(1 + (i & 3) for i in range(n))
        ids, status = (C.c_uint32 * n)(), C.create_string_buffer(n)
        leaves = {"distinct": (C.c_uint64 * n)(*rnd.sample(range(1 << DEPTH), n)), "one_member": (C.c_uint64 * n)(*([12345] * n))}

        def draw(leaf):
            check(lib().rlnamd_quota_draw(q._h, n, leaf, ext, limits, ids, status))

        def draw_counts(leaf):
            check(lib().rlnamd_quota_draw_counts(q._h, n, leaf, ext, limits, counts, ids, status))
        series = [(kind + "_" + shape, fn, leaf) for shape, leaf in leaves.items() for kind, fn in (("draw", draw), ("counts", draw_counts))]
        ts = {name: [] for name, _, _ in series}
        for c in range(2 + calls):
            for name, fn, leaf in series:
                t0 = time.perf_counter()
                fn(leaf)
                t1 = time.perf_counter()
                assert status.raw == b"\0" * n          # 65 536 x 4 ids a call: far below the limit
                if c >= 2:
                    ts[name].append(t1 - t0)
        r = {name: row(n, t) for name, t in ts.items()}
        for shape in leaves:
            r["counts_over_draw_" + shape] = round(r["counts_" + shape]["median_ms"] / r["draw_" + shape]["median_ms"], 3)
        for kind in ("draw", "counts"):
            r[kind + "_one_member_over_distinct"] = round(r[kind + "_one_member"]["median_ms"] / r[kind + "_distinct"]["median_ms"], 3)
        r["plan"] = list(QuotaLedger.plan(n, DEPTH))
        rows.append(r)
    info = q.info()
    q.close()
    return {"depth": DEPTH, "rows": rows, "residue": info["residue"]}


def step_prove_counts(calls):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import BatchProver, PoseidonTree, QuotaLedger
    need_device()
    p = BatchProver(max_batch=1024, multi=True)
    k, n = int(p.info.max_out), 1024
    tree = PoseidonTree(DEPTH)
    tree.fill_sequential(0, n, 1)
    q = QuotaLedger(DEPTH, 4)
    q.set_epochs([EA, EB])
    rnd = random.Random(7)
    cnt = [1 + (i % k) for i in range(n)]
    ws = [dict(identity_secret=rnd.randrange(1, R), user_message_limit=1 << 20, x=rnd.randrange(R),
               external_nullifier=EA if i & 1 else EB, message_id=[(7 * i + t) % 1000 if t < cnt[i] else 0 for t in range(k)],
               selector_used=[int(t < cnt[i]) for t in range(k)]) for i in range(n)]
    inputs = p.pack_member_inputs(ws)
    rsb = p.pack_rs([(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)])
    idx, counts = (C.c_uint64 * n)(*range(n)), bytes(cnt)
    proofs, values, public = C.create_string_buffer(128 * n), C.create_string_buffer(160 * n), C.create_string_buffer(32 * p.num_public * n)
    errs, status = (C.c_uint32 * n)(), C.create_string_buffer(n)

    def host_ids():
        check(lib().rlnamd_prover_prove_stream_members(p._h, tree._h, n, idx, inputs, rsb, proofs, values, errs))

    def host_ids_public():
        check(lib().rlnamd_prover_prove_stream_members_public(p._h, tree._h, n, idx, inputs, rsb, proofs, public, errs))

    def drawn_counts():
        check(lib().rlnamd_prover_prove_stream_members_drawn_counts(p._h, tree._h, q._h, n, idx, inputs, rsb, counts, status, proofs,
                                                                    public, errs))
    fns = (("host_ids", host_ids), ("host_ids_public", host_ids_public), ("drawn_counts", drawn_counts))
    ts = {name: [] for name, _ in fns}
    for c in range(1 + calls):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            assert not any(errs)
            if c >= 1:
                ts[name].append(t1 - t0)
    assert status.raw == b"\0" * n
    r = {name: row(n, t) for name, t in ts.items()}
    r["drawn_counts_over_host_ids"] = round(r["drawn_counts"]["median_ms"] / r["host_ids"]["median_ms"], 4)
    r["drawn_counts_over_host_ids_public"] = round(r["drawn_counts"]["median_ms"] / r["host_ids_public"]["median_ms"], 4)
    out = {"capacity": 1024, "max_out": k, "rows": [r], "ledger_residue": q.info()["residue"]}
    q.close()
    tree.close()
    p.close()
    return out


def step_store(calls):
    from zerokit_amd.batch import QuotaLedger
    need_device()
    os.makedirs(STORE["store"], exist_ok=True)
    d = tempfile.mkdtemp(prefix="quota_full_", dir=STORE["store"])
    q = QuotaLedger.open(d, DEPTH, 4, 1 << 40)          # no automatic compaction: the timed ones are the only ones
    q.set_epochs([EA])
    n = 1 << 16
    for k in range((1 << DEPTH) // n):                  # every member of the slot once
        ids, status = q.draw(list(range(k * n, (k + 1) * n)), [EA] * n, [0xFFFFFFFF] * n)
        assert not any(status)
    compact, reopen = [], []
    for c in range(1 + calls):
        t0 = time.perf_counter()
        q.compact()
        t1 = time.perf_counter()
        if c >= 1:
            compact.append(t1 - t0)
    snapshot_bytes = os.path.getsize(os.path.join(d, "rlnamd_quota.bin"))
    for c in range(1 + calls):
        t0 = time.perf_counter()
        q.close()
        t1 = time.perf_counter()
        q = QuotaLedger.open(d, DEPTH, 4, 1 << 40)
        t2 = time.perf_counter()
        assert q.store_info()["restored_pairs"] == 1 << DEPTH and q.used([0, (1 << DEPTH) - 1], [EA, EA]) == [1, 1]
        if c >= 1:
            reopen.append(t2 - t1)
    out = {"depth": DEPTH, "nonzero_counters": 1 << DEPTH, "snapshot_bytes": snapshot_bytes, "compact": row(1 << DEPTH, compact),
           "reopen": row(1 << DEPTH, reopen), "store_info": q.store_info(), "residue": q.info()["residue"]}
    q.close()
    return out


STEPS = {"store": step_store, "draw": step_draw, "prove": step_prove, "draw_counts": step_draw_counts, "prove_counts": step_prove_counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--counts", action="store_true", help="measure the draw by count (draw_counts, prove_counts)")
    ap.add_argument("--store", metavar="DIR", help="measure the durable ledger too, its store in a fresh directory under DIR")
    ap.add_argument("--store-mem", metavar="DIR", help="with --store: a second durable ledger under DIR (a memory file system)")
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("--calls: at least 5")
    if (a.store_mem or a.step == "store") and not a.store:
        ap.error("--store-mem and --step store go with --store")
    STORE["store"], STORE["store_mem"] = a.store, a.store_mem
    if a.step:
        print(json.dumps(STEPS[a.step](a.calls)))
        return 0
    out = {"tool": "quota_draw_throughput", "calls": a.calls}
    steps = ("draw_counts", "prove_counts") if a.counts else ("draw", "prove") + (("store",) if a.store else ())
    passed = (["--store", a.store] if a.store else []) + (["--store-mem", a.store_mem] if a.store_mem else [])
    for name in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls)] + passed,
                               stdout=subprocess.PIPE, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            out[name] = {"error": "time limit of %d s" % STEP_LIMIT_S[name]}
            break
        if r.returncode != 0:
            out[name] = {"error": "exit status %d" % r.returncode}
            break   # nothing more is started on the device after a failed step
        out[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    good = all("error" not in out.get(k, {"error": 1}) for k in steps)
    if good and not a.counts:
        draw_1024 = next(r["distinct"]["median_ms"] for r in out["draw"]["rows"] if r["distinct"]["n"] == 1024)
        batch_1024 = next(r["drawn"]["median_ms"] for r in out["prove"]["rows"] if r["drawn"]["n"] == 1024)
        out["draw_share_1024"] = round(draw_1024 / batch_1024, 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
