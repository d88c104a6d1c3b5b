#!/usr/bin/env python3
"""Verification throughput: the device verifier (rlnamd_verify_many_gpu_ex), a lane per proof and a team of 8 lanes
per proof, against 16 host threads (rlnamd_verify_many), compressed proof bytes in, verdicts out, copies to and from the
device inside the timed region.

    python tools/verify_throughput.py [--calls 9] [--lanes 1,8] [--optimistic] [--out FILE]

prints ONE JSON line.  Torch-free (ctypes through zerokit_amd).  Each of the two steps runs in a child process of its
own under a time limit; a step that fails or runs out of time ends the run there.

  sweep       host at n = 1 ... 8 192; device at n = 1 ... 65 536, one column per shape of --lanes (1: a lane per
              proof, 8: teams, 0: the verifier's choice), the shapes alternated call by call at each size; median and
              spread of `calls` calls after a warm-up call per size and shape; per shape the crossover (smallest measured
              n where the device's median beats the host's at that n); with both shapes measured, team_max: the largest
              measured n at which the teams' median is below the minimum of a lane per proof
  concurrent  device verification at n = 8 192 while a proving stream runs, and the proving rate alone and meanwhile
  optimistic  (with --optimistic) rlnamd_verify_many_gpu_optimistic against the exact lane-per-proof call of the same
              build at n = 8 192 and 65 536, alternated call by call: all rows valid, and the worst case of one damaged
              proof in every chunk with cool-down 0 (a combined check and an exact pass per chunk; left out when
              --lanes names 8 alone).  With 8 among --lanes: rlnamd_verify_many_gpu_optimistic_ex(lanes = 8), the combined check in team form, against the
              exact team call and beside the lane-per-proof combined check at n = 64, 256, 512, 1 024 and 8 192, all
              rows valid, the three alternated call by call; and the share of the host's finish in a team-form call
              (rlnamd_verify_gpu_finish_time)
"""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_THREADS = 16
DEVICE_N = (1, 8, 64, 96, 128, 192, 256, 384, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
HOST_N = (1, 8, 64, 96, 128, 192, 256, 384, 512, 1024, 8192)
STEP_LIMIT_S = {"sweep": 540, "concurrent": 240, "optimistic": 240}
OPTIMISTIC_N = (8192, 65536)
OPTIMISTIC_TEAM_N = (64, 256, 512, 1024, 8192)


def setup():
    from zerokit_amd import lib, workload
    from zerokit_amd.batch import BatchProver
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("verify_throughput: no HIP device (there is no CPU fallback for the device side)")
    p = BatchProver(max_batch=1024)
    ws, rs = workload.config2_range(0, 1024)
    inp, rsb = p.pack_inputs(ws), p.pack_rs(rs)
    t, n = p.submit(inp, rsb)
    proofs, values, errs = p.collect_raw(t, n)
    assert not any(errs)
    return p, inp, rsb, proofs, values


def tiled(proofs, values, n):
    reps = (n + 1023) // 1024
    return (proofs * reps)[:128 * n], (values * reps)[:160 * n]


def timed(fn, calls):
    fn()   # warm-up: code objects, buffers at their size
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def row(n, ts):
    med = statistics.median(ts)
    return {"n": n, "calls": len(ts), "median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3), "per_s": round(n / med, 1)}


def step_sweep(calls, shapes=(1, 8)):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    p, _inp, _rsb, proofs, values = setup()
    host, dev = [], {k: [] for k in shapes}
    for n in DEVICE_N:
        pr, va = tiled(proofs, values, n)
        ok = C.create_string_buffer(n)

        def gpu(lanes):
            check(lib().rlnamd_verify_many_gpu_ex(p._h, n, pr, va, 5, lanes, ok, None))
        ts = {k: [] for k in shapes}
        for k in shapes:   # warm-up: code objects, buffers at their size
            gpu(k)
            assert ok.raw == b"\x01" * n
        for _ in range(calls):
            for k in shapes:
                t0 = time.perf_counter()
                gpu(k)
                ts[k].append(time.perf_counter() - t0)
        for k in shapes:
            dev[k].append(row(n, ts[k]))
    for n in HOST_N:
        pr, va = tiled(proofs, values, n)
        ok = C.create_string_buffer(n)

        def cpu():
            check(lib().rlnamd_verify_many(p._h, n, pr, va, 5, HOST_THREADS, ok))
        host.append(row(n, timed(cpu, calls if n < 8192 else max(3, calls // 3))))
        assert ok.raw == b"\x01" * n
    hmed = {r["n"]: r["median_ms"] for r in host}
    out = {"host_threads": HOST_THREADS, "host": host}
    for k in shapes:
        wins = [r["n"] for r in dev[k] if r["n"] in hmed and r["median_ms"] < hmed[r["n"]]]
        out["device_lanes%d" % k] = dev[k]
        out["crossover_n_lanes%d" % k] = min(wins) if wins else None
    if 1 in dev and 8 in dev:
        lane_min = {r["n"]: r["min_ms"] for r in dev[1]}
        faster = [r["n"] for r in dev[8] if r["median_ms"] < lane_min[r["n"]]]
        out["team_max"] = max(faster) if faster else 0
    p.close()
    return out


def step_concurrent(calls, shapes=(0,)):
    lanes = shapes[0] if len(shapes) == 1 else 0
    from zerokit_amd import lib
    from zerokit_amd._native import check
    p, inp, rsb, proofs, values = setup()
    pr, va = tiled(proofs, values, 8192)
    ok = C.create_string_buffer(8192)

    def gpu():
        check(lib().rlnamd_verify_many_gpu_ex(p._h, 8192, pr, va, 5, lanes, ok, None))

    def prove_stream(batches):
        nslots, inflight = p.n_slots(), collections.deque()
        p.sync()
        t0 = time.perf_counter()
        for _ in range(batches):
            if len(inflight) == nslots:
                p.collect_raw(inflight.popleft(), 1024)
            inflight.append(p.submit(inp, rsb)[0])
        while inflight:
            p.collect_raw(inflight.popleft(), 1024)
        p.sync()
        return batches * 1024 / (time.perf_counter() - t0)
    prove_stream(4)
    alone_prove = prove_stream(24)
    alone_verify = row(8192, timed(gpu, calls))
    res = {}
    th = threading.Thread(target=lambda: res.update(rate=prove_stream(48)))
    th.start()
    time.sleep(0.2)   # the stream's first batches are in flight
    ts, t_end = [], None
    while th.is_alive():
        t0 = time.perf_counter()
        gpu()
        ts.append(time.perf_counter() - t0)
    th.join()
    assert ok.raw == b"\x01" * 8192
    p.close()
    return {"lanes": lanes, "prove_alone_per_s": round(alone_prove, 1), "verify_alone": alone_verify,
            "prove_meanwhile_per_s": round(res["rate"], 1), "verify_meanwhile": row(8192, ts) if ts else None}


def optimistic_teams(p, proofs, values, calls):
    """the combined check in team form against the exact team call, the lane-per-proof combined check beside them"""
    from zerokit_amd import lib
    from zerokit_amd._native import check
    out = []
    for n in OPTIMISTIC_TEAM_N:
        pr, va = tiled(proofs, values, n)
        ok = C.create_string_buffer(n)
        fns = (("optimistic_team", lambda: check(lib().rlnamd_verify_many_gpu_optimistic_ex(p._h, n, pr, va, 5, None, 8, ok))),
               ("exact_team", lambda: check(lib().rlnamd_verify_many_gpu_ex(p._h, n, pr, va, 5, 8, ok, None))),
               ("optimistic_lane", lambda: check(lib().rlnamd_verify_many_gpu_optimistic_ex(p._h, n, pr, va, 5, None, 1, ok))))
        ts = {name: [] for name, _ in fns}
        for _, fn in fns:   # warm-up: code objects, buffers at their size
            fn()
            assert ok.raw == b"\x01" * n
        fin = {name: 0 for name, _ in fns}
        ft = (C.c_uint64 * 2)()
        for _ in range(calls):
            for name, fn in fns:
                check(lib().rlnamd_verify_gpu_finish_time(p._h, ft))
                f0 = int(ft[0])
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
                check(lib().rlnamd_verify_gpu_finish_time(p._h, ft))
                fin[name] += int(ft[0]) - f0
        r = {"n": n}
        for name, _ in fns:
            r[name] = row(n, ts[name])
            r[name]["finish_host_ms_mean"] = round(fin[name] / calls / 1e6, 3)
        r["optimistic_team_over_exact_team"] = round(r["optimistic_team"]["median_ms"] / r["exact_team"]["median_ms"], 3)
        out.append(r)
    return out


def step_optimistic(calls, shapes=(1,)):
    from zerokit_amd import lib
    from zerokit_amd._native import check
    p, _inp, _rsb, proofs, values = setup()
    out = {"all_valid": [], "one_damaged_per_chunk_cooldown_0": []}
    if 8 in shapes:
        p.verify_set_cooldown(0)
        out["teams_all_valid"] = optimistic_teams(p, proofs, values, calls)
    for n in OPTIMISTIC_N if 1 in shapes or 8 not in shapes else ():
        pr, va = tiled(proofs, values, n)
        bad = bytearray(va)
        bad[0] ^= 1                      # one changed public input: the pairing rejects row 0
        bad = bytes(bad)
        ok = C.create_string_buffer(n)

        def exact(vals=va):
            check(lib().rlnamd_verify_many_gpu_ex(p._h, n, pr, vals, 5, 1, ok, None))

        def optimistic(vals=va):
            check(lib().rlnamd_verify_many_gpu_optimistic(p._h, n, pr, vals, 5, None, ok))
        for key, vals, want in (("all_valid", va, b"\x01" * n),
                                ("one_damaged_per_chunk_cooldown_0", bad, b"\x00" + b"\x01" * (n - 1))):
            p.verify_set_cooldown(0)
            ts = {"optimistic": [], "exact": []}
            for fn in (optimistic, exact):   # warm-up: code objects, buffers at their size
                fn(vals)
                assert ok.raw == want
            for _ in range(calls):
                for name, fn in (("optimistic", optimistic), ("exact", exact)):
                    t0 = time.perf_counter()
                    fn(vals)
                    ts[name].append(time.perf_counter() - t0)
            r = {"n": n, "optimistic": row(n, ts["optimistic"]), "exact": row(n, ts["exact"])}
            r["optimistic_over_exact"] = round(r["optimistic"]["median_ms"] / r["exact"]["median_ms"], 3)
            out[key].append(r)
    out["stats"] = p.verify_optimistic_stats()
    p.verify_set_cooldown(16)
    p.close()
    return out


STEPS = {"sweep": step_sweep, "concurrent": step_concurrent, "optimistic": step_optimistic}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--lanes", default="1,8", help="shapes to measure, of 1 (a lane per proof), 8 (teams), 0 (the "
                    "verifier's choice): a column each in the sweep; the concurrent step takes a single one, else 0")
    ap.add_argument("--optimistic", action="store_true", help="add the optimistic step")
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.calls < 9:
        ap.error("--calls: at least 9")
    shapes = tuple(int(k) for k in a.lanes.split(","))
    if not shapes or any(k not in (0, 1, 8) for k in shapes) or len(set(shapes)) != len(shapes):
        ap.error("--lanes: a list of distinct values of 0, 1, 8")
    if a.step:
        print(json.dumps(STEPS[a.step](a.calls, shapes)))
        return 0
    out = {"tool": "verify_throughput", "calls": a.calls, "lanes": list(shapes)}
    for name in ("sweep", "concurrent") + (("optimistic",) if a.optimistic else ()):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls), "--lanes",
                                a.lanes],
                               stdout=subprocess.PIPE, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            out[name] = {"error": "time limit of %d s" % STEP_LIMIT_S[name]}
            break
        if r.returncode != 0:
            out[name] = {"error": "exit status %d" % r.returncode}
            break   # nothing more is started on the device after a failed step
        out[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    wanted = ("sweep", "concurrent") + (("optimistic",) if a.optimistic else ())
    return 0 if all("error" not in out.get(k, {"error": 1}) for k in wanted) else 1


if __name__ == "__main__":
    sys.exit(main())
