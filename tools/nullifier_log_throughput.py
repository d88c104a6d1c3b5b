#!/usr/bin/env python3
"""Nullifier-log throughput: rlnamd_nullifier_log_observe on the device against one host thread feeding the same
stream through the sequential policy of nullifier_log.h (tests/host/nullifierlog.cpp, built with g++ -O2), and the
device verifier's pass at the same sizes -- the stage a relay loop runs before the log.

    python tools/nullifier_log_throughput.py [--calls 9] [--out FILE]

prints ONE JSON line.  Torch-free (ctypes and numpy).  Each of the two steps runs in a child process of its own under a
time limit; a step that fails or runs out of time ends the run there.

  log       calls of 1 024, 8 192 and 65 536 shares into a log of capacity 2^24, starting empty and starting half full
            (2^23 records), with 1 % and 50 % of each call's shares repeating an earlier nullifier (half of the repeats
            are exact replays, DUPLICATE; half carry another x, SPAM: the path with the field inversion).  Packed shares
            in, statuses, secrets and first tags out, the copies to and from the device inside the timed region; device
            and host take the same call alternately, and their outputs are compared on every call.  Median and min-max
            of `calls` calls after 2 warm-up calls.  Every call adds its shares to the log, so "empty" and "half full"
            name the state before the first warm-up call.
  verifier  rlnamd_verify_many_gpu_ex (the verifier's own choice of shape) at the same three sizes, as
            tools/verify_throughput.py measures it

The condition a relay loop sets: a stage behind verification must not be slower than it, so `observe` of 65 536 shares
must take less than the verifier's pass of 65 536 measured in the same run ("observe_65536_below_verifier").
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = (1024, 8192, 65536)
CAPACITY = 1 << 24
HALF = 1 << 23
PREFILL_CHUNK = 1 << 18
DUPLICATES = (0.01, 0.5)
WARMUP = 2
STEP_LIMIT_S = {"log": 500, "verifier": 240}
U64P = C.POINTER(C.c_uint64)


def host_lib():
    host = os.path.join(ROOT, "tests", "host")
    so, src = os.path.join(host, "libnullifierlog.so"), os.path.join(host, "nullifierlog.cpp")
    hdr = os.path.join(ROOT, "zerokit_amd", "csrc", "nullifier_log.h")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I",
                               os.path.join(ROOT, "zerokit_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    lib.nl_new.argtypes = [C.c_uint64, C.c_uint64]
    lib.nl_new.restype = C.c_void_p
    lib.nl_free.argtypes = [C.c_void_p]
    lib.nl_free.restype = None
    lib.nl_clear.argtypes = [C.c_void_p]
    lib.nl_clear.restype = None
    lib.nl_observe.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, U64P, C.c_char_p, C.c_char_p, U64P, C.c_int]
    lib.nl_observe.restype = C.c_int
    return lib


def make_batch(rng, n, dup, pool):
    """n packed shares; a fraction `dup` of them repeats the nullifier of a share of `pool` (or of the batch itself while
    the pool is empty), half of those as exact replays, the others with an x and a y of their own.  Every field element
    has a zero top byte: canonical."""
    import numpy as np
    b = rng.integers(0, 256, size=(n, 128), dtype=np.uint8)
    b[:, 31::32] = 0
    b[:, 96:127] = 7     # one epoch, one external nullifier
    k = int(n * dup)
    if k:
        rows = rng.choice(n, size=k, replace=False)
        src = pool if len(pool) else b.copy()
        picked = src[rng.integers(0, len(src), size=k)]
        b[rows, :32] = picked[:, :32]
        b[rows[:k // 2]] = picked[:k // 2]
    return b


def row(n, ts):
    med = statistics.median(ts)
    return {"n": n, "calls": len(ts), "median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3), "per_s": round(n / med, 1)}


def step_log(calls):
    import numpy as np
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import NullifierLog
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("nullifier_log_throughput: no HIP device (there is no CPU fallback for the device side)")
    H = host_lib()
    rng = np.random.default_rng(20260118)
    dev, host = NullifierLog(CAPACITY, 7), H.nl_new(CAPACITY, 7)
    nmax = max(max(SIZES), PREFILL_CHUNK)
    out_d = (C.create_string_buffer(nmax), C.create_string_buffer(32 * nmax), (C.c_uint64 * nmax)())
    out_h = (C.create_string_buffer(nmax), C.create_string_buffer(32 * nmax), (C.c_uint64 * nmax)())

    def both(batch, ts_d=None, ts_h=None):
        n, raw = len(batch), batch.tobytes()
        t0 = time.perf_counter()
        check(lib().rlnamd_nullifier_log_observe(dev._h, n, raw, None, out_d[0], out_d[1], out_d[2]))
        t1 = time.perf_counter()
        rc = H.nl_observe(host, n, raw, None, out_h[0], out_h[1], out_h[2], 0)
        t2 = time.perf_counter()
        assert rc == 0
        assert out_d[0].raw[:n] == out_h[0].raw[:n] and out_d[1].raw[:32 * n] == out_h[1].raw[:32 * n]
        assert out_d[2][:n] == out_h[2][:n]
        if ts_d is not None:
            ts_d.append(t1 - t0)
            ts_h.append(t2 - t1)
        return bytes(out_d[0].raw[:n])

    rows = []
    pool = np.zeros((0, 128), dtype=np.uint8)
    for fill in ("empty", "half"):
        if fill == "half":
            dev.clear()
            H.nl_clear(host)
            for _ in range(HALF // PREFILL_CHUNK):
                pool = make_batch(rng, PREFILL_CHUNK, 0.0, pool)
                both(pool)
        for n in SIZES:
            for dup in DUPLICATES:
                if fill == "empty":
                    dev.clear()
                    H.nl_clear(host)
                    pool = np.zeros((0, 128), dtype=np.uint8)
                ts_d, ts_h, seen = [], [], [0] * 4
                for c in range(WARMUP + calls):
                    batch = make_batch(rng, n, dup, pool)
                    status = both(batch, *((ts_d, ts_h) if c >= WARMUP else (None, None)))
                    for k in range(4):
                        seen[k] += status.count(bytes([k]))
                    pool = np.concatenate([pool, batch])[-(1 << 20):]
                r = {"fill": fill, "duplicates": dup, "device": row(n, ts_d), "host_1_thread": row(n, ts_h),
                     "statuses": dict(zip(("new", "duplicate", "spam", "foreign"), seen))}
                r["device_beats_host"] = r["device"]["median_ms"] < r["host_1_thread"]["median_ms"]
                rows.append(r)
    info = dev.info()
    H.nl_free(host)
    dev.close()
    return {"capacity": CAPACITY, "rows": rows, "longest_walk": info[5], "secret_words_left": info[6]}


def step_verifier(calls):
    import verify_throughput as vt
    from zerokit_amd import lib
    from zerokit_amd._native import check
    p, _inp, _rsb, proofs, values = vt.setup()
    out = []
    for n in SIZES:
        pr, va = vt.tiled(proofs, values, n)
        ok = C.create_string_buffer(n)

        def gpu():
            check(lib().rlnamd_verify_many_gpu_ex(p._h, n, pr, va, 5, 0, ok, None))
        gpu()
        out.append(row(n, vt.timed(gpu, calls)))
        assert ok.raw == b"\x01" * n
    p.close()
    return {"lanes": 0, "device": out}


STEPS = {"log": step_log, "verifier": step_verifier}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.calls < 9:
        ap.error("--calls: at least 9")
    if a.step:
        print(json.dumps(STEPS[a.step](a.calls)))
        return 0
    out = {"tool": "nullifier_log_throughput", "calls": a.calls, "warmup": WARMUP}
    for name in ("log", "verifier"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls)],
                               stdout=subprocess.PIPE, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            out[name] = {"error": "time limit of %d s" % STEP_LIMIT_S[name]}
            break
        if r.returncode != 0:
            out[name] = {"error": "exit status %d" % r.returncode}
            break   # nothing more is started on the device after a failed step
        out[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    good = all("error" not in out.get(k, {"error": 1}) for k in STEPS)
    if good:
        worst = max(r["device"]["median_ms"] for r in out["log"]["rows"] if r["device"]["n"] == 65536)
        verify = next(r["median_ms"] for r in out["verifier"]["device"] if r["n"] == 65536)
        out["observe_65536_worst_median_ms"] = worst
        out["verify_65536_median_ms"] = verify
        out["observe_65536_below_verifier"] = worst < verify
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
