#!/usr/bin/env python3
"""hash_to_field throughput: rlnamd_hasher_hash_to_field on the device against one host thread looping
rlnamd_hash_to_field_le over the same messages (a loop of C: tests/host/keccakbatch.cpp, kb_loop_single), and against
the device verifier's pass for the same n -- the stage a relay loop runs behind the hashing.

    python tools/hash_to_field_throughput.py [--calls 9] [--out FILE] [--md profiles/hash_to_field_batch.md]

prints ONE JSON line and writes the table as markdown.  Torch-free (ctypes and numpy).  The measuring runs in a child
process under a time limit.

  rows       n in 1 024, 8 192, 65 536; messages of 32, 256 and 1 024 bytes, and a mixed row (lengths drawn from
             0 .. 4 096, seed fixed) with and without the lane ordering (the latter on a second hasher, made under
             RLNAMD_HASH_LANE_ORDER=0).  Packed messages in, field elements out, the plan, the packing and the copies
             to and from the device inside the timed region; device and host take the same call alternately and their
             outputs are compared on every call.  Median and min-max of `calls` calls after 2 warm-up calls.
  crossover  32-byte messages at n = 16 .. 512 as well: the smallest n at which the device call beats the host loop
  lone lane  one message of 1 .. 2 048 blocks on a hasher with lane_max_blocks = 4 096, and the host's time for it

The two defaults and the pace of the host route are derived from the table: hash_gpu_min is the crossover rounded up
to a power of two, lane_max_blocks the block count at which a lone lane's chain takes as long as a call of 1 024
32-byte messages (to a power of two), HOST_PACE the lone lane's time per block over the host's.

The verifier's pass is not run here: VERIFIER_MS holds the medians of profiles/nullifier_log.md (the verifier's own
choice of shape: 12.767, 30.179, 37.800 ms) and profiles/verify_gpu.md (a lane per proof: 29.94, 30.10, 37.84 ms),
and a row is held against the smaller of the two.  The bar: at every n, 1 KiB signals take less than that pass.
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

SIZES = (1024, 8192, 65536)
SMALL = (16, 32, 64, 128, 256, 512)
LENGTHS = (32, 256, 1024)
LONE = (1, 2, 8, 32, 128, 512, 2048)
VERIFIER_MS = {1024: 12.767, 8192: 30.10, 65536: 37.800}
WARMUP = 2
LIMIT_S = 900
U64P = C.POINTER(C.c_uint64)


def host_lib():
    host = os.path.join(ROOT, "tests", "host")
    csrc = os.path.join(ROOT, "zerokit_amd", "csrc")
    so, src = os.path.join(host, "libkeccakbatch.so"), os.path.join(host, "keccakbatch.cpp")
    deps = [src] + [os.path.join(csrc, h) for h in ("keccak_batch.h", "keccak.h", "field.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", csrc, src, "-o", so])
    lib = C.CDLL(so)
    lib.kb_loop_single.argtypes = [C.c_void_p, C.c_char_p, U64P, C.c_size_t, C.c_char_p]
    lib.kb_loop_single.restype = C.c_int
    return lib


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4),
            "max_ms": round(max(ts) * 1e3, 4)}


def measure(calls):
    import numpy as np
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import Hasher
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("hash_to_field_throughput: no HIP device (there is no CPU fallback for the device side)")
    H = host_lib()
    single = C.cast(lib().rlnamd_hash_to_field_le, C.c_void_p)
    rng = np.random.default_rng(20261018)
    ordered = Hasher()
    os.environ["RLNAMD_HASH_LANE_ORDER"] = "0"
    unordered = Hasher()
    del os.environ["RLNAMD_HASH_LANE_ORDER"]
    lone = Hasher(lane_max_blocks=4096)

    def both(hasher, lens, n_calls):
        """-> (device times, host times) of n_calls calls behind WARMUP warm-up calls, fresh bytes every call"""
        n = len(lens)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        offs = (C.c_uint64 * (n + 1)).from_buffer_copy(off.tobytes())
        total = int(off[-1])
        out_d, out_h = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
        ts_d, ts_h = [], []
        for c in range(WARMUP + n_calls):
            data = rng.integers(0, 256, size=max(total, 1), dtype=np.uint8).tobytes()
            t0 = time.perf_counter()
            check(lib().rlnamd_hasher_hash_to_field(hasher._h, data, total, offs, n, out_d))
            t1 = time.perf_counter()
            rc = H.kb_loop_single(single, data, offs, n, out_h)
            t2 = time.perf_counter()
            assert rc == 0 and out_d.raw == out_h.raw, "the device and the host disagree"
            if c >= WARMUP:
                ts_d.append(t1 - t0)
                ts_h.append(t2 - t1)
        return ts_d, ts_h

    def row(hasher, n, lens, label):
        ts_d, ts_h = both(hasher, lens, calls)
        info = hasher.info()
        r = {"n": n, "length": label, "device": stats(ts_d), "host_1_thread": stats(ts_h), "chunks": info["chunks"],
             "device_blocks": info["device_blocks"], "host_messages": info["host_messages"]}
        r["device_beats_host"] = r["device"]["median_ms"] < r["host_1_thread"]["median_ms"]
        if n in VERIFIER_MS:
            r["verifier_ms"] = VERIFIER_MS[n]
            r["below_verifier"] = r["device"]["median_ms"] < VERIFIER_MS[n]
        return r

    rows, small = [], []
    for n in SMALL:
        small.append(row(ordered, n, np.full(n, 32, dtype=np.uint64), "32"))
    for n in SIZES:
        for length in LENGTHS:
            rows.append(row(ordered, n, np.full(n, length, dtype=np.uint64), str(length)))
        mixed = np.random.default_rng(4096 + n).integers(0, 4097, size=n, dtype=np.uint64)
        rows.append(row(ordered, n, mixed, "mixed 0 .. 4 096, lanes ordered"))
        rows.append(row(unordered, n, mixed, "mixed 0 .. 4 096, lanes in index order"))
    lone_rows = []
    for blocks in LONE:
        ts_d, ts_h = both(lone, np.array([blocks * 136 - 1], dtype=np.uint64), calls)
        assert lone.info()["host_messages"] == 0 and lone.info()["longest_lane_blocks"] == blocks
        lone_rows.append({"blocks": blocks, "device": stats(ts_d), "host_1_thread": stats(ts_h)})
    for h in (ordered, unordered, lone):
        h.close()
    return {"small": small, "rows": rows, "lone_lane": lone_rows}


def pow2_up(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def pow2_nearest(v):
    up = pow2_up(v)
    return up if up == 1 or up / v <= v / (up // 2) else up // 2


def derive(out):
    at32 = out["small"] + [r for r in out["rows"] if r["length"] == "32"]
    wins = [r["n"] for r in at32 if r["device_beats_host"]]
    out["hash_gpu_min"] = pow2_up(min(wins)) if wins else None
    fixed = next(r["device"]["median_ms"] for r in out["rows"] if r["n"] == 1024 and r["length"] == "32")
    a, b = out["lone_lane"][0], out["lone_lane"][-1]
    out["lone_lane_device_us_per_block"] = round((b["device"]["median_ms"] - a["device"]["median_ms"]) * 1e3 / (b["blocks"] - a["blocks"]), 3)
    out["lone_lane_host_us_per_block"] = round((b["host_1_thread"]["median_ms"] - a["host_1_thread"]["median_ms"]) * 1e3 / (b["blocks"] - a["blocks"]), 3)
    out["fixed_cost_ms"] = fixed
    out["lane_max_blocks_exact"] = round(fixed * 1e3 / out["lone_lane_device_us_per_block"], 1)
    out["lane_max_blocks"] = pow2_nearest(out["lane_max_blocks_exact"])
    out["host_pace"] = round(out["lone_lane_device_us_per_block"] / out["lone_lane_host_us_per_block"], 1)
    out["bar_1_kib_below_verifier"] = all(r["below_verifier"] for r in out["rows"] if r["length"] == "1024")


def cell(s):
    return "%.3f (%.3f – %.3f)" % (s["median_ms"], s["min_ms"], s["max_ms"])


def markdown(out):
    L = ["# Signals to field elements on the device: `tools/hash_to_field_throughput.py`", "",
         "One MI355X, one hasher (8 MiB of staging, the default; a second one for the rows without the lane ordering), %d calls behind %d warm-up calls per row; the plan, the"
         % (out["calls"], out["warmup"]),
         "packing and the copies are inside the timed region; every call's output is compared with the host's.  Times are",
         "medians in ms (min – max).  The host is one thread looping `rlnamd_hash_to_field_le` in C.  The verifier's pass is",
         "not run here: it is the smaller of the medians in `profiles/nullifier_log.md` and `profiles/verify_gpu.md`.",
         "\"On the host\" counts the messages the call's plan gave to the calling thread (keccak_batch.h: the host route).", "",
         "| n | message bytes | device call | one host thread | host / device | chunks | on the host | verifier's pass | below it |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in out["small"] + out["rows"]:
        L.append("| %d | %s | %s | %s | %.2f × | %d | %d | %s | %s |" % (
            r["n"], r["length"], cell(r["device"]), cell(r["host_1_thread"]),
            r["host_1_thread"]["median_ms"] / r["device"]["median_ms"], r["chunks"], r["host_messages"],
            "%.3f" % r["verifier_ms"] if "verifier_ms" in r else "—",
            ("yes" if r["below_verifier"] else "**no**") if "below_verifier" in r else "—"))
    L += ["", "Rows where the device does not win: " +
          (", ".join("n = %d at %s bytes" % (r["n"], r["length"]) for r in out["small"] + out["rows"] if not r["device_beats_host"]) or "none") + ".",
          "", "## A lone lane", "",
          "One message on a hasher with `lane_max_blocks = 4096`, so that it runs on a lane whatever its length.", "",
          "| blocks | device | one host thread |", "|---|---|---|"]
    for r in out["lone_lane"]:
        L.append("| %d | %s | %s |" % (r["blocks"], cell(r["device"]), cell(r["host_1_thread"])))
    L += ["", "Per block, from the first row to the last: %.3f µs on a lone lane, %.3f µs on a host core."
          % (out["lone_lane_device_us_per_block"], out["lone_lane_host_us_per_block"]), "",
          "## The two defaults", "",
          "- `hash_gpu_min` (`HASH_GPU_MIN_DEFAULT`, ffi.cpp): the smallest measured n at which the device call beats the host",
          "  thread at 32-byte messages, rounded up to a power of two: **%s**." % out["hash_gpu_min"],
          "- `lane_max_blocks` (`DEFAULT_LANE_MAX_BLOCKS`, keccak_batch.h): the fixed cost of a device call, %.3f ms (n = 1 024,"
          % out["fixed_cost_ms"],
          "  32 bytes), over a lone lane's %.3f µs per block is %.1f blocks; to a power of two: **%d**."
          % (out["lone_lane_device_us_per_block"], out["lane_max_blocks_exact"], out["lane_max_blocks"]),
          "- `HOST_PACE` (keccak_batch.h): a lone lane's time per block over a host core's: **%.1f**." % out["host_pace"], "",
          "## Against the verifier", "",
          "The bar: at every measured n, hashing 1 KiB signals on the device takes less time than the verifier's pass for that n: "
          + ("**met** in all three rows." if out["bar_1_kib_below_verifier"] else "**missed**, see the table."), ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "hash_to_field_batch.md"))
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.calls < 9:
        ap.error("--calls: at least 9")
    if a.measure:
        print(json.dumps(measure(a.calls)))
        return 0
    out = {"tool": "hash_to_field_throughput", "calls": a.calls, "warmup": WARMUP}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls)],
                           stdout=subprocess.PIPE, timeout=LIMIT_S)
        if r.returncode != 0:
            out["error"] = "exit status %d" % r.returncode
        else:
            out.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    except subprocess.TimeoutExpired:
        out["error"] = "time limit of %d s" % LIMIT_S
    if "error" not in out:
        derive(out)
        with open(a.md, "w") as f:
            f.write(markdown(out))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if "error" not in out else 1


if __name__ == "__main__":
    sys.exit(main())
