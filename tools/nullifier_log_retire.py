#!/usr/bin/env python3
"""Nullifier-log retire: rlnamd_nullifier_log_retire of one epoch out of three against the only alternative a caller had
before it -- rlnamd_nullifier_log_clear followed by observe of the survivors from host memory.

    python tools/nullifier_log_retire.py [--calls 9] [--log2-capacity 24] [--out FILE]

prints ONE JSON line.  Torch-free (ctypes and numpy).  The measurement runs in a child process of its own under a time
limit; if it fails or runs out of time, nothing more is started on the device.

  retire      a log of capacity 2^24, full, holding three external nullifiers in equal parts, interleaved (share i under
              external nullifier 1 + i mod 3, every nullifier random: all distinct); retire external nullifier 2.  Host
              clock around the call, which ends in a stream wait.  Every call runs on a freshly filled log (clear, then
              observe of the whole fill in calls of 2^18, outside the timed region).
  reobserve   on a second log that never retires: clear, then observe of the survivors -- the same shares with the same
              tags, packed in host memory beforehand -- in calls of 65 536.  This path runs no code of the retire.

The two take turns, `calls` timed rounds after 2 warm-up rounds.  After the last round both logs are asked about the
same 65 536 replays (half of them of retired shares) and must answer alike, and a few records are read back by sequence
number.  Host memory: 128 + 85 bytes per record of capacity (3.6 GB at 2^24).
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

FILL_CHUNK = 1 << 18
REOBSERVE_CHUNK = 1 << 16
WARMUP = 2
STEP_LIMIT_S = 540
RETIRED = 2


def row(n, ts):
    med = statistics.median(ts)
    return {"records": n, "calls": len(ts), "median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3)}


def measure(calls, log2_capacity):
    import numpy as np
    from zerokit_amd import lib
    from zerokit_amd._native import check
    from zerokit_amd.batch import NullifierLog
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("nullifier_log_retire: no HIP device (there is no CPU fallback)")
    capacity = 1 << log2_capacity
    rng = np.random.default_rng(20260119)
    fill = np.empty((capacity, 128), dtype=np.uint8)
    for o in range(0, capacity, FILL_CHUNK):
        fill[o:o + FILL_CHUNK] = rng.integers(0, 256, size=(min(FILL_CHUNK, capacity - o), 128), dtype=np.uint8)
    fill[:, 31::32] = 0                      # every field element has a zero top byte: canonical
    fill[:, 96:128] = 0
    fill[:, 96] = 1 + np.arange(capacity) % 3
    tags = np.arange(capacity, dtype=np.uint64) * 2 + 1
    keep = fill[:, 96] != RETIRED
    kept, kept_tags = np.ascontiguousarray(fill[keep]), np.ascontiguousarray(tags[keep])
    n_kept = len(kept)
    nmax = max(FILL_CHUNK, REOBSERVE_CHUNK)
    status, first = C.create_string_buffer(nmax), (C.c_uint64 * nmax)()
    secrets = C.create_string_buffer(32 * nmax)
    U64P = C.POINTER(C.c_uint64)

    def observe(log, shares, tg, chunk, sec=None):
        for o in range(0, len(shares), chunk):
            part = shares[o:o + chunk]
            check(lib().rlnamd_nullifier_log_observe(log._h, len(part), part.ctypes.data_as(C.c_char_p),
                                                     tg[o:o + chunk].ctypes.data_as(U64P), status, sec, first))

    dev, base = NullifierLog(capacity, 7), NullifierLog(capacity, 7)
    ext = (RETIRED).to_bytes(32, "little")
    removed = C.c_uint64()
    t_retire, t_reobserve = [], []
    for c in range(WARMUP + calls):
        dev.clear()
        observe(dev, fill, tags, FILL_CHUNK)
        assert dev.info()[1] == capacity
        t0 = time.perf_counter()
        check(lib().rlnamd_nullifier_log_retire(dev._h, ext, 1, C.byref(removed)))
        t1 = time.perf_counter()
        assert removed.value == capacity - n_kept and dev.info()[:4] == [capacity, n_kept, 2 * capacity, n_kept]
        t2 = time.perf_counter()
        base.clear()
        observe(base, kept, kept_tags, REOBSERVE_CHUNK)
        t3 = time.perf_counter()
        assert base.info()[:4] == dev.info()[:4]
        if c >= WARMUP:
            t_retire.append(t1 - t0)
            t_reobserve.append(t3 - t2)
    # the two logs hold the same records: the same answers about the same replays, and the same records by number
    picks = rng.integers(0, capacity, size=REOBSERVE_CHUNK)
    replays, retags = np.ascontiguousarray(fill[picks]), np.arange(REOBSERVE_CHUNK, dtype=np.uint64) + (1 << 40)
    answers = []
    for log in (dev, base):
        observe(log, replays, retags, REOBSERVE_CHUNK, secrets)
        answers.append((status.raw[:REOBSERVE_CHUNK], secrets.raw[:32 * REOBSERVE_CHUNK], list(first[:REOBSERVE_CHUNK])))
    assert answers[0] == answers[1]
    seen = {k: answers[0][0].count(bytes([k])) for k in range(4)}
    for seq in (0, 3, capacity // 2 + (0 if (capacity // 2) % 3 != 1 else 1), capacity - 1 - (1 if (capacity - 1) % 3 == 1 else 0)):
        share, tag = dev.get(seq)
        assert b"".join(v.to_bytes(32, "little") for v in share) == fill[seq].tobytes() and tag == tags[seq]
    rinfo, info = dev.retire_info(), dev.info()
    dev.close()
    base.close()
    return {"capacity": capacity, "removed": capacity - n_kept, "kept": n_kept, "retire": row(capacity, t_retire),
            "clear_and_reobserve": row(n_kept, t_reobserve), "reobserve_chunk": REOBSERVE_CHUNK,
            "replay_statuses": dict(zip(("new", "duplicate", "spam", "foreign"), (seen[k] for k in range(4)))),
            "rebuild_longest_walk": rinfo[4], "longest_walk": info[5], "secret_words_left": info[6]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--log2-capacity", type=int, default=24)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.calls < 1 or not 10 <= a.log2_capacity <= 26:
        ap.error("--calls: at least 1; --log2-capacity: 10 .. 26")
    if a.child:
        print(json.dumps(measure(a.calls, a.log2_capacity)))
        return 0
    out = {"tool": "nullifier_log_retire", "calls": a.calls, "warmup": WARMUP}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--log2-capacity",
                            str(a.log2_capacity)], stdout=subprocess.PIPE, timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            out["error"] = "exit status %d" % r.returncode
        else:
            out.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    except subprocess.TimeoutExpired:
        out["error"] = "time limit of %d s" % STEP_LIMIT_S
    if "error" not in out:
        a_ms, b_ms = out["retire"]["median_ms"], out["clear_and_reobserve"]["median_ms"]
        out["reobserve_over_retire"] = round(b_ms / a_ms, 2)
        out["retire_is_faster"] = a_ms < b_ms
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if "error" not in out else 1


if __name__ == "__main__":
    sys.exit(main())
