#!/usr/bin/env python3
"""What durability costs on a persistent tree of 2^20 leaves (depth 20, every leaf set), through the C ABI:
  set_leaf_flush_ms   ffi_set_leaf + ffi_flush                         (median of 15)
  set_leaf_ms         a lone ffi_set_leaf, the flusher at 500 ms       (median of 200)
  open_ms             ffi_rln_new on the closed store, prover included (median of 3), and the same constructor on a
                      temporary tree, so that the store's share can be read off
The script uses nothing newer than RLN.flush(), so it runs unchanged on a commit from before the journal, where a
flush rewrites the whole snapshot.  Prints one JSON line."""
import json
import os
import random
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zerokit_amd.public import RLN  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N = 1 << 20


def median(ts):
    return round(sorted(ts)[len(ts) // 2], 3)


def main():
    tmp = tempfile.mkdtemp(prefix="tree_store_latency_")
    try:
        cfg = os.path.join(tmp, "cfg.json")
        with open(cfg, "w") as f:
            json.dump({"profile": "small", "path": os.path.join(tmp, "db"), "temporary": False, "flush_every_ms": 500}, f)
        plain = os.path.join(tmp, "plain.json")
        with open(plain, "w") as f:
            json.dump({"profile": "small"}, f)
        rnd = random.Random(1)
        r = RLN(20, cfg)
        for start in range(0, N, 1 << 16):
            r.set_leaves_from(start, [rnd.randrange(1, R) for _ in range(1 << 16)])
        r.flush()
        out = {"leaves": r.leaves_set()}
        ts = []
        for k in range(15):
            t0 = time.perf_counter()
            r.set_leaf(rnd.randrange(N), rnd.randrange(1, R))
            r.flush()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["set_leaf_flush_ms"] = median(ts)
        ts = []
        for k in range(200):
            t0 = time.perf_counter()
            r.set_leaf(rnd.randrange(N), rnd.randrange(1, R))
            ts.append((time.perf_counter() - t0) * 1e3)
        out["set_leaf_ms"] = median(ts)
        root = r.get_root()
        t0 = time.perf_counter()
        r.close()
        out["close_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        ts, base = [], []
        for k in range(3):
            t0 = time.perf_counter()
            r = RLN(20, cfg)
            ts.append((time.perf_counter() - t0) * 1e3)
            assert r.get_root() == root and r.leaves_set() == N
            r.close()
            t0 = time.perf_counter()
            p = RLN(20, plain)
            base.append((time.perf_counter() - t0) * 1e3)
            p.close()
        out["open_ms"] = median(ts)
        out["open_temporary_tree_ms"] = median(base)
        if hasattr(RLN, "tree_store_info"):
            r = RLN(20, cfg)
            out["store_info"] = r.tree_store_info()
            r.close()
        out["store_files"] = {n: os.path.getsize(os.path.join(tmp, "db", n)) for n in sorted(os.listdir(os.path.join(tmp, "db")))}
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
