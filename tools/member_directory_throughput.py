#!/usr/bin/env python3
"""Member directory throughput on one GPU: rlnamd_directory_register / _resolve / _slash against what a caller can
compose without the directory.

    python tools/member_directory_throughput.py [--calls 7] [--depth 20] [--out FILE]

prints ONE JSON line.  Torch-free (ctypes).  Every timed region is a host clock around a call that ends in a device
synchronise, inputs packed beforehand; medians and min-max of `calls` calls after one warm-up call of the same shape.

  register   2^depth members (random commitments, limits 1 .. 2^20) into a fresh tree and directory, one call
  composed   the same leaves without a directory: rlnamd_poseidon_hash (arity 2, one batch) + rlnamd_tree_set_range.
             It yields no directory at all: nothing can resolve a secret afterwards.
  resolve    65 536 secrets of registered members, one call
  slash      1, 64 and 1 024 secrets of registered members, one call; the members are registered again, untimed,
             between calls
  host map   the same slashes with a Python dict from commitment to (leaf, limit), one host Poseidon per secret
             (oracle/c's, one call a secret) and rlnamd_tree_set_leaves with zero leaves.  The dict is built untimed.
  The roots of directory and composition are compared after every pair of calls.
The clock line is what rocm-smi reports while the tool runs; nothing is set."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), calls=len(ms))


def clock_line():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l][:1]
    except Exception:
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--resolve", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    from zerokit_amd._native import check, lib
    from zerokit_amd.batch import MemberDirectory, PoseidonTree
    from oracle.c import binding as ob
    if lib().rlnamd_device_count() < 1:
        raise SystemExit("member_directory_throughput needs a HIP device")
    n = 1 << a.depth
    n_res = min(a.resolve, n)
    rnd = random.Random(20)
    secrets = b"".join(rnd.randrange(1, R).to_bytes(32, "little") for _ in range(n_res))
    known = C.create_string_buffer(32 * n_res)
    check(lib().rlnamd_poseidon_hash(secrets, n_res, 1, known))          # the commitments of the known secrets (setup)
    idcs = known.raw + b"".join(rnd.getrandbits(248).to_bytes(32, "little") for _ in range(n - n_res))
    limits = [rnd.randrange(1, 1 << 20) for _ in range(n)]
    idx = (C.c_uint64 * n)(*range(n))
    lim = (C.c_uint32 * n)(*limits)
    status = C.create_string_buffer(n)
    pairs = b"".join(idcs[32 * i:32 * i + 32] + limits[i].to_bytes(32, "little") for i in range(n))
    leaves = C.create_string_buffer(32 * n)
    res = dict(tool="member_directory_throughput", depth=a.depth, members=n, clock_before=clock_line())

    # ---- register against hash + set_range, alternating
    reg, comp = [], []
    tree = d = None
    for call in range(a.calls + 1):
        for x in (d, tree):
            if x is not None:
                x.close()
        tree, plain = PoseidonTree(a.depth), PoseidonTree(a.depth)
        d = MemberDirectory(tree, seed=7)
        t0 = time.perf_counter()
        check(lib().rlnamd_directory_register(d._h, n, idx, idcs, lim, status))
        t1 = time.perf_counter()
        check(lib().rlnamd_poseidon_hash(pairs, n, 2, leaves))
        check(lib().rlnamd_tree_set_range(plain._h, 0, leaves, n))
        t2 = time.perf_counter()
        assert status.raw == bytes(n), "every registration is OK"
        assert tree.root() == plain.root(), "directory and composition disagree on the root"
        plain.close()
        if call:
            reg.append((t1 - t0) * 1e3)
            comp.append((t2 - t1) * 1e3)
    res["register"] = stats(reg)
    res["composed_hash_set_range"] = stats(comp)
    res["register_members_per_s"] = round(n / (statistics.median(reg) * 1e-3))

    # ---- resolve
    ms = []
    st, ix, lm = C.create_string_buffer(n_res), (C.c_uint64 * n_res)(), (C.c_uint32 * n_res)()
    for call in range(a.calls + 1):
        t0 = time.perf_counter()
        check(lib().rlnamd_directory_resolve(d._h, n_res, secrets, None, st, ix, lm))
        t1 = time.perf_counter()
        assert st.raw == bytes(n_res) and list(ix[:64]) == list(range(64)) and list(lm[:64]) == limits[:64]
        if call:
            ms.append((t1 - t0) * 1e3)
    res["resolve_%d" % n_res] = stats(ms)
    res["resolve_secrets_per_s"] = round(n_res / (statistics.median(ms) * 1e-3))

    # ---- slash against the host map
    table = {idcs[32 * i:32 * i + 32]: (i, limits[i]) for i in range(n_res)}       # (the host map, built untimed)
    mirror = PoseidonTree(a.depth)
    check(lib().rlnamd_poseidon_hash(pairs, n, 2, leaves))
    check(lib().rlnamd_tree_set_range(mirror._h, 0, leaves, n))
    removed = C.c_uint64()
    for k in (1, 64, 1024):
        k = min(k, n_res)
        dev, host = [], []
        for call in range(a.calls + 1):
            sec = secrets[:32 * k]
            t0 = time.perf_counter()
            check(lib().rlnamd_directory_slash(d._h, k, sec, None, st, ix, lm, C.byref(removed)))
            t1 = time.perf_counter()
            found = []
            for i in range(k):
                s = int.from_bytes(sec[32 * i:32 * i + 32], "little")
                hit = table.get(ob.poseidon_batch([[s]])[0].to_bytes(32, "little"))
                if hit:
                    found.append(hit[0])
            zidx = (C.c_uint64 * len(found))(*found)
            check(lib().rlnamd_tree_set_leaves(mirror._h, zidx, bytes(32 * len(found)), len(found)))
            t2 = time.perf_counter()
            assert removed.value == k and found == list(range(k)) and tree.root() == mirror.root()
            # back in, untimed
            check(lib().rlnamd_directory_register(d._h, k, idx, idcs, lim, status))
            assert status.raw[:k] == bytes(k)
            check(lib().rlnamd_tree_set_range(mirror._h, 0, leaves, k))
            if call:
                dev.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
        res["slash_%d" % k] = stats(dev)
        res["host_map_slash_%d" % k] = stats(host)
    info = d.info()
    res["info"] = info
    assert info[7] == 0
    res["clock_after"] = clock_line()
    for x in (d, tree, mirror):
        x.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
