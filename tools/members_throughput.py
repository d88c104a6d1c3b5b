#!/usr/bin/env python3
"""Proving for random members of a 2^20-leaf tree, three ways, each timed from "leaf indices known" to "proofs on the
host":

  a        n x ffi_get_merkle_proof + n x ffi_rln_witness_input_new_single + ffi_generate_rln_proofs_batch
           (the only way before rlnamd_tree_proofs_at / *_members existed: one synchronous path round trip per proof)
  b        rlnamd_tree_proofs_at (one call) + the paths packed into the inputs on the host + rlnamd_prover_prove_stream
  c_ext    rlnamd_prover_prove_stream_members: the paths gathered on the device, straight into the staged inputs
  c_ffi    ffi_generate_rln_proofs_for_members on the object of (a)

    python tools/members_throughput.py [--n 1024,8192] [--calls 5] [--out FILE]

prints ONE JSON line: per n and way the median and the spread (min, max) of `calls` timed calls in ms, after one warm-up
call.  (a) and c_ffi run on one FFI object (the default 20 GiB tables, max_batch 1024), (b) and c_ext on one extension
prover of the same size with a tree of its own holding the same leaves.  What every way knows in advance: the leaf
indices and, per proof, secret, limit, message id, x, external nullifier and (r, s) -- as CFr arrays / packed inputs
without a path.  Inside the timed region of (a): the calls through ctypes (about a microsecond each), no conversion to
Python integers; the witness and proof objects are freed outside it.  Torch-free.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTH = 20
LEAVES = 1 << DEPTH
LIMIT = 100


def cfr_array(np, values64):
    """n field elements below 2^64 as a ctypes CFr array"""
    from zerokit_amd._native import CFr
    a = np.zeros((len(values64), 4), dtype="<u8")
    a[:, 0] = values64
    return (CFr * len(values64)).from_buffer_copy(a.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1024,8192")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = [int(t) for t in args.n.split(",")]
    import numpy as np
    from zerokit_amd._native import CFr, MerkleProof, VecCFr, lib
    from zerokit_amd.batch import BatchProver, PoseidonTree
    from zerokit_amd.public import RLN, _ok_bool, _ok_ptr
    L = lib()
    if L.rlnamd_device_count() < 1:
        raise SystemExit("members_throughput: no HIP device")
    rng = np.random.default_rng(20)
    # the tree: leaf i = i + 1 on every leaf (the proofs are valid for the root the circuit computes from the path; whether
    # that is the tree's root does not change what any of the ways does)
    leaf_values = np.arange(1, LEAVES + 1, dtype="<u8")
    rln = RLN(DEPTH)
    arr = cfr_array(np, leaf_values)
    v = VecCFr(C.cast(arr, C.POINTER(CFr)), LEAVES, LEAVES)
    _ok_bool(L.ffi_set_leaves_from(C.byref(rln._h), 0, C.byref(v)))
    rln.get_root()
    tree = PoseidonTree(DEPTH)
    tree.fill_sequential(0, LEAVES, 1)
    assert tree.root() == rln.get_root()
    p = BatchProver(max_batch=1024)
    NI = p.inputs_size
    po, pl = p.slots["pathElements"][0], p.slots["identityPathIndex"][0]
    res = {"depth": DEPTH, "calls": args.calls, "describe": p.describe(), "sizes": {}}
    for n in sizes:
        idx = rng.integers(0, LEAVES, size=n, dtype=np.uint64)
        secret, msg, x, ext = (rng.integers(1, 1 << 62, size=n, dtype=np.uint64) for _ in range(4))
        msg = msg % LIMIT
        limit = np.full(n, LIMIT, dtype=np.uint64)
        r_s = rng.integers(1, 1 << 62, size=2 * n, dtype=np.uint64)
        cols = [cfr_array(np, c) for c in (secret, limit, msg, x, ext)]
        rs_arr = cfr_array(np, r_s)
        rsb = bytes(rs_arr)
        # packed inputs without a path (extension ways)
        base = np.zeros((n, NI, 32), dtype=np.uint8)
        base[:, 0, 0] = 1
        for name, col in (("identitySecret", secret), ("userMessageLimit", limit), ("messageId", msg), ("x", x),
                          ("externalNullifier", ext)):
            base[:, p.slots[name][0], :8] = col.astype("<u8").view(np.uint8).reshape(n, 8)
        base_bytes = base.tobytes()
        idx_sz = (C.c_size_t * n)(*[int(i) for i in idx])
        idx_list = [int(i) for i in idx]
        handle = C.byref(rln._h)

        def way_a():
            ws = (C.c_void_p * n)()
            for i in range(n):
                h = _ok_ptr(L.ffi_get_merkle_proof(handle, idx_sz[i]))
                mp = C.cast(h, C.POINTER(MerkleProof)).contents
                ws[i] = _ok_ptr(L.ffi_rln_witness_input_new_single(
                    C.byref(cols[0][i]), C.byref(cols[1][i]), C.byref(cols[2][i]), C.byref(mp.path_elements),
                    C.byref(mp.path_index), C.byref(cols[3][i]), C.byref(cols[4][i]))).value
                L.ffi_merkle_proof_free(h)
            outs = (C.c_void_p * n)()
            _ok_bool(L.ffi_generate_rln_proofs_batch(handle, ws, n, C.cast(rs_arr, C.POINTER(CFr)), outs))
            return ws, outs

        def free_a(r):
            ws, outs = r
            for i in range(n):
                L.ffi_rln_witness_input_free(C.c_void_p(ws[i]))
                L.ffi_rln_proof_free(C.c_void_p(outs[i]))

        def way_b():
            e, b = tree.proofs_at_raw(idx_list)
            inp = base.copy()
            inp[:, po:po + DEPTH, :] = np.frombuffer(e, dtype=np.uint8).reshape(n, DEPTH, 32)
            inp[:, pl:pl + DEPTH, 0] = np.frombuffer(b, dtype=np.uint8).reshape(n, DEPTH)
            return p.prove_stream_raw(inp.tobytes(), rsb)

        def way_c_ext():
            return p.prove_members_raw(tree, idx_list, base_bytes, rsb)

        def way_c_ffi():
            outs = (C.c_void_p * n)()
            _ok_bool(L.ffi_generate_rln_proofs_for_members(handle, idx_sz, n, *[C.cast(c, C.POINTER(CFr)) for c in cols],
                                                           C.cast(rs_arr, C.POINTER(CFr)), outs))
            return outs

        def free_c(outs):
            for i in range(n):
                L.ffi_rln_proof_free(C.c_void_p(outs[i]))

        ways = (("a", way_a, free_a), ("b", way_b, None), ("c_ext", way_c_ext, None), ("c_ffi", way_c_ffi, free_c))
        row = {}
        first = {}
        for name, fn, free in ways:
            ts = []
            for k in range(args.calls + 1):
                t0 = time.perf_counter()
                out = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if k == 0:          # warm-up; its proofs are compared across the ways below
                    if name in ("b", "c_ext"):
                        first[name] = out[0]
                        assert not any(out[2])
                else:
                    ts.append(dt)
                if free:
                    free(out)
            row[name] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                         "max_ms": round(max(ts), 3), "proofs_per_s": round(n / statistics.median(ts) * 1e3)}
        assert first["b"] == first["c_ext"], "by index and by path disagree"
        res["sizes"][str(n)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    p.close()
    tree.close()


if __name__ == "__main__":
    main()
