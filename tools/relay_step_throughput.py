#!/usr/bin/env python3
"""Relay-step throughput: rlnamd_relay_step against the three-call composition it replaces --
rlnamd_hasher_hash_to_field, rlnamd_verify_many_gpu_ex, the host glue between the stages restated over packed rows
(signal check, shares gathered from the accepted rows, results scattered back; numpy), rlnamd_nullifier_log_observe --
in the method of tools/nullifier_log_throughput.py.

    python tools/relay_step_throughput.py [--calls 9] [--sizes 1024,8192,65536] [--out FILE]

prints ONE JSON line.  Torch-free (ctypes and numpy).

  inputs    n all-valid proofs of the depth-20 circuit made on the device, message i's x = hash_to_field(signal i), 1 % of
            the rows replaced by an earlier row (a repeated nullifier: DUPLICATE); signals of 32 bytes and of 1 KiB
  forms     the two forms take the same call alternately in one process, each on a log of its own of capacity 2^24 with
            the same seed, emptied (untimed) before every call so that every call sees the same log; the outputs of
            every call are compared with the other form's
  timing    a host clock around each call (both end in a stream wait); median and min-max of `calls` calls after 2
            warm-up calls

  --ffi     the drop-in entry as well: ffi_relay_step on an object with "relay_gpu_min": 0 against
            ffi_verify_rln_signals_batch + ffi_nullifier_log_observe(take = ok) on an object with the default config (what
            ffi_relay_step itself runs below "relay_gpu_min"), over the same proofs as FFI objects, 32-byte signals, an empty
            roots window; the handle arrays, the signals' vectors and the proof values (one ffi_rln_proof_get_values per
            proof, which a caller of the three-call loop pays on every call) are made outside the timed region
            (sizes up to 8 192: every proof object is parsed and subgroup-checked on the host when it is made)

  --optimistic   another measurement instead (optimistic_main): the exact relay against the relay made with
            RLNAMD_RELAY_OPTIMISTIC | RLNAMD_RELAY_OPTIMISTIC_TEAMS, alternated, all-valid and with one forged proof per
            call under cool-down 0; with --ffi the drop-in entry of an optimistic object on its two routes; and the
            seeded aggregate against the one that draws its scalars on the host (profiles/relay_step_optimistic.md)

  --window  another measurement instead (window_main): the same step on three relays that take the call alternately, each
            on a log of its own -- no epoch window, a window of 3 external nullifiers, a window of 64 whose matching
            ones come last -- over rows under three external nullifiers, all of them in the window, so that the three
            do the same work but for the compares; then rlnamd_relay_set_epochs that drops one epoch of three from a
            log of 2^20 records against rlnamd_nullifier_log_retire of that epoch on a twin (profiles/relay_window.md)

"relay_gpu_min" is the smallest measured n at which the step's median is below the composition's minimum, for both
signal lengths (the rule profiles/verify_gpu_lanes.md used for verify_team_max); null if there is none.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAPACITY = 1 << 24
WARMUP = 2
SEED = 0x5EED0002
PROVE_CHUNK = 1024
U64P = C.POINTER(C.c_uint64)


def make_rows(prover, hasher, n, signal_len, rnd, epochs=None):
    """-> (proofs n x 128, values n x 160, signals, offsets); epochs: row i proves under external nullifier
    epochs[i % len(epochs)] instead of the workload's own"""
    from zerokit_amd import workload
    signals = rnd.integers(0, 256, size=(n, signal_len), dtype=np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint64) * signal_len
    xs = np.frombuffer(hasher.hash_to_field_raw(signals.tobytes(), offsets.tolist()), dtype=np.uint8).reshape(n, 32)
    off_x = prover.slots["x"][0]
    proofs, values = [], []
    for first in range(0, n, PROVE_CHUNK):
        c = min(PROVE_CHUNK, n - first)
        inp, rsb = workload.config2_packed(prover.slots, prover.inputs_size, first, c)
        buf = np.frombuffer(inp, dtype=np.uint8).reshape(c, prover.inputs_size, 32).copy()
        buf[:, off_x, :] = xs[first:first + c]
        if epochs:
            off_e = prover.slots["externalNullifier"][0]
            for i in range(c):
                buf[i, off_e, :] = np.frombuffer(int(epochs[(first + i) % len(epochs)]).to_bytes(32, "little"), dtype=np.uint8)
        t, got = prover.submit(buf.tobytes(), rsb)
        pr, va, errs = prover.collect_raw(t, got)
        assert not any(errs)
        proofs.append(pr)
        values.append(va)
    proofs = np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(n, 128).copy()
    values = np.frombuffer(b"".join(values), dtype=np.uint8).reshape(n, 160).copy()
    for i in rnd.choice(np.arange(1, n), size=max(1, n // 100), replace=False):   # 1 %: an earlier row again
        j = int(rnd.integers(0, i))
        proofs[i], values[i], signals[i] = proofs[j], values[j], signals[j]
    return proofs.tobytes(), values.tobytes(), signals.tobytes(), offsets


def composition(lib, check, prover, hasher, log, n, proofs, values, signals, offsets_c):
    """the three calls and the glue; -> (verdict, status, secrets, first tags) as numpy arrays"""
    xs = C.create_string_buffer(32 * n)
    check(lib.rlnamd_hasher_hash_to_field(hasher._h, signals, len(signals), offsets_c, n, xs))
    ok = C.create_string_buffer(n)
    check(lib.rlnamd_verify_many_gpu_ex(prover._h, n, proofs, values, 5, 0, ok, None))
    v = np.frombuffer(values, dtype=np.uint8).reshape(n, 5, 32)
    passed = np.frombuffer(ok, dtype=np.uint8, count=n) != 0
    signal_ok = (v[:, 3, :] == np.frombuffer(xs, dtype=np.uint8, count=32 * n).reshape(n, 32)).all(axis=1)
    verdict = np.where(~passed, 1, np.where(~signal_ok, 3, 0)).astype(np.uint8)
    take = np.flatnonzero(verdict == 0)
    m = len(take)
    shares = np.ascontiguousarray(v[take][:, (2, 3, 0, 4), :]).tobytes()   # nullifier | x | y | external nullifier
    tags = np.ascontiguousarray(take.astype(np.uint64))
    st, sec, ft = C.create_string_buffer(max(m, 1)), C.create_string_buffer(max(32 * m, 1)), np.zeros(max(m, 1), dtype=np.uint64)
    check(lib.rlnamd_nullifier_log_observe(log._h, m, shares, tags.ctypes.data_as(U64P), st, sec, ft.ctypes.data_as(U64P)))
    status = np.full(n, 4, dtype=np.uint8)
    secrets = np.zeros((n, 32), dtype=np.uint8)
    first = np.zeros(n, dtype=np.uint64)
    status[take] = np.frombuffer(st, dtype=np.uint8, count=m)
    secrets[take] = np.frombuffer(sec, dtype=np.uint8, count=32 * m).reshape(m, 32)
    first[take] = ft[:m]
    return verdict, status, secrets, first


def ffi_rows(lib, sizes, calls, proofs, values, signals, signal_len, tmp):
    """ffi_relay_step against the composition over FFI objects; -> rows like main()'s"""
    from zerokit_amd._native import CFr, VecCFr, VecU8
    from zerokit_amd.batch import NullifierLog
    from zerokit_amd.public import RLN, RLNProof, _err
    cfg = os.path.join(tmp, "relay_step_cfg.json")
    with open(cfg, "w") as f:
        f.write(json.dumps({"relay_gpu_min": 0}))
    step_obj, comp_obj = RLN(20, tree_config=cfg), RLN(20)
    logs = NullifierLog(CAPACITY, SEED), NullifierLog(CAPACITY, SEED)

    def call(res):
        if not res.ok:
            raise SystemExit("an FFI call failed: " + _err(res.err))

    n_max = max(sizes)
    v = np.frombuffer(values, dtype=np.uint8).reshape(-1, 5, 32)
    objs = []
    for i in range(n_max):   # 0x00 | proof | 0x00 | root | external nullifier | x | y | nullifier
        objs.append(RLNProof.from_bytes_le(b"\0" + proofs[128 * i:128 * i + 128] + b"\0" + v[i, (1, 4, 3, 0, 2), :].tobytes()))
    vals = [p.values for p in objs]
    sig = np.frombuffer(signals, dtype=np.uint8).reshape(-1, signal_len)
    sig_bufs = [(C.c_uint8 * signal_len).from_buffer_copy(sig[i].tobytes()) for i in range(n_max)]
    rows = []
    for n in sizes:
        hs = (C.c_void_p * n)(*[p._h.value for p in objs[:n]])
        vs = (C.c_void_p * n)(*[x._h.value for x in vals[:n]])
        vecs = (VecU8 * n)(*[VecU8(C.cast(b, C.POINTER(C.c_uint8)), signal_len, signal_len) for b in sig_bufs[:n]])
        any_root = VecCFr(None, 0, 0)
        tags = (C.c_uint64 * n)(*range(n))
        out = [(C.create_string_buffer(n), C.create_string_buffer(n), (CFr * n)(), (C.c_uint64 * n)()) for _ in range(2)]
        ok = (C.c_bool * n)()
        ms = {"step": [], "composition": []}
        for k in range(WARMUP + calls):
            for log in logs:
                log.clear()
            t0 = time.perf_counter()
            call(lib.ffi_relay_step(C.byref(step_obj._h), logs[0]._h, hs, n, vecs, C.byref(any_root), tags, *out[0]))
            t1 = time.perf_counter()
            call(lib.ffi_verify_rln_signals_batch(C.byref(comp_obj._h), hs, n, vecs, C.byref(any_root), ok))
            call(lib.ffi_nullifier_log_observe(logs[1]._h, vs, n, ok, tags, out[1][1], out[1][2], out[1][3]))
            t2 = time.perf_counter()
            same = [a == 0 for a in out[0][0].raw] == list(ok) and out[0][1].raw == out[1][1].raw and \
                bytes(out[0][2]) == bytes(out[1][2]) and list(out[0][3]) == list(out[1][3])
            if not same or logs[0].info()[1] != logs[1].info()[1]:
                raise SystemExit("ffi_relay_step and the composition differ: n %d, call %d" % (n, k))
            if k >= WARMUP:
                ms["step"].append((t1 - t0) * 1e3)
                ms["composition"].append((t2 - t1) * 1e3)
        row = dict(n=n, signal_bytes=signal_len, accepted=int(sum(ok)), duplicates=int(out[1][1].raw.count(b"\1")))
        for form, t in ms.items():
            row[form + "_ms"] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))
        rows.append(row)
    for log in logs:
        log.close()
    return rows


def summary(t):
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))


def optimistic_ffi_rows(lib, sizes, calls, proofs, values, signals, signal_len, tmp):
    """ffi_relay_step of an object with "verify_optimistic" (and "verify_optimistic_teams", cool-down 0) on the device
    route against the same call on an object whose "relay_gpu_min" keeps it on the composition, which is what such an
    object ran at every n before its relays could take the combined check"""
    from zerokit_amd._native import CFr, VecCFr, VecU8
    from zerokit_amd.batch import NullifierLog
    from zerokit_amd.public import RLN, RLNProof, _err
    objs = []
    for name, gpu_min in (("device", 0), ("composition", 1000000000)):
        cfg = os.path.join(tmp, "relay_opt_%s.json" % name)
        with open(cfg, "w") as f:
            f.write(json.dumps({"verify_optimistic": True, "verify_optimistic_teams": True, "verify_optimistic_cooldown": 0,
                                "relay_gpu_min": gpu_min}))
        objs.append(RLN(20, tree_config=cfg))
    logs = NullifierLog(CAPACITY, SEED), NullifierLog(CAPACITY, SEED)
    n_max = max(sizes)
    v = np.frombuffer(values, dtype=np.uint8).reshape(-1, 5, 32)
    pobjs = [RLNProof.from_bytes_le(b"\0" + proofs[128 * i:128 * i + 128] + b"\0" + v[i, (1, 4, 3, 0, 2), :].tobytes())
             for i in range(n_max)]
    sig = np.frombuffer(signals, dtype=np.uint8).reshape(-1, signal_len)
    sig_bufs = [(C.c_uint8 * signal_len).from_buffer_copy(sig[i].tobytes()) for i in range(n_max)]
    rows = []
    for n in sizes:
        hs = (C.c_void_p * n)(*[p._h.value for p in pobjs[:n]])
        vecs = (VecU8 * n)(*[VecU8(C.cast(b, C.POINTER(C.c_uint8)), signal_len, signal_len) for b in sig_bufs[:n]])
        any_root = VecCFr(None, 0, 0)
        tags = (C.c_uint64 * n)(*range(n))
        out = [(C.create_string_buffer(n), C.create_string_buffer(n), (CFr * n)(), (C.c_uint64 * n)()) for _ in range(2)]
        ms = ([], [])
        for k in range(WARMUP + calls):
            for log in logs:
                log.clear()
            for j in (0, 1):
                t0 = time.perf_counter()
                res = lib.ffi_relay_step(C.byref(objs[j]._h), logs[j]._h, hs, n, vecs, C.byref(any_root), tags, *out[j])
                t1 = time.perf_counter()
                if not res.ok:
                    raise SystemExit("ffi_relay_step failed: " + _err(res.err))
                if k >= WARMUP:
                    ms[j].append((t1 - t0) * 1e3)
            if any(bytes(x) != bytes(y) for x, y in zip(out[0][:3], out[1][:3])) or list(out[0][3]) != list(out[1][3]):
                raise SystemExit("the two routes of ffi_relay_step differ: n %d, call %d" % (n, k))
        rows.append(dict(n=n, device_ms=summary(ms[0]), composition_ms=summary(ms[1]),
                         device_stats=objs[0].verify_stats(), composition_stats=objs[1].verify_stats()))
    for log in logs:
        log.close()
    return rows


def optimistic_main(a):
    """--optimistic: the exact relay (flags 0) and the optimistic relay (both flags) take the same call alternately, each
    on a log of its own, emptied before every call; all-valid rows, then the same rows with ONE forged proof (row 1's
    points under row 0's values, in the middle of the call) under cool-down 0, so that every call of the optimistic
    relay pays a combined check AND the exact pass.  Then the drop-in entry (--ffi), and the seeded aggregate against
    the one that draws n scalars on the host, at the largest size."""
    from zerokit_amd import lib as load
    from zerokit_amd._native import check
    from zerokit_amd.batch import BatchProver, Hasher, NullifierLog, Relay
    lib = load()
    sizes = [int(s) for s in a.sizes.split(",")]
    signal_len = 32
    prover = BatchProver(max_batch=PROVE_CHUNK)
    prover.verify_set_cooldown(0)
    hasher = Hasher()
    logs = NullifierLog(CAPACITY, SEED), NullifierLog(CAPACITY, SEED)
    relays = Relay(prover, logs[0], hasher, 0), Relay(prover, logs[1], hasher, 0, optimistic=True, team_checks=True)
    rnd = np.random.default_rng(20261020)
    proofs, values, signals, offsets = make_rows(prover, hasher, max(sizes), signal_len, rnd)
    rows = []
    for forged in (False, True):
        for n in sizes:
            pr, va, sg = bytearray(proofs[:128 * n]), values[:160 * n], signals[:signal_len * n]
            if forged:
                at = n // 2
                pr[128 * at:128 * at + 128] = proofs[128:256]
                va = va[:160 * at] + values[:160] + va[160 * at + 160:]
                sg = sg[:signal_len * at] + signals[:signal_len] + sg[signal_len * at + signal_len:]
            pr = bytes(pr)
            off_c = np.ascontiguousarray(offsets[:n + 1]).ctypes.data_as(U64P)
            tags = np.arange(n, dtype=np.uint64)
            outs = [(C.create_string_buffer(n), C.create_string_buffer(n), C.create_string_buffer(32 * n), np.zeros(n, dtype=np.uint64))
                    for _ in range(2)]
            ms = ([], [])
            s0, p0 = prover.verify_optimistic_stats(), prover.verify_gpu_passes()
            for call in range(WARMUP + a.calls):
                for log in logs:
                    log.clear()
                for j in (0, 1):
                    o = outs[j]
                    t0 = time.perf_counter()
                    check(lib.rlnamd_relay_step(relays[j]._h, n, pr, va, 5, sg, len(sg), off_c, None, None, 0,
                                                tags.ctypes.data_as(U64P), o[0], o[1], o[2], o[3].ctypes.data_as(U64P)))
                    t1 = time.perf_counter()
                    if call >= WARMUP:
                        ms[j].append((t1 - t0) * 1e3)
                if any(x.raw != y.raw for x, y in zip(outs[0][:3], outs[1][:3])) or not np.array_equal(outs[0][3], outs[1][3]):
                    raise SystemExit("the exact and the optimistic step differ: n %d, call %d" % (n, call))
                if logs[0].info()[1] != logs[1].info()[1] or logs[0].info()[3] != logs[1].info()[3]:
                    raise SystemExit("the two logs differ: n %d, call %d" % (n, call))
            s1, p1 = prover.verify_optimistic_stats(), prover.verify_gpu_passes()
            rows.append(dict(n=n, forged=int(forged), bad_proofs=int(outs[0][0].raw.count(b"\1")), exact_ms=summary(ms[0]),
                             optimistic_ms=summary(ms[1]),
                             stats={k: s1[k] - s0[k] for k in ("combined", "accepted", "fell_back", "combined_team")},
                             passes=[p1[0] - p0[0], p1[1] - p0[1]]))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = dict(tool="relay_step_throughput --optimistic", calls=a.calls, warmup=WARMUP, capacity=CAPACITY, rows=rows)
    # the scalars: derived on the device from a seed, against n x 16 bytes drawn on the calling thread and copied in
    n = max(sizes)
    gt, rej = C.create_string_buffer(384), C.create_string_buffer(n)
    seed = bytes(range(32))
    ms = dict(seeded=[], drawn=[], getrandom=[])
    for call in range(WARMUP + a.calls):
        t0 = time.perf_counter()
        check(lib.rlnamd_verify_gpu_aggregate_seeded(prover._h, n, proofs[:128 * n], values[:160 * n], 5, seed, 1, gt, rej))
        t1 = time.perf_counter()
        check(lib.rlnamd_verify_gpu_aggregate_ex(prover._h, n, proofs[:128 * n], values[:160 * n], 5, None, 1, gt, rej))
        t2 = time.perf_counter()
        os.getrandom(16 * n)
        t3 = time.perf_counter()
        if call >= WARMUP:
            ms["seeded"].append((t1 - t0) * 1e3)
            ms["drawn"].append((t2 - t1) * 1e3)
            ms["getrandom"].append((t3 - t2) * 1e3)
    out["scalars"] = dict(n=n, aggregate_seeded_ms=summary(ms["seeded"]), aggregate_drawn_ms=summary(ms["drawn"]),
                          getrandom_16n_bytes_ms=summary(ms["getrandom"]))
    for r in relays:
        r.close()
    if a.ffi:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            out["ffi_rows"] = optimistic_ffi_rows(lib, [n for n in sizes if n <= 8192], a.calls, proofs, values, signals,
                                                  signal_len, tmp)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for log in logs:
        log.close()
    hasher.close()
    prover.close()


def window_main(a):
    """--window: see the module's text"""
    from zerokit_amd import lib as load
    from zerokit_amd._native import check
    from zerokit_amd.batch import BatchProver, Hasher, NullifierLog, Relay
    lib = load()
    sizes = [int(s) for s in a.sizes.split(",")]
    signal_len = 32
    epochs = [900001, 900002, 900003]
    windows = dict(none=[], window_3=epochs, window_64=[800000 + j for j in range(61)] + epochs)
    prover = BatchProver(max_batch=PROVE_CHUNK)
    hasher = Hasher()
    logs = [NullifierLog(CAPACITY, SEED) for _ in windows]
    relays = [Relay(prover, log, hasher, 0) for log in logs]
    for relay, w in zip(relays, windows.values()):
        relay.set_epochs(w)
    rnd = np.random.default_rng(20261021)
    proofs, values, signals, offsets = make_rows(prover, hasher, max(sizes), signal_len, rnd, epochs)
    rows = []
    for n in sizes:
        pr, va, sg = proofs[:128 * n], values[:160 * n], signals[:signal_len * n]
        off_c = np.ascontiguousarray(offsets[:n + 1]).ctypes.data_as(U64P)
        tags = np.arange(n, dtype=np.uint64)
        outs = [(C.create_string_buffer(n), C.create_string_buffer(n), C.create_string_buffer(32 * n), np.zeros(n, dtype=np.uint64))
                for _ in relays]
        ms = [[] for _ in relays]
        for call in range(WARMUP + a.calls):
            for log in logs:
                log.clear()
            for j, relay in enumerate(relays):
                o = outs[j]
                t0 = time.perf_counter()
                check(lib.rlnamd_relay_step(relay._h, n, pr, va, 5, sg, len(sg), off_c, None, None, 0, tags.ctypes.data_as(U64P),
                                            o[0], o[1], o[2], o[3].ctypes.data_as(U64P)))
                t1 = time.perf_counter()
                if call >= WARMUP:
                    ms[j].append((t1 - t0) * 1e3)
            for o in outs[1:]:
                if any(x.raw != y.raw for x, y in zip(outs[0][:3], o[:3])) or not np.array_equal(outs[0][3], o[3]):
                    raise SystemExit("the steps with and without a window differ: n %d, call %d" % (n, call))
        row = dict(n=n, accepted=int(outs[0][0].raw.count(b"\0")), bad_epoch=[r.info()["bad_epoch"] for r in relays])
        for name, t in zip(windows, ms):
            row[name + "_ms"] = summary(t)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    for r in relays:
        r.close()
    for log in logs:
        log.close()
    # moving the window on a log of 2^20 records under three epochs in equal parts: set_epochs keeps two, retire drops one
    m = 1 << 20
    raw = np.zeros((m, 4, 32), dtype=np.uint8)
    raw[:, :3, :24] = rnd.integers(0, 256, size=(m, 3, 24), dtype=np.uint8)   # nullifier, x, y: random, below r
    for i, e in enumerate(epochs):
        raw[i::3, 3, :] = np.frombuffer(int(e).to_bytes(32, "little"), dtype=np.uint8)
    shares = raw.tobytes()
    pair = NullifierLog(m, SEED), NullifierLog(m, SEED)
    relay = Relay(prover, pair[0], None, 0)
    status = C.create_string_buffer(m)
    ms = dict(set_epochs=[], retire=[])
    removed = []
    for call in range(WARMUP + a.calls):
        relay.set_epochs([])
        for log in pair:
            log.clear()
            check(lib.rlnamd_nullifier_log_observe(log._h, m, shares, None, status, None, None))
        t0 = time.perf_counter()
        gone = relay.set_epochs(epochs[1:])
        t1 = time.perf_counter()
        other = pair[1].retire(epochs[:1])
        t2 = time.perf_counter()
        if gone != other or pair[0].info()[:4] != pair[1].info()[:4]:
            raise SystemExit("set_epochs and the retire of the complement differ")
        removed.append(gone)
        if call >= WARMUP:
            ms["set_epochs"].append((t1 - t0) * 1e3)
            ms["retire"].append((t2 - t1) * 1e3)
    out = dict(tool="relay_step_throughput --window", calls=a.calls, warmup=WARMUP, capacity=CAPACITY, rows=rows,
               move=dict(records=m, removed=removed[-1], set_epochs_ms=summary(ms["set_epochs"]), retire_ms=summary(ms["retire"])))
    relay.close()
    for log in pair:
        log.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    hasher.close()
    prover.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--sizes", default="1024,8192,65536")
    ap.add_argument("--signal-bytes", default="32,1024")
    ap.add_argument("--ffi", action="store_true")
    ap.add_argument("--optimistic", action="store_true")
    ap.add_argument("--window", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.optimistic:
        return optimistic_main(a)
    if a.window:
        return window_main(a)
    from zerokit_amd import lib as load
    from zerokit_amd._native import check
    from zerokit_amd.batch import BatchProver, Hasher, NullifierLog, Relay
    lib = load()
    sizes = [int(s) for s in a.sizes.split(",")]
    prover = BatchProver(max_batch=PROVE_CHUNK)
    hasher = Hasher()
    logs = NullifierLog(CAPACITY, SEED), NullifierLog(CAPACITY, SEED)
    relay = Relay(prover, logs[0], hasher, 0)
    rnd = np.random.default_rng(20261019)
    rows, drop_in = [], None
    for signal_len in [int(s) for s in a.signal_bytes.split(",")]:
        proofs, values, signals, offsets = make_rows(prover, hasher, max(sizes), signal_len, rnd)
        if a.ffi and drop_in is None:
            import tempfile
            with tempfile.TemporaryDirectory() as tmp:
                drop_in = ffi_rows(lib, [n for n in sizes if n <= 8192], a.calls, proofs, values, signals, signal_len, tmp)
        for n in sizes:
            pr, va, sg = proofs[:128 * n], values[:160 * n], signals[:signal_len * n]
            off = np.ascontiguousarray(offsets[:n + 1])
            off_c = off.ctypes.data_as(U64P)
            tags = np.arange(n, dtype=np.uint64)
            verdict, status = C.create_string_buffer(n), C.create_string_buffer(n)
            secrets, first = C.create_string_buffer(32 * n), np.zeros(n, dtype=np.uint64)
            ms = {"step": [], "composition": []}
            for call in range(WARMUP + a.calls):
                for log in logs:
                    log.clear()
                t0 = time.perf_counter()
                check(lib.rlnamd_relay_step(relay._h, n, pr, va, 5, sg, len(sg), off_c, None, None, 0, tags.ctypes.data_as(U64P),
                                            verdict, status, secrets, first.ctypes.data_as(U64P)))
                t1 = time.perf_counter()
                want = composition(lib, check, prover, hasher, logs[1], n, pr, va, sg, off_c)
                t2 = time.perf_counter()
                got = (np.frombuffer(verdict, dtype=np.uint8, count=n), np.frombuffer(status, dtype=np.uint8, count=n),
                       np.frombuffer(secrets, dtype=np.uint8, count=32 * n).reshape(n, 32), first)
                if not all(np.array_equal(g, w) for g, w in zip(got, want)):
                    raise SystemExit("the step and the composition differ: n %d, signals of %d bytes, call %d" % (n, signal_len, call))
                if logs[0].info()[1] != logs[1].info()[1] or logs[0].info()[3] != logs[1].info()[3]:
                    raise SystemExit("the two logs differ: n %d, call %d" % (n, call))
                if call >= WARMUP:
                    ms["step"].append((t1 - t0) * 1e3)
                    ms["composition"].append((t2 - t1) * 1e3)
            row = dict(n=n, signal_bytes=signal_len, accepted=int((want[0] == 0).sum()), duplicates=int((want[1] == 1).sum()))
            for form, t in ms.items():
                row[form + "_ms"] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))
            rows.append(row)
    wins = [n for n in sizes if all(r["step_ms"]["median"] < r["composition_ms"]["min"] for r in rows if r["n"] == n)]
    out = dict(tool="relay_step_throughput", calls=a.calls, warmup=WARMUP, capacity=CAPACITY, rows=rows,
               relay_gpu_min=min(wins) if wins else None, relay_info=relay.info())
    if drop_in is not None:
        ffi_wins = [r["n"] for r in drop_in if r["step_ms"]["median"] < r["composition_ms"]["min"]]
        out["ffi_rows"], out["ffi_relay_gpu_min"] = drop_in, (min(ffi_wins) if ffi_wins else None)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    relay.close()
    for log in logs:
        log.close()
    hasher.close()
    prover.close()


if __name__ == "__main__":
    main()
