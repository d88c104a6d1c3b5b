"""Extension surface (include/rln_amd.h): device-resident batch prover and Poseidon tree."""
import ctypes as C
import os

from ._native import ProverInfo, RLNError, check, lib

_HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = 8


def resource_paths(depth=20, multi=False):
    d = os.path.join(_HERE, "resources", "tree_depth_%d%s" % (depth, "_multi_max_out_4" if multi else ""))
    return os.path.join(d, "rln_final.arkzkey"), os.path.join(d, "graph.bin")


_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def _b(x: int, modulus: int = _R) -> bytes:
    """canonical 32-byte LE form; values outside [0, modulus) are refused (the kernels would silently see a
    different residue from the one the host-side checks compared)"""
    x = int(x)
    if not 0 <= x < modulus:
        raise RLNError("Non-canonical field element: value is not in [0, %s-1]" % ("r" if modulus == _R else "q"))
    return x.to_bytes(32, "little")


def _check_verify_shapes(proofs, public_inputs):
    """the C entry points index proofs + 128 i and values + 32 nv i: refuse anything that is not exactly that shape"""
    if len(proofs) != len(public_inputs):
        raise RLNError("verify_many: %d proofs but %d public-input rows" % (len(proofs), len(public_inputs)))
    nv = len(public_inputs[0])
    for i, (p, row) in enumerate(zip(proofs, public_inputs)):
        if len(p) != 128:
            raise RLNError("verify_many: proof %d is %d bytes, expected 128" % (i, len(p)))
        if len(row) != nv:
            raise RLNError("verify_many: public-input row %d has %d entries, expected %d" % (i, len(row), nv))
    return nv


def _unpack_results(proofs, values, errs):
    out = []
    for i in range(len(errs)):
        v = values[160 * i:160 * (i + 1)]
        vals = [int.from_bytes(v[32 * k:32 * k + 32], "little") for k in range(5)]
        out.append(dict(proof=proofs[128 * i:128 * (i + 1)],
                        values=dict(y=vals[0], root=vals[1], nullifier=vals[2], x=vals[3], external_nullifier=vals[4]),
                        public_inputs=vals, error=int(errs[i])))
    return out


class BatchProver:
    """n x generate_zk_proof_with_rs (/root/reference/rln/src/protocol/proof.rs:753-777) +
    proof_values_from_witness (protocol/witness.rs:759-804) in one device batch."""

    def __init__(self, zkey: bytes = None, graph: bytes = None, max_batch=1024, window_bits=0, depth=20, multi=False):
        if zkey is None or graph is None:
            zp, gp = resource_paths(depth, multi)
            zkey, graph = open(zp, "rb").read(), open(gp, "rb").read()
        self._h = C.c_void_p()
        check(lib().rlnamd_prover_new(zkey, len(zkey), graph, len(graph), max_batch, window_bits, C.byref(self._h)))
        info = ProverInfo()
        check(lib().rlnamd_prover_get_info(self._h, C.byref(info)))
        self.info = info
        self.inputs_size = int(info.inputs_size)
        self.slots = {}
        for name in ("identitySecret", "userMessageLimit", "messageId", "pathElements", "identityPathIndex", "x",
                     "externalNullifier", "selectorUsed"):
            off, ln = C.c_uint32(), C.c_uint32()
            if lib().rlnamd_prover_input_slot(self._h, name.encode(), C.byref(off), C.byref(ln)) == 0:
                self.slots[name] = (off.value, ln.value)
        self.num_public = int(lib().rlnamd_prover_num_public(self._h))

    def close(self):
        if self._h:
            lib().rlnamd_prover_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pack_inputs(self, witnesses):
        """witnesses: dicts with identity_secret, user_message_limit, message_id, path_elements,
        identity_path_index, x, external_nullifier (ints).  -> bytes (n * inputs_size * 32), the
        witness-graph inputs buffer of iden3calc.rs:122-181 (slot 0 = 1)."""
        out = bytearray(len(witnesses) * self.inputs_size * 32)
        names = {"identitySecret": "identity_secret", "userMessageLimit": "user_message_limit",
                 "messageId": "message_id", "pathElements": "path_elements",
                 "identityPathIndex": "identity_path_index", "x": "x", "externalNullifier": "external_nullifier",
                 "selectorUsed": "selector_used"}
        for i, w in enumerate(witnesses):
            base = i * self.inputs_size * 32
            out[base] = 1
            for sig, key in names.items():
                if sig not in self.slots:
                    continue
                off, ln = self.slots[sig]
                v = w[key]
                vals = list(v) if isinstance(v, (list, tuple)) else [v]
                if len(vals) != ln:
                    raise RLNError("invalid input length for %s: expected %d, got %d" % (sig, ln, len(vals)))
                for k, x in enumerate(vals):
                    out[base + (off + k) * 32: base + (off + k + 1) * 32] = _b(x)
        return bytes(out)

    def pack_named_inputs(self, named):
        """named: list of {graph signal name: [ints]} (any circuit): the populate_inputs of iden3calc.rs:122-146"""
        out = bytearray(len(named) * self.inputs_size * 32)
        for i, w in enumerate(named):
            base = i * self.inputs_size * 32
            out[base] = 1
            for sig, vals in w.items():
                if sig not in self.slots:
                    raise RLNError("MissingInput: " + sig)
                off, ln = self.slots[sig]
                if len(vals) != ln:
                    raise RLNError("invalid input length for %s: expected %d, got %d" % (sig, ln, len(vals)))
                for k, x in enumerate(vals):
                    out[base + (off + k) * 32: base + (off + k + 1) * 32] = _b(x)
        return bytes(out)

    def upload(self, inputs: bytes, rs):
        n = len(inputs) // (self.inputs_size * 32)
        rsb = b"".join(_b(r) + _b(s) for r, s in rs)
        assert len(rsb) == 64 * n
        check(lib().rlnamd_prover_upload(self._h, n, inputs, rsb))
        return n

    def run(self, n):
        check(lib().rlnamd_prover_run(self._h, n))

    def run_async(self, n):
        """enqueue only; consecutive batches pipeline on the device (see Prover::run_async)"""
        check(lib().rlnamd_prover_run_async(self._h, n))

    def sync(self):
        check(lib().rlnamd_prover_sync(self._h))

    def download(self, n):
        proofs = C.create_string_buffer(128 * n)
        coords = C.create_string_buffer(256 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * n)()
        check(lib().rlnamd_prover_download(self._h, n, proofs, coords, values, errs))
        out = []
        for i in range(n):
            c = coords.raw[256 * i:256 * (i + 1)]
            co = [int.from_bytes(c[32 * k:32 * k + 32], "little") for k in range(8)]
            v = values.raw[160 * i:160 * (i + 1)]
            vals = [int.from_bytes(v[32 * k:32 * k + 32], "little") for k in range(5)]
            out.append(dict(proof=proofs.raw[128 * i:128 * (i + 1)],
                            a=(co[0], co[1]), b=((co[2], co[3]), (co[4], co[5])), c=(co[6], co[7]),
                            values=dict(y=vals[0], root=vals[1], nullifier=vals[2], x=vals[3],
                                        external_nullifier=vals[4]),
                            public_inputs=vals, error=int(errs[i])))
        return out

    def prove(self, witnesses, rs):
        n = self.upload(self.pack_inputs(witnesses), rs)
        self.run(n)
        return self.download(n)

    # ---- streamed batches (rlnamd_prover_submit / _collect): fresh inputs per batch, no pipeline drain
    @staticmethod
    def pack_rs(rs):
        return b"".join(_b(r) + _b(s) for r, s in rs)

    def n_slots(self):
        """workspace slots = batches that can be in flight between submit and collect"""
        return int(lib().rlnamd_prover_slots(self._h))

    def submit(self, inputs: bytes, rsb: bytes, mode=0, partials=None):
        """inputs = pack_inputs(...), rsb = pack_rs(...); returns (ticket, n).  Enqueue only."""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n:
            raise RLNError("submit: inputs / rs sizes do not match")
        pp = None
        if partials is not None:
            pp = b"".join(partials)
            if len(pp) != 320 * n:
                raise RLNError("submit: one 320-byte partial proof per proof expected")
        t = C.c_uint64()
        check(lib().rlnamd_prover_submit(self._h, n, inputs, rsb, mode, pp, C.byref(t)))
        return int(t.value), n

    def submit_members(self, tree: "PoseidonTree", leaf_indices, inputs: bytes, rsb: bytes, mode=0):
        """submit() for members of `tree` named by leaf index: the pathElements / identityPathIndex slots of `inputs` are
        ignored, the paths are read from the tree on the device at its current root (rlnamd_prover_submit_members).
        mode 0 (full) or 1 (partial); returns (ticket, n)."""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n:
            raise RLNError("submit_members: leaf indices / inputs / rs sizes do not match")
        idx = (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices])
        t = C.c_uint64()
        check(lib().rlnamd_prover_submit_members(self._h, tree._h, n, idx, inputs, rsb, mode, C.byref(t)))
        return int(t.value), n

    def prove_members_raw(self, tree: "PoseidonTree", leaf_indices, inputs: bytes, rsb: bytes):
        """any n members through rlnamd_prover_prove_stream_members: chunks of `capacity`, all of them at one root"""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n:
            raise RLNError("prove_members: leaf indices / inputs / rs sizes do not match")
        idx = (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices])
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * max(n, 1))()
        check(lib().rlnamd_prover_prove_stream_members(self._h, tree._h, n, idx, inputs, rsb, proofs, values, errs))
        return proofs.raw, values.raw, list(errs)[:n]

    def pack_member_inputs(self, witnesses):
        """pack_inputs for witnesses without a path (submit_members fills it in): the two path inputs stay zero"""
        d = int(self.info.tree_depth)
        return self.pack_inputs([dict(w, path_elements=[0] * d, identity_path_index=[0] * d) for w in witnesses])

    def prove_members(self, tree: "PoseidonTree", leaf_indices, witnesses, rs):
        """witnesses: pack_inputs' dicts without path_elements / identity_path_index, one per leaf index"""
        return _unpack_results(*self.prove_members_raw(tree, leaf_indices, self.pack_member_inputs(witnesses),
                                                       self.pack_rs(rs)))

    def submit_members_drawn(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, inputs: bytes, rsb: bytes):
        """submit_members (full proofs) with the message ids drawn from `quota` on the device: the messageId slot of
        `inputs` is ignored, each row's own limit and external nullifier make its request, one draw covers the call
        (rlnamd_prover_submit_members_drawn).  Returns (ticket, n, statuses); a request that is not QuotaLedger.OK
        collects with a non-zero error and no proof."""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n:
            raise RLNError("submit_members_drawn: leaf indices / inputs / rs sizes do not match")
        idx = (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices])
        t = C.c_uint64()
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_prover_submit_members_drawn(self._h, tree._h, quota._h, n, idx, inputs, rsb, status, C.byref(t)))
        return int(t.value), n, list(status.raw[:n])

    def prove_members_drawn_raw(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, inputs: bytes, rsb: bytes):
        """any n members through rlnamd_prover_prove_stream_members_drawn: one draw for all n, chunks of `capacity`
        -> (proofs, values, errors, statuses)"""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n:
            raise RLNError("prove_members_drawn: leaf indices / inputs / rs sizes do not match")
        idx = (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices])
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * max(n, 1))()
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_prover_prove_stream_members_drawn(self._h, tree._h, quota._h, n, idx, inputs, rsb, status, proofs,
                                                             values, errs))
        return proofs.raw, values.raw, list(errs)[:n], list(status.raw[:n])

    def prove_members_drawn(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, witnesses, rs):
        """witnesses: dicts with identity_secret, user_message_limit, x and external_nullifier, one per leaf index; a
        message_id, if given, is ignored -> (results as prove_members gives them, statuses)"""
        ws = [dict(w, message_id=0) for w in witnesses]
        p, v, e, st = self.prove_members_drawn_raw(tree, quota, leaf_indices, self.pack_member_inputs(ws), self.pack_rs(rs))
        return _unpack_results(p, v, e), st

    # ---- blocks of ids for the multi-message-id circuit (rlnamd_prover_*_members_drawn_counts)
    def _drawn_counts_args(self, what, leaf_indices, inputs, rsb, counts):
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n or len(counts) != n:
            raise RLNError("%s: leaf indices / inputs / rs / counts sizes do not match" % what)
        for i, c in enumerate(counts):      # what a byte cannot carry to the library's own check, in the library's words
            if not 0 <= int(c) <= 255:
                raise RLNError("quota ledger: request %d of draw_counts asks for %d ids, more than 255" % (i, int(c)))
        return n, (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices]), bytes(int(c) for c in counts) or b"\0"

    def submit_members_drawn_counts(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, inputs: bytes, rsb: bytes,
                                    counts):
        """submit_members_drawn for a proof that uses counts[i] = 1 .. max_out message slots: one QuotaLedger.draw_counts
        covers the call, a granted row gets the ids first .. first + counts[i] - 1 in its first counts[i] message slots
        with their selectors set, the messageId and selectorUsed slots of `inputs` are ignored
        (rlnamd_prover_submit_members_drawn_counts).  Returns (ticket, n, statuses); read the public values with
        collect_public before collect_raw."""
        n, idx, cb = self._drawn_counts_args("submit_members_drawn_counts", leaf_indices, inputs, rsb, counts)
        t = C.c_uint64()
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_prover_submit_members_drawn_counts(self._h, tree._h, quota._h, n, idx, inputs, rsb, cb, status, C.byref(t)))
        return int(t.value), n, list(status.raw[:n])

    def prove_members_drawn_counts_raw(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, inputs: bytes, rsb: bytes,
                                       counts):
        """any n members through rlnamd_prover_prove_stream_members_drawn_counts: one draw for all n, chunks of `capacity`
        -> (proofs, public values n * num_public * 32 bytes, errors, statuses)"""
        n, idx, cb = self._drawn_counts_args("prove_members_drawn_counts", leaf_indices, inputs, rsb, counts)
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(max(32 * self.num_public * n, 1))
        errs = (C.c_uint32 * max(n, 1))()
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_prover_prove_stream_members_drawn_counts(self._h, tree._h, quota._h, n, idx, inputs, rsb, cb, status,
                                                                    proofs, values, errs))
        return proofs.raw, values.raw[:32 * self.num_public * n], list(errs)[:n], list(status.raw[:n])

    def pack_member_inputs_multi(self, witnesses):
        """pack_member_inputs for witnesses without message ids and selectors either (the drawn calls fill them in)"""
        k = self.slots["messageId"][1]
        extra = dict(message_id=[0] * k)
        if "selectorUsed" in self.slots:
            extra["selector_used"] = [0] * k
        return self.pack_member_inputs([dict(w, **extra) for w in witnesses])

    def prove_members_drawn_counts(self, tree: "PoseidonTree", quota: "QuotaLedger", leaf_indices, witnesses, rs, counts):
        """witnesses: dicts with identity_secret, user_message_limit, x and external_nullifier, one per leaf index; message
        ids and selectors, if given, are ignored -> ([dict(proof, public_inputs: num_public ints, error)], statuses)"""
        p, v, e, st = self.prove_members_drawn_counts_raw(tree, quota, leaf_indices, self.pack_member_inputs_multi(witnesses),
                                                          self.pack_rs(rs), counts)
        row = 32 * self.num_public
        return [dict(proof=p[128 * i:128 * i + 128], error=e[i],
                     public_inputs=[int.from_bytes(v[row * i + 32 * j:row * i + 32 * j + 32], "little") for j in range(self.num_public)])
                for i in range(len(e))], st

    def prove_members_public_raw(self, tree: "PoseidonTree", leaf_indices, inputs: bytes, rsb: bytes):
        """prove_members_raw with every public signal of a proof (num_public * 32 bytes a row) in the place of the 160
        bytes of the single message-id circuit (rlnamd_prover_prove_stream_members_public)"""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(leaf_indices) != n:
            raise RLNError("prove_members: leaf indices / inputs / rs sizes do not match")
        idx = (C.c_uint64 * max(n, 1))(*[int(i) for i in leaf_indices])
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(max(32 * self.num_public * n, 1))
        errs = (C.c_uint32 * max(n, 1))()
        check(lib().rlnamd_prover_prove_stream_members_public(self._h, tree._h, n, idx, inputs, rsb, proofs, values, errs))
        return proofs.raw, values.raw[:32 * self.num_public * n], list(errs)[:n]

    def collect_public(self, ticket, n):
        """every public signal of a finished batch, n * num_public * 32 bytes; call it BEFORE collect_raw, which ends the
        batch (rlnamd_prover_collect_public)"""
        buf = C.create_string_buffer(max(32 * self.num_public * n, 1))
        check(lib().rlnamd_prover_collect_public(self._h, ticket, n, buf))
        return buf.raw[:32 * self.num_public * n]

    def hints_for(self, inputs: bytes):
        """the hints of the proofs packed in `inputs`, one proof at a time on this thread (rlnamd_prover_hints_for): a list
        of ctypes arrays, or None when the circuit has no segments form"""
        hw = int(lib().rlnamd_prover_hint_words(self._h))
        if not hw:
            return None
        isz = self.inputs_size * 32
        out = []
        for i in range(len(inputs) // isz):
            h = (C.c_uint32 * hw)()
            check(lib().rlnamd_prover_hints_for(self._h, inputs[i * isz:(i + 1) * isz], h))
            out.append(h)
        return out

    def submit_hinted(self, inputs: bytes, rsb: bytes, hints):
        """submit() for full proofs whose hints (hints_for) are at hand: nothing is hashed inside the call"""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(hints) != n:
            raise RLNError("submit_hinted: inputs / rs / hints sizes do not match")
        hw = len(hints[0])
        flat = (C.c_uint32 * (hw * n))()
        for i, h in enumerate(hints):
            flat[i * hw:(i + 1) * hw] = h[:]
        t = C.c_uint64()
        check(lib().rlnamd_prover_submit_hinted(self._h, n, inputs, rsb, flat, C.byref(t)))
        return int(t.value), n

    def describe(self):
        """the switches this prover was built with (ProverTuning)"""
        buf = C.create_string_buffer(1024)
        check(lib().rlnamd_prover_describe(self._h, buf, 1024))
        return buf.value.decode()

    def wipe(self):
        """overwrite the resident inputs and the last run's witness values (the streamed calls do it by themselves)"""
        check(lib().rlnamd_prover_wipe(self._h))

    def collect_raw(self, ticket, n):
        """waits for that batch only -> (proofs bytes n*128, values bytes n*160, errors list)"""
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * n)()
        check(lib().rlnamd_prover_collect(self._h, ticket, n, proofs, None, values, errs, None))
        return proofs.raw, values.raw, list(errs)

    def collect(self, ticket, n):
        proofs, values, errs = self.collect_raw(ticket, n)
        return _unpack_results(proofs, values, errs)

    def collect_partial(self, ticket, n):
        buf = C.create_string_buffer(320 * n)
        check(lib().rlnamd_prover_collect(self._h, ticket, n, None, None, None, None, buf))
        return [buf.raw[320 * i:320 * (i + 1)] for i in range(n)]

    def collect_partial_cached(self, ticket, n):
        """collect of a mode-1 batch that keeps the known stored values on the device -> ([partial320], [handle], errors);
        handle 0 = not cached (such a proof finishes through the full interpreter)"""
        buf = C.create_string_buffer(320 * n)
        hs = (C.c_uint64 * n)()
        errs = (C.c_uint32 * n)()
        check(lib().rlnamd_prover_collect_partial_cached(self._h, ticket, n, buf, hs, errs))
        return [buf.raw[320 * i:320 * (i + 1)] for i in range(n)], [int(h) for h in hs], list(errs)

    def submit_finish(self, inputs: bytes, rsb: bytes, partials, handles):
        """finish_zk_proof_with_rs with the partial runs' cache handles: the cone of the witness graph only when every
        handle is live (rlnamd_prover_submit_finish); returns (ticket, n)"""
        n = len(inputs) // (self.inputs_size * 32)
        pp = b"".join(partials)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n or len(pp) != 320 * n or len(handles) != n:
            raise RLNError("submit_finish: sizes do not match")
        hs = (C.c_uint64 * n)(*handles)
        t = C.c_uint64()
        check(lib().rlnamd_prover_submit_finish(self._h, n, inputs, rsb, pp, hs, C.byref(t)))
        return int(t.value), n

    def release_partial(self, handles):
        hs = (C.c_uint64 * len(handles))(*handles)
        check(lib().rlnamd_prover_release_partial(self._h, hs, len(handles)))

    def hint_stats(self):
        """the witness graph as segments behind hints (rlnamd_prover_hint_stats)"""
        out = (C.c_uint64 * 7)()
        check(lib().rlnamd_prover_hint_stats(self._h, out))
        return dict(zip(("segments", "hints", "longest_segment_steps", "full_steps", "hinted_batches", "fallbacks", "chains_remembered"),
                        [int(v) for v in out]))

    def device_shared(self):
        """bit 0: another prover of this process on the device; bit 1: a prover of another process"""
        who = C.c_int()
        check(lib().rlnamd_prover_device_shared(self._h, C.byref(who)))
        return int(who.value)

    def partial_cache_info(self):
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_prover_partial_cache_info(self._h, out))
        return dict(zip(("capacity", "in_use", "entry_bytes", "residue_in_free_entries", "cone_batches", "cone_nodes",
                         "cone_steps", "full_steps"), [int(v) for v in out]))

    def prove_stream_raw(self, inputs: bytes, rsb: bytes):
        """any n through rlnamd_prover_prove_stream (chunks of `capacity`, all slots in flight)"""
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n:
            raise RLNError("prove_stream: inputs / rs sizes do not match")
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * max(n, 1))()
        check(lib().rlnamd_prover_prove_stream(self._h, n, inputs, rsb, proofs, values, errs))
        return proofs.raw, values.raw, list(errs)[:n]

    def prove_stream(self, witnesses, rs):
        return _unpack_results(*self.prove_stream_raw(self.pack_inputs(witnesses), self.pack_rs(rs)))

    # ---- partial proofs (protocol/proof.rs:783-849)
    def known_mask(self):
        buf = C.create_string_buffer(int(self.info.num_signals))
        check(lib().rlnamd_prover_known_mask(self._h, buf))
        return list(buf.raw)

    def prove_partial(self, partial_witnesses):
        """partial_witnesses: dicts with identity_secret, user_message_limit, path_elements,
        identity_path_index.  -> list of 320-byte partial proofs (pi_a | rho | pi_b | pi_c, affine LE)."""
        full = [dict(w, message_id=0, x=0, external_nullifier=0) for w in partial_witnesses]
        n = self.upload(self.pack_inputs(full), [(0, 0)] * len(full))
        check(lib().rlnamd_prover_run_mode(self._h, n, 1))
        buf = C.create_string_buffer(320 * n)
        check(lib().rlnamd_prover_download_partial(self._h, n, buf))
        return [buf.raw[320 * i:320 * (i + 1)] for i in range(n)]

    def upload_partial(self, partials):
        check(lib().rlnamd_prover_upload_partial(self._h, len(partials), b"".join(partials)))

    def prove_with_witness(self, witnesses, rs, calculated):
        """generate_zk_proof_with_witness for a batch: `calculated` = per proof the full witness (ints below 2^256, taken
        mod r; or all of them as bytes, 32 little-endian bytes per value).  The witness need not satisfy the circuit: w_0
        enters the quotient as given, the constant row (query[0], alpha, beta) is added whatever it is.  `witnesses`: the
        inputs (pack_inputs' dicts, or packed bytes) -- the proof values of a single-message circuit come from them."""
        n = self.upload(witnesses if isinstance(witnesses, (bytes, bytearray)) else self.pack_inputs(witnesses), rs)
        blob = bytes(calculated) if isinstance(calculated, (bytes, bytearray)) else \
            b"".join(int(v).to_bytes(32, "little") for w in calculated for v in w)
        if len(blob) != n * int(self.info.num_signals) * 32:
            raise RLNError("prove_with_witness: one full witness per proof expected")
        check(lib().rlnamd_prover_upload_witness(self._h, n, blob))
        check(lib().rlnamd_prover_run_mode(self._h, n, 0))
        return self.download(n)

    def finish(self, witnesses, rs, partials):
        """finish_zk_proof_with_rs for a batch: only the message-dependent rows + h + blinding are walked"""
        n = self.upload(self.pack_inputs(witnesses), rs)
        self.upload_partial(partials)
        check(lib().rlnamd_prover_run_mode(self._h, n, 2))
        return self.download(n)

    def run_async_mode(self, n, mode):
        check(lib().rlnamd_prover_run_async_mode(self._h, n, mode))

    def download_public(self, n):
        """public signals w[1..] of the first n proofs of the last run, from the witness (circuit-generic)"""
        buf = C.create_string_buffer(32 * self.num_public * n)
        check(lib().rlnamd_prover_download_public(self._h, n, buf))
        k = self.num_public
        return [[int.from_bytes(buf.raw[32 * (i * k + j):32 * (i * k + j + 1)], "little") for j in range(k)]
                for i in range(n)]

    def verify_public(self, proof: bytes, public_inputs):
        ok = C.c_int()
        check(lib().rlnamd_verify_public(self._h, proof, b"".join(_b(v) for v in public_inputs), len(public_inputs),
                                         C.byref(ok)))
        return bool(ok.value)

    def stage_ms(self):
        ms = (C.c_float * STAGES)()
        check(lib().rlnamd_prover_stage_ms(self._h, ms))
        return {lib().rlnamd_prover_stage_name(i).decode(): float(ms[i]) for i in range(STAGES)}

    def walk_clock_mhz(self):
        """mean shader clock under the G1 / G2 table walks since the previous call (drains the pipeline)"""
        mhz = (C.c_double * 2)()
        check(lib().rlnamd_prover_walk_clock_mhz(self._h, mhz))
        return {"g1_walk": float(mhz[0]), "g2_walk": float(mhz[1])}

    def fetch_witness(self, index):
        n = int(self.info.num_signals)
        buf = C.create_string_buffer(32 * n)
        check(lib().rlnamd_prover_fetch_witness(self._h, index, buf))
        return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def fetch_h(self, index):
        n = int(self.info.domain_size)
        buf = C.create_string_buffer(32 * n)
        check(lib().rlnamd_prover_fetch_h(self._h, index, buf))
        return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def init_ms(self):
        """where the constructor's time went (rlnamd_prover_init_ms)"""
        ms = (C.c_float * 4)()
        check(lib().rlnamd_prover_init_ms(self._h, ms))
        return dict(zip(("parse", "table_alloc", "table_build", "rest"), (round(float(v), 1) for v in ms)))

    def residue(self):
        """tap of the wipes (rlnamd_prover_residue): non-zero 16-byte words left in the last batch's slot"""
        out = (C.c_uint64 * 6)()
        check(lib().rlnamd_prover_residue(self._h, out))
        return dict(zip(("digits_g1", "digits_g2", "abc", "partial_g1", "partial_g2", "inputs"), (int(v) for v in out)))

    RESIDUE_SLOT = ("digits_g1", "digits_g2", "abc", "partial_g1", "partial_g2", "inputs", "staging", "hints", "v29",
                    "reserved")

    def residue_slot(self, k):
        """the same tap for workspace slot k (rlnamd_prover_residue_slot), with the pinned staging buffer, the pinned
        hints and the interpreter's stored values; an error for k >= n_slots()"""
        out = (C.c_uint64 * len(self.RESIDUE_SLOT))()
        check(lib().rlnamd_prover_residue_slot(self._h, k, out))
        return dict(zip(self.RESIDUE_SLOT, (int(v) for v in out)))

    def verify_many(self, proofs, public_inputs, threads=0):
        """n independent verifications on host threads (rlnamd_verify_many); returns a list of bools"""
        n = len(proofs)
        if n == 0:
            return []
        nv = _check_verify_shapes(proofs, public_inputs)
        ok = C.create_string_buffer(n)
        check(lib().rlnamd_verify_many(self._h, n, b"".join(proofs), b"".join(_b(v) for pi in public_inputs for v in pi),
                                       nv, threads, ok))
        return [bool(x) for x in ok.raw]

    def verify_many_gpu(self, proofs, public_inputs, lanes=0):
        """n independent verifications on the device (rlnamd_verify_many_gpu_ex): the verdicts of verify_many; returns
        a list of bools.  lanes: 1 a lane per proof, 8 a team of 8 lanes per proof, 0 the verifier chooses by n"""
        n = len(proofs)
        if n == 0:
            return []
        nv = _check_verify_shapes(proofs, public_inputs)
        ok = C.create_string_buffer(n)
        check(lib().rlnamd_verify_many_gpu_ex(self._h, n, b"".join(proofs),
                                              b"".join(_b(v) for pi in public_inputs for v in pi), nv, lanes, ok, None))
        return [bool(x) for x in ok.raw]

    def verify_many_gpu_gt(self, proofs, public_inputs, lanes=0):
        """the final-exponentiated pairing product of each proof as computed on the device
        (rlnamd_verify_many_gpu_ex): a list of 384-byte strings, 12 canonical LE field elements in pairing.h's
        coefficient order; the encoding of 1 for an accepted proof, all zero for one rejected before the pairing"""
        n = len(proofs)
        if n == 0:
            return []
        nv = _check_verify_shapes(proofs, public_inputs)
        gt = C.create_string_buffer(384 * n)
        check(lib().rlnamd_verify_many_gpu_ex(self._h, n, b"".join(proofs),
                                              b"".join(_b(v) for pi in public_inputs for v in pi), nv, lanes, None, gt))
        return [gt.raw[384 * i:384 * (i + 1)] for i in range(n)]

    def verify_gpu_passes(self):
        """(chunks the device verifier has run with a lane per proof, chunks in team form) so far"""
        out = (C.c_size_t * 2)()
        check(lib().rlnamd_verify_gpu_passes(self._h, out))
        return int(out[0]), int(out[1])

    def verify_many_gpu_optimistic(self, proofs, public_inputs, scalars=None, lanes=None):
        """verify_many_gpu with one combined pairing check per chunk first and the exact pass only for a chunk it
        rejects (rlnamd_verify_many_gpu_optimistic): the same verdicts, up to about 2^-128 per chunk.  scalars: None
        (drawn inside the call) or n non-zero ints below 2^128, a test hook.  lanes: None (calls that take teams are
        verify_many_gpu unchanged), or 0 / 1 / 8 (rlnamd_verify_many_gpu_optimistic_ex: the shape as in
        verify_many_gpu, and a call that takes teams is checked combined in team form)"""
        n = len(proofs)
        if n == 0:
            return []
        nv = _check_verify_shapes(proofs, public_inputs)
        ok = C.create_string_buffer(n)
        sc = None if scalars is None else b"".join(int(r).to_bytes(16, "little") for r in scalars)
        vals = b"".join(_b(v) for pi in public_inputs for v in pi)
        if lanes is None:
            check(lib().rlnamd_verify_many_gpu_optimistic(self._h, n, b"".join(proofs), vals, nv, sc, ok))
        else:
            check(lib().rlnamd_verify_many_gpu_optimistic_ex(self._h, n, b"".join(proofs), vals, nv, sc, int(lanes), ok))
        return [bool(x) for x in ok.raw]

    def verify_aggregate(self, proofs, public_inputs, scalars=None, lanes=1):
        """test / diagnosis (rlnamd_verify_gpu_aggregate_ex): (the final-exponentiated combined value of all n proofs as
        384 bytes in pairing.h's coefficient order, the encoding of 1 = accept; a list of bools, True where the
        per-proof checks refuse a proof).  No fallback.  lanes: 1 a lane per proof, 8 a team of 8 lanes per proof"""
        n = len(proofs)
        nv = _check_verify_shapes(proofs, public_inputs) if n else self.num_public
        gt, rej = C.create_string_buffer(384), C.create_string_buffer(max(n, 1))
        sc = None if scalars is None else b"".join(int(r).to_bytes(16, "little") for r in scalars)
        check(lib().rlnamd_verify_gpu_aggregate_ex(self._h, n, b"".join(proofs),
                                                   b"".join(_b(v) for pi in public_inputs for v in pi), nv, sc,
                                                   int(lanes), gt, rej))
        return gt.raw, [bool(x) for x in rej.raw[:n]]

    verify_gpu_aggregate = verify_aggregate

    def verify_aggregate_seeded(self, proofs, public_inputs, seed: bytes, lanes=1):
        """test / diagnosis (rlnamd_verify_gpu_aggregate_seeded): verify_aggregate with the scalars of chunk c derived on
        the device from (seed, c), seed = 32 bytes; equals verify_aggregate over agg_scalars(seed, c, ...) per chunk"""
        n = len(proofs)
        if len(seed) != 32:
            raise RLNError("verify_aggregate_seeded: the seed is 32 bytes")
        nv = _check_verify_shapes(proofs, public_inputs) if n else self.num_public
        gt, rej = C.create_string_buffer(384), C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_verify_gpu_aggregate_seeded(self._h, n, b"".join(proofs),
                                                       b"".join(_b(v) for pi in public_inputs for v in pi), nv, seed,
                                                       int(lanes), gt, rej))
        return gt.raw, [bool(x) for x in rej.raw[:n]]

    def verify_optimistic_stats(self):
        """rlnamd_verify_gpu_optimistic_stats as a dict"""
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_verify_gpu_optimistic_stats(self._h, out))
        keys = ("combined", "accepted", "fell_back", "skipped_in_cooldown", "refused_proofs", "cooldown_left", "cooldown",
                "combined_team")
        return dict(zip(keys, (int(v) for v in out)))

    def verify_set_cooldown(self, chunks):
        check(lib().rlnamd_verify_gpu_set_cooldown(self._h, chunks))

    def verify(self, proof: bytes, public_inputs):
        """verify_zk_proof (protocol/proof.rs:856-894); public_inputs = [y, root, nullifier, x, ext]."""
        ok = C.c_int()
        check(lib().rlnamd_verify(self._h, proof, b"".join(_b(v) for v in public_inputs), C.byref(ok)))
        return bool(ok.value)


def agg_scalars(seed: bytes, chunk: int, n: int):
    """the n scalars a combined check derives for chunk `chunk` from a 32-byte seed (rlnamd_verify_agg_scalars, host
    only; include/rln_amd.h states the layout) -> a list of n ints in [1, 2^128)"""
    if len(seed) != 32:
        raise RLNError("agg_scalars: the seed is 32 bytes")
    out = C.create_string_buffer(max(16 * n, 1))
    check(lib().rlnamd_verify_agg_scalars(seed, chunk, n, out))
    return [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(n)]


def verify_many_with_zkey(zkey: bytes, proofs, public_inputs, threads=0):
    """n independent Groth16 verifications on host threads, straight from arkzkey bytes (no GPU): proofs = list of
    128-byte compressed proofs, public_inputs = list of equally long lists of ints.  Returns a list of bools."""
    n = len(proofs)
    if n == 0:
        return []
    nv = _check_verify_shapes(proofs, public_inputs)
    ok = C.create_string_buffer(n)
    check(lib().rlnamd_verify_many_with_zkey(zkey, len(zkey), n, b"".join(proofs),
                                             b"".join(_b(v) for pi in public_inputs for v in pi), nv, threads, ok))
    return [bool(x) for x in ok.raw]


class ProverPool:
    """rlnamd_pool: one prover replica + one host thread per device of this process; a job of n proofs is cut into
    contiguous index shards (BASELINE config 4: 8 x 8 192) and every replica streams its shard."""

    def __init__(self, devices=None, zkey: bytes = None, graph: bytes = None, max_batch=1024, window_bits=0, depth=20,
                 multi=False):
        if zkey is None or graph is None:
            zp, gp = resource_paths(depth, multi)
            zkey, graph = open(zp, "rb").read(), open(gp, "rb").read()
        self._h = C.c_void_p()
        devs = list(devices) if devices else []
        arr = (C.c_int * max(len(devs), 1))(*devs)
        check(lib().rlnamd_pool_new(zkey, len(zkey), graph, len(graph), max_batch, window_bits, arr if devs else None,
                                    len(devs), C.byref(self._h)))
        self.info = ProverInfo()
        check(lib().rlnamd_pool_get_info(self._h, C.byref(self.info)))
        self.inputs_size = int(self.info.inputs_size)
        self.size = int(lib().rlnamd_pool_size(self._h))
        self.devices = [int(lib().rlnamd_pool_device(self._h, i)) for i in range(self.size)]

    def close(self):
        if self._h:
            lib().rlnamd_pool_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prove_raw(self, inputs: bytes, rsb: bytes):
        n = len(inputs) // (self.inputs_size * 32)
        if len(inputs) != n * self.inputs_size * 32 or len(rsb) != 64 * n:
            raise RLNError("pool: inputs / rs sizes do not match")
        proofs = C.create_string_buffer(128 * n)
        values = C.create_string_buffer(160 * n)
        errs = (C.c_uint32 * max(n, 1))()
        check(lib().rlnamd_pool_prove(self._h, n, inputs, rsb, proofs, values, errs))
        return proofs.raw, values.raw, list(errs)[:n]

    def last_ms(self):
        ms = (C.c_float * self.size)()
        check(lib().rlnamd_pool_last_ms(self._h, ms))
        return [float(x) for x in ms]

    def set_dynamic(self, on=True):
        """chunk-granular dynamic assignment (a cursor shared by the replicas) instead of contiguous shards"""
        check(lib().rlnamd_pool_set_dynamic(self._h, 1 if on else 0))

    def last_proofs(self):
        k = (C.c_size_t * self.size)()
        check(lib().rlnamd_pool_last_proofs(self._h, k))
        return [int(x) for x in k]

    def inject_fault(self, replica, after_chunks=0):
        check(lib().rlnamd_pool_inject_fault(self._h, replica, after_chunks))

    def set_failover(self, rounds=1):
        """rounds > 0: the chunks of a failing replica are proved again by the others (the replica is quarantined until
        revive()); 0: a failing replica fails the job"""
        check(lib().rlnamd_pool_set_failover(self._h, rounds))

    def health(self):
        """[(quarantined, failed dispatches)] per replica"""
        q = (C.c_int * self.size)()
        f = (C.c_size_t * self.size)()
        check(lib().rlnamd_pool_health(self._h, q, f))
        return [(bool(a), int(b)) for a, b in zip(q, f)]

    def revive(self, replica):
        check(lib().rlnamd_pool_revive(self._h, replica))

    def set_probation(self, jobs):
        """jobs > 0: a quarantined replica sits out that many jobs and is then handed work again by itself"""
        check(lib().rlnamd_pool_set_probation(self._h, jobs))

    def verify_many(self, proofs, public_inputs, threads=0):
        n = len(proofs)
        if n == 0:
            return []
        nv = _check_verify_shapes(proofs, public_inputs)
        ok = C.create_string_buffer(n)
        check(lib().rlnamd_pool_verify_many(self._h, n, b"".join(proofs),
                                            b"".join(_b(v) for pi in public_inputs for v in pi), nv, threads, ok))
        return [bool(x) for x in ok.raw]


class Comm:
    """rlnamd_comm: an RCCL communicator created through the C ABI (no torch type crosses it)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().rlnamd_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def init_rank(cls, uid: bytes, nranks: int, rank: int):
        h = C.c_void_p()
        check(lib().rlnamd_comm_init_rank(uid, nranks, rank, C.byref(h)))
        return cls(h)

    def ranks(self):
        return int(lib().rlnamd_comm_ranks(self._h))

    def close(self):
        if self._h:
            lib().rlnamd_comm_free(self._h)
            self._h = C.c_void_p()


class PoseidonTree:
    """HBM-resident FullMerkleTree (/root/reference/utils/src/merkle_tree/full_merkle_tree.rs)."""

    def __init__(self, depth):
        self._h = C.c_void_p()
        self.depth = depth
        check(lib().rlnamd_tree_new(depth, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rlnamd_tree_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_range(self, start, leaves):
        buf = b"".join(_b(v) for v in leaves)
        check(lib().rlnamd_tree_set_range(self._h, start, buf, len(leaves)))

    def set(self, index, leaf):
        self.set_range(index, [leaf])

    def set_leaves(self, updates):
        """[(index, leaf)] in any order, later entries win: ONE bottom-up pass over the union of the dirty paths"""
        k = len(updates)
        idx = (C.c_uint64 * max(k, 1))(*[int(i) for i, _ in updates])
        check(lib().rlnamd_tree_set_leaves(self._h, idx, b"".join(_b(v) for _, v in updates), k))

    def root(self):
        out = C.create_string_buffer(32)
        check(lib().rlnamd_tree_root(self._h, out))
        return int.from_bytes(out.raw, "little")

    def get(self, index):
        out = C.create_string_buffer(32)
        check(lib().rlnamd_tree_get_leaf(self._h, index, out))
        return int.from_bytes(out.raw, "little")

    def proof(self, index):
        e = C.create_string_buffer(32 * self.depth)
        b = C.create_string_buffer(max(self.depth, 1))
        check(lib().rlnamd_tree_proof(self._h, index, e, b))
        return ([int.from_bytes(e.raw[32 * i:32 * i + 32], "little") for i in range(self.depth)],
                list(b.raw[:self.depth]))

    def proofs_raw(self, first, count):
        """the paths of leaves [first, first + count) in one call -> (elems count*depth*32 bytes, bits count*depth)"""
        e = C.create_string_buffer(max(32 * self.depth * count, 1))
        b = C.create_string_buffer(max(self.depth * count, 1))
        check(lib().rlnamd_tree_proofs(self._h, first, count, e, b))
        return e.raw[:32 * self.depth * count], b.raw[:self.depth * count]

    def proofs(self, first, count):
        e = C.create_string_buffer(32 * self.depth * count)
        b = C.create_string_buffer(max(self.depth * count, 1))
        check(lib().rlnamd_tree_proofs(self._h, first, count, e, b))
        out = []
        for p in range(count):
            o = p * self.depth
            out.append(([int.from_bytes(e.raw[32 * (o + i):32 * (o + i + 1)], "little") for i in range(self.depth)],
                        list(b.raw[o:o + self.depth])))
        return out

    def proofs_at_raw(self, indices):
        """the paths of the listed leaves (any order, repeats allowed) in one call -> (elems k*depth*32 bytes, bits k*depth)"""
        k = len(indices)
        idx = (C.c_uint64 * max(k, 1))(*[int(i) for i in indices])
        e = C.create_string_buffer(max(32 * self.depth * k, 1))
        b = C.create_string_buffer(max(self.depth * k, 1))
        check(lib().rlnamd_tree_proofs_at(self._h, idx, k, e, b))
        return e.raw[:32 * self.depth * k], b.raw[:self.depth * k]

    def proofs_at(self, indices):
        e, b = self.proofs_at_raw(indices)
        out = []
        for p in range(len(indices)):
            o = p * self.depth
            out.append(([int.from_bytes(e[32 * (o + i):32 * (o + i + 1)], "little") for i in range(self.depth)],
                        list(b[o:o + self.depth])))
        return out

    def fill_sequential(self, start, n, first_value):
        check(lib().rlnamd_tree_fill_sequential(self._h, start, n, first_value))

    def bench(self, n_leaves, first_value=1, verify=True):
        ms = (C.c_float * 2)()
        bad = C.c_size_t()
        check(lib().rlnamd_tree_bench(self._h, n_leaves, first_value, 1 if verify else 0, ms, C.byref(bad)))
        return dict(build_ms=float(ms[0]), proofs_ms=float(ms[1]), bad=int(bad.value))


class NullifierLog:
    """Device-resident log of the rate-limiting shares of the epochs in a relay's window (rlnamd_nullifier_log_*): for
    each observed share, whether its nullifier is new, a repeat of the same message or a second message of one member --
    and then that member's identity secret (compute_id_secret, rln/src/protocol/slashing.rs:12-36).

    One log serves the whole window: nullifiers of different epochs do not collide, shares of two or three epochs may
    arrive interleaved, and retire() drops the records of the epochs that have left the window -- the log is then what
    it would have been had those shares never been observed, and their room is free again.  `capacity` counts records
    held.  A record is named by its sequence number, its arrival index since the last clear(); that is also a share's
    tag when observe gets no tags, it survives a retire unchanged and is never issued twice.  clear() drops everything.
    From its first retire on a log holds a spare set of record arrays, so its record memory doubles; a log that never
    retires pays nothing."""
    NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED = range(5)

    def __init__(self, capacity, seed=0):
        self._h = C.c_void_p()
        check(lib().rlnamd_nullifier_log_new(capacity, seed, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rlnamd_nullifier_log_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def observe_raw(self, shares: bytes, tags=None):
        """n packed shares (128 bytes each: nullifier | x | y | external_nullifier, canonical LE) ->
        (status n bytes, secrets n * 32 bytes, first tags: list of n ints)"""
        n = len(shares) // 128
        if len(shares) != 128 * n or (tags is not None and len(tags) != n):
            raise RLNError("NullifierLog.observe: %d bytes of shares and %s tags" % (len(shares), "no" if tags is None else len(tags)))
        tg = None if tags is None else (C.c_uint64 * max(n, 1))(*[int(t) for t in tags])
        status = C.create_string_buffer(max(n, 1))
        secrets = C.create_string_buffer(max(32 * n, 1))
        first = (C.c_uint64 * max(n, 1))()
        check(lib().rlnamd_nullifier_log_observe(self._h, n, shares, tg, status, secrets, first))
        return status.raw[:n], secrets.raw[:32 * n], list(first[:n])

    def observe(self, shares, tags=None):
        """shares: [(nullifier, x, y, external_nullifier)] as ints -> (status, secrets, first_tag), three lists of ints"""
        status, secrets, first = self.observe_raw(b"".join(_b(v) for s in shares for v in s), tags)
        return (list(status), [int.from_bytes(secrets[32 * i:32 * i + 32], "little") for i in range(len(status))], first)

    def clear(self):
        """everything goes: the table empty, no records, sequence numbers from 0 again, the same seed"""
        check(lib().rlnamd_nullifier_log_clear(self._h))

    def retire(self, external_nullifiers):
        """0 .. 64 external nullifiers (ints): every record under one of them is removed -> how many"""
        k = len(external_nullifiers)
        removed = C.c_uint64()
        check(lib().rlnamd_nullifier_log_retire(self._h, b"".join(_b(e) for e in external_nullifiers), k, C.byref(removed)))
        return int(removed.value)

    def retain(self, external_nullifiers):
        """1 .. 64 external nullifiers (ints): every record under NONE of them is removed, however many others there
        are -> how many.  Everything else as retire(); an empty list is refused (that is clear())."""
        k = len(external_nullifiers)
        removed = C.c_uint64()
        check(lib().rlnamd_nullifier_log_retain(self._h, b"".join(_b(e) for e in external_nullifiers), k, C.byref(removed)))
        return int(removed.value)

    def retire_info(self):
        """[retire and retain calls, records removed so far, next default tag, records held, longest probe walk of the last
        rebuild, 1 once the spare record arrays exist, 0, 0]"""
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_nullifier_log_retire_info(self._h, out))
        return [int(v) for v in out]

    def get(self, seq):
        """the record with sequence number `seq` -> ((nullifier, x, y, external_nullifier), tag); an error that says so
        if it was retired"""
        out = C.create_string_buffer(128)
        tag = C.c_uint64()
        check(lib().rlnamd_nullifier_log_get(self._h, seq, out, C.byref(tag)))
        return tuple(int.from_bytes(out.raw[32 * k:32 * k + 32], "little") for k in range(4)), int(tag.value)

    def home_slot(self, nullifier):
        slot = C.c_uint64()
        check(lib().rlnamd_nullifier_log_home_slot(self._h, _b(nullifier), C.byref(slot)))
        return int(slot.value)

    def info(self):
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_nullifier_log_info(self._h, out))
        return [int(v) for v in out]


class MemberDirectory:
    """Device-resident member directory beside a PoseidonTree (rlnamd_directory_*): who sits at which leaf.  register()
    takes (index, identity commitment, limit) events and writes the rate commitments Poseidon(idc, limit) into the tree
    on the device; resolve() turns recovered identity secrets into leaf indices and limits; slash() removes them.  The
    contract is the header comment of include/rln_amd.h (zerokit_amd/csrc/member_directory.h is its sequential text).

    The directory borrows `tree`, which must outlive it, and writes only the leaves of indices it registers or removes.
    It is not persisted: after a restart, registering the same events again rebuilds it and leaves the root where it
    was.  In one register call with duplicate commitments the lowest index wins; across calls the first call wins."""
    OK, OCCUPIED, KNOWN = range(3)
    FOUND, UNKNOWN, SKIPPED = range(3)
    REMOVED, VACANT = range(2)
    NO_INDEX = (1 << 64) - 1

    def __init__(self, tree: "PoseidonTree", capacity=None, seed=0):
        self._h = C.c_void_p()
        self.tree = tree               # (kept alive: the directory borrows it)
        if capacity is None:
            capacity = min(1 << tree.depth, 1 << 31)
        check(lib().rlnamd_directory_new(tree._h, capacity, seed, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rlnamd_directory_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _w(x):
        """32 bytes LE of any 256-bit value: whether it is a field element is the library's check, with its own text"""
        return int(x).to_bytes(32, "little")

    def register(self, members):
        """[(index, identity commitment, limit)] -> [status]"""
        n = len(members)
        idx = (C.c_uint64 * max(n, 1))(*[int(m[0]) for m in members])
        lim = (C.c_uint32 * max(n, 1))(*[int(m[2]) for m in members])
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_directory_register(self._h, n, idx, b"".join(self._w(m[1]) for m in members) or b"\0", lim, status))
        return list(status.raw[:n])

    def _lookup(self, fn, n, front, tail=()):
        status = C.create_string_buffer(max(n, 1))
        index = (C.c_uint64 * max(n, 1))()
        limit = (C.c_uint32 * max(n, 1))()
        check(fn(self._h, n, *front, status, index, limit, *tail))
        return list(status.raw[:n]), [int(v) for v in index[:n]], [int(v) for v in limit[:n]]

    def find(self, idcs):
        """[identity commitment] -> (status, index, limit), three lists; UNKNOWN: index NO_INDEX, limit 0"""
        return self._lookup(lib().rlnamd_directory_find, len(idcs), (b"".join(self._w(v) for v in idcs) or b"\0",))

    @staticmethod
    def _take(take, n):
        if take is None:
            return None
        take = bytes(1 if t else 0 for t in take)
        if len(take) != n:
            raise RLNError("MemberDirectory: %d secrets and %d take marks" % (n, len(take)))
        return take or b"\0"

    def resolve_raw(self, secrets: bytes, take=None):
        """n packed secrets (32 bytes each, canonical LE) and n take marks (bytes or bools; None: all) ->
        (status, index, limit).  A relay step's `secrets` and (status == SPAM) go in unchanged."""
        n = len(secrets) // 32
        if len(secrets) != 32 * n:
            raise RLNError("MemberDirectory.resolve: %d bytes of secrets" % len(secrets))
        return self._lookup(lib().rlnamd_directory_resolve, n, (secrets or b"\0", self._take(take, n)))

    def resolve(self, secrets, take=None):
        return self.resolve_raw(b"".join(self._w(s) for s in secrets), take)

    def slash_raw(self, secrets: bytes, take=None):
        """resolve_raw, and every FOUND member is removed -> (status, index, limit, distinct members removed)"""
        n = len(secrets) // 32
        if len(secrets) != 32 * n:
            raise RLNError("MemberDirectory.slash: %d bytes of secrets" % len(secrets))
        removed = C.c_uint64()
        out = self._lookup(lib().rlnamd_directory_slash, n, (secrets or b"\0", self._take(take, n)), (C.byref(removed),))
        return out + (int(removed.value),)

    def slash(self, secrets, take=None):
        return self.slash_raw(b"".join(self._w(s) for s in secrets), take)

    def remove(self, indices):
        """a withdrawal by index: [index] -> [REMOVED | VACANT]"""
        n = len(indices)
        status = C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_directory_remove(self._h, n, (C.c_uint64 * max(n, 1))(*[int(i) for i in indices]), status))
        return list(status.raw[:n])

    def get(self, indices):
        """[index], repeats allowed -> [(live, identity commitment, limit)]; FREE rows read as (False, 0, 0)"""
        n = len(indices)
        live, idcs = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(32 * n, 1))
        limits = (C.c_uint32 * max(n, 1))()
        check(lib().rlnamd_directory_get(self._h, n, (C.c_uint64 * max(n, 1))(*[int(i) for i in indices]), live, idcs, limits))
        return [(bool(live.raw[i]), int.from_bytes(idcs.raw[32 * i:32 * i + 32], "little"), int(limits[i])) for i in range(n)]

    def info(self):
        """[capacity, live members, table slots, slots taken (those of removed members included), table rebuilds, longest
        walk of any call, calls, non-zero 16-byte words left in the staging that held secrets (0 expected)]"""
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_directory_info(self._h, out))
        return [int(v) for v in out]


class QuotaLedger:
    """Device-resident ledger of the message ids a signer has handed out (rlnamd_quota_*): max_epochs x 2^depth counters,
    the next message id of each member under each external nullifier of the window, and draw(), which hands out the
    next ids of a batch of requests.  A request past its member's limit gets no id, so no proof, and no two proofs under
    one (external nullifier, member) ever carry the same id -- the NullifierLog of a relay never says SPAM.

    An external nullifier that has left the window must not come back (its counters are gone).  QuotaLedger(depth,
    max_epochs) is not persisted: a restarted process must not sign under an external nullifier that was open before
    the restart.  QuotaLedger.open(path, ...) is: every draw is journalled and synced before an id of it is returned,
    and a reopen, however the process ended, restores the window and every counter at or above everything ever issued
    (rlnamd_quota_open).  The directory is as secret as the ledger: its files are 0600 and not encrypted."""
    OK, OVER, NO_EPOCH = range(3)
    EPOCHS_MAX = 64
    INFO = ("window", "draws", "issued", "over", "no_epoch", "residue", "depth", "max_epochs")
    STORE_INFO = ("generation", "journal_bytes", "records", "syncs", "compactions", "replayed", "torn_bytes", "restored_pairs")

    def __init__(self, depth, max_epochs):
        self._h = C.c_void_p()
        check(lib().rlnamd_quota_new(depth, max_epochs, C.byref(self._h)))

    @classmethod
    def open(cls, path, depth, max_epochs, journal_max_bytes=0):
        """the ledger on the directory `path`: created if it is empty or absent, otherwise reopened; refused (RLNError)
        for damage that would lower a counter, another depth or max_epochs, or a directory another ledger holds.
        journal_max_bytes: the journal's size behind which a call compacts; 0: max(1 MiB, the snapshot's bytes)"""
        q = cls.__new__(cls)
        q._h = C.c_void_p()
        check(lib().rlnamd_quota_open(os.fsencode(path), depth, max_epochs, journal_max_bytes, C.byref(q._h)))
        return q

    def compact(self):
        """the snapshot of the next generation and an empty journal, now (a ledger opened on a directory only)"""
        check(lib().rlnamd_quota_compact(self._h))

    def store_info(self):
        """the store's counts as a dict of STORE_INFO; all zero for a ledger without a store"""
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_quota_store_info(self._h, out))
        return dict(zip(self.STORE_INFO, (int(v) for v in out)))

    def close(self):
        """frees the ledger; one opened on a directory compacts first if its journal holds records"""
        if self._h:
            lib().rlnamd_quota_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_epochs(self, external_nullifiers):
        """0 .. max_epochs external nullifiers (ints): one that stays keeps its counters, one that leaves loses them,
        a new one starts at zero; an empty list empties the window"""
        check(lib().rlnamd_quota_set_epochs(self._h, b"".join(_b(e) for e in external_nullifiers), len(external_nullifiers)))

    def epochs(self):
        """the window in the order it was given, duplicates once: a list of ints"""
        out = C.create_string_buffer(32 * self.EPOCHS_MAX)
        k = C.c_size_t()
        check(lib().rlnamd_quota_epochs(self._h, out, C.byref(k)))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(k.value)]

    def draw(self, leaf_indices, external_nullifiers, limits):
        """n requests -> (ids, statuses), two lists of ints; ids[i] is limits[i] where statuses[i] is not OK"""
        n = len(leaf_indices)
        if len(external_nullifiers) != n or len(limits) != n:
            raise RLNError("QuotaLedger.draw: %d leaf indices, %d external nullifiers, %d limits" % (n, len(external_nullifiers), len(limits)))
        ids, status = (C.c_uint32 * max(n, 1))(), C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_quota_draw(self._h, n, (C.c_uint64 * max(n, 1))(*[int(v) for v in leaf_indices]),
                                      b"".join(_b(e) for e in external_nullifiers) or b"\0",
                                      (C.c_uint32 * max(n, 1))(*[int(v) for v in limits]), ids, status))
        return list(ids[:n]), list(status.raw[:n])

    COUNT_MAX = 255

    def draw_counts(self, leaf_indices, external_nullifiers, limits, counts):
        """n requests of counts[i] ids each (1 .. COUNT_MAX: the message slots a multi-message-id proof uses) ->
        (firsts, statuses); an OK request owns the ids firsts[i] .. firsts[i] + counts[i] - 1, and firsts[i] is
        limits[i] where statuses[i] is not OK.  A request is granted whole or not at all, and one that is refused still
        counts in the ranks behind it: a call is NOT what every split of it gives (rlnamd_quota_draw_counts)."""
        n = len(leaf_indices)
        if len(external_nullifiers) != n or len(limits) != n or len(counts) != n:
            raise RLNError("QuotaLedger.draw_counts: %d leaf indices, %d external nullifiers, %d limits, %d counts" %
                           (n, len(external_nullifiers), len(limits), len(counts)))
        for i, c in enumerate(counts):      # what a byte cannot carry to the library's own check, in the library's words
            if not 0 <= int(c) <= self.COUNT_MAX:
                raise RLNError("quota ledger: request %d of draw_counts asks for %d ids, more than %d" % (i, int(c), self.COUNT_MAX))
        firsts, status = (C.c_uint32 * max(n, 1))(), C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_quota_draw_counts(self._h, n, (C.c_uint64 * max(n, 1))(*[int(v) for v in leaf_indices]),
                                             b"".join(_b(e) for e in external_nullifiers) or b"\0",
                                             (C.c_uint32 * max(n, 1))(*[int(v) for v in limits]),
                                             bytes(int(c) for c in counts) or b"\0", firsts, status))
        return list(firsts[:n]), list(status.raw[:n])

    def used(self, leaf_indices, external_nullifiers):
        """the counters of n (leaf, external nullifier) pairs -> [next id, or None outside the window]"""
        n = len(leaf_indices)
        if len(external_nullifiers) != n:
            raise RLNError("QuotaLedger.used: %d leaf indices, %d external nullifiers" % (n, len(external_nullifiers)))
        out, inside = (C.c_uint32 * max(n, 1))(), C.create_string_buffer(max(n, 1))
        check(lib().rlnamd_quota_used(self._h, n, (C.c_uint64 * max(n, 1))(*[int(v) for v in leaf_indices]),
                                      b"".join(_b(e) for e in external_nullifiers) or b"\0", out, inside))
        return [int(out[i]) if inside.raw[i] else None for i in range(n)]

    def info(self):
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_quota_info(self._h, out))
        return dict(zip(self.INFO, (int(v) for v in out)))

    @staticmethod
    def plan(n, depth):
        """the passes of a draw of n requests: (sort passes, workgroups a pass, scan levels over a pass's bins, scan
        levels over the requests); no device needed"""
        out = (C.c_uint64 * 4)()
        check(lib().rlnamd_quota_plan(n, depth, out))
        return tuple(int(v) for v in out)


class Hasher:
    """hash_to_field (rln/src/hashers.rs:73-93) of many messages in one call on the device (rlnamd_hasher_*): a lane per
    message, the lanes dealt by descending length; the longest of the messages of more than lane_max_blocks 136-byte
    blocks are hashed on the calling thread meanwhile (as many as it is done with before a lane would be), and a call
    larger than stage_bytes of pinned staging goes through it in chunks."""
    INFO = ("device_messages", "host_messages", "chunks", "device_blocks", "longest_lane_blocks", "half_blocks",
            "lane_max_blocks", "calls")

    def __init__(self, stage_bytes=0, lane_max_blocks=0):
        self._h = C.c_void_p()
        check(lib().rlnamd_hasher_new(stage_bytes, lane_max_blocks, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rlnamd_hasher_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hash_to_field_raw(self, data: bytes, offsets) -> bytes:
        """message i is data[offsets[i]:offsets[i + 1]] -> n * 32 bytes, row i its field element (canonical LE)"""
        n = len(offsets) - 1
        if n < 0:
            raise RLNError("Hasher.hash_to_field: offsets must hold n + 1 entries")
        off = (C.c_uint64 * (n + 1))(*[int(o) for o in offsets])
        out = C.create_string_buffer(max(32 * n, 1))
        check(lib().rlnamd_hasher_hash_to_field(self._h, data, len(data), off, n, out))
        return out.raw[:32 * n]

    def hash_to_field(self, messages):
        """messages: a list of bytes -> a list of ints"""
        offsets = [0]
        for m in messages:
            offsets.append(offsets[-1] + len(m))
        out = self.hash_to_field_raw(b"".join(messages), offsets)
        return [int.from_bytes(out[32 * i:32 * i + 32], "little") for i in range(len(messages))]

    def info(self):
        """of the last call: messages on the device and on the host, chunks, blocks on the device, the longest lane;
        of the hasher: blocks per staging half, lane_max_blocks, calls so far"""
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_hasher_info(self._h, out))
        return dict(zip(self.INFO, (int(v) for v in out)))


class Relay:
    """One relay step on the device (rlnamd_relay_*): the signals of n messages hashed, their proofs verified and the
    shares of the accepted ones run through the nullifier log in one call -- exactly what Hasher.hash_to_field,
    BatchProver.verify_many_gpu and one NullifierLog.observe give over the same inputs, with the public values staying
    on the device in between and the hashing running beside the pairing kernels.  It borrows the prover, the log and
    the hasher (keep them alive); without a hasher every step brings xs.

    optimistic: the chunks that would run a lane per proof take one combined pairing check (verify_many_gpu_optimistic's,
    the scalars derived on the device from one seed per chunk) and the exact pass only when it rejects; team_checks: the
    chunks in team form too (needs optimistic).  The same results, up to about 2^-128 per accepted chunk; progress is
    read from BatchProver.verify_optimistic_stats and verify_gpu_passes.

    The epoch window: set_epochs(W) names the external nullifiers the relay follows.  The log retains them
    (NullifierLog.retain), and from then on a message that would be OK under an external nullifier outside W is
    BAD_EPOCH and never reaches the log.  No window (as made, or set_epochs([])): any external nullifier."""
    OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_EPOCH = range(5)
    ROOTS_MAX = 64
    EPOCHS_MAX = 64
    OPTIMISTIC, OPTIMISTIC_TEAMS = 1, 2
    INFO = ("steps", "chunks", "messages", "accepted", "shares", "residue_words", "host_hashed", "bad_epoch")

    def __init__(self, prover: "BatchProver", log: "NullifierLog", hasher: "Hasher" = None, lanes=0, optimistic=False,
                 team_checks=False):
        self._h = C.c_void_p()
        self._keep = (prover, log, hasher)
        flags = (self.OPTIMISTIC if optimistic else 0) | (self.OPTIMISTIC_TEAMS if team_checks else 0)
        check(lib().rlnamd_relay_new_ex(prover._h, log._h, hasher._h if hasher is not None else None, lanes, flags,
                                        C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rlnamd_relay_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step_raw(self, proofs: bytes, values: bytes, n_values, signals=None, offsets=None, xs=None, roots=b"", tags=None):
        """n packed proofs (128 bytes each) and their values (n_values * 32 bytes each, canonical LE, verifier order);
        either signals (bytes) with offsets (n + 1 ints) or xs (n * 32 bytes); roots: packed accepted roots, empty for
        any root -> (verdict n bytes, status n bytes, secrets n * 32 bytes, first tags: list of n ints)"""
        n = len(proofs) // 128
        if len(proofs) != 128 * n or len(values) != 32 * n_values * n or (tags is not None and len(tags) != n) or \
                len(roots) % 32 or (offsets is not None and len(offsets) != n + 1) or (xs is not None and len(xs) != 32 * n):
            raise RLNError("Relay.step: the lengths of proofs, values, offsets, xs, roots and tags do not agree")
        off = None if offsets is None else (C.c_uint64 * (n + 1))(*[int(o) for o in offsets])
        tg = None if tags is None else (C.c_uint64 * max(n, 1))(*[int(t) for t in tags])
        verdict, status = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(n, 1))
        secrets = C.create_string_buffer(max(32 * n, 1))
        first = (C.c_uint64 * max(n, 1))()
        check(lib().rlnamd_relay_step(self._h, n, proofs, values, n_values, signals, len(signals) if signals is not None else 0,
                                      off, xs, roots if roots else None, len(roots) // 32, tg, verdict, status, secrets, first))
        return verdict.raw[:n], status.raw[:n], secrets.raw[:32 * n], list(first[:n])

    def step(self, proofs, public_inputs, signals=None, xs=None, roots=(), tags=None):
        """proofs: a list of 128-byte strings; public_inputs: their values as lists of ints; signals: a list of bytes,
        or xs: a list of ints; roots: accepted roots as ints (none: any root) -> (verdict, status, secrets, first_tag),
        four lists of ints"""
        n = len(proofs)
        nv = _check_verify_shapes(proofs, public_inputs) if n else 0
        offsets = None
        if signals is not None:
            offsets = [0]
            for m in signals:
                offsets.append(offsets[-1] + len(m))
        v, st, sec, first = self.step_raw(
            b"".join(proofs), b"".join(_b(x) for pi in public_inputs for x in pi), nv,
            None if signals is None else b"".join(signals), offsets,
            None if xs is None else b"".join(_b(x) for x in xs), b"".join(_b(r) for r in roots), tags)
        return list(v), list(st), [int.from_bytes(sec[32 * i:32 * i + 32], "little") for i in range(n)], first

    def set_epochs(self, external_nullifiers):
        """0 .. 64 external nullifiers (ints).  One or more: the log drops every record outside them, then they are the
        window -> how many records went.  None: the window is switched off, nothing is removed -> 0."""
        k = len(external_nullifiers)
        removed = C.c_uint64()
        check(lib().rlnamd_relay_set_epochs(self._h, b"".join(_b(e) for e in external_nullifiers), k, C.byref(removed)))
        return int(removed.value)

    def epochs(self):
        """the window, as it was given: a list of ints, empty for none"""
        out = C.create_string_buffer(32 * self.EPOCHS_MAX)
        k = C.c_size_t()
        check(lib().rlnamd_relay_epochs(self._h, out, C.byref(k)))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(k.value)]

    def info(self):
        out = (C.c_uint64 * 8)()
        check(lib().rlnamd_relay_info(self._h, out))
        d = dict(zip(self.INFO, (int(v) for v in out)))
        d["reserved"] = 0   # the name [7] had before it counted BAD_EPOCH
        return d


class MsmG1:
    """Variable-base MSM (VariableBaseMSM::msm_bigint, ark-ec 0.5.0; BASELINE config 5) on G1; MsmG2 below is the same
    object on the twist: points are (x, y) ints for G1, ((x.c0, x.c1), (y.c0, y.c1)) for G2, None = infinity."""
    GROUP = 1

    def __init__(self, capacity):
        self._h = C.c_void_p()
        check((lib().rlnamd_msm_new if self.GROUP == 1 else lib().rlnamd_msm_new_g2)(capacity, C.byref(self._h)))
        self.ws_bytes = int(lib().rlnamd_msm_window_sums_bytes_of(self._h))
        self.pt_bytes = int(lib().rlnamd_msm_point_bytes(self._h))

    def close(self):
        if self._h:
            lib().rlnamd_msm_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pt_bytes(self, p):
        if p is None:
            return bytes(self.pt_bytes)
        if self.GROUP == 1:
            return _b(p[0], _Q) + _b(p[1], _Q)
        return _b(p[0][0], _Q) + _b(p[0][1], _Q) + _b(p[1][0], _Q) + _b(p[1][1], _Q)

    def _pt_from(self, raw):
        v = [int.from_bytes(raw[32 * k:32 * k + 32], "little") for k in range(self.pt_bytes // 32)]
        if not any(v):
            return None
        return (v[0], v[1]) if self.GROUP == 1 else ((v[0], v[1]), (v[2], v[3]))

    def set(self, points, scalars):
        """points: list of affine points (see the class docstring) or None for infinity"""
        pb = b"".join(self._pt_bytes(p) for p in points)
        check(lib().rlnamd_msm_set(self._h, pb, b"".join(_b(s) for s in scalars), len(points)))

    def set_raw(self, points_bytes, scalars_bytes, n):
        """the same from bytes: n canonical little-endian points (pt_bytes each, all zero = infinity) and n 32-byte scalars"""
        if len(points_bytes) != self.pt_bytes * n or len(scalars_bytes) != 32 * n:
            raise ValueError("set_raw: %d points need %d + %d bytes" % (n, self.pt_bytes * n, 32 * n))
        check(lib().rlnamd_msm_set(self._h, points_bytes, scalars_bytes, n))

    EQUAL_SCALARS, FOUR_POINTS = 1, 2

    def generate(self, seed, first_index, n, mode=0):
        """config-5 workload in HBM (P_i = k_i G, s_i from the SplitMix64 stream); the expected sum is not ours to
        state -- tests and bench.py take it from the oracle (oracle.c.binding.msm_expected)"""
        check(lib().rlnamd_msm_generate_mode(self._h, seed, first_index, n, mode))

    def fetch(self, first, count):
        """-> [(point or None, scalar)] of the loaded / generated workload"""
        p, s = C.create_string_buffer(self.pt_bytes * count), C.create_string_buffer(32 * count)
        check(lib().rlnamd_msm_fetch(self._h, first, count, p, s))
        return [(self._pt_from(p.raw[self.pt_bytes * i:self.pt_bytes * (i + 1)]),
                 int.from_bytes(s.raw[32 * i:32 * i + 32], "little")) for i in range(count)]

    def run_windows(self):
        """-> (window-sum blob to all-gather, stage ms dict)"""
        buf = C.create_string_buffer(self.ws_bytes)
        ms = (C.c_float * 3)()
        check(lib().rlnamd_msm_run(self._h, buf, ms))
        return buf.raw, dict(sort_ms=float(ms[0]), bucket_acc_ms=float(ms[1]), bucket_reduce_ms=float(ms[2]))

    def combine(self, blobs):
        out = C.create_string_buffer(self.pt_bytes)
        check(lib().rlnamd_msm_combine(self._h, b"".join(blobs), len(blobs), out))
        return self._pt_from(out.raw)

    def run_sharded(self, comm: "Comm"):
        """config 5 on this rank of an RCCL communicator (collective): -> (point or None, stage ms dict)"""
        out = C.create_string_buffer(self.pt_bytes)
        ms = (C.c_float * 4)()
        check(lib().rlnamd_msm_run_sharded(self._h, comm._h, out, ms))
        return self._pt_from(out.raw), dict(sort_ms=float(ms[0]), buckets_ms=float(ms[1]),
                                            all_gather_ms=float(ms[2]), combine_ms=float(ms[3]))

    def msm(self, points, scalars):
        self.set(points, scalars)
        blob, _ = self.run_windows()
        return self.combine([blob])


class MsmG2(MsmG1):
    """the same Pippenger on G2 (rlnamd_msm_new_g2): 128-byte points, 4 KiB of window sums per rank"""
    GROUP = 2
