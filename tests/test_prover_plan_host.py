"""The prover's host planning (zerokit_amd/csrc/prover_plan.cpp) without a GPU, on all three shipped circuits:
tests/host/proverplan.cpp runs the k_witness29 program -- product / addition fusion, ring and stored operands, static
bounds -- with the product's own host field arithmetic against the golden witness digests, checks the invariants of every
table-walk plan the constructor uploads, compares the host-hashed hints with a plain evaluation of the graph at the
discovered cut nodes, and asks batch_shape for the operating point on both sides of every default threshold of
ProverTuning."""
import ctypes
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CIRCUITS = ["tree_depth_20", "tree_depth_10", "tree_depth_20_multi_max_out_4"]


@pytest.fixture(scope="module")
def PP():
    so = os.path.join(ROOT, "tests", "host", "libproverplan.so")
    srcs = [os.path.join(ROOT, "tests", "host", "proverplan.cpp")] + \
           [os.path.join(CSRC, f) for f in ("prover_plan.cpp", "poseidon_host.cpp", "witness_sched.cpp", "zkey.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("prover_plan.h", "prover_desc.h", "prover.h", "poseidon.h", "witness_sched.h",
                                                   "witness_ops.h", "zkey.h", "field.h", "curve.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I",
                               "/opt/rocm/include", "-I", CSRC] + srcs + ["-o", so])
    lib = ctypes.CDLL(so)
    lib.proverplan_error.restype = ctypes.c_char_p
    return lib


def _resource(sub, name):
    return open(os.path.join(ROOT, "zerokit_amd", "resources", sub, name), "rb").read()


def _inputs(graph_bytes, named_inputs):
    from oracle.pyref import wtns_graph
    g = wtns_graph.parse(graph_bytes)
    size = g.inputs_size()
    buf = bytearray(size * 32)
    buf[0] = 1
    for name, vals in named_inputs.items():
        off, ln = g.input_mapping[name]
        assert ln == len(vals)
        for k, v in enumerate(vals):
            buf[(off + k) * 32:(off + k + 1) * 32] = (int(v) % R).to_bytes(32, "little")
    return bytes(buf), size, len(g.signals)


def _golden_cases():
    """(circuit, instance variables, named inputs, witness digest, name) of every golden case that carries a digest"""
    out = []
    for c in json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["cases"]:
        w = c["witness"]
        named = {"identitySecret": [w["identity_secret"]], "userMessageLimit": [w["user_message_limit"]],
                 "messageId": [w["message_id"]], "pathElements": w["path_elements"],
                 "identityPathIndex": w["identity_path_index"], "x": [w["x"]],
                 "externalNullifier": [w["external_nullifier"]]}
        out.append(("tree_depth_20", len(c["public_inputs"]) + 1, named, c["witness_sha256"], c["name"]))
    for c in json.load(open(os.path.join(ROOT, "tests", "golden", "rln_other_circuits.json")))["cases"]:
        sub = "tree_depth_%d%s" % (c["depth"], "_multi_max_out_4" if c["multi"] else "")
        if c.get("witness_sha256"):
            out.append((sub, len(c["public"]) + 1, c["inputs"], c["witness_sha256"], c["name"]))
    return out


def test_the_witness29_program_reproduces_the_golden_witness(PP):
    """every golden case of every shipped circuit; the emulator itself refuses a ring reference that reaches back
    WIT29_RING or more, a far operand that reads a slot before it is stored, and a slot that does not fit 16 bits"""
    seen = set()
    for sub, ni, named, digest, name in _golden_cases():
        gb = _resource(sub, "graph.bin")
        buf, size, nsig = _inputs(gb, named)
        out = ctypes.create_string_buffer(32 * nsig)
        stats = (ctypes.c_uint32 * 8)()
        rc = PP.proverplan_run_program(gb, len(gb), ni, buf, size, out, stats)
        assert rc == 0, (name, PP.proverplan_error().decode())
        assert hashlib.sha256(out.raw).hexdigest() == digest, name
        nprog, nstore, err, ncuts, nred, nrare, nfused = list(stats)[:7]
        assert err == 0 and nstore < 65536, name
        depth, max_out = (10 if "10" in sub else 20), (4 if "multi" in sub else 1)
        assert ncuts == depth + 1 + max_out, name
        # the additions of the Poseidon rounds fold into their products: about a third of the graph's nodes
        assert nfused * 4 > nprog and nred > 0 and nrare < nprog // 4, (name, list(stats))
        seen.add(sub)
    assert seen == set(CIRCUITS)


def test_an_out_of_range_input_sets_the_error_flag_of_the_program(PP):
    from oracle.pyref import wtns_graph
    gb = _resource("tree_depth_10", "graph.bin")
    g = wtns_graph.parse(gb)
    size = g.inputs_size()
    buf = bytearray(size * 32)
    buf[0] = 1
    off, _ = g.input_mapping["x"]
    buf[off * 32:(off + 1) * 32] = R.to_bytes(32, "little")
    out = ctypes.create_string_buffer(32 * len(g.signals))
    stats = (ctypes.c_uint32 * 8)()
    assert PP.proverplan_run_program(gb, len(gb), 6, bytes(buf), size, out, stats) == 0
    assert stats[2] == 1


@pytest.mark.parametrize("sub", CIRCUITS)
def test_every_walk_plan_walks_exactly_its_rows(PP, sub):
    """plan1 (pair chunks), plan1s, the plain tiny plan, plan1f, plan1tf, plan2, plan2s, plan2t in the three modes: the row
    words of the chunks are the rows the mode walks, each (row, half) once; partial and finish partition full (unfused
    families); no chunk above chunk_pts; early and late ids partition the non-pair chunks and late chunks hold only h rows;
    a pair chunk's two slots are distinct empty chunks inside its members' segments; segchunks, groups / segs and segblocks
    cover every segment's chunk range exactly once"""
    zb, gb = _resource(sub, "rln_final.arkzkey"), _resource(sub, "graph.bin")
    log = ctypes.create_string_buffer(8192)
    stats = (ctypes.c_uint32 * 8)()
    failures = PP.proverplan_check_plans(zb, len(zb), gb, len(gb), log, len(log), stats)
    assert failures == 0, (failures, PP.proverplan_error().decode() if failures < 0 else log.value.decode())
    plans, npts1, npaired, npts2, npchunks = list(stats)[:5]
    assert plans == 24 and npts1 > npts2 > 0
    # A_i, B1_i and L_i share w_i: most G1 points that are not h rows are pair members, and the throughput plan has pair chunks
    assert npaired % 2 == 0 and npaired > 0 and npchunks > 0


def test_hints_equal_the_graph_at_the_cut_nodes_and_a_second_call_hits_the_chain_cache(PP):
    seen = set()
    for sub, ni, named, _, name in _golden_cases():
        gb = _resource(sub, "graph.bin")
        buf, size, _ = _inputs(gb, named)
        stats = (ctypes.c_uint32 * 8)()
        rc = PP.proverplan_check_hints(gb, len(gb), ni, buf, size, stats)
        assert rc == 0, (name, PP.proverplan_error().decode())
        ncuts, nhints, bad1, bad2, hits1, hits2, differ = list(stats)[:7]
        depth, max_out = (10 if "10" in sub else 20), (4 if "multi" in sub else 1)
        assert ncuts == nhints == depth + 1 + max_out, name
        assert bad1 == 0 and bad2 == 0 and differ == 0, (name, list(stats))
        assert hits1 == 0 and hits2 == 1, (name, list(stats))
        seen.add(sub)
    assert seen == set(CIRCUITS)


FULL, PARTIAL, FINISH = 0, 1, 2
BIG, SMALL, FUSED, TINY = 0, 1, 2, 3
FIELDS = ["lone", "small", "wl_used", "cone", "hinted", "probe_chains", "early", "fused", "tiny_partial", "tiny", "walk_lp",
          "g2_on_front", "values_w", "ntt_lds", "plan1", "plan2", "PB", "dB"]


def _shape(lib, n, mode=FULL, inputs=1, partial_points=0, handles=0, pre_hints=0, idle=1, shared=0, capacity=1024, lone=-1):
    q = (ctypes.c_uint32 * 9)(n, mode, inputs, partial_points, handles, pre_hints, idle, shared, capacity)
    out = (ctypes.c_uint32 * 18)()
    lib.proverplan_shape(q, lone, out)
    return dict(zip(FIELDS, list(out)))


def test_batch_shape_gives_the_documented_operating_points(PP):
    """at and on both sides of every default threshold of ProverTuning (prover.h)"""
    # tiny_max = 5: one (row, half) per lane, the fused tiny plan, partial sums [chunk][8], compact digits
    s = _shape(PP, 5)
    assert s["tiny"] and s["fused"] and s["plan1"] == TINY and s["plan2"] == TINY and s["PB"] == 8 and s["dB"] == 5
    s = _shape(PP, 6)
    assert not s["tiny"] and s["fused"] and s["plan1"] == FUSED and s["plan2"] == SMALL and s["PB"] == 128 and s["dB"] == 6
    assert s["lone"] and s["early"] and s["g2_on_front"] and s["values_w"] and s["wl_used"]
    # hint_max = 24, hint_max_warm = 64: hinted outright, hinted if the chains are remembered, never
    assert _shape(PP, 24)["hinted"] and not _shape(PP, 24)["probe_chains"]
    assert _shape(PP, 25)["hinted"] and _shape(PP, 25)["probe_chains"] and _shape(PP, 64)["probe_chains"]
    assert not _shape(PP, 65)["hinted"] and not _shape(PP, 64, inputs=0)["hinted"]
    assert _shape(PP, 64, pre_hints=1)["hinted"] and not _shape(PP, 64, pre_hints=1)["probe_chains"]
    # 16 proofs: lanes = proofs over the short chunks when the batch is not alone
    assert not _shape(PP, 15, lone=0)["walk_lp"] and _shape(PP, 15, lone=0)["dB"] == 15
    s = _shape(PP, 16, lone=0)
    assert s["walk_lp"] and s["dB"] == 1024 and not s["lone"] and not s["fused"] and s["plan1"] == SMALL and not s["g2_on_front"]
    assert not _shape(PP, 16)["walk_lp"] and not _shape(PP, 16, idle=0)["walk_lp"]
    # lone_small_max = 48: the lone shapes behind a batch in flight; lanechunk_walk_max = 48: lanes = chunks
    s = _shape(PP, 48, idle=0)
    assert s["lone"] and s["fused"] and not s["walk_lp"] and s["dB"] == 48
    s = _shape(PP, 49, idle=0)
    assert not s["lone"] and not s["fused"] and s["walk_lp"] and s["plan1"] == SMALL and not s["hinted"]
    s = _shape(PP, 49)
    assert s["lone"] and s["fused"] and s["walk_lp"] and s["dB"] == 1024 and s["plan1"] == FUSED
    # 96: the fused plan and the NTTs in LDS (ntt_lg_max)
    s = _shape(PP, 96)
    assert s["fused"] and s["ntt_lds"] and s["plan1"] == FUSED
    s = _shape(PP, 97)
    assert not s["fused"] and not s["ntt_lds"] and s["plan1"] == SMALL and s["lone"] and s["early"]
    # lanechunk_max = 128: the small-batch shapes
    s = _shape(PP, 128)
    assert s["small"] and s["early"] and s["plan1"] == SMALL and s["plan2"] == SMALL and s["PB"] == 128 and s["values_w"]
    assert _shape(PP, 128, idle=0)["wl_used"]
    s = _shape(PP, 129)
    assert not s["small"] and not s["early"] and s["plan1"] == BIG and s["plan2"] == BIG and s["PB"] == 1024 and s["dB"] == 1024
    assert s["wl_used"] and s["values_w"] and not s["g2_on_front"] and not s["ntt_lds"]
    s = _shape(PP, 129, idle=0)
    assert not s["wl_used"] and not s["values_w"] and not s["lone"]
    # witlanes_max = 1 024 alone on the device, 256 beside another prover
    assert _shape(PP, 256, shared=1)["wl_used"] and not _shape(PP, 257, shared=1)["wl_used"]
    assert _shape(PP, 1024)["wl_used"] and not _shape(PP, 1025, capacity=2048)["wl_used"]
    # finish: the fused plan only with the inputs and the partial points at hand; the cone only with live handles
    s = _shape(PP, 8, mode=FINISH, partial_points=1, handles=1)
    assert s["fused"] and s["cone"] and not s["hinted"] and s["plan1"] == FUSED and not s["tiny"]
    s = _shape(PP, 8, mode=FINISH, partial_points=1)
    assert s["fused"] and not s["cone"] and s["hinted"]
    s = _shape(PP, 8, mode=FINISH, partial_points=0)
    assert not s["fused"] and s["early"] and s["plan1"] == SMALL
    assert _shape(PP, 5, mode=FINISH, partial_points=1)["tiny"]
    assert not _shape(PP, 8, mode=FINISH, inputs=0)["fused"] and not _shape(PP, 8, mode=FINISH, inputs=0, handles=1)["cone"]
    assert _shape(PP, 129, mode=FINISH, partial_points=1, handles=1)["cone"]
    assert not _shape(PP, 129, mode=FINISH, partial_points=1, handles=1, idle=0)["cone"]
    # partial: never early; at most five proofs alone take the tiny plain plan
    s = _shape(PP, 5, mode=PARTIAL)
    assert s["tiny_partial"] and s["tiny"] and not s["early"] and not s["fused"] and s["plan1"] == TINY and s["PB"] == 8 and s["dB"] == 1024
    s = _shape(PP, 6, mode=PARTIAL)
    assert not s["tiny_partial"] and not s["tiny"] and s["plan1"] == SMALL and s["PB"] == 128
    assert not _shape(PP, 5, mode=PARTIAL, lone=0)["tiny_partial"]
