"""Inputs shared by tests/test_verify_math_host.py (CPU) and tests/test_gpu_verify.py (GPU): the golden proofs of the
three shipped circuits and the hand-made rejects a verifier has to get right.  A case is (name, proof128, [ints])."""
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
GT_ONE = (1).to_bytes(32, "little") + bytes(352)


def le(x):
    return int(x).to_bytes(32, "little")


def zkey_bytes(depth=20, multi=False):
    d = "tree_depth_%d%s" % (depth, "_multi_max_out_4" if multi else "")
    return open(os.path.join(ROOT, "zerokit_amd", "resources", d, "rln_final.arkzkey"), "rb").read()


def golden_h20():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "rln_h20_vectors.json")))["cases"]
    return [(c["name"], bytes.fromhex(c["proof_compressed"]), [int(v) for v in c["public_inputs"]]) for c in cases]


def golden_other():
    """[(name, depth, multi, proof, public inputs)] of the depth-10 and the multi-message-id circuit"""
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "rln_other_circuits.json")))["cases"]
    return [(c["name"], c["depth"], c["multi"], bytes.fromhex(c["proof_compressed"]), [int(v) for v in c["public"]])
            for c in cases]


def non_subgroup_b():
    """64 compressed bytes of a point on the twist outside the order-r subgroup: the first x = (k, 1) that has a y
    (the twist's cofactor is ~2^254, so a point found this way is outside with overwhelming probability; checked)"""
    from oracle.pyref import arkzkey
    from oracle.pyref.bn254 import G2, G2_B, f2_add, f2_mul, f2_sqr
    k = 1
    while True:
        x = (k, 1)
        y = arkzkey._sqrt_fq2(f2_add(f2_mul(f2_sqr(x), x), G2_B))
        if y is not None and G2.mul((x, y), R) is not None:
            break
        k += 1
    assert G2.on_curve((x, y))
    neg = (y[1] > (Q - 1) // 2) if y[1] else (y[0] > (Q - 1) // 2)
    out = bytearray(le(x[0]) + le(x[1]))
    if neg:
        out[63] |= 0x80
    return bytes(out)


def off_curve_x():
    """32 bytes of a canonical x with x^3 + 3 a non-residue (no such point on G1)"""
    x = 1
    while pow((x * x * x + 3) % Q, (Q - 1) // 2, Q) == 1:
        x += 1
    return le(x)


def rejects(name, proof, pub):
    """the mutations of one golden case: every public input changed in turn, A and C swapped, an input >= r, an x off
    the curve, the infinity encoding for A, a B outside the subgroup"""
    out = []
    for k in range(len(pub)):
        bad = list(pub)
        bad[k] = (bad[k] + 1) % R
        out.append(("%s/input%d" % (name, k), proof, bad))
    out.append((name + "/swapAC", proof[96:128] + proof[32:96] + proof[0:32], pub))
    big = list(pub)
    big[1] = R
    out.append((name + "/input_eq_r", proof, big))
    big = list(pub)
    big[-1] = (1 << 256) - 1
    out.append((name + "/input_max", proof, big))
    out.append((name + "/A_off_curve", off_curve_x() + proof[32:], pub))
    out.append((name + "/C_off_curve", proof[:96] + off_curve_x(), pub))
    out.append((name + "/A_noncanonical_x", le(Q) + proof[32:], pub))
    out.append((name + "/A_infinity", bytes(31) + b"\x40" + proof[32:], pub))
    out.append((name + "/C_infinity", proof[:96] + bytes(31) + b"\x40", pub))
    out.append((name + "/B_infinity", proof[:32] + bytes(63) + b"\x40" + proof[96:], pub))
    out.append((name + "/B_outside_subgroup", proof[:32] + non_subgroup_b() + proof[96:], pub))
    return out


def byte_mutations(cases, count, seed):
    """`count` single-byte mutations of golden proofs and inputs (seeded): a random byte of the 128 proof bytes or of
    the public-input bytes is xored with a random non-zero value.  Returns (name, proof, raw value bytes)."""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        name, proof, pub = cases[rnd.randrange(len(cases))]
        vals = bytearray(b"".join(le(v) for v in pub))
        proof = bytearray(proof)
        if rnd.random() < 0.7:
            proof[rnd.randrange(128)] ^= rnd.randrange(1, 256)
        else:
            vals[rnd.randrange(len(vals))] ^= rnd.randrange(1, 256)
        out.append(("%s/mut%d" % (name, i), bytes(proof), bytes(vals)))
    return out
