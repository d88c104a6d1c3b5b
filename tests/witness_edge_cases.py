"""Adversarial witnesses for the prover's supplied-witness path (rlnamd_prover_upload_witness, BatchProver.prove_with_witness):
the scalars that an honest RLN witness -- Poseidon outputs and a few bits -- never holds, and that the kernels between a
scalar and a sum treat specially: glv_split (glv.h), emit_digits (prover_front.hip), the signed-digit table walks and the
reductions behind them.  A Groth16 prover does not need its witness to satisfy the circuit, so any vector of field
elements is a valid input and the oracle (oracle/c: oracle_prove_witness) says what bytes must come out.

No GPU and no compiled code in here: tests/test_witness_edge_cases_host.py checks the module itself on the CPU (the CPU
build of glv_split returns exactly the halves each scalar was made from; the restatement of emit_digits below re-sums to the
half with every digit in range; every category occurs), tests/test_gpu_adversarial_witness.py runs the witnesses on the device.

Scalars are built from chosen halves: s = (+-k1) + lambda (+-k2) mod r.  The split is Babai rounding against the lattice
basis of tools/gen_glv.py; `glv_model` restates it from the committed constants (glv_constants.h), and a scalar is only
kept when the model returns the halves it was made from."""
import os
import random
import re

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WITNESSES = 129
HALF_BITS = 127
DEFAULT_WINDOW_BITS = 120010   # ProverTuning::window_bits (prover.h): G1 c = 10, G2 c = 12


def glv_constants():
    txt = open(os.path.join(ROOT, "zerokit_amd", "csrc", "glv_constants.h")).read()
    out = {}
    for name, body in re.findall(r"(\w+)\[\d+\]\s*=\s*\{([^}]*)\}", txt):
        out[name] = sum(int(w.strip().rstrip("u"), 16) << (32 * k) for k, w in enumerate(body.split(",")))
    return out


_C = glv_constants()
LAMBDA = _C["LAMBDA"]


def glv_model(k):
    """tools/gen_glv.py's model of glv_split on the committed constants -> (k1, neg1, k2, neg2)"""
    c1 = (k * _C["G1"] + (1 << 287)) >> 288
    c2 = (k * _C["G2"] + (1 << 287)) >> 288
    M = (1 << 128) - 1
    k1 = (k - c1 * _C["A1"] - c2 * _C["A2"]) & M
    k2 = (c1 * _C["B1ABS"] - c2 * _C["B2"]) & M
    s1, s2 = k1 >> 127, k2 >> 127
    return ((-k1) & M if s1 else k1), s1, ((-k2) & M if s2 else k2), s2


def scalar_of(k1, n1, k2, n2):
    return ((-k1 if n1 else k1) + LAMBDA * (-k2 if n2 else k2)) % R


def schedule(spec):
    """make_sched (prover_plan.cpp): spec = c + 100 * wide -> the window widths, low window first"""
    c, wide = spec % 100, spec // 100
    W = (HALF_BITS - wide + c - 1) // c
    return [c + (1 if j < wide else 0) for j in range(W)]


def schedules(window_bits):
    """the two schedules of a prover's window_bits (g1 + 10000 * g2, no g2: the same as g1; Prover's constructor)
    -> (G1 widths, G2 widths)"""
    spec1 = window_bits % 10000
    return schedule(spec1), schedule(window_bits // 10000 or spec1)


def emit_digits(half, neg, cw):
    """emit_digits (prover_front.hip) in plain integers -> (digits, ties): a window of c bits gives d in
    [-2^(c-1), 2^(c-1)]; a value of exactly 2^(c-1) -- the tie -- goes to the end the scalar's sign leaves representable."""
    carry, out, ties = 0, [], 0
    for c in cw:
        E = 1 << (c - 1)
        raw = (half & ((1 << c) - 1)) + carry
        half >>= c
        ties += raw == E
        if raw > E or (raw == E and not neg):
            d, carry = raw - (1 << c), 1
        else:
            d, carry = raw, 0
        out.append(-d if neg else d)
    assert half == 0 and carry == 0, "the schedule does not cover the half"
    return out, ties


def resum(digits, cw):
    v, off = 0, 0
    for d, c in zip(digits, cw):
        v += d << off
        off += c
    return v


def _windows(cw, value_of, limit):
    """the half whose window j holds value_of(j, c_j), over the low windows that keep it below `limit`"""
    v, off = 0, 0
    for j, c in enumerate(cw):
        nv = v + (value_of(j, c) << off)
        if nv >= limit:
            break
        v, off = nv, off + c
    return v


def special_halves(cw1, cw2):
    """{name: half} for both schedules: the recoding edges"""
    lim = 1 << 125     # inside the region the split returns for either half, whatever the other half is below it
    H = {}
    for tag, cw in (("g1", cw1), ("g2", cw2)):
        H["tie_neg_" + tag] = _windows(cw, lambda j, c: 1 << (c - 1), lim)           # raw = 2^(c-1) in every window (no carry)
        H["tie_pos_" + tag] = _windows(cw, lambda j, c: (1 << (c - 1)) - (j > 0), lim)   # ... with the carry a positive tie sends up
        H["below_tie_" + tag] = _windows(cw, lambda j, c: (1 << (c - 1)) - 1, lim)
        H["above_tie_" + tag] = _windows(cw, lambda j, c: (1 << (c - 1)) + 1, lim)
    H["ripple"] = lim - 1                           # all ones: the lowest window's carry goes through every window
    return H


def _corner(sign1, sign2):
    """the largest halves the split returns with these signs: next to a corner of the basis' parallelogram"""
    a1, a2, b1, b2 = _C["A1"], _C["A2"], _C["B1ABS"], _C["B2"]
    # corners +-(v1 + v2) / 2 = +-((a1 + a2) / 2, (b2 - b1) / 2) and +-(v1 - v2) / 2 = +-((a1 - a2) / 2, (-b1 - b2) / 2)
    m1, m2 = ((a1 + a2) // 2, (b1 - b2) // 2) if sign1 != sign2 else ((a2 - a1) // 2, (b1 + b2) // 2)
    # glv_split rounds with g_i = round(2^288 |b_i| / r): its region differs from the parallelogram by up to ~2^-35 of a
    # side, so the nearest point that splits back lies up to ~2^92 inside the corner
    for d in (1 << j for j in range(101)):
        k1, k2 = m1 - d, m2 - d
        if glv_model(scalar_of(k1, sign1, k2, sign2)) == (k1, sign1, k2, sign2):
            return k1, k2, d
    raise AssertionError("no scalar next to the corner splits into its halves")


def special_scalars(cw1, cw2):
    """[(category, k1, neg1, k2, neg2)]: every scalar the categories below are made of"""
    rnd = random.Random(0x61D)
    H = special_halves(cw1, cw2)
    S = [("half_k1_only", rnd.getrandbits(124) | 1 << 123, 0, 0, 0), ("half_k2_only", 0, 0, rnd.getrandbits(124) | 1 << 123, 0)]
    for n1 in (0, 1):
        for n2 in (0, 1):
            k1, k2, _ = _corner(n1, n2)
            S.append(("max_halves", k1, n1, k2, n2))
            S.append(("signs_%d%d" % (n1, n2), rnd.getrandbits(125) | 1 << 124, n1, rnd.getrandbits(125) | 1 << 124, n2))
    for tag in ("g1", "g2"):
        S.append(("tie_pos_" + tag, H["tie_pos_" + tag], 0, H["tie_pos_" + tag], 0))
        S.append(("tie_neg_" + tag, H["tie_neg_" + tag], 1, H["tie_neg_" + tag], 1))
        S.append(("tie_other_sign_" + tag, H["tie_neg_" + tag], 0, H["tie_pos_" + tag], 1))   # the same bits, no tie above window 0
        S.append(("below_tie_" + tag, H["below_tie_" + tag], 0, H["below_tie_" + tag], 1))
        S.append(("above_tie_" + tag, H["above_tie_" + tag], 1, H["above_tie_" + tag], 0))
    S.append(("ripple", H["ripple"], 0, H["ripple"], 1))
    S.append(("ripple", H["ripple"], 1, H["ripple"], 0))
    for name, k1, n1, k2, n2 in S:
        assert glv_model(scalar_of(k1, n1, k2, n2)) == (k1, n1, k2, n2), name
    return S


# the plain field values of the issue's list: every signal holds the value
PLAIN = [("all_one", 1), ("all_r_minus_1", R - 1), ("all_lambda", LAMBDA), ("all_lambda_minus_1", LAMBDA - 1),
         ("all_half_down", (R - 1) // 2), ("all_half_up", (R + 1) // 2)]
RS_EDGES = [(0, 0), (0, 5), (7, 0), (R - 1, R - 1)]


def build(n_signals, n_public, window_bits, honest, honest_rs):
    """-> (witnesses, rs, labels, counts): N_WITNESSES witnesses of n_signals ints below 2^256 with their (r, s).
    n_public: public signals without the constant (signals 1 .. n_public); honest: full witnesses of valid inputs (w_0 = 1),
    at least 8 of them, with their (r, s).  counts: witnesses per category and the ties that occur per schedule and sign."""
    ns = n_signals
    cw1, cw2 = schedules(window_bits)
    assert len(honest) >= 8 and all(len(h) == ns and h[0] == 1 for h in honest)
    rnd = random.Random(0xED6E)
    W, RS, LB = [], [], []

    def add(label, w, rs=None):
        assert len(w) == ns
        W.append(list(w))
        LB.append(label)
        RS.append(rs)

    add("zero_rs_zero", [0] * ns, (0, 0))
    add("zero", [0] * ns, (rnd.randrange(1, R), rnd.randrange(1, R)))
    for name, v in PLAIN:
        add(name, [v] * ns)
    for name, at in (("single_at_1", 1), ("single_at_last_public", n_public), ("single_at_first_private", n_public + 1),
                     ("single_at_last", ns - 1)):
        w = [0] * ns
        w[at] = R - 1 if at & 1 else rnd.randrange(1, R)
        add(name, w)
    S = special_scalars(cw1, cw2)
    for name, k1, n1, k2, n2 in S:
        add(name, [scalar_of(k1, n1, k2, n2)] * ns)
    # every special scalar in ONE witness, at rotating rows, between honest values: the lanes of a wave then hold
    # different scalars of the list at the same row
    vals = [scalar_of(*s[1:]) for s in S] + [v for _, v in PLAIN] + [0]
    for rot in range(8):
        h = honest[rot % len(honest)]
        add("mosaic", [h[i] if i == 0 or i % 3 == 2 else vals[(i + 5 * rot) % len(vals)] for i in range(ns)])
    for k, w0 in enumerate((0, 2, R - 1)):
        add("w0_%s" % ("r_minus_1" if w0 == R - 1 else w0), [w0] + honest[k][1:], honest_rs[k])
    add("above_r", [v + R if i % 2 and v + R < 1 << 256 else v for i, v in enumerate(honest[3])], honest_rs[3])
    add("above_r", [(1 << 256) - 1] * ns)
    k = 0
    while len(W) < N_WITNESSES:
        add("honest", honest[k % len(honest)], honest_rs[k % len(honest)])
        k += 1
    assert len(W) == N_WITNESSES and k >= 8, "the edge cases leave too little room for honest witnesses"
    # (r, s): the four edge pairs laid across the categories (every third witness, so each pair meets several categories),
    # random pairs elsewhere; the witnesses that came with a pair keep it
    for i in range(N_WITNESSES):
        if RS[i] is None:
            RS[i] = RS_EDGES[(i // 3) % 4] if i % 3 == 0 else (rnd.randrange(R), rnd.randrange(R))
    counts = {}
    for lb in LB:
        counts[lb] = counts.get(lb, 0) + 1
    for tag, cw in (("g1", cw1), ("g2", cw2)):
        for name, k1, n1, k2, n2 in S:
            for half, neg in ((k1, n1), (k2, n2)):
                t = emit_digits(half, neg, cw)[1]
                key = "ties_%s_%s" % (tag, "neg" if neg else "pos")
                counts[key] = counts.get(key, 0) + t
    for pair in RS_EDGES:
        counts["rs_%d" % RS_EDGES.index(pair)] = sum(1 for x in RS if x == pair)
    return W, RS, LB, counts


CATEGORIES = (["zero_rs_zero", "zero", "single_at_1", "single_at_last_public", "single_at_first_private", "single_at_last",
               "half_k1_only", "half_k2_only", "max_halves", "signs_00", "signs_01", "signs_10", "signs_11", "ripple", "mosaic",
               "w0_0", "w0_2", "w0_r_minus_1", "above_r", "honest"] + [n for n, _ in PLAIN] +
              [k + t for k in ("tie_pos_", "tie_neg_", "tie_other_sign_", "below_tie_", "above_tie_") for t in ("g1", "g2")])
TIE_KEYS = ["ties_%s_%s" % (t, s) for t in ("g1", "g2") for s in ("pos", "neg")]


def check_counts(counts):
    """every category has a witness, both ties occur on both schedules, every edge (r, s) is used more than once"""
    missing = [c for c in CATEGORIES if counts.get(c, 0) < 1]
    assert not missing, missing
    assert counts["max_halves"] == 4 and counts["honest"] >= 8
    assert all(counts[k] >= 8 for k in TIE_KEYS), {k: counts[k] for k in TIE_KEYS}
    assert all(counts["rs_%d" % k] >= 2 for k in range(4)), counts
    assert sum(counts[c] for c in CATEGORIES) == N_WITNESSES


def edge_indices(labels):
    """the witnesses whose quotient h the device test compares as well: everything but the honest ones and the mosaics"""
    return [i for i, lb in enumerate(labels) if lb not in ("honest", "mosaic")]
