"""What the shipped proving keys share between their A and B1 queries, read from the key files through
oracle/pyref/arkzkey.py: the expectation that tests/test_shared_rows_host.py holds the prover's detector to and that
tests/test_gpu_shared_rows.py holds rlnamd_prover_info.g1_rows to."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583

# circuit -> (wires with A_i == B1_i, wires with A_i == -B1_i)
COUNTS = {
    "tree_depth_20": (30, 1909),
    "tree_depth_10": (30, 1109),
    "tree_depth_20_multi_max_out_4": (124, 2383),
}


def circuit_dir(depth, multi):
    return "tree_depth_%d%s" % (depth, "_multi_max_out_4" if multi else "")


def resource(sub, name):
    return os.path.join(ROOT, "zerokit_amd", "resources", sub, name)


_keys = {}


def key_facts(sub):
    """dict(eq, opp: the wires i >= 1 with both rows finite, x equal and y equal / summing to q; finite_a, finite_b1;
    table_rows: the finite points of the G1 walk -- A, B1, L, the first `domain` H rows, alpha, beta, delta three times)"""
    if sub not in _keys:
        from oracle.pyref import arkzkey
        z = arkzkey.parse(open(resource(sub, "rln_final.arkzkey"), "rb").read())
        assert len(z.a_query) == len(z.b_g1_query)
        eq, opp = [], []
        for i in range(1, len(z.a_query)):
            a, b = z.a_query[i], z.b_g1_query[i]
            if a is None or b is None or a[0] != b[0]:
                continue
            if a[1] == b[1]:
                eq.append(i)
            elif (a[1] + b[1]) % Q == 0:
                opp.append(i)
        domain = 1
        while domain < z.num_constraints + z.num_instance_variables:
            domain <<= 1
        finite = lambda pts: sum(p is not None for p in pts)  # noqa: E731
        fixed = [z.alpha_g1, z.beta_g1, z.delta_g1, z.delta_g1, z.delta_g1]
        _keys[sub] = dict(eq=eq, opp=opp, finite_a=finite(z.a_query), finite_b1=finite(z.b_g1_query),
                          table_rows=finite(z.a_query) + finite(z.b_g1_query) + finite(z.l_query) + finite(z.h_query[:domain]) +
                          finite(fixed))
    return _keys[sub]
