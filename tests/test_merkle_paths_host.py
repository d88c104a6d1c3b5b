"""The index arithmetic of a Merkle path step (zerokit_amd/csrc/merkle_paths.h: leaf -> ancestor at level l -> sibling
-> bit), the function the device gather k_proofs_at inlines, built for the CPU and checked against the oracle's
FullMerkleTree.proof for every level of depths 1, 2, 10, 20 and 30.  No GPU needed."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle.pyref.rln import FullMerkleTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "tests", "host", "libmerklepaths.so")
    src = os.path.join(ROOT, "tests", "host", "merklepaths.cpp")
    hdr = os.path.join(ROOT, "zerokit_amd", "csrc", "merkle_paths.h")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "zerokit_amd", "csrc"), src, "-o", so])
    _check_the_stand_in()
    lib = ctypes.CDLL(so)
    lib.mp_path.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    lib.mp_path.restype = None
    lib.mp_dest_offsets.argtypes = [ctypes.c_uint64] * 6 + [ctypes.POINTER(ctypes.c_uint64)]
    lib.mp_dest_offsets.restype = None
    return lib


class _HeapIndices:
    """a node array whose value at heap index i is i: the oracle's proof() then returns the siblings' heap indices"""

    def __getitem__(self, i):
        return i


def oracle_path(depth, leaf):
    """(sibling heap indices, bits) by the oracle's own FullMerkleTree.proof, without building 2^(depth+1) nodes"""
    t = FullMerkleTree.__new__(FullMerkleTree)
    t.depth = depth
    t.nodes = _HeapIndices()
    return t.proof(leaf)


def leaves_of(depth):
    cap = 1 << depth
    rnd = random.Random(depth)
    picked = {0, cap - 1, cap // 2, max(cap // 2 - 1, 0), 1 % cap} | {rnd.randrange(cap) for _ in range(200)}
    return sorted(picked)


def _check_the_stand_in():
    """the heap-index stand-in gives what a real oracle tree gives (asked by the library fixture, before any comparison)"""
    t = FullMerkleTree(3, hash_pair=lambda a, b: (a * 31 + b * 17 + 1) % 1009)
    t.set_range(0, range(1, 9))
    for leaf in range(8):
        sib, bits = oracle_path(3, leaf)
        elems, want_bits = t.proof(leaf)
        assert [t.nodes[i] for i in sib] == elems and bits == want_bits


@pytest.mark.parametrize("depth", [1, 2, 10, 20, 30])
def test_path_step_matches_the_oracle_at_every_level(L, depth):
    anc = (ctypes.c_uint64 * depth)()
    sib = (ctypes.c_uint64 * depth)()
    bits = (ctypes.c_uint32 * depth)()
    for leaf in leaves_of(depth):
        L.mp_path(depth, leaf, anc, sib, bits)
        want_sib, want_bits = oracle_path(depth, leaf)
        assert list(sib) == want_sib, (depth, leaf)
        assert list(bits) == want_bits, (depth, leaf)
        # the ancestors: the leaf's own node, then the parent of the previous one (heap: (i - 1) // 2)
        node = (1 << depth) - 1 + leaf
        for l in range(depth):
            assert anc[l] == node, (depth, leaf, l)
            assert {anc[l], sib[l]} == {2 * ((node - 1) // 2) + 1, 2 * ((node - 1) // 2) + 2}
            node = (node - 1) // 2
        assert node == 0


def test_destination_offsets_of_both_layouts(L):
    out = (ctypes.c_uint64 * 2)()
    depth, inputs_size = 20, 46
    # packed [k][depth][32] + [k][depth]
    L.mp_dest_offsets(depth * 32, 32, depth, 1, 7, 19, out)
    assert list(out) == [(7 * depth + 19) * 32, 7 * depth + 19]
    # a prover's staged inputs [p][inputs_size][32]: element and bit strides are those of the inputs
    L.mp_dest_offsets(inputs_size * 32, 32, inputs_size * 32, 32, 1023, 19, out)
    assert list(out) == [(1023 * inputs_size + 19) * 32] * 2
    # proof 2^27 of a packed depth-30 buffer: the offset passes 2^32 (64-bit arithmetic throughout)
    L.mp_dest_offsets(30 * 32, 32, 30, 1, 1 << 27, 29, out)
    assert out[0] == ((1 << 27) * 30 + 29) * 32 and out[0] > 1 << 32


def test_index_header_under_asan_and_ubsan(tmp_path):
    """a stand-alone program of its own (tests/host/merklepaths_main.cpp), built with the sanitizers and run once"""
    exe = str(tmp_path / "merklepaths_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "zerokit_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "merklepaths_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])
