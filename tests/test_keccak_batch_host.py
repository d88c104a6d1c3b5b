"""The batch hash_to_field's host side (zerokit_amd/csrc/keccak_batch.h: the permutation and the reduce that
k_hash_to_field inlines, the plan of a call and the packing), built for the CPU: judged by the oracle's Keccak and by
padding built here, and run once more in a stand-alone sanitizer program.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from oracle.pyref.bn254 import R
from oracle.pyref.keccak import hash_to_field_le as o_htf, keccak256 as o_keccak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC]   # (field.h: #pragma unroll)
U64P = ctypes.POINTER(ctypes.c_uint64)
U32P = ctypes.POINTER(ctypes.c_uint32)
RATE = 136


def m(L):
    return bytes((L * 131 + j * 7 + (j >> 8)) & 0xff for j in range(L))


MESSAGES = [m(L) for L in range(410)]


@pytest.fixture(scope="module")
def oracle_rows():
    """the oracle's field element of each of the 410 messages, computed once"""
    return [o_htf(msg).to_bytes(32, "little") for msg in MESSAGES]


@pytest.fixture(scope="module")
def K():
    so = os.path.join(HOST, "libkeccakbatch.so")
    src = os.path.join(HOST, "keccakbatch.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("keccak_batch.h", "keccak.h", "field.h", "modinv30.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.kb_hash_message.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.kb_hash_message.restype = ctypes.c_int
    lib.kb_header_bytes.argtypes = [ctypes.c_size_t]
    lib.kb_header_bytes.restype = ctypes.c_size_t
    lib.kb_plan.argtypes = [ctypes.c_char_p, ctypes.c_uint64, U64P, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t,
                            ctypes.c_int, U32P, U64P, U64P, U64P, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.kb_plan.restype = ctypes.c_int
    lib.kb_pack_chunk.argtypes = [ctypes.c_char_p, ctypes.c_uint64, U64P, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t,
                                  ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.kb_pack_chunk.restype = ctypes.c_size_t
    lib.kb_hash_call.argtypes = [ctypes.c_char_p, ctypes.c_uint64, U64P, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t,
                                 ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.kb_hash_call.restype = ctypes.c_int
    lib.kb_selfcheck.argtypes = [U64P]
    lib.kb_selfcheck.restype = ctypes.c_int
    return lib


def flat(messages, lead=0):
    offsets = [lead]
    for msg in messages:
        offsets.append(offsets[-1] + len(msg))
    return bytes(lead) + b"".join(messages), (ctypes.c_uint64 * len(offsets))(*offsets)


def plan(K, messages, half_blocks, lane_max, ordered=True):
    n = len(messages)
    data, off = flat(messages)
    order, nblocks = (ctypes.c_uint32 * n)(), (ctypes.c_uint64 * n)()
    meta, chunks = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * (3 * 1024))()
    err = ctypes.create_string_buffer(128)
    assert K.kb_plan(data, len(data), off, n, half_blocks, lane_max, int(ordered), order, nblocks, meta, chunks, 1024,
                     err, 128) == 0, err.value
    assert meta[1] <= 1024
    return dict(order=list(order), nblocks=list(nblocks), n_host=int(meta[0]), device_blocks=int(meta[2]),
                longest=int(meta[3]), chunks=[tuple(chunks[3 * k:3 * k + 3]) for k in range(meta[1])])


def padded(msg):
    p = bytearray(msg) + bytes((len(msg) // RATE + 1) * RATE - len(msg))
    p[len(msg)] ^= 0x01
    p[-1] ^= 0x80
    return bytes(p)


def test_shared_permutation_and_reduce_match_the_oracle(K, oracle_rows):
    """every message through the text the lanes run; every quotient of the reduce, 0 .. 5, occurs among the digests"""
    seen = [0] * 6
    for msg, want in zip(MESSAGES, oracle_rows):
        out = ctypes.create_string_buffer(32)
        q = K.kb_hash_message(msg, len(msg), out)
        assert out.raw == want, len(msg)
        assert q == int.from_bytes(o_keccak(msg), "little") // R, len(msg)
        seen[q] += 1
    assert seen == [69, 73, 79, 73, 87, 29]


def test_whole_call_on_the_host_matches_the_oracle(K, oracle_rows):
    """plan, pack and a loop over the lanes, in one chunk and in chunks of 16 blocks, with and without the lane order"""
    data, off = flat(MESSAGES, lead=3)
    for half_blocks, lane_max, ordered in ((4096, 1024, 1), (16, 1024, 1), (16, 2, 1), (4096, 1, 1), (16, 1024, 0)):
        out = ctypes.create_string_buffer(32 * 410)
        assert K.kb_hash_call(data, len(data), off, 410, half_blocks, lane_max, ordered, out, None, 0) == 0
        assert out.raw == b"".join(oracle_rows), (half_blocks, lane_max, ordered)


def test_staged_bytes_are_the_padded_messages(K):
    """one chunk of all 410: first_block is the prefix sum of the block counts in lane order, and the blocks are the
    messages padded here -- L = 0, 135 (the 0x81 byte), 136, 271 and 272 among them"""
    p = plan(K, MESSAGES, 4096, 1024)
    assert p["n_host"] == 0 and len(p["chunks"]) == 1 and p["chunks"][0] == (0, 410, sum(p["nblocks"]))
    assert p["nblocks"] == [L // RATE + 1 for L in range(410)]
    data, off = flat(MESSAGES)
    buf = ctypes.create_string_buffer(K.kb_header_bytes(410) + RATE * sum(p["nblocks"]))
    got = K.kb_pack_chunk(data, len(data), off, 410, 4096, 1024, 0, buf, len(buf))
    assert got == len(buf)
    first = [int.from_bytes(buf.raw[4 * j:4 * j + 4], "little") for j in range(411)]
    want_first = [0]
    for i in p["order"]:
        want_first.append(want_first[-1] + p["nblocks"][i])
    assert first == want_first
    assert K.kb_header_bytes(410) == 1648 and buf.raw[4 * 411:1648] == bytes(4)
    blocks = buf.raw[1648:]
    for j, i in enumerate(p["order"]):
        assert blocks[RATE * first[j]:RATE * first[j + 1]] == padded(MESSAGES[i]), i
    assert padded(MESSAGES[135])[-1] == 0x81 and len(padded(MESSAGES[136])) == 272 and padded(MESSAGES[271])[-1] == 0x81


HOST_PACE = 50   # keccak_batch.h: a lone lane's time per block over a host core's


def host_count(nblocks, half_blocks, lane_max):
    """the host's share by the rule of keccak_batch.h: what fits no half, then the longest above lane_max_blocks while
    the blocks the host has taken, the next one included, are at most HOST_PACE times that message's"""
    taken = k = 0
    for b in sorted(nblocks, reverse=True):
        if not (b > half_blocks or (b > lane_max and taken + b <= HOST_PACE * b)):
            break
        taken += b
        k += 1
    return k


def check_order(p, half_blocks, lane_max):
    n = len(p["order"])
    assert sorted(p["order"]) == list(range(n))
    counts = [p["nblocks"][i] for i in p["order"]]
    assert counts == sorted(counts, reverse=True)
    for a, b in zip(p["order"], p["order"][1:]):
        assert p["nblocks"][a] > p["nblocks"][b] or a < b   # stable within equal counts
    assert p["n_host"] == host_count(p["nblocks"], half_blocks, lane_max)
    assert p["longest"] == max(counts[p["n_host"]:], default=0) <= half_blocks


def test_lane_order_chunks_and_the_host_route(K):
    mixed = [MESSAGES[(37 * k) % 410] for k in range(410)]   # the lengths out of order
    p = plan(K, mixed, 4096, 1024)
    check_order(p, 4096, 1024)
    assert p["n_host"] == 0 and p["longest"] == 4 and p["device_blocks"] == sum(p["nblocks"])
    # a staging half of 16 blocks: the chunks cover the lanes' messages exactly once, in order, none above 16 blocks
    p = plan(K, mixed, 16, 1024)
    check_order(p, 16, 1024)
    at = p["n_host"]
    for first, count, blocks in p["chunks"]:
        assert first == at and count >= 1
        assert blocks == sum(p["nblocks"][i] for i in p["order"][first:first + count]) and blocks <= 16
        at += count
    assert at == 410 and len(p["chunks"]) > 1
    # the next message would not have fitted: no chunk is cut early
    for (first, count, blocks), nxt in zip(p["chunks"], p["chunks"][1:]):
        assert blocks + p["nblocks"][p["order"][nxt[0]]] > 16
    # above one staging half: the host's, whatever lane_max_blocks says
    long = mixed + [bytes(5000), bytes(16 * RATE - 1), bytes(16 * RATE)]
    p = plan(K, long, 16, 1024)
    check_order(p, 16, 1024)
    assert p["order"][:p["n_host"]] == [410, 412] and p["nblocks"][411] == 16
    # above lane_max_blocks: the host's, longest first, while it keeps pace -- here 37 + 17 + 16 + 2 * 4 blocks, then 24 of
    # the 136 messages of 3 blocks (78 + 3 k <= 50 * 3), and the lanes take the rest of those
    p = plan(K, long, 4096, 2)
    check_order(p, 4096, 2)
    assert p["n_host"] == 29 and p["longest"] == 3
    with_order = p["order"]
    # a lone long message among short ones, a few of them, and nothing but long ones
    p = plan(K, [bytes(10)] * 100 + [bytes(200 * RATE - 1)] + [bytes(10)] * 100, 4096, 4)
    assert p["order"][:p["n_host"]] == [100] and p["longest"] == 1
    p = plan(K, [bytes(8 * RATE - 1)] * 1000, 4096, 4)
    check_order(p, 4096, 4)
    assert p["n_host"] == HOST_PACE and p["order"][:HOST_PACE] == list(range(HOST_PACE)) and p["longest"] == 8
    p = plan(K, [bytes(4 * RATE - 1)] * 1000, 4096, 4)
    assert p["n_host"] == 0                                   # not above lane_max_blocks: never the host's
    # without the lane order: the host's share is the same, the lanes are in index order
    p = plan(K, long, 4096, 2, ordered=False)
    host = with_order[:29]
    assert p["order"] == host + [i for i in range(len(long)) if i not in set(host)] and p["n_host"] == 29


def test_each_refusal_has_its_own_text_and_writes_nothing(K):
    data = bytes(range(8))
    texts = []

    def refused(data, data_len, offsets, n):
        off = None if offsets is None else (ctypes.c_uint64 * len(offsets))(*offsets)
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        err = ctypes.create_string_buffer(128)
        assert K.kb_hash_call(data, data_len, off, n, 16, 4, 1, out, err, 128) == 1
        assert out.raw == b"\x55" * 64 and err.value
        order = (ctypes.c_uint32 * 2)(7, 7)
        nblocks, meta, chunks = (ctypes.c_uint64 * 2)(7, 7), (ctypes.c_uint64 * 4)(7, 7, 7, 7), (ctypes.c_uint64 * 3)(7, 7, 7)
        assert K.kb_plan(data, data_len, off, n, 16, 4, 1, order, nblocks, meta, chunks, 1, err, 128) == 1
        assert list(order) + list(nblocks) + list(meta) + list(chunks) == [7] * 11
        texts.append(err.value)

    refused(data, 8, None, 2)              # null offsets
    refused(None, 8, [0, 3, 8], 2)         # null data
    refused(data, 8, [0, 5, 3], 2)         # decreasing offsets
    refused(data, 8, [0, 3, 9], 2)         # the end beyond data_len
    refused(data, 8, [0, 3, 8], 1 << 32)   # sizes that overflow
    assert len(set(texts)) == 5
    assert K.kb_hash_call(None, 0, None, 0, 16, 4, 1, None, None, 0) == 0   # n = 0 is no refusal


def test_header_under_asan_and_ubsan(K, tmp_path):
    """the stand-alone program (tests/host/keccakbatch_main.cpp) built with the sanitizers and run once as it is:
    it exits 0 and prints the digest of its rows, which is the unsanitized library's"""
    exe = str(tmp_path / "keccakbatch_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                          [os.path.join(HOST, "keccakbatch_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])
    digest = ctypes.c_uint64()
    assert K.kb_selfcheck(ctypes.byref(digest)) == 0
    assert r.stdout.split()[1] == "%016x" % digest.value
