"""The scalars of a seeded combined check (zerokit_amd/csrc/verify_agg_scalars.h) on the CPU: rlnamd_verify_agg_scalars
against a restatement of include/rln_amd.h's layout over the oracle's Keccak-f[1600], the same source as a stand-alone
program under ASan + UBSan, and the flags rlnamd_relay_new_ex refuses before it looks at anything else.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from oracle.pyref.keccak import _f1600

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
SEED_A = bytes(range(1, 33))
SEED_B = bytes(range(1, 32)) + b"\xff"
BIG = (1 << 32) + 1
SIZES = (1, 7, 8, 9, 65536 - 3, 65536)   # 8 192 groups; 65 533 has a partial last group, 7 and 9 have one too
DOMAIN = b"RLNAMD-AGG-SCAL1"


def restated_group(seed, chunk, group):
    """include/rln_amd.h, rlnamd_verify_agg_scalars: the 8 scalars of one group as ints"""
    block = seed + DOMAIN + chunk.to_bytes(8, "little") + group.to_bytes(8, "little")
    assert len(block) == 64
    block += b"\x01" + bytes(70) + b"\x80" + bytes(64)
    assert len(block) == 200
    lanes = [int.from_bytes(block[8 * i:8 * i + 8], "little") for i in range(25)]
    A = _f1600([[lanes[x + 5 * y] for y in range(5)] for x in range(5)])
    out = b"".join(A[i % 5][i // 5].to_bytes(8, "little") for i in range(16))
    return [int.from_bytes(out[16 * j:16 * j + 16], "little") or 1 for j in range(8)]


def restated(seed, chunk, n):
    out = []
    for g in range(-(-n // 8)):
        out += restated_group(seed, chunk, g)
    return out[:n]


def native(seed, chunk, n):
    from zerokit_amd.batch import agg_scalars
    return agg_scalars(seed, chunk, n)


@pytest.fixture(scope="module")
def wanted():
    """the restatement at the largest size, once: smaller sizes are its prefixes"""
    return {chunk: restated(SEED_A, chunk, max(SIZES)) for chunk in (0, BIG)}


@pytest.mark.parametrize("chunk", (0, BIG))
def test_the_library_gives_the_restated_layout(wanted, chunk):
    for n in SIZES:
        got = native(SEED_A, chunk, n)
        assert len(got) == n and got == wanted[chunk][:n], n
        assert all(0 < s < (1 << 128) for s in got)
    assert native(SEED_A, chunk, 0) == []


def test_the_output_buffer_is_written_to_its_length_only():
    from zerokit_amd import lib
    for n in (1, 7, 9):
        buf = C.create_string_buffer(b"\xa5" * (16 * n + 64))
        assert lib().rlnamd_verify_agg_scalars(SEED_A, 3, n, buf) == 0
        assert buf.raw[16 * n:16 * n + 64] == b"\xa5" * 64 and buf.raw[16 * n - 16:16 * n] != b"\xa5" * 16
    assert lib().rlnamd_verify_agg_scalars(None, 0, 1, buf) != 0


def test_another_seed_or_counter_gives_other_scalars(wanted):
    a = wanted[0][:64]
    assert len(set(a)) == 64
    for other in (native(SEED_B, 0, 64), native(SEED_A, 1, 64), native(SEED_A, BIG, 64), native(SEED_A, 1 << 32, 64)):
        assert not set(a) & set(other)
    assert native(SEED_A, BIG, 64) != native(SEED_A, 1, 64)   # the counter's high word counts


def test_stand_alone_program_under_asan_ubsan(tmp_path, wanted):
    """tests/host/aggscalars_main.cpp (its own main; never loaded into python) built with -fsanitize=address,undefined
    and run once over every size: the restated scalars come out, into buffers of exactly 16 n bytes, and the sanitizers
    stay silent"""
    exe = str(tmp_path / "aggscalars_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I", "/opt/rocm/include", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "aggscalars_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    sizes = SIZES
    r = subprocess.run([exe, SEED_A.hex(), str(BIG)] + [str(n) for n in sizes], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
    assert "%d sizes, 0 failures" % len(sizes) in r.stderr
    lines = r.stdout.split("\n")
    for n, line in zip(sizes, lines):
        raw = bytes.fromhex(line)
        assert len(raw) == 16 * n
        m = min(n, max(SIZES))
        assert [int.from_bytes(raw[16 * i:16 * i + 16], "little") for i in range(m)] == wanted[BIG][:m], n


@pytest.mark.parametrize("flags,text", [(2, "RLNAMD_RELAY_OPTIMISTIC_TEAMS needs RLNAMD_RELAY_OPTIMISTIC"),
                                        (4, "unknown flag bits 4 in flags 4"), (8, "unknown flag bits 8 in flags 8"),
                                        (7, "unknown flag bits 4 in flags 7")])
def test_relay_new_ex_refuses_flags_before_anything_else(flags, text):
    from zerokit_amd import lib
    from zerokit_amd._native import last_error
    h = C.c_void_p()
    assert lib().rlnamd_relay_new_ex(None, None, None, 0, flags, C.byref(h)) != 0
    assert last_error() == "rlnamd_relay_new_ex: " + text
    assert not h.value
    for ok_flags in (0, 1, 3):   # flags that pass reach the next check
        assert lib().rlnamd_relay_new_ex(None, None, None, 0, ok_flags, C.byref(h)) != 0
        assert last_error() == "rlnamd_relay_new_ex: null pointer"
