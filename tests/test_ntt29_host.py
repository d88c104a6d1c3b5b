"""The big batches' quotient transforms on 29-bit limbs (prover_front.hip: k_ntt_pass / k_ntt_turn) without a GPU.

tests/host/ntt29.cpp is a program of its own: the kernels' bodies with the wave's group index as a loop -- the same base /
stride / twiddle-index formulas, the same K, normalize() and reduction per level -- in 29-bit limb arithmetic on 64-bit
integers, the loose eight-word store and load between launches included.  It checks the limb, column and value bounds at
every step and compares the canonical words of the last launch, word for word, with the replay in plain Fr arithmetic for
logn = 3, 4, 5, 12 and 13 over inputs chosen for lazy growth (all r - 1, all 1, alternating 0 / r - 1, a single r - 1 at 0,
n / 2 and n - 1, two random vectors).  tools/check_fq29_bounds.py proves the same bounds for ALL inputs (every limb and
value at its maximum) and compares the constants in prover_front.hip with its own.  The program is built and run with
-fsanitize=address,undefined as well."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "host", "ntt29.cpp")] + \
       [os.path.join(CSRC, f) for f in ("prover_plan.cpp", "poseidon_host.cpp", "witness_sched.cpp", "zkey.cpp")]
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC]


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.endswith(" 0 failed"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(last.split()[0]) > 1000000      # (13 levels alone are 53 248 butterflies per input)
    return r


def test_the_replay_on_29_bit_limbs_keeps_its_bounds_and_equals_the_fr_replay(tmp_path):
    exe = str(tmp_path / "ntt29")
    subprocess.check_call(["g++", "-O2"] + FLAGS + SRCS + ["-o", exe, "-lpthread"])
    _run(exe)


def test_the_bounds_tool_replays_every_pass_and_turn():
    spec = importlib.util.spec_from_file_location("check_fq29_bounds", os.path.join(ROOT, "tools", "check_fq29_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows, stored = mod.ntt29_main()
    assert len(rows) >= 8 and all(r[0] == "Fr" and r[2] == "wide" and r[3] < 16.0 for r in rows)
    assert max(r[3] for r in rows) > 15.0       # the difference of two sums of two products sits at 15.93: not vacuous
    assert 1.0 < stored < (1 << 256) / mod.R
    mod.ntt29_check_source(os.path.join(CSRC, "prover_front.hip"))
    assert len(mod.main(verbose=False)) >= 25 + len(rows)
    # the replay fails where it must: a DIF difference of two sums of two loads against the constant made for products
    rp = mod.NttReplay()
    with pytest.raises(AssertionError):
        rp.sub(rp.load(), "K4B2", rp.add(rp.load(), rp.load()))
    with pytest.raises(AssertionError):       # and a sum of eight loads stored without its reduction
        rp.store(rp.norm(rp.add(rp.add(rp.add(rp.load(), rp.load()), rp.add(rp.load(), rp.load())),
                                rp.add(rp.add(rp.load(), rp.load()), rp.add(rp.load(), rp.load())))), False)


def test_the_same_program_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "ntt29_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer"] + FLAGS + SRCS + ["-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
