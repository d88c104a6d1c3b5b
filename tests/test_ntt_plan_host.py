"""ntt_pass_list and ntt_tables (zerokit_amd/csrc/prover_plan.cpp) without a GPU: the launches that carry the three
transforms of the quotient in big batches -- DIF passes of three levels, the turn (the lowest levels of both directions
around the coset scaling), DIT passes of three levels.  tests/host/nttplan.cpp is a program of its own: it checks the list
for logn = 1 .. 20 (every level once per direction, blocks of at most eight points, the turn's width, the fall-back below
four levels) and replays the list on the host for logn = 3, 4, 5, 12 and 13 -- the kernels' own index formulas in plain Fr
arithmetic -- against a direct evaluation of iNTT, coset scaling, NTT, exactly.  The same program is built and run with
-fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "host", "nttplan.cpp")] + \
       [os.path.join(CSRC, f) for f in ("prover_plan.cpp", "poseidon_host.cpp", "witness_sched.cpp", "zkey.cpp")]
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC]


@pytest.fixture(scope="module")
def nttplan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nttplan") / "nttplan")
    subprocess.check_call(["g++", "-O2"] + FLAGS + SRCS + ["-o", exe, "-lpthread"])
    return exe


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.endswith(" 0 failed"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(last.split()[0]) > 500
    return r


def test_the_pass_list_covers_every_level_once_and_its_replay_equals_the_definition(nttplan):
    _run(nttplan)


def _list(exe, logn):
    out = subprocess.run([exe, "list", str(logn)], capture_output=True, text=True, timeout=60, check=True).stdout
    return [(k, int(a), int(b)) for k, a, b in (ln.split() for ln in out.strip().splitlines())]


def test_thirteen_levels_are_nine_launches_and_twelve_are_seven(nttplan):
    assert _list(nttplan, 13) == [("dif", 3, 0), ("dif", 3, 3), ("dif", 3, 6), ("dif", 3, 9), ("turn", 1, 12),
                                  ("dit", 3, 1), ("dit", 3, 4), ("dit", 3, 7), ("dit", 3, 10)]
    assert _list(nttplan, 12) == [("dif", 3, 0), ("dif", 3, 3), ("dif", 3, 6), ("turn", 3, 9),
                                  ("dit", 3, 3), ("dit", 3, 6), ("dit", 3, 9)]
    assert _list(nttplan, 11) == [("dif", 3, 0), ("dif", 3, 3), ("dif", 3, 6), ("turn", 2, 9),
                                  ("dit", 3, 2), ("dit", 3, 5), ("dit", 3, 8)]


@pytest.mark.parametrize("logn", [1, 2, 3])
def test_a_transform_of_at_most_three_levels_is_the_turn_alone(nttplan, logn):
    assert _list(nttplan, logn) == [("turn", logn, 0)]
    assert _list(nttplan, 0) == []


def test_the_same_program_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "nttplan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer"] + FLAGS + SRCS + ["-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
