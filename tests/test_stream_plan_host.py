"""stream_plan (zerokit_amd/csrc/prover_plan.cpp) without a GPU: which stream every role of a big batch takes for 1, 2, 4,
7, 8 and 32 hardware queues and 2 .. 6 workspace slots.  tests/host/streamplan.cpp is a program of its own (it can be built
with -fsanitize=address,undefined and run as it is); it checks that `wide` is the map of eight streams, that `compact`
keeps at most four busy, that the walks share a stream neither with each other nor with a front end, that every consumer
follows its producer in stream order or needs an event, that a slot's wipe and the slot's next batch are ordered, and
that a replay of nslot + 3 batches -- submission order per stream plus the events, as a graph on the host -- has no cyclic
wait."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerokit_amd", "csrc")


@pytest.fixture(scope="module")
def streamplan():
    exe = os.path.join(ROOT, "tests", "host", "streamplan")
    srcs = [os.path.join(ROOT, "tests", "host", "streamplan.cpp")] + \
           [os.path.join(CSRC, f) for f in ("prover_plan.cpp", "poseidon_host.cpp", "witness_sched.cpp", "zkey.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("prover_plan.h", "prover_desc.h", "prover.h", "tree_config.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC] +
                              srcs + ["-o", exe])
    return exe


def test_every_plan_keeps_its_invariants_and_replays_without_a_cyclic_wait(streamplan):
    r = subprocess.run([streamplan], capture_output=True, text=True, timeout=120)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.endswith(" 0 failed"), r.stdout[-4000:] + r.stderr[-2000:]
    assert int(last.split()[0]) > 1000


def _dump(exe, queues, nslot):
    out = subprocess.run([exe, "dump", str(queues), str(nslot)], capture_output=True, text=True, timeout=60, check=True).stdout
    lines = out.strip().splitlines()
    head = dict(zip(lines[0].split()[0::2], lines[0].split()[1::2]))
    at = {(int(p), role): st for p, role, st in (ln.split() for ln in lines[1:])}
    return head, at


def test_wide_is_the_map_of_eight_streams_and_auto_takes_it_from_eight_queues(streamplan):
    for queues in (8, 32):
        head, at = _dump(streamplan, queues, 5)
        assert head["shape"] == "wide" and head["values_front"] == "0"
        for p, interp in ((0, "sA"), (1, "sAb")):
            assert [at[p, r] for r in ("interp", "values", "quotient", "walk1", "walk2", "sums1", "sums2", "wipe")] == \
                [interp, "sV", "sA2", "sB", "sB2", "sC", "sC", "sW"]


@pytest.mark.parametrize("queues", [4, 7])
@pytest.mark.parametrize("nslot", [2, 3, 4, 5, 6])
def test_auto_takes_compact_where_its_four_streams_fit_the_queues(streamplan, queues, nslot):
    head, at = _dump(streamplan, queues, nslot)
    assert head["shape"] == "compact" and head["values_front"] == "1"
    busy = {st for (p, role), st in at.items() if role != "wipe"}
    assert len(busy) == int(head["busy"]) == 4 <= queues
    walks = {at[0, "walk1"], at[0, "walk2"]}
    fronts = {at[p, r] for p in (0, 1) for r in ("interp", "values", "quotient")}
    assert len(walks) == 2 and len(fronts) == 2 and not walks & fronts
    # a slot's wipe sits on the stream of the batch that takes the slot next, nslot batches later
    for p in (0, 1):
        assert at[p, "wipe"] == at[(p + nslot) & 1, "interp"]
        assert at[p, "sums1"] == at[p, "walk1"] and at[p, "sums2"] == at[p, "walk2"]


@pytest.mark.parametrize("queues", [1, 2, 3])
def test_auto_keeps_the_wide_map_below_four_queues(streamplan, queues):
    """no map with both walks and a front end on streams of their own fits fewer than four queues: auto leaves such a
    process what it had, and never picks a shape whose busy streams outnumber the queues where one fits"""
    head, at = _dump(streamplan, queues, 5)
    assert head["shape"] == "wide" and head["values_front"] == "0"


def _fields(exe, *a):
    lines = subprocess.run([exe, "shape"] + [str(v) for v in a], capture_output=True, text=True, timeout=60,
                           check=True).stdout.strip().splitlines()
    first = lines[0].split()
    return dict(zip(first[0::2], (int(v) for v in first[1::2]))), int(lines[1].split()[-1])


def test_batch_shape_says_where_the_public_values_come_from(streamplan):
    """values_front: big batches of a compact prover, full and finish -- and partial only where the batch reads the
    circuit's outputs anyway (values_w: alone on the device, the lanes = nodes interpreter); never the small shapes, the wide
    map or a circuit without the values kernel"""
    FULL, PARTIAL, FINISH = 0, 1, 2
    for n in (129, 1024):
        for mode in (FULL, FINISH):
            for idle in (0, 1):
                s, multi = _fields(streamplan, n, mode, idle, 1)
                assert s["values_front"] == 1 and s["small"] == 0 and multi == 0, (n, mode, idle)
                assert _fields(streamplan, n, mode, idle, 0)[0]["values_front"] == 0
        s, _ = _fields(streamplan, n, PARTIAL, 0, 1)
        assert s["values_front"] == 0 and s["values_w"] == 0
        s, _ = _fields(streamplan, n, PARTIAL, 1, 1)
        assert s["values_front"] == 1 and s["values_w"] == 1
    for n in (1, 128):
        s, _ = _fields(streamplan, n, FULL, 0, 1)
        assert s["small"] == 1 and s["values_w"] == 1 and s["values_front"] == 0


def test_the_config_key_names_the_shape_or_is_refused(streamplan):
    def cfg(js):
        return subprocess.run([streamplan, "config", js], capture_output=True, text=True, timeout=60, check=True).stdout.strip()
    assert cfg('{"stream_shape": "auto"}') == "stream_shape 0"
    assert cfg('{"stream_shape": "wide"}') == "stream_shape 1"
    assert cfg('{"stream_shape": "compact", "max_batch": 64}') == "stream_shape 2"
    assert cfg('{"max_batch": 64}') == "stream_shape -1"          # the environment's switch, or auto
    assert cfg('{"stream_shape": "narrow"}') == \
        'error Configuration error: stream_shape: expected "auto", "wide" or "compact", got "narrow"'
