"""Signals to field elements on the device (zerokit_amd/csrc/keccak_batch.hip: rlnamd_hasher_*, and the FFI calls over it,
ffi_hash_to_field_batch_le and ffi_verify_rln_signals_batch) against the oracle's Keccak and the single-message host
calls."""
import json

import pytest

from oracle.pyref.keccak import hash_to_field_le as o_htf

pytestmark = pytest.mark.gpu


def m(L):
    return bytes((L * 131 + j * 7 + (j >> 8)) & 0xff for j in range(L))


MESSAGES = [m(L) for L in range(410)]


@pytest.fixture(scope="module")
def oracle_410():
    return [o_htf(msg) for msg in MESSAGES]


@pytest.fixture(scope="module")
def hasher():
    from zerokit_amd.batch import Hasher
    h = Hasher()
    yield h
    h.close()


def test_410_messages_in_index_order(hasher, oracle_410):
    """lengths 0 .. 409 in one call on a default hasher: messages of 1 to 4 blocks share a wave"""
    assert hasher.hash_to_field(MESSAGES) == oracle_410
    info = hasher.info()
    assert (info["device_messages"], info["host_messages"], info["chunks"]) == (410, 0, 1)
    assert info["device_blocks"] == sum(L // 136 + 1 for L in range(410)) and info["longest_lane_blocks"] == 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_launch_tails(hasher, n):
    from zerokit_amd import hashers
    msgs = [k.to_bytes(2, "little") + bytes((k * 29 + j * 5 + 1) & 0xff for j in range(30)) for k in range(n)]
    assert len(set(msgs)) == n
    assert hasher.hash_to_field(msgs) == [hashers.hash_to_field_le(s) for s in msgs]


def test_long_message_among_short_ones():
    from zerokit_amd.batch import Hasher
    msgs = [m(L) for L in (5, 20000, 0, 408, 135)]
    want = [o_htf(s) for s in msgs]
    on_lane, on_host = Hasher(lane_max_blocks=1024), Hasher(lane_max_blocks=1)
    try:
        a = on_lane.hash_to_field(msgs)
        info = on_lane.info()
        assert (info["device_messages"], info["host_messages"], info["longest_lane_blocks"]) == (5, 0, 148)
        b = on_host.hash_to_field(msgs)
        info = on_host.info()
        assert (info["device_messages"], info["host_messages"], info["longest_lane_blocks"]) == (3, 2, 1)
        assert a == b == want
    finally:
        on_lane.close()
        on_host.close()


def test_chunks(hasher, oracle_410):
    from zerokit_amd.batch import Hasher
    small = Hasher(stage_bytes=2 * 16 * 136)
    try:
        assert small.info()["half_blocks"] == 16
        assert small.hash_to_field(MESSAGES) == hasher.hash_to_field(MESSAGES) == oracle_410
        info = small.info()
        assert info["chunks"] > 1 and (info["device_messages"], info["host_messages"]) == (410, 0)
        # 5 000 bytes are 37 blocks: more than a half holds
        big = m(5000)
        assert small.hash_to_field(MESSAGES[:200] + [big] + MESSAGES[200:]) == oracle_410[:200] + [o_htf(big)] + oracle_410[200:]
        info = small.info()
        assert (info["device_messages"], info["host_messages"]) == (410, 1) and info["longest_lane_blocks"] == 4
    finally:
        small.close()


def test_repeated_calls_and_an_empty_call(oracle_410):
    from zerokit_amd.batch import Hasher
    h = Hasher(stage_bytes=2 * 64 * 136)
    try:
        assert h.hash_to_field(MESSAGES) == oracle_410
        # smaller than the call before it, other lengths in other places: stale staging or stale first_block rows would show
        assert h.hash_to_field(MESSAGES[300:280:-1]) == oracle_410[300:280:-1]
        calls = h.info()["calls"]
        assert h.hash_to_field([]) == [] and h.hash_to_field_raw(b"", [0]) == b""
        assert h.info()["calls"] == calls and h.info()["device_messages"] == 20
        assert h.hash_to_field([b""]) == [o_htf(b"")]
    finally:
        h.close()


def test_refusals_leave_the_hasher_working(hasher, oracle_410):
    from zerokit_amd import RLNError
    with pytest.raises(RLNError) as down:
        hasher.hash_to_field_raw(bytes(8), [0, 5, 3])
    with pytest.raises(RLNError) as beyond:
        hasher.hash_to_field_raw(bytes(8), [0, 3, 9])
    assert "offsets decrease" in str(down.value) and "beyond data_len" in str(beyond.value)
    assert hasher.hash_to_field(MESSAGES[130:140]) == oracle_410[130:140]


def test_hash_to_field_many_is_the_loop():
    from zerokit_amd import hashers
    msgs = [m(3 * k) for k in range(100)]
    assert hashers.hash_to_field_many(msgs) == [hashers.hash_to_field_le(s) for s in msgs]
    assert hashers.hash_to_field_many([]) == []
    # 100 messages are below the default "hash_gpu_min" and stay on the calling thread: 300 go through the process's hasher
    msgs = [m((7 * k) % 300) for k in range(300)]
    assert hashers.hash_to_field_many(msgs) == [hashers.hash_to_field_le(s) for s in msgs]


def test_verify_rln_signals_batch(tmp_path):
    """ffi_verify_rln_signals_batch == ffi_verify_rln_proofs_batch with the xs hashed one by one -- own root, a roots
    window, an empty window -- with the signals hashed on the device ("hash_gpu_min": 0) and on the calling thread
    (1 000 000); one signal has a flipped byte, one message is empty"""
    from zerokit_amd import RLNError, hashers
    from zerokit_amd.public import RLN, RLNWitnessInput
    objs = []
    for k, gpu_min in enumerate((0, 1000000)):
        cfgp = tmp_path / ("cfg%d.json" % k)
        cfgp.write_text(json.dumps({"hash_gpu_min": gpu_min}))
        objs.append(RLN(20, tree_config=str(cfgp)))
    secret = hashers.hash_to_field_le(b"signals-batch-member")
    for obj in objs:
        obj.set_leaf(3, hashers.poseidon_hash_pair(hashers.poseidon_hash([secret]), 100))
    path = objs[0].get_merkle_proof(3)
    signals = [b"relay message %d " % i * (1 + 9 * i) for i in range(8)]
    signals[5] = b""
    xs = [hashers.hash_to_field_le(s) for s in signals]
    ws = [RLNWitnessInput(secret, 100, i, path[0], path[1], xs[i], 4242) for i in range(8)]
    proofs = objs[0].generate_rln_proofs_batch(ws, [(11 + i, 23 + i) for i in range(8)])
    root = proofs[0].values.root
    sent = list(signals)
    sent[2] = sent[2][:4] + bytes([sent[2][4] ^ 1]) + sent[2][5:]
    sent_xs = [hashers.hash_to_field_le(s) for s in sent]
    for roots in (None, [12345, root], []):
        want = objs[1].verify_rln_proofs_batch(proofs, sent_xs, roots)
        assert want == [i != 2 for i in range(8)]
        for obj in objs:
            assert obj.verify_rln_signals_batch(proofs, sent, roots) == want
    assert objs[0].verify_rln_signals_batch(proofs, signals) == [True] * 8
    assert objs[0].verify_rln_signals_batch(proofs, sent, [12345]) == [False] * 8
    assert objs[0].verify_rln_signals_batch([], []) == []
    for bad in (-2, 1000000001):
        cfgp = tmp_path / "bad.json"
        cfgp.write_text(json.dumps({"hash_gpu_min": bad}))
        with pytest.raises(RLNError, match="Configuration error: hash_gpu_min"):
            RLN(20, tree_config=str(cfgp))
