"""The member directory on the device (rlnamd_directory_*, zerokit_amd.batch.MemberDirectory), judged by the model of
tests/member_directory_cases.py: a dict from leaf index to (identity commitment, limit), written from the contract alone,
with leaves from oracle/c's Poseidon and roots from tests/tree_model.TreeModel."""
import ctypes as C
import random

import pytest

import member_directory_cases as cases
from member_directory_cases import FOUND, KNOWN, NO_INDEX, OCCUPIED, OK, R, REMOVED, SKIPPED, UNKNOWN, VACANT

pytestmark = pytest.mark.gpu


def pack(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def pair(depth, capacity=None, seed=1):
    """a fresh tree with a directory over it, and the model of both"""
    from zerokit_amd.batch import MemberDirectory, PoseidonTree
    tree = PoseidonTree(depth)
    return tree, MemberDirectory(tree, capacity, seed), cases.Model(depth, capacity)


def same_state(d, tree, m, indices):
    assert d.get(indices) == m.get(indices)
    assert d.info()[1] == m.live()
    assert tree.root() == m.root()


def small_requests():
    mem, indices = cases.small()
    return [(i, x[1], x[2]) for i, x in zip(indices, mem)]


# --------------------------------------------------------------------------------------------------- 1. register
def test_twenty_members_at_scattered_indices():
    tree, d, m = pair(5, 32)
    reqs = small_requests()
    assert d.register(reqs) == m.register(reqs) == [OK] * 20
    same_state(d, tree, m, list(range(32)) + [reqs[0][0]] * 2)
    leaves = cases.rate_commitments([(r[1], r[2]) for r in reqs])
    assert [tree.get(r[0]) for r in reqs] == leaves
    assert d.info()[:5] == [32, 20, 64, 20, 0] and d.info()[6] == 1
    idcs = [r[1] for r in reqs] + [5, R - 1, R]            # (>= r is never live: UNKNOWN)
    assert d.find(idcs) == m.find(idcs)
    d.close()
    tree.close()


def test_one_call_that_meets_every_status_in_three_shuffles():
    first, second, want, _ = cases.every_status()
    outcomes = []
    for shuffle in (None, 1, 2, 3):
        reqs = list(second)
        if shuffle:
            random.Random(shuffle).shuffle(reqs)
        tree, d, m = pair(5)
        assert d.register(list(first)) == m.register(list(first)) == [OK] * 3
        got = d.register(reqs)
        assert got == m.register(reqs)
        assert dict(zip(reqs, got)) == dict(zip(second, want))
        same_state(d, tree, m, list(range(32)))
        outcomes.append((d.get(list(range(32))), tree.root()))
        d.close()
        tree.close()
    assert all(o == outcomes[0] for o in outcomes)


@pytest.fixture(scope="module")
def big_model():
    """the model after the 5 000 requests in one call -> (statuses, model)"""
    m = cases.Model(13)
    status = m.register(list(cases.big()))
    m.root()
    return status, m


def test_five_thousand_requests_in_one_call(big_model):
    reqs = list(cases.big())
    want, m = big_model
    assert reqs[0][1] == reqs[-1][1] and reqs[1][1] == reqs[-2][1]       # equal keys in the first and the last workgroup
    assert 300 <= want.count(KNOWN) <= 700 and want.count(OCCUPIED) == 0
    tree, d, _ = pair(13, seed=3)
    assert d.register(reqs) == want
    same_state(d, tree, m, [r[0] for r in reqs])
    info = d.info()
    assert info[1] == info[3] == want.count(OK) and info[4] == 0 and 1 <= info[5] <= info[2]
    idcs = [r[1] for r in reqs[::9]]
    assert d.find(idcs) == m.find(idcs)
    d.close()
    tree.close()


@pytest.mark.parametrize("chunk", [1, 63, 64, 65, 257])
def test_the_same_set_split_into_calls(chunk):
    reqs = list(cases.big())
    tree, d, m = pair(13, seed=3)
    for o in range(0, len(reqs), chunk):
        assert d.register(reqs[o:o + chunk]) == m.register(reqs[o:o + chunk]), o
    same_state(d, tree, m, [r[0] for r in reqs])
    d.close()
    tree.close()


# ---------------------------------------------------------------------------------------------- 2. resolve, slash
def test_resolve_live_removed_and_unknown_secrets_and_the_take_mask():
    mem, indices = cases.small()
    tree, d, m = pair(5, 32)
    reqs = small_requests()
    assert d.register(reqs) == m.register(reqs)
    gone = [indices[4], indices[9]]
    assert d.remove(gone) == m.remove(gone) == [REMOVED] * 2
    secrets = [mem[0][0], mem[4][0], 424242, mem[7][0], mem[9][0], mem[19][0]]
    got = d.resolve(secrets)
    assert got == m.resolve(secrets) and got[0] == [FOUND, UNKNOWN, UNKNOWN, FOUND, UNKNOWN, FOUND]
    assert got[1][0] == indices[0] and got[2][0] == mem[0][2] and got[1][1] == NO_INDEX and got[2][1] == 0
    take = [1, 0, 1, 0, 1, 1]
    got = d.resolve(secrets, take)
    assert got == m.resolve(secrets, take) and got[0] == [FOUND, SKIPPED, UNKNOWN, SKIPPED, UNKNOWN, FOUND]
    assert d.resolve([R, mem[0][0]], [0, 1]) == m.resolve([R, mem[0][0]], [0, 1])      # not taken: not read
    assert d.info()[7] == 0
    # a non-canonical secret refuses the call: state, root and the staging as they were
    from zerokit_amd._native import RLNError
    before = (d.get(list(range(32))), tree.root(), d.info()[1], d.info()[7])
    for call in (d.resolve, d.slash):
        with pytest.raises(RLNError) as e:
            call([mem[0][0], R + 3, mem[7][0]])
        assert str(e.value) == cases.resolve_refusal(call.__name__, [mem[0][0], R + 3])
        assert (d.get(list(range(32))), tree.root(), d.info()[1], d.info()[7]) == before and before[3] == 0
    same_state(d, tree, m, list(range(32)))
    d.close()
    tree.close()


def test_slash_of_64_secrets_and_reregistration():
    tree, d, m = pair(7, 100)
    tree2, twin, _ = pair(7, 100)
    mem = cases.members(90, 64)
    reqs = [(i, x[1], x[2]) for i, x in enumerate(mem)]
    for impl in (d, twin, m):
        assert impl.register(reqs) == [OK] * 90
    rnd = random.Random(64)
    secrets = [x[0] for x in rnd.sample(mem, 60)]
    secrets += [secrets[0], secrets[1], secrets[2], 987654321]            # three pairs naming one member each, one unknown
    rnd.shuffle(secrets)
    assert len(secrets) == 64
    got = d.slash(secrets)
    assert got == m.slash(secrets) and got[3] == 60 and got[0].count(UNKNOWN) == 1
    assert d.info()[7] == 0
    same_state(d, tree, m, list(range(100)))
    found = sorted({i for s, i in zip(got[0], got[1]) if s == FOUND})
    assert [tree.get(i) for i in found] == [0] * 60
    # the same as resolve + remove of the distinct found indices, on a twin
    assert twin.resolve(secrets) == got[:3]
    assert twin.remove(found) == [REMOVED] * 60
    assert twin.get(list(range(100))) == d.get(list(range(100))) and tree2.root() == tree.root()
    assert twin.info()[1] == d.info()[1] == 30 and twin.info()[3] == d.info()[3] == 90
    # a removed commitment comes back at the same index and at another one, and resolve finds the new index
    a, b = found[0], found[1]
    again = [(a, mem[a][1], 7), (found[2], mem[b][1], 9)]
    assert d.register(again) == m.register(again) == [OK, OK]
    got = d.resolve([mem[a][0], mem[b][0], mem[found[2]][0]])
    assert got == m.resolve([mem[a][0], mem[b][0], mem[found[2]][0]]) == ([FOUND, FOUND, UNKNOWN], [a, found[2], NO_INDEX], [7, 9, 0])
    assert d.slash([]) == ([], [], [], 0) and d.remove([]) == []
    same_state(d, tree, m, list(range(100)))
    for x in (d, twin, tree, tree2):
        x.close()


def test_churn_needs_the_rebuild():
    """capacity 8, 16 slots: 40 rounds fill and empty the directory.  A removed member's slot is not handed out again, so
    without the rebuild the second round's walks find no empty slot."""
    tree, d, m = pair(5, 8)
    for reqs in cases.churn_rounds():
        assert d.register(reqs) == m.register(reqs) == [OK] * 8
        info = d.info()
        assert info[3] <= info[2] // 2 and info[2] == 16
        idcs = [r[1] for r in reqs]
        assert d.find(idcs + [3]) == m.find(idcs + [3])
        assert d.remove(list(range(8))) == m.remove(list(range(8))) == [REMOVED] * 8
        assert d.info()[3] <= 8 and d.find(idcs)[0] == [UNKNOWN] * 8
    assert d.info()[4] >= 1 and d.info()[1] == 0 and d.remove([0, 7]) == [VACANT] * 2
    same_state(d, tree, m, list(range(8)))
    d.close()
    tree.close()


# ------------------------------------------------------------------------------------------- 3. with the log, restart
def test_spam_secrets_of_the_log_go_straight_into_slash():
    import nullifier_log_cases as lc
    from zerokit_amd.batch import NullifierLog
    shares, tags, a0 = lc.stream()
    want = lc.expected()
    n = 512
    owners = sorted(set(a0[:n]))
    idcs = cases.commitments(owners)
    tree, d, m = pair(10)
    reqs = [(2 * k + 1, idc, 20) for k, idc in enumerate(idcs)]
    assert d.register(reqs) == m.register(reqs) == [OK] * len(owners)
    where = {s: r[0] for s, r in zip(owners, reqs)}
    # two shares of one member first
    j = next(i for i in range(n) if want[i][0] == lc.SPAM)
    i = next(k for k in range(j) if shares[k][0] == shares[j][0])
    log = NullifierLog(2 * n)
    status, secrets, _ = log.observe_raw(lc.pack([shares[i], shares[j]]))
    assert list(status) == [lc.NEW, lc.SPAM]
    got = d.slash_raw(secrets, [s == lc.SPAM for s in status])
    assert got == m.slash([0, a0[j]], [0, 1]) == ([SKIPPED, FOUND], [NO_INDEX, where[a0[j]]], [0, 20], 1)
    # then a batch, the step's outputs unchanged
    log.clear()
    status, secrets, _ = log.observe_raw(lc.pack(shares[:n]), tags[:n])
    take = [s == lc.SPAM for s in status]
    assert sum(take) >= 10
    got = d.slash_raw(secrets, take)
    ints = [int.from_bytes(secrets[32 * k:32 * k + 32], "little") for k in range(n)]
    assert got == m.slash(ints, take) and got[3] >= 5
    assert all(where[a0[k]] == got[1][k] for k in range(n) if got[0][k] == FOUND)
    assert d.info()[7] == 0
    same_state(d, tree, m, [r[0] for r in reqs])
    for x in (log, d, tree):
        x.close()


def test_a_restart_registers_the_same_events_again():
    from zerokit_amd.batch import MemberDirectory
    tree, d, m = pair(5, 32)
    reqs = small_requests()
    assert d.register(reqs) == m.register(reqs)
    root = tree.root()
    d.close()
    again = MemberDirectory(tree, 32, seed=9)            # over a tree that holds leaves: empty
    assert again.info()[1] == 0 and again.get([reqs[0][0]]) == [(False, 0, 0)] and again.find([reqs[0][1]])[0] == [UNKNOWN]
    assert again.register(reqs) == [OK] * 20 and tree.root() == root == m.root()
    same_state(again, tree, m, list(range(32)))
    again.close()
    tree.close()


def test_the_seed_moves_walks_never_a_status():
    reqs = [(i, r[1], r[2]) for i, r in enumerate(cases.big()[:2000])]
    want = cases.Model(11).register(reqs)
    walks = set()
    for seed in (1, 2, 3, 4, 5, 6):
        tree, d, _ = pair(11, seed=seed)
        assert d.register(reqs) == want
        walks.add(d.info()[5])
        d.close()
        tree.close()
    assert len(walks) > 1 and all(1 <= w <= 1 << 12 for w in walks)


# ------------------------------------------------------------------------------------------------------ 4. refusals
def test_each_refusal_leaves_root_and_members_as_they_were():
    from zerokit_amd._native import RLNError, last_error, lib
    tree, d, m = pair(5, 24)
    reqs = [r for r in small_requests() if r[0] < 24]
    assert d.register(reqs) == m.register(reqs)
    before = (tree.root(), d.info()[1], d.get(list(range(24))))
    free = next(i for i in range(24) if i not in m.rows)
    refused = [
        [(24, 1, 1)],                                   # an index >= capacity (inside the tree, outside the directory)
        [(free, 1, 1), (2, 2, 1), (free, 3, 1)],        # an index twice
        [(free, R, 1)],                                 # an identity commitment >= r
        [(free, 1, 1), (23 if free != 23 else 22, 2, 0)],   # a limit of 0
    ]
    for members in refused:
        with pytest.raises(RLNError) as e:
            d.register(members)
        assert str(e.value) == cases.register_refusal(members, 24) != ""
        assert (tree.root(), d.info()[1], d.get(list(range(24)))) == before
    for indices in ([24], [3, 3]):
        with pytest.raises(RLNError) as e:
            d.remove(indices)
        assert str(e.value) == cases.indices_refusal("remove", indices, 24) != ""
    with pytest.raises(RLNError) as e:
        d.get([0, 24])
    assert str(e.value) == cases.indices_refusal("get", [0, 24], 24, False)
    st, ix, lm = C.create_string_buffer(4), (C.c_uint64 * 4)(), (C.c_uint32 * 4)()
    assert lib().rlnamd_directory_register(d._h, 1, None, pack([1]), (C.c_uint32 * 1)(1), st) != 0
    assert last_error() == cases.null_refusal("register")
    assert lib().rlnamd_directory_resolve(d._h, 1, pack([1]), None, None, ix, lm) != 0
    assert last_error() == cases.null_refusal("resolve", "secrets")
    assert lib().rlnamd_directory_slash(d._h, 1, None, None, st, ix, lm, None) != 0
    assert last_error() == cases.null_refusal("slash", "secrets")
    assert lib().rlnamd_directory_remove(d._h, 1, None, st) != 0 and last_error() == cases.null_refusal("remove")
    from zerokit_amd.batch import MemberDirectory
    for capacity in (0, 33):
        with pytest.raises(RLNError) as e:
            MemberDirectory(tree, capacity)
        assert str(e.value) == cases.new_refusal(capacity, 5) != ""
    assert (tree.root(), d.info()[1], d.get(list(range(24)))) == before and d.info()[7] == 0
    same_state(d, tree, m, list(range(24)))
    d.close()
    tree.close()
