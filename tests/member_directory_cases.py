"""The cases and the model that tests/test_member_directory_host.py (CPU build of member_directory.h) and
tests/test_gpu_member_directory.py (the device directory) judge by.

The model is written from the contract alone (include/rln_amd.h, "member directory"): a dict from leaf index to
(identity commitment, limit), leaves from oracle/c's Poseidon, roots from tests/tree_model.TreeModel.  It knows nothing of
tables, slots, walks or passes."""
import functools
import random

from oracle.c import binding as ob

from tree_model import TreeModel

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OK, OCCUPIED, KNOWN = range(3)
FOUND, UNKNOWN, SKIPPED = range(3)
REMOVED, VACANT = range(2)
NO_INDEX = (1 << 64) - 1
MAX_CAPACITY = 1 << 31


class Refused(Exception):
    pass


def commitments(secrets):
    """Poseidon(secret), t = 2"""
    return ob.poseidon_batch([[s] for s in secrets]) if secrets else []


def rate_commitments(pairs):
    """Poseidon(idc, limit), t = 3"""
    return ob.poseidon_batch([[idc, limit] for idc, limit in pairs]) if pairs else []


# ------------------------------------------------------------------------------------------------ refusal texts
def new_refusal(capacity, depth):
    if capacity == 0:
        return "member directory: the capacity must be at least 1"
    if capacity > MAX_CAPACITY:
        return "member directory: the capacity must be at most 2^31 leaves"
    if capacity > 1 << depth:
        return "member directory: a capacity of %d is more than the 2^%d leaves of the tree" % (capacity, depth)
    return ""


def indices_refusal(call, indices, capacity, distinct=True):
    for i, index in enumerate(indices):
        if index >= capacity:
            return "member directory: index %d of request %d of the %s is outside a directory of %d leaves" % (index, i, call, capacity)
    if distinct:
        seen = sorted(indices)
        for a, b in zip(seen, seen[1:]):
            if a == b:
                return "member directory: index %d occurs twice in the %s" % (a, call)
    return ""


def null_refusal(call, what="requests"):
    return "member directory: %s was given a null pointer for n > 0 %s" % (call, what)


def register_refusal(members, capacity):
    bad = indices_refusal("register", [m[0] for m in members], capacity)
    if bad:
        return bad
    for i, m in enumerate(members):
        if m[1] >= R:
            return "member directory: identity commitment %d of the register is not canonical (>= r)" % i
    for i, m in enumerate(members):
        if m[2] == 0:
            return "member directory: request %d of the register has a limit of 0" % i
    return ""


def resolve_refusal(call, secrets, take=None):
    for i, s in enumerate(secrets):
        if (take is None or take[i]) and s >= R:
            return "member directory: secret %d of the %s is not canonical (>= r)" % (i, call)
    return ""


# ------------------------------------------------------------------------------------------------------ the model
class Model:
    def __init__(self, depth, capacity=None, tree=None):
        self.capacity = min(1 << depth, MAX_CAPACITY) if capacity is None else capacity
        self.tree = TreeModel(depth) if tree is None else tree
        self.rows = {}            # index -> (idc, limit): the LIVE ones
        self.where = {}           # idc -> index, for the same rows (kept beside them: a call of one request stays cheap)
        self._pending = {}        # leaves not yet written into the tree model: root() writes them, the last value of each

    def _write(self, updates):
        self._pending.update(updates)

    def register(self, members):
        """[(index, idc, limit)] -> [status]; a set of requests: nothing below looks at their order"""
        refused = register_refusal(members, self.capacity)
        if refused:
            raise Refused(refused)
        live_before = self.where
        free = [m for m in members if m[0] not in self.rows]
        lowest = {}
        for index, idc, _ in free:
            lowest[idc] = min(index, lowest.get(idc, index))
        status, new = [], {}
        for index, idc, limit in members:
            if index in self.rows:
                status.append(OCCUPIED)
            elif idc in live_before or lowest[idc] != index:
                status.append(KNOWN)
            else:
                status.append(OK)
                new[index] = (idc, limit)
        leaves = rate_commitments([new[i] for i in sorted(new)])
        self.rows.update(new)
        self.where.update({idc: index for index, (idc, _) in new.items()})
        self._write(dict(zip(sorted(new), leaves)))
        return status

    def find(self, idcs):
        status, index, limit = [], [], []
        for idc in idcs:
            at = self.where.get(idc)
            hit = None if at is None else (at, self.rows[at][1])
            status.append(FOUND if hit else UNKNOWN)
            index.append(hit[0] if hit else NO_INDEX)
            limit.append(hit[1] if hit else 0)
        return status, index, limit

    def resolve(self, secrets, take=None, call="resolve"):
        refused = resolve_refusal(call, secrets, take)
        if refused:
            raise Refused(refused)
        taken = [i for i in range(len(secrets)) if take is None or take[i]]
        st, ix, lm = self.find(commitments([secrets[i] for i in taken]))
        status, index, limit = [SKIPPED] * len(secrets), [NO_INDEX] * len(secrets), [0] * len(secrets)
        for k, i in enumerate(taken):
            status[i], index[i], limit[i] = st[k], ix[k], lm[k]
        return status, index, limit

    def remove(self, indices):
        refused = indices_refusal("remove", indices, self.capacity)
        if refused:
            raise Refused(refused)
        status = [REMOVED if i in self.rows else VACANT for i in indices]
        gone = {i: 0 for i in indices if i in self.rows}
        for i in gone:
            del self.where[self.rows.pop(i)[0]]
        self._write(gone)
        return status

    def slash(self, secrets, take=None):
        status, index, limit = self.resolve(secrets, take, "slash")
        found = sorted({ix for st, ix in zip(status, index) if st == FOUND})
        self.remove(found)
        return status, index, limit, len(found)

    def get(self, indices):
        refused = indices_refusal("get", indices, self.capacity, distinct=False)
        if refused:
            raise Refused(refused)
        return [(True,) + self.rows[i] if i in self.rows else (False, 0, 0) for i in indices]

    def live(self):
        return len(self.rows)

    def root(self):
        if self._pending:
            self.tree.set_leaves(sorted(self._pending.items()))
            self._pending = {}
        return self.tree.root()


# ------------------------------------------------------------------------------------------------------ the cases
def members(n, seed, limit_max=1000):
    """n secrets with their commitments and limits -> [(secret, idc, limit)]"""
    rnd = random.Random(seed)
    secrets = [rnd.randrange(1, R) for _ in range(n)]
    return list(zip(secrets, commitments(secrets), [rnd.randrange(1, limit_max) for _ in range(n)]))


@functools.lru_cache(maxsize=None)
def small():
    """depth 5, capacity 32: 20 members at scattered indices -> (members, indices)"""
    rnd = random.Random(505)
    return tuple(members(20, 5)), tuple(rnd.sample(range(32), 20))


@functools.lru_cache(maxsize=None)
def every_status(depth=5):
    """-> (first call, second call, what the second must answer, members).  The second call meets, against the first:
    OCCUPIED; KNOWN against the earlier call; KNOWN among its own duplicates, where the lowest index wins; OCCUPIED taking
    precedence over KNOWN; and an OCCUPIED request that does not block its commitment at a free index."""
    m = members(12, 77)
    idc, lim = [x[1] for x in m], [x[2] for x in m]
    first = [(3, idc[0], lim[0]), (9, idc[1], lim[1]), (17, idc[2], lim[2])]
    second = [
        (3, idc[3], 5),        # OCCUPIED: index 3 is live ... and its commitment goes in below, at a free index
        (20, idc[3], 6),       # OK: the OCCUPIED request above does not block it
        (4, idc[1], 7),        # KNOWN against the earlier call
        (9, idc[2], 8),        # OCCUPIED takes precedence over KNOWN (index live AND commitment live)
        (30, idc[4], 9),       # KNOWN: a duplicate inside the call, the lowest index (11) wins
        (11, idc[4], 10),      # OK
        (25, idc[4], 11),      # KNOWN
        (0, idc[5], 12),       # OK
        (31, idc[6], 13),      # OK: the last index
    ]
    want = [OCCUPIED, OK, KNOWN, OCCUPIED, KNOWN, OK, KNOWN, OK, OK]
    return tuple(first), tuple(second), tuple(want), tuple(m)


@functools.lru_cache(maxsize=None)
def big(depth=13, n=5000, seed=1313):
    """5 000 requests at distinct indices of a depth-13 tree, about 10 % duplicate commitments; request 0 and request
    n - 1 carry one commitment, and so do request 1 and request n - 2: equal keys in the first and the last workgroup."""
    rnd = random.Random(seed)
    fresh = members(n - n // 10, seed)
    idcs = [m[1] for m in fresh] + [rnd.choice(fresh)[1] for _ in range(n // 10)]
    rnd.shuffle(idcs)
    idcs[n - 1], idcs[n - 2] = idcs[0], idcs[1]
    indices = rnd.sample(range(1 << depth), n)
    return tuple((indices[i], idcs[i], rnd.randrange(1, 1 << 32)) for i in range(n))


def duplicate_heavy(n=4000, seed=4242, depth=12):
    """n requests over n // 8 commitments: every key eight times on average, for the threaded run"""
    rnd = random.Random(seed)
    pool = [rnd.randrange(1, R) for _ in range(n // 8)]
    indices = rnd.sample(range(1 << depth), n)
    return [(indices[i], rnd.choice(pool), rnd.randrange(1, 99)) for i in range(n)]


def churn_rounds(rounds=40, capacity=8, seed=88):
    """`rounds` x (capacity fresh commitments at all the indices, then all of them removed)"""
    rnd = random.Random(seed)
    return [[(i, rnd.randrange(1, R), rnd.randrange(1, 50)) for i in range(capacity)] for _ in range(rounds)]


def compare_register(model, impl, reqs):
    assert impl.register(reqs) == model.register(reqs)


def compare_state(model, impl, indices):
    assert impl.get(indices) == model.get(indices)
    assert impl.info()[1] == model.live()
