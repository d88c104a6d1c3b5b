"""The quota ledger's meaning as a Python dict model (zerokit_amd/csrc/quota_ledger.h states it; include/rln_amd.h:
rlnamd_quota_draw), and the cases the host text and the device are held to.  No GPU and no native code in here.

A case is a ledger shape and a list of steps; run() plays them on the model and on an implementation side by side and
compares every answer, the window and the counters of every (member, external nullifier) the case ever named."""
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OK, OVER, NO_EPOCH = range(3)
EPOCHS_MAX = 64
DEPTH_MAX = 24
U32 = (1 << 32) - 1


class Refused(Exception):
    pass


def new_refusal(depth, max_epochs):
    if not 1 <= depth <= DEPTH_MAX:
        return "quota ledger: the depth must be 1 .. 24, not %d" % depth
    if not 1 <= max_epochs <= EPOCHS_MAX:
        return "quota ledger: max_epochs must be 1 .. 64 (RLNAMD_RELAY_EPOCHS_MAX), not %d" % max_epochs
    return ""


class Model:
    """used: {(external nullifier, leaf): next id}; window: the external nullifiers in the order given, duplicates once.
    pointers=False plays a call whose pointers are null (the C layers' first refusal)."""

    def __init__(self, depth, max_epochs):
        assert new_refusal(depth, max_epochs) == ""
        self.depth, self.max_epochs = depth, max_epochs
        self.window, self.used = [], {}
        self.draws = self.issued = self.over = self.no_epoch = 0

    def epochs_refusal(self, exts, pointers=True):
        k = len(exts)
        if k == 0:
            return ""
        if not pointers:
            return "quota ledger: set_epochs was given a null pointer for k > 0 external nullifiers"
        if k > self.max_epochs:
            return "quota ledger: a window holds at most %d external nullifiers (max_epochs), not %d" % (self.max_epochs, k)
        for j, e in enumerate(exts):
            if e >= R:
                return "quota ledger: external nullifier %d of set_epochs is not canonical (>= r)" % j
        return ""

    def set_epochs(self, exts, pointers=True):
        text = self.epochs_refusal(exts, pointers)
        if text:
            raise Refused(text)
        self.window = list(dict.fromkeys(exts))
        self.used = {k: v for k, v in self.used.items() if k[0] in self.window}   # what leaves loses its counters

    def draw_refusal(self, leaves, pointers=True):
        n = len(leaves)
        if n == 0:
            return ""
        if not pointers:
            return "quota ledger: draw was given a null pointer for n > 0 requests"
        if n >> 32:
            return "quota ledger: a draw takes fewer than 2^32 requests, not %d" % n
        for i, leaf in enumerate(leaves):
            if leaf >> self.depth:
                return "quota ledger: leaf index %d of request %d is outside a ledger of depth %d" % (leaf, i, self.depth)
        return ""

    def draw(self, leaves, exts, limits, pointers=True):
        """the closed form: rank among the call's earlier requests with the same key, whatever became of them"""
        text = self.draw_refusal(leaves, pointers)
        if text:
            raise Refused(text)
        ids, status, rank, highest = [], [], {}, {}
        for leaf, ext, limit in zip(leaves, exts, limits):
            if ext not in self.window:
                ids.append(limit)
                status.append(NO_EPOCH)
                self.no_epoch += 1
                continue
            key = (ext, leaf)
            r = rank.get(key, 0)
            rank[key] = r + 1
            ident = self.used.get(key, 0) + r     # `used` is not written before the loop ends: as it was before the call
            if ident < limit:
                ids.append(ident)
                status.append(OK)
                highest[key] = max(highest.get(key, -1), ident)
                self.issued += 1
            else:
                ids.append(limit)
                status.append(OVER)
                self.over += 1
        for key, h in highest.items():
            self.used[key] = h + 1
        if leaves:
            self.draws += 1
        return ids, status

    def draw_one_by_one(self, leaves, exts, limits):
        """drawing in index order, a call a request: what the closed form must equal with one limit per member"""
        ids, status = [], []
        for leaf, ext, limit in zip(leaves, exts, limits):
            i, s = self.draw([leaf], [ext], [limit])
            ids += i
            status += s
        return ids, status


# ------------------------------------------------------------------------------------------------------ the cases
E1, E2, E3, E4, OUTSIDE = 1001, R - 1, 1 << 200, 77, 31337


def _distinct(n, depth):
    rnd = random.Random(n)
    leaves = rnd.sample(range(1 << depth), n) if n <= (1 << depth) else None
    return leaves


def draw_shapes(n, depth=20):
    """the draws every size is put through, on one ledger in this order: [(leaves, exts, limits)]"""
    rnd = random.Random(1000 + n)
    last = (1 << depth) - 1
    out = []
    if n <= (1 << depth):
        out.append((_distinct(n, depth), [E1] * n, [5] * n))                               # all distinct
    out.append(([last] * n, [E2] * n, [n // 2] * n))                                         # one member, limit < n
    few = [0, last] + [rnd.randrange(1 << depth) for _ in range(5)]
    limit_of = {leaf: rnd.choice([0, 1, 3, U32]) for leaf in few}
    limit_of[0], limit_of[last] = 3, U32
    who = [rnd.choice(few) for _ in range(n)]
    out.append((who, [rnd.choice([E1, E2, E3, OUTSIDE]) for _ in range(n)], [limit_of[w] for w in who]))   # interleaved epochs
    out.append((who, [rnd.choice([E1, E2]) for _ in range(n)], [limit_of[w] for w in who]))                # the same members again
    return out


def two_limits():
    """one member under two limits, in both orders: ids may be skipped, none is issued twice"""
    return [([7] * 6, [E1] * 6, [1, 5, 1, 5, 5, 1]), ([9] * 6, [E1] * 6, [5, 1, 5, 1, 1, 5]),
            ([7] * 4, [E1] * 4, [9, 2, 9, 2]), ([9] * 4, [E1] * 4, [2, 9, 2, 9])]


def split_sequences(n, count, seed):
    """request sequences with one limit per member, members repeating, an epoch outside the window among them"""
    rnd = random.Random(seed)
    limit_of = {0: 0, 1: 1, 2: 2, 3: 4}
    for _ in range(count):
        who = [rnd.randrange(4) for _ in range(n)]
        yield who, [rnd.choice([E1, E1, E2, OUTSIDE]) for _ in range(n)], [limit_of[w] for w in who]


# ------------------------------------------------------------------------------------------------------ the runner
def compare_draw(model, impl, leaves, exts, limits):
    """impl.draw(leaves, exts, limits) -> (ids, statuses), impl.used(leaves, exts) -> [int | None]"""
    want = model.draw(leaves, exts, limits)
    got = impl.draw(leaves, exts, limits)
    assert got[1] == want[1], "statuses"
    assert got[0] == want[0], "ids"
    assert all(i == lim for i, s, lim in zip(got[0], got[1], limits) if s != OK)
    return got


def compare_counters(model, impl, keys):
    """keys: (external nullifier, leaf) pairs; None stands for "not in the window" """
    keys = sorted(set(keys))
    want = [model.used.get(k, 0) if k[0] in model.window else None for k in keys]
    assert impl.used([k[1] for k in keys], [k[0] for k in keys]) == want, "counters"
