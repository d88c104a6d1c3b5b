"""The quota ledger's draw by count (zerokit_amd/csrc/quota_ledger.h: draw_counts; include/rln_amd.h:
rlnamd_quota_draw_counts) as a Python model beside the Model of tests/quota_cases.py, the cases the host text and the
device are held to, and a checker of the one invariant the ledger exists for -- the blocks of ids granted for a member
under an external nullifier are pairwise disjoint and lie below their limits -- that reads the granted (first, count)
pairs alone and none of the model's counters.  No GPU and no native code in here."""
import random

import quota_cases as cases
from quota_cases import E1, E2, E3, OUTSIDE, NO_EPOCH, OK, OVER, U32, Refused

COUNT_MAX = 255
COUNTS_N_MAX = 1 << 24


def count_refusal(i, count):
    if count == 0:
        return "quota ledger: request %d of draw_counts asks for no id (a count is 1 .. 255)" % i
    if count > COUNT_MAX:
        return "quota ledger: request %d of draw_counts asks for %d ids, more than 255" % (i, count)
    return ""


class CountsModel(cases.Model):
    """cases.Model with draw_counts: the closed form, a dict and a loop"""

    def draw_counts_refusal(self, leaves, counts, pointers=True, counts_pointer=True, n=None):
        n = len(leaves) if n is None else n
        if n == 0:
            return ""
        if not pointers:
            return "quota ledger: draw was given a null pointer for n > 0 requests"
        if not counts_pointer:
            return "quota ledger: draw_counts was given a null pointer for the counts of n > 0 requests"
        if n >= COUNTS_N_MAX:                      # before any array is read
            return "quota ledger: a draw by count takes fewer than 2^24 requests, not %d" % n
        text = self.draw_refusal(leaves)
        if text:
            return text
        for i, c in enumerate(counts):
            if count_refusal(i, c):
                return count_refusal(i, c)
        return ""

    def draw_counts(self, leaves, exts, limits, counts):
        """rank: the sum of the counts of the call's earlier requests with the same key, whatever became of them;
        granted whole (first + count <= limit) or not at all; a refused request counts in the ranks behind it"""
        text = self.draw_counts_refusal(leaves, counts)
        if text:
            raise Refused(text)
        firsts, status, rank, end = [], [], {}, {}
        for leaf, ext, limit, count in zip(leaves, exts, limits, counts):
            if ext not in self.window:
                firsts.append(limit)
                status.append(NO_EPOCH)
                self.no_epoch += 1
                continue
            key = (ext, leaf)
            r = rank.get(key, 0)
            rank[key] = r + count
            first = self.used.get(key, 0) + r      # `used` is not written before the loop ends: as it was before the call
            if first + count <= limit:
                firsts.append(first)
                status.append(OK)
                end[key] = first + count           # firsts rise with the rank: the last OK request ends highest
                self.issued += count
            else:
                firsts.append(limit)
                status.append(OVER)
                self.over += 1
        self.used.update(end)
        if leaves:
            self.draws += 1
        return firsts, status


class Blocks:
    """every block ever granted, per (external nullifier, leaf), as the answers state it: add() after each call, check()
    at the end.  An epoch that leaves the window and a fresh ledger start a new Blocks."""

    def __init__(self):
        self.granted = {}

    def add(self, leaves, exts, limits, counts, firsts, status):
        for leaf, ext, limit, count, first, st in zip(leaves, exts, limits, counts, firsts, status):
            if st == OK:
                assert first + count <= limit, "a block reaches past its limit"
                self.granted.setdefault((ext, leaf), []).append((first, count))
            else:
                assert first == limit, "a refused request carries its limit"

    def check(self):
        total = 0
        for key, blocks in self.granted.items():
            blocks = sorted(blocks)
            for (a, ca), (b, _) in zip(blocks, blocks[1:]):
                assert a + ca <= b, "two blocks of %r share an id: %d+%d and %d" % (key, a, ca, b)
            total += sum(c for _, c in blocks)
        return total


# ------------------------------------------------------------------------------------------------------ the cases
SIZES = [1, 255, 256, 257, 65537]          # the workgroup edge, and one more scan level twice (rlnamd_quota_plan)
MIX = [1, 2, 3, 4]


def one_member_255(n, depth=20):
    """one member for all n, 255 ids a request, the limit reached half way"""
    last = (1 << depth) - 1
    return [last] * n, [E2] * n, [255 * (n // 2) + 7] * n, [255] * n


def straddling(n, depth=20):
    """one member whose group starts inside the first workgroup of the sorted order and runs on past its end (from
    n = 257 on), counts 1 .. 4 mixed; the requests before it are of lower leaves, one each"""
    rnd = random.Random(7000 + n)
    fill = min(200, n // 2)
    member = (1 << depth) - 2
    leaves = list(range(fill)) + [member] * (n - fill)
    counts = [rnd.choice(MIX) for _ in range(n)]
    order = list(range(n))
    rnd.shuffle(order)                        # the call's order is not the sorted one
    limit_of = {member: 2 * (n - fill) + 1}   # about 2.5 ids a request: over near four fifths of the group
    leaves = [leaves[i] for i in order]
    return leaves, [E1] * n, [limit_of.get(leaf, 3) for leaf in leaves], counts


def all_distinct(n, depth=20):
    rnd = random.Random(8000 + n)
    leaves = rnd.sample(range(1 << depth), n)
    return leaves, [E1] * n, [rnd.choice([0, 3, 300, U32]) for _ in range(n)], [rnd.choice(MIX + [255]) for _ in range(n)]


def interleaved(n, depth=20, seed=None):
    """the randomised case of size n: a few members that repeat, three epochs of the window and one outside it, counts
    1 .. 4 and 255, one limit per member.  calls x n requests, at least 48 requests in all, so that the preconditions
    below can hold at n = 1 too: [(leaves, exts, limits, counts)], to be played in this order on one ledger"""
    rnd = random.Random(SEEDS[n] if seed is None else seed)
    last = (1 << depth) - 1
    few = [0, last] + [rnd.randrange(1 << depth) for _ in range(5)]
    limit_of = {leaf: rnd.choice([0, 2, 9, 600, U32]) for leaf in few}
    limit_of[0], limit_of[last] = 9, U32
    out = []
    for _ in range(max(2, -(-48 // n))):
        who = [rnd.choice(few) for _ in range(n)]
        out.append((who, [rnd.choice([E1, E2, E3, OUTSIDE]) for _ in range(n)], [limit_of[w] for w in who],
                    [rnd.choice(MIX + [255]) for _ in range(n)]))
    return out


# the seeds of interleaved(), chosen so that the model alone meets preconditions_hold (test_quota_counts_host.py asserts
# it for every size here, on the CPU)
SEEDS = {1: 9001, 63: 9063, 64: 9064, 65: 9065, 255: 9255, 256: 9256, 257: 9257, 2000: 9200, 65537: 9537}


def preconditions_hold(calls, depth=20, max_epochs=4):
    """OK, OVER and NO_EPOCH each occur, and so does every count 1 .. 4 and the count 255 -- by the model alone"""
    m = CountsModel(depth, max_epochs)
    m.set_epochs([E1, E2, E3])
    seen, counts_seen = set(), set()
    for leaves, exts, limits, counts in calls:
        seen |= set(m.draw_counts(leaves, exts, limits, counts)[1])
        counts_seen |= set(counts)
    return seen == {OK, OVER, NO_EPOCH} and counts_seen >= set(MIX + [255])


def counts_shapes(n, depth=20):
    """the draws every size is put through, on one ledger in this order: [(leaves, exts, limits, counts)].  The
    interleaved calls come twice over the same members (two and more consecutive calls on one ledger)."""
    return [all_distinct(n, depth), one_member_255(n, depth), straddling(n, depth)] + interleaved(n, depth)


def two_limits_counts():
    """one member under two limits, in both orders, with blocks"""
    return [([7] * 6, [E1] * 6, [3, 20, 3, 20, 20, 3], [2, 3, 2, 4, 1, 1]), ([9] * 6, [E1] * 6, [20, 3, 20, 3, 3, 20], [3, 2, 4, 2, 1, 1]),
            ([7] * 4, [E1] * 4, [40, 22, 40, 22], [4, 1, 255, 2]), ([9] * 4, [E1] * 4, [4, 40, 4, 40], [4, 4, 1, 4])]


# ------------------------------------------------------------------------------------------------------ the runner
def compare_draw_counts(model, impl, leaves, exts, limits, counts, blocks=None):
    """impl.draw_counts(leaves, exts, limits, counts) -> (firsts, statuses)"""
    want = model.draw_counts(leaves, exts, limits, counts)
    got = impl.draw_counts(leaves, exts, limits, counts)
    assert got[1] == want[1], "statuses"
    assert got[0] == want[0], "firsts"
    if blocks is not None:
        blocks.add(leaves, exts, limits, counts, got[0], got[1])
    return got
