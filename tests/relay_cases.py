"""The messages and the model that tests/test_relay_host.py (CPU build of relay.h) judges the relay step by, and the
composition tests/test_gpu_relay.py restates over the existing calls.

A message is its proof's public values in the verifier's order -- single: y | root | nullifier | x | ext; multi with k
slots: ys[k] | root | nullifiers[k] | x | ext | selector_used[k] -- plus what the verifier said of the proof (ok), what
its signal hashes to (xs) and a tag.  The shares are real line shares: member a0, message id j, a1 = a1[member][j],
y = a0 + x a1 mod r, so a SPAM secret must be the member's a0."""
import functools
import random

import nullifier_log_cases as log_cases

R = log_cases.R
OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL = range(4)
NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED = range(5)
PATTERNS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 0, 0, 1))


def n_values(k):
    return 5 if k == 1 else 3 * k + 3


def split(row, k):
    """a row of values -> (ys, root, nullifiers, x, ext, selectors)"""
    if k == 1:
        return [row[0]], row[1], [row[2]], row[3], row[4], [1]
    return row[:k], row[k], row[k + 1:2 * k + 1], row[2 * k + 1], row[2 * k + 2], row[2 * k + 3:]


def join(ys, root, nuls, x, ext, sel, k):
    if k == 1:
        return [ys[0], root, nuls[0], x, ext]
    return list(ys) + [root] + list(nuls) + [x, ext] + list(sel)


def model(rows, ok, xs, roots, tags, k, seen, next_seq):
    """One step over the log `seen` (a dict, nullifier_log_cases.model's) whose next sequence number is next_seq.
    tags: a list, or None for the sequence numbers.  -> (verdict, status, secret, first_tag, shares, share tags): four
    lists per message and what the step recorded, in order"""
    verdict, counts, shares, share_tags = [], [], [], []
    for i, row in enumerate(rows):
        ys, root, nuls, x, ext, sel = split(row, k)
        if not ok[i] or any(s not in (0, 1) for s in sel):
            v = BAD_PROOF
        elif roots and root not in roots:
            v = BAD_ROOT
        elif xs[i] != x:
            v = BAD_SIGNAL
        else:
            v = OK
        verdict.append(v)
        used = [s for s in range(k) if sel[s] == 1] if v == OK else []
        counts.append(len(used))
        for s in used:
            share_tags.append(tags[i] if tags is not None else next_seq + len(shares))
            shares.append((nuls[s], x, ys[s], ext))
    judged = log_cases.model(shares, share_tags, seen)
    status, secret, first, at = [], [], [], 0
    for c in counts:
        mine = judged[at:at + c]
        at += c
        pick = (SKIPPED, 0, 0)
        for want in (SPAM, FOREIGN, DUPLICATE, NEW):
            hit = [j for j in mine if j[0] == want]
            if hit:
                pick = hit[0]
                break
        status.append(pick[0])
        secret.append(pick[1])
        first.append(pick[2])
    return verdict, status, secret, first, shares, share_tags


@functools.lru_cache(maxsize=None)
def messages(k, n=2000, seed=20261019):
    """-> dict(rows, ok, xs, roots, tags): n messages of the k-slot layout in which every verdict, every pair of failing
    checks, every status and (k = 4) every selector pattern occurs, some selector elements are 2 or 1 + 2^64, and members
    repeat message ids under other x, the same x and the other external nullifier.  Computed once, never changed."""
    rnd = random.Random(seed + k)
    fr = lambda: rnd.randrange(1, R)
    exts = (fr(), fr())
    roots = tuple(fr() for _ in range(64))
    n_members = max(4, n // 8)
    a0 = [fr() for _ in range(n_members)]
    line = {}

    def slot(m, j):
        if (m, j) not in line:
            line[(m, j)] = (fr(), fr())   # a1, nullifier
        return line[(m, j)]

    rows, ok, xs, sent = [], [], [], {}
    for i in range(n):
        m = rnd.randrange(n_members)
        kind = rnd.choice(("line", "line", "replay", "foreign")) if m in sent else "line"
        if kind == "replay":
            x, ext, ids = rnd.choice(sent[m])
        else:
            x, ext = fr(), exts[(m & 1) ^ (kind == "foreign")]
            ids = rnd.sample(range(6), k)
        sent.setdefault(m, []).append((x, ext, ids))
        sel = list(rnd.choice(PATTERNS)) if k == 4 else [rnd.randrange(2) for _ in range(k)]
        if k > 1 and rnd.randrange(16) == 0:
            sel[rnd.randrange(k)] = rnd.choice((2, 1 + (1 << 64), R - 1))
        ys = [(a0[m] + x * slot(m, j)[0]) % R for j in ids]
        nuls = [slot(m, j)[1] for j in ids]
        root = fr() if rnd.randrange(6) == 0 else rnd.choice(roots)
        rows.append(tuple(join(ys, root, nuls, x, ext, sel, k)))
        ok.append(0 if rnd.randrange(6) == 0 else 1)
        xs.append(fr() if rnd.randrange(6) == 0 else x)
    tags = tuple(rnd.getrandbits(64) for _ in range(n))
    case = dict(rows=tuple(rows), ok=tuple(ok), xs=tuple(xs), roots=roots, tags=tags)
    # the stream exercises what it is meant to
    verdict, status, secret, _first, _shares, _tags = model(rows, ok, xs, roots, tags, k, {}, 0)
    for v in (OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL):
        assert verdict.count(v) >= 20, v
    for s in (NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED):
        assert status.count(s) >= 20, s
    pairs = [0, 0, 0]
    for i, row in enumerate(rows):
        _ys, root, _nuls, x, _ext, _sel = split(row, k)
        pairs[0] += (not ok[i]) and root not in roots
        pairs[1] += root not in roots and xs[i] != x and bool(ok[i])
        pairs[2] += (not ok[i]) and xs[i] != x
    assert min(pairs) >= 10, pairs
    if k > 1:
        assert sum(1 for v, s, r in zip(verdict, status, rows) if v == OK and s == SKIPPED) >= 5   # accepted, no used slot
        assert sum(1 for r in rows if any(t not in (0, 1) for t in split(r, k)[5])) >= 20
    return case


def pack_rows(rows):
    return b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)


def pack_frs(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)
