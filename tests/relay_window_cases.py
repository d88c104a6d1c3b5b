"""The messages and the model that tests/test_relay_window_host.py (CPU build of relay.h and nullifier_log.h) and
tests/test_gpu_relay_window.py judge the relay step's epoch window by, over tests/relay_cases.py,
tests/nullifier_log_cases.py and tests/nullifier_retire_cases.py, none of which is changed.

The window W is a set of external nullifiers.  A step with a window is the windowless step with one change: a message
whose verdict would be OK and whose external nullifier is not in W is BAD_EPOCH, and its shares never reach the log.
The model says that with relay_cases.model alone: ok[i] forced to 0 where ext is not in W, and the verdict BAD_EPOCH
where the windowless verdict was OK.

The streams of relay_cases use two external nullifiers; with one of them as the window FOREIGN no longer occurs.  The
stream here uses THREE, two of them in the window, so that a nullifier can still be seen under two external
nullifiers that both pass."""
import functools
import random

import nullifier_log_cases as log_cases
import nullifier_retire_cases as retire_cases   # noqa: F401  (survivors(): what a retain leaves, for the importers)
import relay_cases

R = relay_cases.R
OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_EPOCH = range(5)
NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED = range(5)


def ext_of(row, k):
    return relay_cases.split(row, k)[4]


def model(rows, ok, xs, roots, tags, k, seen, next_seq, window):
    """relay_cases.model with the window: a set (or list) of external nullifiers, empty for none.  `seen` is the log
    and moves as the windowed step moves it.  -> (verdict, status, secret, first_tag, shares, share tags)"""
    window = set(window)
    if not window:
        return relay_cases.model(rows, ok, xs, roots, tags, k, seen, next_seq)
    plain = relay_cases.model(rows, ok, xs, roots, tags, k, dict(seen), next_seq)[0]
    inside = [ext_of(row, k) in window for row in rows]
    forced = [o if w else 0 for o, w in zip(ok, inside)]
    _v, status, secret, first, shares, share_tags = relay_cases.model(rows, forced, xs, roots, tags, k, seen, next_seq)
    verdict = [BAD_EPOCH if v == OK and not w else v for v, w in zip(plain, inside)]
    return verdict, status, secret, first, shares, share_tags


def retained(shares, tags, window):
    """the (share, tag, sequence number) that a retain of `window` leaves: retire_cases.survivors of everything else"""
    window = set(window)
    return retire_cases.survivors(shares, tags, {s[3] for s in shares} - window)


@functools.lru_cache(maxsize=None)
def messages(k, n=2000, seed=20261020):
    """-> dict(rows, ok, xs, roots, tags, exts, window): relay_cases.messages' stream over three external nullifiers,
    window = the first two.  A member's home is exts[m % 3]; a "foreign" message takes one of the other two, so a
    nullifier is met under a second external nullifier inside the window (FOREIGN stays) and outside it (the record
    the windowless log holds first is one the windowed log never saw).  Computed once, never changed."""
    rnd = random.Random(seed + k)
    fr = lambda: rnd.randrange(1, R)
    exts = (fr(), fr(), fr())
    window = exts[:2]
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
            x, ext = fr(), exts[(m + (rnd.randrange(1, 3) if kind == "foreign" else 0)) % 3]
            ids = rnd.sample(range(6), k)
        sent.setdefault(m, []).append((x, ext, ids))
        sel = list(rnd.choice(relay_cases.PATTERNS)) if k == 4 else [rnd.randrange(2) for _ in range(k)]
        if k > 1 and rnd.randrange(16) == 0:
            sel[rnd.randrange(k)] = rnd.choice((2, 1 + (1 << 64), R - 1))
        ys = [(a0[m] + x * slot(m, j)[0]) % R for j in ids]
        nuls = [slot(m, j)[1] for j in ids]
        root = fr() if rnd.randrange(8) == 0 else rnd.choice(roots)
        rows.append(tuple(relay_cases.join(ys, root, nuls, x, ext, sel, k)))
        ok.append(0 if rnd.randrange(8) == 0 else 1)
        xs.append(fr() if rnd.randrange(8) == 0 else x)
    tags = tuple(rnd.getrandbits(64) for _ in range(n))
    case = dict(rows=tuple(rows), ok=tuple(ok), xs=tuple(xs), roots=roots, tags=tags, exts=exts, window=window)
    # the stream exercises what it is meant to
    verdict, status, _secret, _first, _shares, _tags = model(rows, ok, xs, roots, tags, k, {}, 0, window)
    plain = relay_cases.model(rows, ok, xs, roots, tags, k, {}, 0)
    for v in (OK, BAD_PROOF, BAD_ROOT, BAD_SIGNAL, BAD_EPOCH):
        assert verdict.count(v) >= 20, ("verdict", v, verdict.count(v))
    for s in (NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED):
        assert status.count(s) >= 20, ("status", s, status.count(s))
    # a gate that ignores the window fails: in-window accepted messages whose status the window changes
    moved = sum(1 for i in range(n) if verdict[i] == OK and status[i] != plain[1][i])
    assert moved >= 20, moved
    assert all(v == p or (v == BAD_EPOCH and p == OK) for v, p in zip(verdict, plain[0]))
    return case


def synthetic_log(n, classes):
    """n shares with distinct nullifiers, share i under external nullifier 1000 + i % classes, on the line a0 = 5 + i,
    a1 = 7; tag 10 * i + 3 (retire_cases.synthetic with any number of classes)"""
    return retire_cases.synthetic(n, classes)


n_values = relay_cases.n_values
pack_rows = relay_cases.pack_rows
pack_frs = relay_cases.pack_frs
pack_shares = log_cases.pack
