"""The share stream and the model that tests/test_nullifier_log_host.py (CPU build of nullifier_log.h) and
tests/test_gpu_nullifier_log.py (the device log) judge by.

Shares are real line shares: member (a0, a1), message x, y = a0 + x a1 mod r, so a SPAM secret must equal that member's
a0 as well as what the oracle's compute_id_secret gives for the two shares."""
import functools
import random

from oracle.pyref.keygen import compute_id_secret

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NEW, DUPLICATE, SPAM, FOREIGN, SKIPPED = range(5)


def model(shares, tags, seen=None):
    """[(nullifier, x, y, ext)] taken in index order -> [(status, secret, first_tag)]; `seen` is the log: a dict from
    nullifier to the first (x, y, ext, tag)"""
    seen = {} if seen is None else seen
    out = []
    for (nul, x, y, ext), tag in zip(shares, tags):
        if nul not in seen:
            seen[nul] = (x, y, ext, tag)
            out.append((NEW, 0, tag))
            continue
        fx, fy, fext, ftag = seen[nul]
        if fext != ext:
            out.append((FOREIGN, 0, ftag))
        elif fx == x:
            out.append((DUPLICATE, 0, ftag))
        else:
            out.append((SPAM, compute_id_secret((fx, fy), (x, y)), ftag))
    return out


@functools.lru_cache(maxsize=None)
def stream(n=4096, n_members=1500, seed=20260118):
    """-> (shares, tags, a0 of each share's member): first sights, exact replays, the first x with another y, the
    nullifier under the other external nullifier, and further messages on the member's line (pairs, triples and more of
    one nullifier with different x).  The first and the last share carry one nullifier.  Computed once, never changed:
    the callers get tuples."""
    rnd = random.Random(seed)
    fr = lambda: rnd.randrange(1, R)
    ext = (fr(), fr())
    members = [dict(a0=fr(), a1=fr(), nul=fr(), ext=ext[m & 1], other=ext[(m & 1) ^ 1], sent=[]) for m in range(n_members)]
    shares, owner = [], []
    for i in range(n):
        last = i == n - 1
        mi = owner[0] if last else rnd.randrange(n_members)
        m = members[mi]
        kind = "first" if not m["sent"] else "line" if last else rnd.choice(("replay", "same_x", "foreign", "line", "line"))
        x = fr()
        s = (m["nul"], x, (m["a0"] + x * m["a1"]) % R, m["ext"])
        if kind == "replay":
            s = rnd.choice(m["sent"])
        elif kind == "same_x":
            s = (m["nul"], m["sent"][0][1], fr(), m["ext"])
        elif kind == "foreign":
            s = (m["nul"], s[1], s[2], m["other"])
        m["sent"].append(s)
        shares.append(s)
        owner.append(mi)
    tags = tuple(rnd.getrandbits(64) for _ in range(n))
    return tuple(shares), tags, tuple(members[o]["a0"] for o in owner)


@functools.lru_cache(maxsize=None)
def expected(n=4096, n_members=1500, seed=20260118):
    """the model's verdicts on stream(...), after the checks that the stream exercises something"""
    shares, tags, a0 = stream(n, n_members, seed)
    want = tuple(model(shares, tags))
    for status in (NEW, DUPLICATE, SPAM, FOREIGN):
        assert sum(1 for w in want if w[0] == status) >= 50, "the stream meets status %d fewer than 50 times" % status
    assert shares[0][0] == shares[-1][0] and want[-1][0] == SPAM
    # triples: some nullifier is judged SPAM at least twice, and every SPAM secret is the member's a0
    spam = [shares[i][0] for i, w in enumerate(want) if w[0] == SPAM]
    assert len(spam) - len(set(spam)) >= 50
    assert all(w[1] == a0[i] for i, w in enumerate(want) if w[0] == SPAM)
    return want


def pack(shares):
    return b"".join(int(v).to_bytes(32, "little") for s in shares for v in s)


def flat(want):
    """[(status, secret, first_tag)] -> (status bytes, secrets bytes, [first tags]): what the logs return"""
    return (bytes(w[0] for w in want), b"".join(int(w[1]).to_bytes(32, "little") for w in want), [w[2] for w in want])
