"""The retire flow that tests/test_nullifier_retire_host.py (CPU build of nullifier_log.h) and
tests/test_gpu_nullifier_retire.py (the device log) judge by, over the stream and the model of
tests/nullifier_log_cases.py: observe shares [0, 2048), retire the first external nullifier the stream uses, observe
[2048, 4096).  What a log owes after the retire is what the model says of the second half when it has seen only the
survivors of the first, with their tags, in their order."""
import functools

import nullifier_log_cases as cases
from nullifier_log_cases import DUPLICATE, FOREIGN, NEW, SPAM

HALF = 2048


def survivors(shares, tags, retired):
    """the (share, tag, sequence number) that a retire of the external nullifiers in `retired` leaves"""
    return [(s, t, i) for i, (s, t) in enumerate(zip(shares, tags)) if s[3] not in retired]


@functools.lru_cache(maxsize=None)
def flow():
    """-> dict: ext (the retired external nullifier), first (the model's verdicts on the first half), kept (the
    survivors), second (the verdicts owed on the second half), distinct (nullifiers in the log at the end); after the
    checks that the flow exercises something.  Computed once, never changed."""
    shares, tags, _ = cases.stream()
    ext = shares[0][3]
    first = tuple(cases.model(shares[:HALF], tags[:HALF]))
    kept = survivors(shares[:HALF], tags[:HALF], {ext})
    seen = {}
    cases.model([k[0] for k in kept], [k[1] for k in kept], seen)
    second = tuple(cases.model(shares[HALF:], tags[HALF:], seen))
    plain = cases.model(shares, tags)[HALF:]           # a log that did not retire
    assert HALF - len(kept) == 1014 and len(kept) == 1034
    for status in (NEW, DUPLICATE, SPAM, FOREIGN):
        assert sum(1 for w in second if w[0] == status) >= 389, "the second half meets status %d too rarely" % status
    differ = [(a, b) for a, b in zip(second, plain) if a != b]
    assert len(differ) == 726                          # a retire that does nothing fails
    assert sum(1 for a, b in differ if a[0] != NEW and b[0] != NEW) == 375      # the first record changed
    return dict(ext=ext, first=first, kept=tuple(kept), second=second, distinct=len(seen))


def synthetic(n, classes=3):
    """n shares with distinct nullifiers, share i under external nullifier 1000 + i % classes, on the line a0 = 5 + i,
    a1 = 7; tag 10 * i + 3"""
    return ([(1 + i, 11 + i, (5 + i + (11 + i) * 7) % cases.R, 1000 + i % classes) for i in range(n)],
            [10 * i + 3 for i in range(n)])
