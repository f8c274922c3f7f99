"""The contract of the grep over the record index (include/minlz_hip.h: mlz_dev_reader_grep_records) in plain Python, for
tests/test_stream_grep_host.py and tests/test_gpu_stream_grep.py: data.split(delimiter) with one trailing empty piece dropped,
`pattern in record`, set arithmetic for S and C, the kinds, the four totals and the cut at rec_cap."""


def records(data, delim):
    """The records: data.split(delimiter) with one trailing empty piece dropped (empty data has none)."""
    pieces = bytes(data).split(bytes(delim))
    if pieces[-1] == b"":
        pieces.pop()
    return pieces


def matching(recs, patterns):
    """M: the numbers of the records that hold one of the patterns."""
    pats = [bytes(p) for p in patterns]
    return {r for r, rec in enumerate(recs) if any(p in rec for p in pats)}


def context(S, N, before, after):
    """C: the records r < N with some s in S and s - before <= r <= s + after.  Runs of neighbouring selected records are taken as one
    interval, so that a large context over many selected records stays cheap."""
    C = set()
    covered = 0   # every r < covered is decided
    for s in sorted(S):
        lo, hi = max(s - before, 0, covered), min(s + after, N - 1)
        if hi >= lo:
            C.update(range(lo, hi + 1))
            covered = hi + 1
    return C


def result(data, delim, patterns, invert=False, before=0, after=0, rec_cap=None):
    """-> dict(N, M, S, C: sorted lists; R; numbers, kinds: the first k = min(R, rec_cap) records of C and whether each is in S;
    totals = (R, |S|, the bytes of the k written records, the bytes of all R records))."""
    recs = records(data, delim)
    N = len(recs)
    M = matching(recs, patterns)
    S = set(range(N)) - M if invert else M
    C = sorted(context(S, N, before, after))
    assert S <= set(C)
    k = len(C) if rec_cap is None else min(len(C), rec_cap)
    numbers = C[:k]
    return dict(N=N, M=sorted(M), S=sorted(S), C=C, R=len(C), numbers=numbers, kinds=[1 if r in S else 0 for r in numbers],
                totals=(len(C), len(S), sum(len(recs[r]) for r in numbers), sum(len(recs[r]) for r in C)))


def lines(data, delim, numbers):
    """What read_records over `numbers` gives -> (the packed bytes, the k + 1 starts)."""
    recs = records(data, delim)
    parts = [recs[r] for r in numbers]
    starts = [0]
    for p in parts:
        starts.append(starts[-1] + len(p))
    return b"".join(parts), starts
