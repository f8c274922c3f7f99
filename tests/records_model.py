"""The contract of mlz_dev_reader_search_records (include/minlz_hip.h) in plain Python, for tests/test_stream_records_host.py and
tests/test_gpu_stream_records.py: the occurrences, the record around each, the opening rule, the caps."""

DEFAULT_REACH = 65536
CUT_LEFT, CUT_RIGHT = 1, 2


def occurrences(data, pat):
    """Every position of pat in data, overlapping ones too, ascending."""
    out, p = [], data.find(pat)
    while p >= 0:
        out.append(p)
        p = data.find(pat, p + 1)
    return out


def bounds(data, p, L, delim, W):
    """-> (s, e, cut) of the occurrence at p: the rule, literally."""
    size = len(data)
    lo, hi = max(0, p - W), min(size, p + L + W)
    cut = 0
    j = data.rfind(delim, lo, p)
    if j >= 0:
        s = j + 1
    else:
        s = lo
        if lo > 0:
            cut |= CUT_LEFT
    j = data.find(delim, p + L, hi)
    if j >= 0:
        e = j
    else:
        e = hi
        if hi < size:
            cut |= CUT_RIGHT
    return s, e, cut


def records(data, pat, delim, W=0):
    """-> ([(s, e, flags)], occurrences): occurrence i opens a record when i == 0 or its s differs from the one before; s and the left cut
    come from the occurrence that opens a record, e and the right cut from its last one."""
    W = W or DEFAULT_REACH
    assert len(delim) == 1 and delim not in pat
    occ = occurrences(data, pat)
    recs, prev_s = [], None
    for i, p in enumerate(occ):
        s, e, cut = bounds(data, p, len(pat), delim, W)
        if i == 0 or s != prev_s:
            recs.append([s, e, cut & CUT_LEFT])
        recs[-1][1] = e
        recs[-1][2] = (recs[-1][2] & CUT_LEFT) | (cut & CUT_RIGHT)
        prev_s = s
    return [tuple(r) for r in recs], len(occ)


def result(data, pat, delim, W, rec_cap, dst_cap):
    """What the call returns and writes: dict(R, totals, k, rec_off, rec_start, flags, dst).  rec_start has k + 1 values; with no occurrence
    nothing at all is written (rec_start is then empty too)."""
    recs, n_occ = records(data, pat, delim, W)
    k = used = 0
    while k < len(recs) and k < rec_cap and used + recs[k][1] - recs[k][0] <= dst_cap:
        used += recs[k][1] - recs[k][0]
        k += 1
    starts = [0]
    for s, e, _ in recs[:k]:
        starts.append(starts[-1] + e - s)
    return dict(R=len(recs), totals=(len(recs), sum(e - s for s, e, _ in recs), n_occ, sum(1 for r in recs if r[2])), k=k,
                rec_off=[r[0] for r in recs[:k]], rec_start=starts if recs else [], flags=[r[2] for r in recs[:k]],
                dst=b"".join(data[s:e] for s, e, _ in recs[:k]))


def windows(data_len, occ, L, W):
    """The merged windows of the read phase: [(lo, hi)] — a window opens when i == 0 or lo_i > hi_(i-1)."""
    W = W or DEFAULT_REACH
    out = []
    for i, p in enumerate(occ):
        lo, hi = max(0, p - W), min(data_len, p + L + W)
        if i == 0 or lo > out[-1][1]:
            out.append([lo, hi])
        else:
            out[-1][1] = hi
    return [tuple(w) for w in out]
