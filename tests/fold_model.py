"""The contract of MLZ_SEARCH_IGNORE_CASE (include/minlz_hip.h) in plain Python, in two parts.

The results: fold() and wrappers that run the existing models (tests/search_model.py, records_model.py, grep_model.py) on folded inputs —
a flagged call returns what the unflagged call returns for fold(decoded stream) and fold(pattern), except that the record bytes of
search_records are the stream's original ones and that records are split at the original delimiter, which is no letter.

The plan: a restatement of the folded plan rule over search_model's hash and tables.  A window of the folded pattern is present in a table
when the bit of any of its case variants is set; a window with more than MAX_LETTERS letters abstains (present everywhere, no hashes); a
pattern whose windows all abstain is not served.  Types 2 and 3 use window i only when every case variant of pattern[i - 1] is a prefix
byte, and t_min = 1 only when every variant of pattern[0] is one; type 4 has groups only when the prefix holds no letter."""
import numpy as np

from tests import grep_model as GM
from tests import records_model as RM
from tests import search_model as SMod

MAX_LETTERS = 3
MAX_HASHES = 1 << 22


# ---- the results ----

def fold_byte(b):
    return b | 0x20 if 0x41 <= b <= 0x5A else b


def fold(x):
    """A .. Z -> a .. z, everything else as it is: bytes -> bytes, a uint8 array -> a uint8 array."""
    if isinstance(x, np.ndarray):
        return np.where((x >= 0x41) & (x <= 0x5A), x | 0x20, x).astype(np.uint8)
    return bytes(x).lower()          # (bytes.lower is ASCII only, whatever the locale)


def is_letter(b):
    return 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A


def search(data, pattern):
    return SMod.brute(fold(data), fold(pattern))


def search_many(data, patterns):
    """-> (the pairs (position, pattern) ascending, every pattern's count)"""
    fd = fold(data)
    per = [SMod.brute(fd, fold(p)) for p in patterns]
    return sorted((q, i) for i, qs in enumerate(per) for q in qs), [len(qs) for qs in per]


def records_result(data, pattern, delim, W, rec_cap, dst_cap):
    """records_model.result over the folded inputs, with the record bytes of the original data."""
    assert not is_letter(bytes(delim)[0])
    data = bytes(data)
    want = RM.result(fold(data), fold(pattern), delim, W, rec_cap, dst_cap)
    spans = zip(want["rec_off"], np.diff(want["rec_start"]).tolist()) if want["k"] else []
    return dict(want, dst=b"".join(data[s:s + n] for s, n in spans))


def grep_result(data, delim, patterns, invert=False, before=0, after=0, rec_cap=None):
    assert not is_letter(bytes(delim)[0])
    return GM.result(fold(data), delim, [fold(p) for p in patterns], invert, before, after, rec_cap)


def grep_lines(data, delim, numbers):
    """The original records with these numbers -> (the packed bytes, the k + 1 starts)"""
    return GM.lines(data, delim, numbers)


# ---- the plan ----

def variants(window):
    """The case variants of a folded window in the library's order (bit j of the variant's number: the j-th letter in upper case), or None:
    the window abstains."""
    window = fold(window)
    at = [j for j, b in enumerate(window) if is_letter(b)]
    if len(at) > MAX_LETTERS:
        return None
    out = []
    for v in range(1 << len(at)):
        w = bytearray(window)
        for j, o in enumerate(at):
            if (v >> j) & 1:
                w[o] &= ~0x20 & 0xFF
        out.append(bytes(w))
    return out


def every_variant_is_prefix(mask, b):
    return bool(mask[b | 0x20] and mask[b & ~0x20 & 0xFF]) if is_letter(b) else bool(mask[b])


def windows(pattern, cfg):
    """-> (groups of window starts, t_min): the windows the tables answer for under folding, abstaining ones included."""
    T, M, field = cfg
    P, L = fold(pattern), len(pattern)
    if L < M:
        return [], 1
    if T == 1:
        return [[i] for i in range(0, L - M + 1)], 1
    if T == 4:
        K, E, pfx = SMod.parts_of(field)
        if any(is_letter(b) for b in pfx):
            return [], 0
        G = [i for i in range(0, L - K - M - E + 1) if P[i:i + K] == pfx]
        return [[i + K + j for j in range(E + 1)] for i in G], (1 if G and G[0] == 0 else 0)
    mask = SMod.mask_of(T, field)
    return [[i] for i in range(1, L - M + 1) if every_variant_is_prefix(mask, P[i - 1])], (1 if every_variant_is_prefix(mask, P[0]) else 0)


def checks(cfg, pattern, B):
    """-> (groups of windows of variant hashes — None for a window that abstains —, t_min), or None: the tables cannot serve the pattern."""
    T, M, field = cfg
    P = fold(pattern)
    groups, t_min = windows(pattern, cfg)
    out = []
    for g in groups:
        ws = []
        for i in g:
            vs = variants(P[i:i + M])
            ws.append(None if vs is None else [SMod.hash_value(int.from_bytes(v, "little"), B, M) for v in vs])
        out.append(ws)
    if not any(w is not None for g in out for w in g):
        return None
    return out, t_min


def n_hashes(chk):
    return sum(len(w) for g in chk[0] for w in g if w is not None)


def probe(table, R, B, groups):
    """(a, s): the leading and the trailing groups whose windows are all present — abstaining, or one variant's bit set."""
    n = len(groups)
    if table is None:
        return n, n
    mask = (1 << (B - R)) - 1
    bit = lambda h: (table[(h & mask) >> 3] >> ((h & mask) & 7)) & 1
    has = [all(w is None or any(bit(h) for h in w) for w in g) for g in groups]
    a = next((i for i, x in enumerate(has) if not x), n)
    if a == n:
        return n, n
    return a, next((i for i, x in enumerate(reversed(has)) if not x), n)


def probed(tables, pattern, cfg, B):
    chk = checks(cfg, pattern, B)
    if chk is None:
        return None
    groups, t_min = chk
    pr = [probe(t[0], t[1], B, groups) if t is not None else (len(groups), len(groups)) for t in tables]
    return [p[0] for p in pr], [p[1] for p in pr], len(groups), t_min


def plan_sets(tables_per_cfg, sizes, pattern, cfgs, Bs, sidecar=False, use_tables=True):
    """The chunks a folded search for `pattern` decodes -> (the sorted chunk numbers, served): every table set that serves the pattern
    votes (a sidecar's set abstains in front of a chunk shorter than its overlap), the chunk is a candidate when none refuses."""
    everything = [k for k in range(len(sizes)) if sizes[k]]
    if not use_tables:
        return everything, False
    got = [(ci, probed(tables_per_cfg[ci], pattern, c, Bs[ci])) for ci, c in enumerate(cfgs)]
    got = [(ci, p) for ci, p in got if p is not None]
    if not got or not any(t is not None for ci, _ in got for t in tables_per_cfg[ci]):
        return everything, False
    L = len(pattern)
    votes = [SMod.admits(p[0], p[1], sizes, p[2], L, p[3], SMod.overlap(cfgs[ci]) if sidecar else 0) for ci, p in got]
    return SMod.decoded_set(votes, sizes, L), True


def plan(tables, sizes, pattern, cfg, B, use_tables=True):
    """One configuration (a stream's inline tables) -> the chunks to decode."""
    if cfg is None:
        return [k for k in range(len(sizes)) if sizes[k]]
    return plan_sets([tables], sizes, pattern, [cfg], [B], use_tables=use_tables)[0]


def plan_many(tables_per_cfg, sizes, patterns, cfgs, Bs, sidecar=False, budget=MAX_HASHES):
    """-> (the union of the patterns' plans, the patterns not served): patterns in order against the call's budget of variant hashes; one
    that is not served puts every non-empty chunk into the set."""
    everything = [k for k in range(len(sizes)) if sizes[k]]
    union, unserved, made = set(), 0, 0
    for p in patterns:
        want = sum(n_hashes(c) for c in (checks(cfg, p, B) for cfg, B in zip(cfgs, Bs)) if c is not None)
        pl, served = plan_sets(tables_per_cfg, sizes, p, cfgs, Bs, sidecar)
        if served and made + want > budget:
            pl, served = everything, False
        if served:
            made += want
        else:
            unserved += 1
        union |= set(pl)
    if unserved:
        union = set(everything)
    return sorted(union), unserved


def plan_of_stream(stream, pattern):
    """-> (plan, sizes, served) of a folded search for `pattern` over a stream with inline tables."""
    cfg, B, tables = SMod.read_tables(stream)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    if cfg is None:
        return [k for k in range(len(sizes)) if sizes[k]], sizes, False
    pl, served = plan_sets([tables], sizes, pattern, [cfg], [B])
    return pl, sizes, served


def chunks_with_a_start(sizes, positions):
    """The data chunks that hold the start of an occurrence."""
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {int(np.searchsorted(starts, p, side="right")) - 1 for p in positions}
