"""The contract of a set of streams that keeps its streams' inline search tables (include/minlz_hip_stream_set_tables.h) in plain Python.
What is FOUND is the plain set's model over the concatenated decoded bytes (tests/stream_set_model.py, grep_model.py, regex_model.py,
records_model.py): a plan never changes it.  What is DECODED: per stream the tables a searcher finds (0x45 as search_model.read_tables reads
them, 0x46 through search_compressed_model), the class rule of search_batch_prune_model.plan, the single stream's verdict per chunk inside
the chunk's own stream (rule a), and rules c and d — the crossing flags, the tail chunks and the marking that stops at or passes a stream's
end — as plain loops.  tests/test_stream_set_tables_host.py holds the shared C++ rules (minlz_amd/csrc/mlz_stream_set_tables.h) against
marks(), tests/test_gpu_stream_set_tables.py the library against plan()."""
import oracle as O
from tests import fold_model as FM
from tests import search_batch_prune_model as PM
from tests import search_compressed_model as CM
from tests import search_model as SMod

MAX_CLASSES = PM.MAX_CLASSES
SKIP, WHOLE, PRUNE = 0, 1, 2


def cross_flags(sizes, last_is_delim=None):
    """cross[i] per stream from the streams' decoded sizes: stream i has bytes and a later stream has bytes; with last_is_delim (a
    record-bound call: per stream whether its last byte is the delimiter) in addition the stream does not end with the delimiter."""
    out = []
    for i, s in enumerate(sizes):
        c = s > 0 and any(sizes[i + 1:])
        if last_is_delim is not None:
            c = c and not last_is_delim[i]
        out.append(bool(c))
    return out


def tail(chunks, k, L):
    """Rule c: chunk k of a stream whose chunks decode to `chunks` bytes holds one of the stream's last L - 1 bytes."""
    return chunks[k] > 0 and sum(chunks[k + 1:]) < L - 1


def marks(streams, modes, cross, verdicts, L):
    """streams[i]: the decoded sizes of stream i's chunks; modes[i]: SKIP (left out: its chunks are not in the list), WHOLE or PRUNE;
    verdicts[i][k]: rule a's verdict on chunk k of a pruned stream -> the sorted numbers, in the handle's chunk list, of the chunks one
    pattern of L bytes has decoded."""
    flat = [(i, k, n) for i, ch in enumerate(streams) if modes[i] != SKIP for k, n in enumerate(ch)]
    take = set()
    for g, (i, k, n) in enumerate(flat):
        if not n:
            continue
        if not (modes[i] == WHOLE or verdicts[i][k] or (cross[i] and tail(streams[i], k, L))):
            continue
        take.add(g)
        need, last = L - 1, i
        for h in range(g + 1, len(flat)):
            if need <= 0:
                break
            j, _, m = flat[h]
            if not m:
                continue
            if j != last:
                if not cross[last]:
                    break
                last = j
            take.add(h)
            need -= m
    return sorted(take)


def read_tables(stream, ignore_crc=False):
    """search_model.read_tables with compressed tables: (cfg, B, tables, packed) with tables[k] = (table, R) or None per data chunk — the
    first fitting 0x45 with a good CRC or 0x46 that parses, decodes and has a good CRC between the data chunk before and itself — and
    packed[k]: it came from a 0x46 chunk."""
    cfg = B = None
    seen_id = info_done = False
    tables, packed, cur, cur46 = [], [], None, False
    for p, t, n in SMod.chunks_of(stream):
        body = stream[p + 4:p + 4 + n]
        if t in (0x01, 0x02, 0x03):
            tables.append(cur)
            packed.append(cur46)
            cur, cur46, info_done = None, False, True
        elif t == 0xFF:
            seen_id = True
        elif t == SMod.CHUNK_INFO and seen_id and not info_done:
            info_done = True
            got = SMod.info_of(body, (1, 2, 3, 4))
            if got is not None:
                cfg, B = (got[0], got[1], got[3]), got[2]
        elif t == SMod.CHUNK_TABLE and cfg is not None and cur is None:
            fit = SMod.table_fits(body, cfg, B)
            if fit is not None and (ignore_crc or O.crc(fit[0]) == fit[2]):
                cur = fit[:2]
        elif t == CM.CHUNK_COMPRESSED and cfg is not None and cur is None:
            try:
                R, bm = CM.parse_compressed_table(body, (cfg[0], cfg[1], B, bytes(cfg[2])), ignore_crc)
                cur, cur46 = (bm, R), True
            except CM.Invalid:
                pass
    return cfg, B, tables, packed


def _probes(tables, pattern, cfg, B, fold):
    chk = FM.checks(cfg, FM.fold(pattern), B) if fold else SMod.checks(cfg, pattern, B)
    groups, t_min = chk
    probe = FM.probe if fold else SMod.probe
    pr = [probe(t[0], t[1], B, groups) if t is not None else (len(groups), len(groups)) for t in tables]
    return [p[0] for p in pr], [p[1] for p in pr], len(groups), t_min


def _windowed(cfg, B, pattern, fold):
    if fold:
        return bool(FM.windows(pattern, cfg)[0])
    return SMod.checks(cfg, pattern, B) is not None


def plan(streams, datas, patterns, healthy=None, records=False, delim=10, ignore_crc=False, fold=False):
    """streams: every stream's bytes; datas: their decoded bytes; healthy[i] False: left out for a framing error.  records: a record-bound
    call (grep, the pruned regex grep) with the delimiter `delim` -> dict(take: the chunks decoded, as numbers in the handle's chunk list;
    decoded: their number; nck: the handle's data chunks; info: what mlz_dev_reader_set_tables_info reports; unserved: the patterns to which
    no pruning class gives a window; modes; per: per stream the chunks decoded, numbered inside the stream)."""
    n = len(streams)
    healthy = [True] * n if healthy is None else healthy
    read = [read_tables(s, ignore_crc) if ok else None for s, ok in zip(streams, healthy)]
    sizes = [[m for m, _ in SMod.data_grid(s)] if ok else [] for s, ok in zip(streams, healthy)]
    classes = []
    for r in read:
        if r is not None and r[0] is not None:
            key = (r[0][0], r[0][1], r[1], bytes(r[0][2]))
            if key not in classes:
                classes.append(key)
    modes, used = [], set()
    for r, ok in zip(read, healthy):
        if not ok:
            modes.append(SKIP)
            continue
        key = None if r[0] is None else (r[0][0], r[0][1], r[1], bytes(r[0][2]))
        if key is not None and classes.index(key) < MAX_CLASSES:
            used.add(key)
        prunes = key is not None and classes.index(key) < MAX_CLASSES and PM.served(r[0], r[1], patterns, fold)
        modes.append(PRUNE if prunes else WHOLE)
    total = [sum(s) for s in sizes]
    last_is_delim = [bool(t) and datas[i][-1] == delim for i, t in enumerate(total)] if records else None
    cross = cross_flags(total, last_is_delim)
    take = set()
    for p in patterns:
        verdicts = []
        for i in range(n):
            if modes[i] != PRUNE:
                verdicts.append(None)
                continue
            a, s, nw, t_min = _probes(read[i][2], p, read[i][0], read[i][1], fold)
            verdicts.append(SMod.admits(a, s, sizes[i], nw, len(p), t_min))
        take |= set(marks(sizes, modes, cross, verdicts, len(p)))
    flat = [(i, k) for i in range(n) if modes[i] != SKIP for k in range(len(sizes[i]))]
    per = [[] for _ in range(n)]
    for g in sorted(take):
        per[flat[g][0]].append(flat[g][1])
    pruned = [i for i in range(n) if modes[i] == PRUNE]
    unserved = len(patterns) if not pruned else sum(1 for p in patterns if not any(_windowed((c[0], c[1], c[3]), c[2], p, fold) for c in used))
    info = (len(classes), len(pruned), sum(1 for i in range(n) if modes[i] == WHOLE and total[i]),
            sum(t is not None for i in pruned for t in read[i][2]), sum(bool(x) for i in pruned for x in read[i][3]), sum(cross) if pruned else 0)
    return dict(take=sorted(take), decoded=len(take) if pruned else sum(1 for s in sizes for m in s if m), nck=len(flat), info=info, unserved=unserved, modes=modes, per=per,
                cross=cross)
