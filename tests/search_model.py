"""Block search tables (the reference's SPEC_SEARCH.md, table types 1 to 4, uncompressed table chunks) in plain Python and numpy, written
from the specification alone: the hash, a block's table and its reductions, the chunk bytes, a function that splices tables into any stream,
the searcher's plan rule (Appendix B.4.1) and a brute-force search.  The tests of the Writer's tables, of the searches and of the sidecars
compare the library with this model.

A configuration is cfg = (T, M, field): the table type, the match length and the prefix field as the chunks carry it behind `T M B`; the
table size B goes beside it.
  type 1   no field.  A block's table holds every window of M bytes that starts in the block; the searcher looks up every window of the
           pattern.
  type 2   1 to 8 prefix byte values, the last one repeated to 8 bytes; type 3: a 256-bit mask of them.  The table holds the windows at the
           positions q >= 1 behind a prefix byte; the searcher looks up the pattern's windows that follow a prefix byte of the pattern.
  type 4   `K-1 | E | prefix`.  The table holds, for every start p of the K-byte prefix that belongs to the block, the E + 1 windows at
           p + K + j, j = 0 .. E.  An occurrence belongs to the block in which its prefix starts; a prefix lies inside the stream, the
           windows run into zeros beyond its end.  The searcher looks up the groups of E + 1 windows behind the prefix's occurrences in the
           pattern, group by group.
T is looked at in the first section below only; everything behind it works on hashes, groups of hashes and t_min."""
import numpy as np

import oracle as O
from minlz_amd import stream as S

CHUNK_INFO, CHUNK_TABLE = 0x44, 0x45
PRIMES = {2: 40503, 3: 506832829, 4: 2654435761, 5: 889523592379, 6: 227718039650203, 7: 58295818150454627, 8: 0xCF1BBCDCB7A56463}
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
NON_ALNUM = bytes(v for v in range(256) if not (48 <= v <= 57 or 65 <= v <= 90 or 97 <= v <= 122))   # every non-alphanumeric byte


def hash_value(val, B, M):
    """HashValue(val, tableSize, matchLen) of section 3.1 with Python integers."""
    if M == 1:
        return val & 0xFF
    if M == 2:
        return val & 0xFFFF if B >= 16 else (((val << 16) & M32) * PRIMES[2] & M32) >> (32 - B)
    if M == 3:
        return (((val << 8) & M32) * PRIMES[3] & M32) >> (32 - B)
    if M == 4:
        return ((val & M32) * PRIMES[4] & M32) >> (32 - B)
    return (((val << (64 - 8 * M)) & M64) * PRIMES[M] & M64) >> (64 - B)


def hash_windows(buf, B, M):
    """hash_value of the M-byte little-endian window at every position 0 .. len(buf) - M of a uint8 array."""
    n = len(buf) - M + 1
    if n <= 0:
        return np.zeros(0, np.uint32)
    v = np.zeros(n, dtype=np.uint64)
    for j in range(M):
        v |= buf[j:j + n].astype(np.uint64) << np.uint64(8 * j)
    if M == 1:
        return v.astype(np.uint32)
    if M == 2 and B >= 16:
        return v.astype(np.uint32)
    if M <= 4:
        w = (v << np.uint64({2: 16, 3: 8, 4: 0}[M])).astype(np.uint32)
        return (w * np.uint32(PRIMES[M])) >> np.uint32(32 - B)
    return (((v << np.uint64(64 - 8 * M)) * np.uint64(PRIMES[M])) >> np.uint64(64 - B)).astype(np.uint32)


def table_bits(block_size):
    return max(8, min(23, (block_size - 1).bit_length()))


# ---- the four table types ----

def config(T, M, prefix=b"", extras=0):
    """(T, M, field) as api.search_config describes it: type 2 keeps 1 .. 8 values in the order given (the last one repeated), type 3 makes
    the mask of the values, type 4 is `K-1 | E | prefix`."""
    prefix = bytes(prefix)
    if T == 1:
        return 1, M, b""
    if T == 2:
        assert 1 <= len(prefix) <= 8
        return 2, M, prefix + prefix[-1:] * (8 - len(prefix))
    if T == 3:
        m = bytearray(32)
        for v in prefix:
            m[v >> 3] |= 1 << (v & 7)
        return 3, M, bytes(m)
    assert 1 <= len(prefix) <= 256 and 0 <= extras <= 15
    return 4, M, bytes([len(prefix) - 1, extras]) + prefix


def field_of(values):
    """The prefix field of a set of byte values as the Python front end writes it: 1 .. 8 distinct values -> (2, the sorted values, the last
    one repeated to 8 bytes); otherwise -> (3, the 32 mask bytes)."""
    vals = bytes(sorted(set(bytes(values))))
    T = 2 if 1 <= len(vals) <= 8 else 3
    return T, config(T, 0, vals)[2]


def field_len(T):
    return {1: 0, 2: 8, 3: 32}[T]


def info_of(body, types=(1, 2, 3, 4)):
    """(T, M, B, field) of an info chunk's payload, or None: a type among `types`, valid M and B, a payload that holds the field, and for
    type 4 E <= 15 and M + E <= 16."""
    n = len(body)
    if n < 3 or not (body[0] in types and 1 <= body[1] <= 8 and 8 <= body[2] <= 23):
        return None
    T, M, B = body[0], body[1], body[2]
    if T == 4:
        if n < 5 or body[4] > 15 or M + body[4] > 16 or n < 5 + body[3] + 1:
            return None
        f = 3 + body[3]
    else:
        f = field_len(T)
        if n < 3 + f:
            return None
    return T, M, B, bytes(body[3:3 + f])


def mask_of(T, field):
    """256 booleans: which byte values are prefix bytes (types 2 and 3)."""
    m = np.zeros(256, dtype=bool)
    if T == 2:
        m[list(field[:8])] = True
    elif T == 3:
        for v in range(256):
            m[v] = (field[v >> 3] >> (v & 7)) & 1
    return m


def parts_of(field):
    """Type 4 -> (K, E, prefix)"""
    return field[0] + 1, field[1], bytes(field[2:3 + field[0]])


def overlap(cfg):
    """The bytes behind a block that its table looks at."""
    T, M, field = cfg
    if T == 1:
        return M - 1
    if T in (2, 3):
        return M
    K, E, _ = parts_of(field)
    return K - 1 + M + E


def fold_limit(T):
    """Per cent of the folded bits up to which a table is folded once more."""
    return 25 if T == 1 else 10


def indexed_starts(cfg, block, follow):
    """Type 4: the prefix starts a block of n bytes indexes.  With bytes behind it: every start 0 .. n - 1 whose prefix lies inside the
    stream; the last block (follow None): the starts 0 .. n - K - M - E."""
    _, M, field = cfg
    K, E, pfx = parts_of(field)
    block = bytes(block)
    n = len(block)
    if follow is None:
        hay, hi = block, n - K - M - E
    else:
        hay, hi = block + bytes(follow[:K - 1]), n - 1
    out, p = [], hay.find(pfx)
    while 0 <= p <= hi:
        out.append(p)
        p = hay.find(pfx, p + 1)
    return out


def indexed_hashes(cfg, block, follow, B):
    """The hashes a block's table holds.  follow: the bytes that follow the block (the first overlap(cfg) of them are looked at, zeros
    beyond them), None for the stream's last block, which indexes only what lies inside it."""
    T, M, field = cfg
    ext = np.frombuffer(bytes(block), np.uint8)
    n = len(ext)
    if follow is not None:
        ov = np.zeros(overlap(cfg), np.uint8)
        head = np.frombuffer(bytes(follow[:len(ov)]), np.uint8)
        ov[:len(head)] = head
        ext = np.concatenate([ext, ov])
    h = hash_windows(ext, B, M)           # position q -> h[q], q = 0 .. len(ext) - M
    if T == 1:
        return h
    if T in (2, 3):
        q_hi = n if follow is not None else n - M
        if q_hi < 1:
            return np.zeros(0, np.uint32)
        q = np.arange(1, q_hi + 1)
        return h[q[mask_of(T, field)[ext[q - 1]]]]
    K, E, _ = parts_of(field)
    starts = np.array(indexed_starts(cfg, block, follow), dtype=np.int64)
    if not len(starts):
        return np.zeros(0, np.uint32)
    return np.concatenate([h[starts + K + j] for j in range(E + 1)])


def windows(pattern, cfg):
    """Types 1 to 3 -> (W, t_min): the starts of the checkable windows in ascending order.  Type 1: every window, t_min = 1."""
    T, M, field = cfg
    P, L = bytes(pattern), len(pattern)
    if T == 1:
        return list(range(0, L - M + 1)), 1
    mask = mask_of(T, field)
    return [i for i in range(1, L - M + 1) if mask[P[i - 1]]], (1 if mask[P[0]] else 0)


def groups(pattern, cfg):
    """Type 4 -> (G, t_min): the starts i of the prefix's occurrences in the pattern with i + K + M + E <= L, ascending; t_min = 1 when the
    first group has i = 0."""
    _, M, field = cfg
    K, E, pfx = parts_of(field)
    P, L = bytes(pattern), len(pattern)
    G = [i for i in range(0, L - K - M - E + 1) if P[i:i + K] == pfx]
    return G, (1 if G and G[0] == 0 else 0)


def checks(cfg, pattern, B):
    """What a search looks up -> (groups of hashes, t_min): one group per checkable window (types 1 to 3) or per group of E + 1 windows
    (type 4), in the pattern's order; None when the tables cannot serve the pattern."""
    T, M, field = cfg
    if T == 4:
        (at, t_min), (K, E, _) = groups(pattern, cfg), parts_of(field)
    else:
        (at, t_min), K, E = windows(pattern, cfg), 0, 0
    if not at:
        return None
    h = hash_windows(np.frombuffer(bytes(pattern), np.uint8), B, M)
    return [[int(h[i + K + j]) for j in range(E + 1)] for i in at], t_min


# ---- tables and chunks ----

def build_table(cfg, block, follow, B):
    """-> (table bytes, R) or (None, 0) when more than 70 % of the unfolded bits are set.  Nothing indexed: 32 zero bytes, R = B - 8."""
    bits = np.zeros(1 << B, dtype=bool)
    bits[indexed_hashes(cfg, block, follow, B)] = True
    if int(bits.sum()) * 100 // (1 << B) > 70:
        return None, 0
    R = 0
    while len(bits) // 8 >= 64:
        half = len(bits) // 2
        m = bits[:half] | bits[half:]
        if int(m.sum()) * 100 > half * fold_limit(cfg[0]):
            break
        bits, R = m, R + 1
    return np.packbits(bits, bitorder="little").tobytes(), R


def frame(type_, body):
    n = len(body)
    return bytes([type_, n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF]) + body


def info_chunk(cfg, B):
    T, M, field = cfg
    return frame(CHUNK_INFO, bytes([T, M, B]) + bytes(field))


def table_chunk(cfg, B, table, R, crc=None):
    T, M, field = cfg
    crc = O.crc(table) if crc is None else crc
    return frame(CHUNK_TABLE, bytes([T, M, B]) + bytes(field) + bytes([R]) + crc.to_bytes(4, "little") + table)


def table_fits(body, cfg, B):
    """A 0x45 payload against a configuration -> (table, R, the CRC it names), or None: T, M, B and the field equal the configuration's,
    R <= B - 8 and a payload of 3 + field + 5 + 2^(B - R - 3) bytes."""
    T, M, field = cfg
    f, n = len(field), len(body)
    if n < 8 + f + 32 or bytes(body[:3 + f]) != bytes([T, M, B]) + field:
        return None
    R = body[3 + f]
    if R > B - 8 or n - 8 - f != 1 << (B - R - 3):
        return None
    return bytes(body[8 + f:]), R, int.from_bytes(body[4 + f:8 + f], "little")


def chunks_of(stream):
    """(offset, type, length of the payload) of every chunk."""
    p, out = 0, []
    while p + 4 <= len(stream):
        n = stream[p + 1] | stream[p + 2] << 8 | stream[p + 3] << 16
        out.append((p, stream[p], n))
        p += 4 + n
    assert p == len(stream)
    return out


def data_grid(stream):
    """[(decoded bytes, type)] of the data chunks, in stream order."""
    grid = []
    for p, t, n in chunks_of(stream):
        if t == 0x01:
            grid.append((n - 4, t))
        elif t in (0x02, 0x03):
            grid.append((S.uvarint(stream, p + 8)[0], t))
    return grid


def splice(stream, data, cfg, B, stored_too=False, index=False, skip=(), next_chunk_only=False):
    """The stream with an info chunk behind its identifier and a table chunk in front of every 0x02 / 0x03 data chunk (of 0x01 chunks as
    well with stored_too; never of the data chunks listed in `skip`) whose block passes the population rule.  `data` is the decoded
    stream; a block's table sees the data that follows it in the stream (next_chunk_only: of the next data chunk alone, zeros behind a
    short one, as a writer gives that does not look further).  A seek index at the end is dropped, or with index=True rebuilt over the new
    offsets (a block's entry: where its chunks start).  -> (stream, tables) with tables[k] = (table, R) or None per data chunk."""
    from minlz_amd import index as I
    data = bytes(data)
    ov = overlap(cfg)
    cks = chunks_of(stream)
    sizes = [n for n, _ in data_grid(stream)]
    out, tables, k, u = [], [], 0, 0
    idx = I.Index()
    idx.reset(1 << (stream[9] + 10) if len(stream) >= 10 else 1 << 20)
    o = 0
    if cks:
        idx.add(0, 0)
    for p, t, n in cks:
        raw = stream[p:p + 4 + n]
        if t == 0x40 and raw[4:10] == b"s2idx\x00":
            continue
        if t in (0x01, 0x02, 0x03):
            blk = data[u:u + sizes[k]]
            follow = data[u + sizes[k]:u + sizes[k] + (min(ov, sizes[k + 1]) if next_chunk_only else ov)] if k + 1 < len(sizes) else None
            tab, R = build_table(cfg, blk, follow, B) if ((t != 0x01 or stored_too) and k not in skip) else (None, 0)
            tables.append(None if tab is None else (tab, R))
            idx.add(o, u)
            if tab is not None:
                tc = table_chunk(cfg, B, tab, R)
                out.append(tc)
                o += len(tc)
            u += sizes[k]
            k += 1
        out.append(raw)
        o += len(raw)
        if t == 0xFF:
            ic = info_chunk(cfg, B)
            out.append(ic)
            o += len(ic)
    if index:
        out.append(idx.append_to(len(data), o))
    return b"".join(out), tables


def read_tables(stream, ignore_crc=False, types=(1, 2, 3, 4)):
    """What a searcher that knows the table types `types` finds: (cfg, B, tables) with tables[k] = (table, R) or None per data chunk; cfg and
    B are None without a usable info chunk (the first 0x44 between the identifier and the first data chunk).  A data chunk's table: the
    first 0x45 between the data chunk before it and itself that fits the configuration (table_fits) and (unless ignore_crc) has a good CRC."""
    cfg = B = None
    seen_id = info_done = False
    tables, cur = [], None
    for p, t, n in chunks_of(stream):
        body = stream[p + 4:p + 4 + n]
        if t in (0x01, 0x02, 0x03):
            tables.append(cur)
            cur, info_done = None, True
        elif t == 0xFF:
            seen_id = True
        elif t == CHUNK_INFO and seen_id and not info_done:
            info_done = True
            got = info_of(body, types)
            if got is not None:
                cfg, B = (got[0], got[1], got[3]), got[2]
        elif t == CHUNK_TABLE and cfg is not None and cur is None:
            fit = table_fits(body, cfg, B)
            if fit is not None and (ignore_crc or O.crc(fit[0]) == fit[2]):
                cur = fit[:2]
    return cfg, B, tables


# ---- the search ----

def probe(table, R, B, groups):
    """(a, s): the leading and the trailing whole groups of hashes present in one table; (n, n) without a table."""
    n = len(groups)
    if table is None:
        return n, n
    mask = (1 << (B - R)) - 1
    has = [all((table[(h & mask) >> 3] >> ((h & mask) & 7)) & 1 for h in g) for g in groups]
    a = next((i for i, x in enumerate(has) if not x), n)
    if a == n:
        return n, n
    return a, next((i for i, x in enumerate(reversed(has)) if not x), n)


def probed(tables, pattern, cfg, B):
    """One configuration's tables against the pattern -> (a, s, n, t_min) with a[k], s[k] the probe of chunk k and n the number of groups,
    or None: the tables cannot serve the pattern."""
    chk = checks(cfg, pattern, B)
    if chk is None:
        return None
    hs, t_min = chk
    pr = [probe(t[0], t[1], B, hs) if t is not None else (len(hs), len(hs)) for t in tables]
    return [p[0] for p in pr], [p[1] for p in pr], len(hs), t_min


def admits(a, s, sizes, n, L, t_min, ov=0):
    """One table set's verdict per chunk: all n groups in its own table, or a split with the next chunk's.  ov: only where a block's table
    was built over the next chunk's bytes alone (a sidecar), the set's overlap: in front of a chunk shorter than that, the windows that
    reach beyond the chunk were hashed over zeros, the table proves nothing there, and the set abstains (it admits the chunk)."""
    nck, out = len(sizes), []
    for k in range(nck):
        cand = a[k] == n or (k + 1 < nck and sizes[k + 1] < ov)
        if not cand and k + 1 < nck:
            s_next = n if sizes[k + 1] < L else s[k + 1]
            cand = max(t_min, n - s_next) <= a[k]
        out.append(cand)
    return out


def decoded_set(votes, sizes, L):
    """votes: one list of verdicts per voting table set -> the chunks to decode: every chunk with bytes that no set refuses, plus the chunks
    that hold the L - 1 bytes behind it."""
    n, take = len(sizes), set()
    for k in range(n):
        if not sizes[k] or not all(v[k] for v in votes):
            continue
        take.add(k)
        need, j = L - 1, k + 1
        while need > 0 and j < n:
            if sizes[j]:
                take.add(j)
            need -= sizes[j]
            j += 1
    return sorted(take)


def plan(tables, sizes, pattern, cfg, B, use_tables=True):
    """tables[k] = (table, R) or None -> the chunks a search for `pattern` decodes."""
    everything = [k for k in range(len(sizes)) if sizes[k]]
    if not use_tables or cfg is None or not any(t is not None for t in tables):
        return everything
    got = probed(tables, pattern, cfg, B)
    if got is None:
        return everything
    a, s, n, t_min = got
    return decoded_set([admits(a, s, sizes, n, len(pattern), t_min)], sizes, len(pattern))


def usable_tables(tables, pattern, cfg):
    """What stats[2] reports: the tables found, or 0 when they cannot serve the pattern."""
    if cfg is None or not (groups if cfg[0] == 4 else windows)(pattern, cfg)[0]:
        return 0
    return sum(t is not None for t in tables)


def plan_of_stream(stream, pattern, ignore_crc=False):
    """-> (plan, sizes, usable tables) of a search for `pattern` over `stream` by the model."""
    cfg, B, tables = read_tables(stream, ignore_crc)
    sizes = [n for n, _ in data_grid(stream)]
    return plan(tables, sizes, pattern, cfg, B), sizes, usable_tables(tables, pattern, cfg)


def brute(data, pattern):
    """Every position of `pattern` in `data`, overlapping occurrences included."""
    data, pattern = bytes(data), bytes(pattern)
    out, p = [], data.find(pattern)
    while p >= 0:
        out.append(p)
        p = data.find(pattern, p + 1)
    return out


def chunks_touched(sizes, positions, L):
    """The data chunks that hold a byte of any occurrence."""
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = set()
    for p in positions:
        k0 = int(np.searchsorted(starts, p, side="right")) - 1
        k1 = int(np.searchsorted(starts, p + L - 1, side="right")) - 1
        out.update(k for k in range(k0, k1 + 1) if sizes[k])
    return out
