"""Block search tables with a long prefix and extra matches (the reference's SPEC_SEARCH.md 3.3.4, A.4, B.1: table type 4) in plain Python
and numpy, written from the specification alone, next to tests/search_tables.py (type 1) and tests/search_prefix_tables.py (types 2 and 3),
whose hash, chunk framing, probe and brute-force search it reuses.

A block's table holds, for every start p of the K-byte prefix that belongs to the block, the E + 1 windows of M bytes at p + K + j,
j = 0 .. E.  An occurrence belongs to the block in which its prefix starts; prefix and windows run into the K - 1 + M + E bytes that follow
the block in the stream, the windows into zeros beyond the stream's end (a prefix lies inside the stream).  The searcher looks up the groups
of E + 1 windows behind the prefix's occurrences in the pattern, group by group."""
import numpy as np

import oracle as O
from tests import search_prefix_tables as SP
from tests.search_tables import CHUNK_INFO, CHUNK_TABLE, brute, chunks_of, chunks_touched, data_grid, frame, hash_windows, table_bits  # noqa: F401

FOLD_LIMIT = 10          # per cent of the folded bits, as for types 2 and 3
T4 = 4


def field_of(prefix, extras):
    """`K-1 | E | pfx`: the field behind `T M B` in the info chunk and in every table chunk."""
    prefix = bytes(prefix)
    assert 1 <= len(prefix) <= 256 and 0 <= extras <= 15
    return bytes([len(prefix) - 1, extras]) + prefix


def parts_of(field):
    """-> (K, E, prefix)"""
    return field[0] + 1, field[1], bytes(field[2:3 + field[0]])


def overlap(M, field):
    K, E, _ = parts_of(field)
    return K - 1 + M + E


def indexed_starts(block, follow, M, field):
    """The prefix starts a block of n bytes indexes.  follow: the bytes that follow the block in the stream (the first K - 1 + M + E of them
    are looked at), None for the stream's last block.  With a block behind: every start 0 .. n - 1 whose prefix lies inside the stream; the
    last block: the starts 0 .. n - K - M - E."""
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


def indexed_hashes(block, follow, B, M, field):
    """The hashes a block's table holds: HashValue of the window at p + K + j, j = 0 .. E, for every indexed start p."""
    K, E, _ = parts_of(field)
    starts = np.array(indexed_starts(block, follow, M, field), dtype=np.int64)
    if not len(starts):
        return np.zeros(0, np.uint32)
    ov = K - 1 + M + E
    ext = np.zeros(len(block) + ov, np.uint8)
    ext[:len(block)] = np.frombuffer(bytes(block), np.uint8)
    if follow is not None:
        head = np.frombuffer(bytes(follow[:ov]), np.uint8)
        ext[len(block):len(block) + len(head)] = head
    h = hash_windows(ext, B, M)
    return np.concatenate([h[starts + K + j] for j in range(E + 1)])


def build_table(block, follow, B, M, field):
    """-> (table bytes, R) or (None, 0) when more than 70 % of the unfolded bits are set.  No indexed start: 32 zero bytes, R = B - 8."""
    bits = np.zeros(1 << B, dtype=bool)
    bits[indexed_hashes(block, follow, B, M, field)] = True
    if int(bits.sum()) * 100 // (1 << B) > 70:
        return None, 0
    R = 0
    while len(bits) // 8 >= 64:
        half = len(bits) // 2
        m = bits[:half] | bits[half:]
        if int(m.sum()) * 100 > half * FOLD_LIMIT:
            break
        bits, R = m, R + 1
    return np.packbits(bits, bitorder="little").tobytes(), R


def info_chunk(M, B, field):
    return frame(CHUNK_INFO, bytes([T4, M, B]) + bytes(field))


def table_chunk(table, R, M, B, field, crc=None):
    crc = O.crc(table) if crc is None else crc
    return frame(CHUNK_TABLE, bytes([T4, M, B]) + bytes(field) + bytes([R]) + crc.to_bytes(4, "little") + table)


def splice(stream, data, M, B, field, stored_too=False, index=False, skip=()):
    """The stream with a type 4 info chunk behind its identifier and a table chunk in front of every 0x02 / 0x03 data chunk (of 0x01 chunks
    as well with stored_too; never of the data chunks listed in `skip`) whose block passes the population rule.  `data` is the decoded
    stream.  A seek index at the end is dropped, or with index=True rebuilt over the new offsets.  -> (stream, tables) with
    tables[k] = (table, R) or None per data chunk."""
    from minlz_amd import index as I
    data = bytes(data)
    ov = overlap(M, field)
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
            follow = data[u + sizes[k]:u + sizes[k] + ov] if k + 1 < len(sizes) else None
            tab, R = build_table(blk, follow, B, M, field) if ((t != 0x01 or stored_too) and k not in skip) else (None, 0)
            tables.append(None if tab is None else (tab, R))
            idx.add(o, u)
            if tab is not None:
                tc = table_chunk(tab, R, M, B, field)
                out.append(tc)
                o += len(tc)
            u += sizes[k]
            k += 1
        out.append(raw)
        o += len(raw)
        if t == 0xFF:
            ic = info_chunk(M, B, field)
            out.append(ic)
            o += len(ic)
    if index:
        out.append(idx.append_to(len(data), o))
    return b"".join(out), tables


def info_of(body):
    """(T, M, B, field) of an info chunk's payload, or None: a type 1 .. 4, valid M and B, a payload that holds the field, and for type 4
    E <= 15 and M + E <= 16."""
    n = len(body)
    if n < 3 or not (1 <= body[0] <= 4 and 1 <= body[1] <= 8 and 8 <= body[2] <= 23):
        return None
    T, M, B = body[0], body[1], body[2]
    if T == 4:
        if n < 5 or body[4] > 15 or M + body[4] > 16 or n < 5 + body[3] + 1:
            return None
        f = 3 + body[3]
    else:
        f = SP.field_len(T)
        if n < 3 + f:
            return None
    return T, M, B, bytes(body[3:3 + f])


def read_tables(stream, ignore_crc=False):
    """What a searcher finds: (T, M, B, field, tables), tables[k] = (table, R) or None per data chunk; T is None without a usable info chunk
    (the first 0x44 between the identifier and the first data chunk).  A data chunk's table: the first 0x45 in front of it whose T, M, B
    and field equal the info chunk's, with R <= B - 8, a payload of 3 + field + 5 + 2^(B - R - 3) bytes and (unless ignore_crc) a good CRC."""
    T = M = B = None
    field = b""
    seen_id = info_done = False
    tables, cur, n_data = [], None, 0
    for p, t, n in chunks_of(stream):
        body = stream[p + 4:p + 4 + n]
        if t in (0x01, 0x02, 0x03):
            tables.append(cur)
            cur, info_done, n_data = None, True, n_data + 1
        elif t == 0xFF:
            seen_id = True
        elif t == CHUNK_INFO and seen_id and not info_done:
            info_done = True
            got = info_of(body)
            if got is not None:
                T, M, B, field = got
        elif t == CHUNK_TABLE and T is not None and cur is None:
            f = len(field)
            if n >= 8 + f + 32 and bytes(body[:3 + f]) == bytes([T, M, B]) + field:
                R = body[3 + f]
                if R <= B - 8 and n - 8 - f == 1 << (B - R - 3):
                    tab = bytes(body[8 + f:])
                    if ignore_crc or O.crc(tab) == int.from_bytes(body[4 + f:8 + f], "little"):
                        cur = (tab, R)
    if T is None:
        tables = [None] * n_data
    return T, M, B, field, tables


def groups(pattern, M, field):
    """(G, t_min): the starts i of the prefix's occurrences in the pattern with i + K + M + E <= L, ascending; t_min = 1 when the first
    group has i = 0."""
    K, E, pfx = parts_of(field)
    P, L = bytes(pattern), len(pattern)
    G = [i for i in range(0, L - K - M - E + 1) if P[i:i + K] == pfx]
    return G, (1 if G and G[0] == 0 else 0)


def probe(table, R, B, group_hashes):
    """(a, s): the leading and the trailing whole groups present in one table; (ng, ng) without a table."""
    ng = len(group_hashes)
    if table is None:
        return ng, ng
    mask = (1 << (B - R)) - 1
    has = [all((table[(h & mask) >> 3] >> ((h & mask) & 7)) & 1 for h in hs) for hs in group_hashes]
    a = next((i for i, x in enumerate(has) if not x), ng)
    if a == ng:
        return ng, ng
    return a, next((i for i, x in enumerate(reversed(has)) if not x), ng)


def usable_tables(tables, pattern, T, M, field):
    """What stats[2] reports: the tables found, or 0 when they cannot serve the pattern."""
    if T is None:
        return 0
    if T != 4:
        return SP.usable_tables(tables, pattern, T, M, field)
    if not groups(pattern, M, field)[0]:
        return 0
    return sum(t is not None for t in tables)


def plan(tables, sizes, pattern, T, M, B, field, use_tables=True):
    """The chunks a search for `pattern` decodes."""
    if T is not None and T != 4:
        return SP.plan(tables, sizes, pattern, T, M, B, field, use_tables)
    L = len(pattern)
    everything = [k for k in range(len(sizes)) if sizes[k]]
    if not use_tables or T is None or not any(t is not None for t in tables):
        return everything
    G, t_min = groups(pattern, M, field)
    if not G:
        return everything
    K, E, _ = parts_of(field)
    h = hash_windows(np.frombuffer(bytes(pattern), np.uint8), B, M)
    gh = [[int(h[i + K + j]) for j in range(E + 1)] for i in G]
    ng = len(gh)
    pr = [probe(t[0], t[1], B, gh) if t is not None else (ng, ng) for t in tables]
    return SP.decoded_set([p[0] for p in pr], [p[1] for p in pr], sizes, ng, L, t_min)
