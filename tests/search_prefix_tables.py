"""Block search tables with byte prefixes (the reference's SPEC_SEARCH.md 2.0, 2.1, 3.2, 3.3, A.3, B.1: table type 2, 1 to 8 prefix byte
values, and type 3, a 256-bit mask of them) in plain Python and numpy, written from the specification alone, next to tests/search_tables.py
(type 1), whose hash, chunk framing, probe and brute-force search it reuses.  A block's table holds the windows at the positions q >= 1
whose preceding byte is a prefix byte; the searcher looks up the pattern's windows that follow a prefix byte of the pattern."""
import numpy as np

import oracle as O
from tests.search_tables import CHUNK_INFO, CHUNK_TABLE, brute, chunks_of, chunks_touched, data_grid, frame, hash_windows, probe, table_bits  # noqa: F401

FOLD_LIMIT = 10          # per cent of the folded bits (type 1: 25)
NON_ALNUM = bytes(v for v in range(256) if not (48 <= v <= 57 or 65 <= v <= 90 or 97 <= v <= 122))   # every non-alphanumeric byte


def field_of(values):
    """The prefix field of a set of byte values as the Python front end writes it: 1 .. 8 distinct values -> (2, the sorted values, the last
    one repeated to 8 bytes); otherwise -> (3, the 32 mask bytes)."""
    vals = sorted(set(bytes(values)))
    if 1 <= len(vals) <= 8:
        return 2, bytes(vals + [vals[-1]] * (8 - len(vals)))
    m = bytearray(32)
    for v in vals:
        m[v >> 3] |= 1 << (v & 7)
    return 3, bytes(m)


def field_len(T):
    return {1: 0, 2: 8, 3: 32}[T]


def mask_of(T, field):
    """256 booleans: which byte values are prefix bytes."""
    m = np.zeros(256, dtype=bool)
    if T == 2:
        m[list(field[:8])] = True
    elif T == 3:
        for v in range(256):
            m[v] = (field[v >> 3] >> (v & 7)) & 1
    return m


def indexed_hashes(block, nxt, B, M, mask):
    """The hashes a block's table holds.  nxt: the bytes of the next block, None for the stream's last block."""
    blk = np.frombuffer(bytes(block), np.uint8)
    n = len(blk)
    if nxt is not None:
        ov = np.zeros(M, np.uint8)
        head = np.frombuffer(bytes(nxt[:M]), np.uint8)
        ov[:len(head)] = head
        ext = np.concatenate([blk, ov])
        q_hi = n                      # 1 <= q <= n
    else:
        ext = blk
        q_hi = n - M                  # 1 <= q <= n - M
    if q_hi < 1:
        return np.zeros(0, np.uint32)
    h = hash_windows(ext, B, M)       # position q -> h[q], q = 0 .. len(ext) - M
    q = np.arange(1, q_hi + 1)
    return h[q[mask[ext[q - 1]]]]


def build_table(block, nxt, B, M, mask):
    """-> (table bytes, R) or (None, 0) when more than 70 % of the unfolded bits are set.  No indexed position: 32 zero bytes, R = B - 8."""
    bits = np.zeros(1 << B, dtype=bool)
    bits[indexed_hashes(block, nxt, B, M, mask)] = True
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


def info_chunk(T, M, B, field):
    return frame(CHUNK_INFO, bytes([T, M, B]) + bytes(field))


def table_chunk(table, R, T, M, B, field, crc=None):
    crc = O.crc(table) if crc is None else crc
    return frame(CHUNK_TABLE, bytes([T, M, B]) + bytes(field) + bytes([R]) + crc.to_bytes(4, "little") + table)


def splice(stream, data, T, M, B, field, stored_too=False, index=False, skip=()):
    """The stream with an info chunk behind its identifier and a table chunk in front of every 0x02 / 0x03 data chunk (of 0x01 chunks as
    well with stored_too; never of the data chunks listed in `skip`) whose block passes the population rule.  `data` is the decoded
    stream.  A seek index at the end is dropped, or with index=True rebuilt over the new offsets.  -> (stream, tables) with
    tables[k] = (table, R) or None per data chunk."""
    from minlz_amd import index as I
    data = bytes(data)
    mask = mask_of(T, field)
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
            nxt = data[u + sizes[k]:u + sizes[k] + 8] if k + 1 < len(sizes) else None
            tab, R = build_table(blk, nxt, B, M, mask) if ((t != 0x01 or stored_too) and k not in skip) else (None, 0)
            tables.append(None if tab is None else (tab, R))
            idx.add(o, u)
            if tab is not None:
                tc = table_chunk(tab, R, T, M, B, field)
                out.append(tc)
                o += len(tc)
            u += sizes[k]
            k += 1
        out.append(raw)
        o += len(raw)
        if t == 0xFF:
            ic = info_chunk(T, M, B, field)
            out.append(ic)
            o += len(ic)
    if index:
        out.append(idx.append_to(len(data), o))
    return b"".join(out), tables


def read_tables(stream, ignore_crc=False):
    """What a searcher finds: (T, M, B, field, tables), tables[k] = (table, R) or None per data chunk; T is None without a usable info chunk
    (the first 0x44 between the identifier and the first data chunk, of type 1 .. 3, valid M and B and a payload that holds the field).  A
    data chunk's table: the first 0x45 in front of it whose T, M, B and field equal the info chunk's, with R <= B - 8, a payload of
    3 + field + 5 + 2^(B - R - 3) bytes and (unless ignore_crc) a good CRC."""
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
            if n >= 3 and 1 <= body[0] <= 3 and 1 <= body[1] <= 8 and 8 <= body[2] <= 23 and n >= 3 + field_len(body[0]):
                T, M, B = body[0], body[1], body[2]
                field = bytes(body[3:3 + field_len(T)])
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


def windows(pattern, T, M, field):
    """(W, t_min): the starts of the checkable windows in ascending order.  Type 1: every window, t_min = 1."""
    P, L = bytes(pattern), len(pattern)
    if T == 1:
        return list(range(0, L - M + 1)), 1
    mask = mask_of(T, field)
    return [i for i in range(1, L - M + 1) if mask[P[i - 1]]], (1 if mask[P[0]] else 0)


def decoded_set(a, s, sizes, nw, L, t_min):
    """a[k], s[k]: the leading and trailing runs of present windows per data chunk; sizes[k] its decoded bytes -> the chunks to decode."""
    n = len(sizes)
    take = set()
    for k in range(n):
        if not sizes[k]:
            continue
        last = k + 1 == n
        cand = a[k] == nw
        if not cand and not last:
            s_next = nw if sizes[k + 1] < L else s[k + 1]
            cand = max(t_min, nw - s_next) <= a[k]
        if not cand:
            continue
        take.add(k)
        need, j = L - 1, k + 1
        while need > 0 and j < n:
            if sizes[j]:
                take.add(j)
            need -= sizes[j]
            j += 1
    return sorted(take)


def usable_tables(tables, pattern, T, M, field):
    """What stats[2] reports: the tables found, or 0 when they cannot serve the pattern."""
    if T is None or not windows(pattern, T, M, field)[0]:
        return 0
    return sum(t is not None for t in tables)


def plan(tables, sizes, pattern, T, M, B, field, use_tables=True):
    """The chunks a search for `pattern` decodes."""
    L = len(pattern)
    everything = [k for k in range(len(sizes)) if sizes[k]]
    if not use_tables or T is None or not any(t is not None for t in tables):
        return everything
    W, t_min = windows(pattern, T, M, field)
    if not W:
        return everything
    P = np.frombuffer(bytes(pattern), np.uint8)
    h = hash_windows(P, B, M)
    hs = [int(h[i]) for i in W]
    nw = len(hs)
    pr = [probe(t[0], t[1], B, hs) if t is not None else (nw, nw) for t in tables]
    return decoded_set([p[0] for p in pr], [p[1] for p in pr], sizes, nw, L, t_min)
