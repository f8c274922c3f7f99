"""Block search tables (the reference's SPEC_SEARCH.md, table type 1, uncompressed table chunks) in plain Python and numpy, written from
the specification alone: the hash, a block's table and its reductions, the chunk bytes, a function that splices tables into any stream, the
searcher's plan rule (Appendix B.4.1) and a brute-force search.  The tests of the Writer's tables and of mlz_dev_reader_search compare the
library with this model."""
import numpy as np

import oracle as O
from minlz_amd import stream as S

CHUNK_INFO, CHUNK_TABLE = 0x44, 0x45
PRIMES = {2: 40503, 3: 506832829, 4: 2654435761, 5: 889523592379, 6: 227718039650203, 7: 58295818150454627, 8: 0xCF1BBCDCB7A56463}
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


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


def build_table(block, nxt, B, M):
    """block: the block's bytes; nxt: the bytes of the next block (None for the stream's last block) -> (table bytes, R) or (None, 0)."""
    blk = np.frombuffer(bytes(block), np.uint8)
    if nxt is not None:
        ov = np.zeros(M - 1, np.uint8)
        head = np.frombuffer(bytes(nxt[:M - 1]), np.uint8)
        ov[:len(head)] = head
        blk = np.concatenate([blk, ov])
    bits = np.zeros(1 << B, dtype=bool)
    bits[hash_windows(blk, B, M)] = True
    if int(bits.sum()) * 100 // (1 << B) > 70:
        return None, 0
    R = 0
    while len(bits) // 8 >= 64:
        half = len(bits) // 2
        m = bits[:half] | bits[half:]
        if int(m.sum()) * 100 > half * 25:
            break
        bits, R = m, R + 1
    return np.packbits(bits, bitorder="little").tobytes(), R


def frame(type_, body):
    n = len(body)
    return bytes([type_, n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF]) + body


def info_chunk(M, B):
    return frame(CHUNK_INFO, bytes([1, M, B]))


def table_chunk(table, R, M, B, crc=None):
    crc = O.crc(table) if crc is None else crc
    return frame(CHUNK_TABLE, bytes([1, M, B, R]) + crc.to_bytes(4, "little") + table)


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


def splice(stream, data, M, B, stored_too=False, index=False):
    """The stream with an info chunk behind its identifier and a table chunk in front of every 0x02 / 0x03 data chunk (of 0x01 chunks as
    well with stored_too) whose block passes the population rule.  `data` is the decoded stream.  A seek index at the end is dropped, or
    with index=True rebuilt over the new offsets (a block's entry: where its chunks start).  -> (stream, tables) with tables[k] = (table, R)
    or None per data chunk."""
    from minlz_amd import index as I
    data = bytes(data)
    cks = chunks_of(stream)
    sizes = [n for n, _ in data_grid(stream)]
    out, tables, k, u = [], [], 0, 0
    idx = I.Index()
    block_size = 1 << (stream[9] + 10) if len(stream) >= 10 else 1 << 20
    idx.reset(block_size)
    o = 0
    if cks:
        idx.add(0, 0)
    for p, t, n in cks:
        raw = stream[p:p + 4 + n]
        if t == 0x40 and raw[4:10] == b"s2idx\x00":
            continue
        if t in (0x01, 0x02, 0x03):
            blk = data[u:u + sizes[k]]
            nxt = data[u + sizes[k]:u + sizes[k] + min(8, sizes[k + 1])] if k + 1 < len(sizes) else None   # (zeros beyond a short next block)
            tab, R = build_table(blk, nxt, B, M) if (t != 0x01 or stored_too) else (None, 0)
            tables.append(None if tab is None else (tab, R))
            idx.add(o, u)
            if tab is not None:
                tc = table_chunk(tab, R, M, B)
                out.append(tc)
                o += len(tc)
            u += sizes[k]
            k += 1
        out.append(raw)
        o += len(raw)
        if t == 0xFF:
            ic = info_chunk(M, B)
            out.append(ic)
            o += len(ic)
    if index:
        out.append(idx.append_to(len(data), o))
    return b"".join(out), tables


def probe(table, R, B, hashes):
    """(a, s): the leading and the trailing windows present in one table; (nw, nw) without a table."""
    nw = len(hashes)
    if table is None:
        return nw, nw
    mask = (1 << (B - R)) - 1
    has = [(table[(h & mask) >> 3] >> ((h & mask) & 7)) & 1 for h in hashes]
    a = next((i for i, x in enumerate(has) if not x), nw)
    if a == nw:
        return nw, nw
    s = next((i for i, x in enumerate(reversed(has)) if not x), nw)
    return a, s


def window_hashes(pattern, B, M):
    return [int(h) for h in hash_windows(np.frombuffer(bytes(pattern), np.uint8), B, M)]


def decoded_set(a, s, sizes, nw, L):
    """The plan rule: a[k], s[k] per data chunk, sizes[k] its decoded bytes -> sorted list of the chunks to decode."""
    n = len(sizes)
    take = set()
    for k in range(n):
        if not sizes[k]:
            continue
        last = k + 1 == n
        cand = a[k] == nw
        if not cand and not last:
            s_next = nw if sizes[k + 1] < L else s[k + 1]
            cand = max(1, nw - s_next) <= min(a[k], nw - 1)
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


def plan(tables, sizes, pattern, M, B, use_tables=True):
    """tables[k] = (table, R) or None -> the chunks a search for `pattern` decodes."""
    L = len(pattern)
    if not use_tables or M is None or L < M:
        return [k for k in range(len(sizes)) if sizes[k]]
    hs = window_hashes(pattern, B, M)
    nw = len(hs)
    pr = [probe(t[0], t[1], B, hs) if t is not None else (nw, nw) for t in tables]
    return decoded_set([p[0] for p in pr], [p[1] for p in pr], sizes, nw, L)


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


def read_tables(stream, ignore_crc=False):
    """What a searcher finds in a stream: (M, B, tables) with tables[k] = (table, R) or None per data chunk; M is None without a usable
    info chunk (the first 0x44 between the identifier and the first data chunk).  A data chunk's table: the first 0x45 chunk between the
    data chunk before it and itself of type 1, the stream's M and B, R <= B - 8, a payload that fits and (unless ignore_crc) a good CRC."""
    M = B = None
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
            if n >= 3 and body[0] == 1 and 1 <= body[1] <= 8 and 8 <= body[2] <= 23:
                M, B = body[1], body[2]
        elif t == CHUNK_TABLE and M is not None and cur is None and n >= 40:
            R = body[3]
            if body[0] == 1 and body[1] == M and body[2] == B and R <= B - 8 and n - 8 == 1 << (B - R - 3):
                tab = bytes(body[8:])
                if ignore_crc or O.crc(tab) == int.from_bytes(body[4:8], "little"):
                    cur = (tab, R)
    if M is None:
        tables = [None] * n_data
    return M, B, tables
