"""Sidecar search indexes (the reference's SEARCH.md "Sidecar Streams", SPEC_SEARCH.md 1.1 and 2.3) in plain Python, written from the
specification alone, on top of the three table models (tests/search_tables.py: type 1, tests/search_prefix_tables.py: types 2 and 3,
tests/search_long_prefix_tables.py: type 4).

A sidecar is a valid stream without data chunks: the main stream's identifier, one info chunk (0x44) per table configuration, then for
every data chunk of the main stream its table chunks (0x45, one per configuration whose table is kept) and a remote block reference (0x47:
uvarint(offset of the data chunk's header in the main stream) uvarint(max block size - decoded bytes)), and the EOF chunk.  A searcher
skips a block when ANY configuration proves the pattern absent.

A configuration is (T, M, field): the table type, the match length and the prefix field as the chunks carry it."""
import numpy as np

import oracle as O
from tests import search_long_prefix_tables as SL
from tests import search_prefix_tables as SP
from tests import search_tables as ST

CHUNK_REF = 0x47
EOF_CHUNK = b"\x20\x01\x00\x00\x00"
MAX_CONFIGS = 4


class SidecarError(Exception):
    """kind: "corrupt" (-MLZ_ERR_CORRUPT) or "unsupported" (-MLZ_ERR_UNSUPPORTED)"""

    def __init__(self, kind, why):
        super().__init__("%s: %s" % (kind, why))
        self.kind = kind


def config(T, M=6, prefix=b"", extras=0):
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
    return 4, M, SL.field_of(prefix, extras)


def overlap(cfg):
    T, M, field = cfg
    return M - 1 if T == 1 else M if T in (2, 3) else SL.overlap(M, field)


def uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_uvarint(b, p):
    """binary.Uvarint -> (value, bytes read); bytes read 0 = cut short, < 0 = overflow."""
    x = s = 0
    for i in range(len(b) - p):
        if i == 10:
            return 0, -(i + 1)
        c = b[p + i]
        if c < 0x80:
            if i == 9 and c > 1:
                return 0, -(i + 1)
            return x | c << s, i + 1
        x |= (c & 0x7F) << s
        s += 7
    return 0, 0


def ref_chunk(hdr_off, max_minus_actual):
    return ST.frame(CHUNK_REF, uvarint(hdr_off) + uvarint(max_minus_actual))


def parse_refs(payload, max_block):
    """The references of a 0x47 payload -> [(offset, decoded bytes)], or None: an empty payload, a bad varint, a relative offset of 0, a size
    outside 1 .. max_block."""
    if not payload:
        return None
    out, p, prev = [], 0, None
    while p < len(payload):
        off, n1 = read_uvarint(payload, p)
        if n1 <= 0:
            return None
        p += n1
        mma, n2 = read_uvarint(payload, p)
        if n2 <= 0:
            return None
        p += n2
        if prev is not None and off == 0:
            return None
        a = off if prev is None else prev + off
        if a >= 1 << 63 or mma >= max_block:
            return None
        out.append((a, max_block - mma))
        prev = a
    return out


def main_chunks(stream):
    """[(header offset, decoded bytes)] of the main stream's data chunks."""
    out = []
    for p, t, n in ST.chunks_of(stream):
        if t == 0x01:
            out.append((p, n - 4))
        elif t in (0x02, 0x03):
            out.append((p, ST.S.uvarint(stream, p + 8)[0]))
    return out


def framed(data, sizes, size_byte=6):
    """A stream whose data chunks decode to `sizes` bytes of `data` each, in order (compressed by the oracle's block encoder at level 1,
    stored where that does not pay), under a header of block-size byte `size_byte`, with an EOF chunk that names the length."""
    assert sum(sizes) == len(data)
    out, o = [bytes([0xFF, 6, 0, 0]) + b"MinLz" + bytes([size_byte])], 0
    for sz in sizes:
        blk = data[o:o + sz]
        enc = O.encode(blk, 1)
        stored = len(enc) == sz + 2
        out.append(ST.frame(0x01 if stored else 0x02, O.crc(blk).to_bytes(4, "little") + (blk if stored else enc[1:])))
        o += sz
    n = uvarint(len(data))
    out.append(b"\x20" + bytes([len(n), 0, 0]) + n)
    return b"".join(out)


def identifier(stream):
    for p, t, n in ST.chunks_of(stream):
        if t == 0xFF:
            return bytes(stream[p:p + 10])
    return None


def max_block_of(ident):
    return 1 << ((ident[9] & 15) + 10)


def table_of(cfg, block, nxt, B):
    """(table, R) or (None, 0).  nxt: the next data chunk's bytes (all of them; each model cuts what it needs), None for the last one."""
    T, M, field = cfg
    if T == 1:
        return ST.build_table(block, nxt, B, M)
    if T in (2, 3):
        return SP.build_table(block, nxt, B, M, SP.mask_of(T, field))
    return SL.build_table(block, nxt, B, M, field)


def info_chunk(cfg, B):
    T, M, field = cfg
    return ST.frame(ST.CHUNK_INFO, bytes([T, M, B]) + field)


def table_chunk(cfg, B, table, R, crc=None):
    T, M, field = cfg
    crc = O.crc(table) if crc is None else crc
    return ST.frame(ST.CHUNK_TABLE, bytes([T, M, B]) + field + bytes([R]) + crc.to_bytes(4, "little") + table)


def build(stream, data, cfgs, with_tables=False, cache=None):
    """The sidecar of `stream` (whose decoded bytes are `data`) for the configurations `cfgs` -> its bytes (with_tables: and, per
    configuration, [(table, R) | None per data chunk]).  cache: a dict that keeps (configuration, chunk) -> table between calls over
    one stream."""
    data = bytes(data)
    ident = identifier(stream)
    assert ident is not None and 1 <= len(cfgs) <= MAX_CONFIGS
    mb = max_block_of(ident)
    B = ST.table_bits(mb)
    out = [ident] + [info_chunk(c, B) for c in cfgs]
    dcs = main_chunks(stream)
    tables = [[None] * len(dcs) for _ in cfgs]
    live = [i for i, (_, n) in enumerate(dcs) if n]          # a chunk of no bytes: no table, no reference, nobody's next chunk
    starts = np.concatenate([[0], np.cumsum([n for _, n in dcs])]).astype(np.int64)
    for j, i in enumerate(live):
        p, n = dcs[i]
        blk = data[starts[i]:starts[i] + n]
        nxt = None
        if j + 1 < len(live):
            i2 = live[j + 1]
            nxt = data[starts[i2]:starts[i2] + dcs[i2][1]]
        for ci, c in enumerate(cfgs):
            if cache is not None and (c, i) in cache:
                tab, R = cache[c, i]
            else:
                tab, R = table_of(c, blk, nxt, B)
                if cache is not None:
                    cache[c, i] = (tab, R)
            if tab is not None:
                tables[ci][i] = (tab, R)
                out.append(table_chunk(c, B, tab, R))
        out.append(ref_chunk(p, mb - n))
    out.append(EOF_CHUNK)
    side = b"".join(out)
    return (side, tables) if with_tables else side


def walk(side):
    """The chunks of a sidecar as a Reader sees them -> [(offset, type, payload length)]; SidecarError for a framing error, a missing EOF
    chunk, a data chunk inside or a second identifier."""
    p, out, want_eof, idents = 0, [], False, 0
    data_inside = False
    err = None
    while p < len(side) and err is None:
        if len(side) - p < 4:
            err = "a stub"
            break
        t = side[p]
        n = side[p + 1] | side[p + 2] << 8 | side[p + 3] << 16
        if p + 4 + n > len(side):
            err = "a chunk runs past the end"
            break
        if t in (1, 2, 3):
            data_inside = True
        elif t == 0xFF:
            idents += 1
            want_eof = True
        elif t == 0x20:
            want_eof = False
        out.append((p, t, n))
        p += 4 + n
    if data_inside:
        raise SidecarError("corrupt", "a data chunk inside the sidecar")
    if err or want_eof:
        raise SidecarError("corrupt", err or "no EOF chunk")
    if idents > 1:
        raise SidecarError("unsupported", "a second identifier")
    return out


def parse(side, main_stream, ignore_crc=False):
    """What an attach finds -> (cfgs, B, tables) with tables[c][k] = (table, R) or None per data chunk k of the main stream; raises
    SidecarError.  cfgs: the first up to 4 valid info chunks in front of the first 0x45 or 0x47."""
    cks = walk(side)
    dcs = main_chunks(main_stream)
    where = {p: k for k, (p, _) in enumerate(dcs)}
    ident = next((side[p:p + 10] for p, t, n in cks if t == 0xFF), None)
    if ident is None:
        return [], None, []
    mb = max_block_of(ident)
    cfgs, Bs = [], []
    for p, t, n in cks:
        if t in (ST.CHUNK_TABLE, CHUNK_REF):
            break
        if t == ST.CHUNK_INFO and len(cfgs) < MAX_CONFIGS:
            got = SL.info_of(bytes(side[p + 4:p + 4 + n]))
            if got is not None:
                cfgs.append((got[0], got[1], got[3]))
                Bs.append(got[2])
    tables = [[None] * len(dcs) for _ in cfgs]
    pending, floor = [], None
    for p, t, n in cks:
        body = bytes(side[p + 4:p + 4 + n])
        if t == ST.CHUNK_TABLE:
            pending.append(body)
        elif t == CHUNK_REF:
            refs = parse_refs(body, mb)
            if refs is None:
                raise SidecarError("corrupt", "a bad 0x47 payload")
            for off, size in refs:
                if floor is not None and off <= floor:
                    raise SidecarError("corrupt", "references do not ascend")
                if off not in where or dcs[where[off]][1] != size:
                    raise SidecarError("corrupt", "a reference names no data chunk of this size")
                floor = off
            k = where[refs[0][0]]
            for ci, (T, M, field) in enumerate(cfgs):
                B, f = Bs[ci], len(field)
                for tb in pending:
                    if len(tb) >= 8 + f + 32 and tb[:3 + f] == bytes([T, M, B]) + field:
                        R = tb[3 + f]
                        if R <= B - 8 and len(tb) - 8 - f == 1 << (B - R - 3):
                            tab = tb[8 + f:]
                            if ignore_crc or O.crc(tab) == int.from_bytes(tb[4 + f:8 + f], "little"):
                                tables[ci][k] = (tab, R)
                                break
            pending = []
    return cfgs, Bs, tables


def probes(tables, pattern, cfg, B):
    """One configuration against the pattern -> (a, s, nw, t_min) with a[k], s[k] the probe of chunk k, or None: it cannot serve the pattern."""
    T, M, field = cfg
    P = np.frombuffer(bytes(pattern), np.uint8)
    if T == 4:
        G, t_min = SL.groups(pattern, M, field)
        if not G:
            return None
        K, E, _ = SL.parts_of(field)
        h = ST.hash_windows(P, B, M)
        gh = [[int(h[i + K + j]) for j in range(E + 1)] for i in G]
        pr = [SL.probe(t[0], t[1], B, gh) if t is not None else (len(gh), len(gh)) for t in tables]
        return [p[0] for p in pr], [p[1] for p in pr], len(gh), t_min
    W, t_min = SP.windows(pattern, T, M, field)
    if not W:
        return None
    h = ST.hash_windows(P, B, M)
    hs = [int(h[i]) for i in W]
    pr = [ST.probe(t[0], t[1], B, hs) if t is not None else (len(hs), len(hs)) for t in tables]
    return [p[0] for p in pr], [p[1] for p in pr], len(hs), t_min


def admits(a, s, sizes, nw, L, t_min, ov=0):
    """One table set's verdict per chunk: all windows (groups) in its own table, or a split with the next chunk's.  ov: the set's overlap.
    A block's table is built over the next chunk's bytes alone, so in front of a chunk shorter than the overlap the windows that reach
    beyond that chunk were hashed over zeros: the table proves nothing there, and the set abstains (it admits the chunk)."""
    n, out = len(sizes), []
    for k in range(n):
        cand = a[k] == nw or (k + 1 < n and sizes[k + 1] < ov)
        if not cand and k + 1 < n:
            s_next = nw if sizes[k + 1] < L else s[k + 1]
            cand = max(t_min, nw - s_next) <= a[k]
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


def serving(tables_per_cfg, pattern, cfgs, Bs):
    """The probes of the configurations that vote: those that serve the pattern (all without a single usable table among them: none)."""
    got = [(ci, probes(tables_per_cfg[ci], pattern, c, Bs[ci])) for ci, c in enumerate(cfgs)]
    got = [(ci, p) for ci, p in got if p is not None]
    if not any(t is not None for ci, _ in got for t in tables_per_cfg[ci]):
        return []
    return got


def plan(tables_per_cfg, sizes, pattern, cfgs, Bs):
    """The chunks a search for `pattern` through the sidecar decodes: the AND rule over the configurations that vote."""
    L = len(pattern)
    votes = [admits(p[0], p[1], sizes, p[2], L, p[3], overlap(cfgs[ci])) for ci, p in serving(tables_per_cfg, pattern, cfgs, Bs)]
    return decoded_set(votes, sizes, L)


def usable(tables_per_cfg, patterns, cfgs, Bs):
    """The third statistic: chunks with a usable table of at least one configuration that serves a pattern (0 when none does)."""
    who = set()
    for pat in patterns:
        who.update(ci for ci, _ in serving(tables_per_cfg, pat, cfgs, Bs))
    n = len(tables_per_cfg[0]) if tables_per_cfg else 0
    return sum(any(tables_per_cfg[ci][k] is not None for ci in who) for k in range(n))
