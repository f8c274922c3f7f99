"""Sidecar search indexes (the reference's SEARCH.md "Sidecar Streams", SPEC_SEARCH.md 1.1 and 2.3) in plain Python, written from the
specification alone, on top of the model of the table types (tests/search_model.py).

A sidecar is a valid stream without data chunks: the main stream's identifier, one info chunk (0x44) per table configuration, then for
every data chunk of the main stream its table chunks (0x45, one per configuration whose table is kept) and a remote block reference (0x47:
uvarint(offset of the data chunk's header in the main stream) uvarint(max block size - decoded bytes)), and the EOF chunk.  A searcher
skips a block when ANY configuration proves the pattern absent.

A configuration is (T, M, field): the table type, the match length and the prefix field as the chunks carry it."""
import numpy as np

import oracle as O
from tests import search_model as SMod

CHUNK_REF = 0x47
EOF_CHUNK = b"\x20\x01\x00\x00\x00"
MAX_CONFIGS = 4


class SidecarError(Exception):
    """kind: "corrupt" (-MLZ_ERR_CORRUPT) or "unsupported" (-MLZ_ERR_UNSUPPORTED)"""

    def __init__(self, kind, why):
        super().__init__("%s: %s" % (kind, why))
        self.kind = kind


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
    return SMod.frame(CHUNK_REF, uvarint(hdr_off) + uvarint(max_minus_actual))


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
    for p, t, n in SMod.chunks_of(stream):
        if t == 0x01:
            out.append((p, n - 4))
        elif t in (0x02, 0x03):
            out.append((p, SMod.S.uvarint(stream, p + 8)[0]))
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
        out.append(SMod.frame(0x01 if stored else 0x02, O.crc(blk).to_bytes(4, "little") + (blk if stored else enc[1:])))
        o += sz
    n = uvarint(len(data))
    out.append(b"\x20" + bytes([len(n), 0, 0]) + n)
    return b"".join(out)


def identifier(stream):
    for p, t, n in SMod.chunks_of(stream):
        if t == 0xFF:
            return bytes(stream[p:p + 10])
    return None


def max_block_of(ident):
    return 1 << ((ident[9] & 15) + 10)


def build(stream, data, cfgs, with_tables=False, cache=None):
    """The sidecar of `stream` (whose decoded bytes are `data`) for the configurations `cfgs` -> its bytes (with_tables: and, per
    configuration, [(table, R) | None per data chunk]).  cache: a dict that keeps (configuration, chunk) -> table between calls over
    one stream."""
    data = bytes(data)
    ident = identifier(stream)
    assert ident is not None and 1 <= len(cfgs) <= MAX_CONFIGS
    mb = max_block_of(ident)
    B = SMod.table_bits(mb)
    out = [ident] + [SMod.info_chunk(c, B) for c in cfgs]
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
                tab, R = SMod.build_table(c, blk, nxt, B)
                if cache is not None:
                    cache[c, i] = (tab, R)
            if tab is not None:
                tables[ci][i] = (tab, R)
                out.append(SMod.table_chunk(c, B, tab, R))
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
        if t in (SMod.CHUNK_TABLE, CHUNK_REF):
            break
        if t == SMod.CHUNK_INFO and len(cfgs) < MAX_CONFIGS:
            got = SMod.info_of(bytes(side[p + 4:p + 4 + n]))
            if got is not None:
                cfgs.append((got[0], got[1], got[3]))
                Bs.append(got[2])
    tables = [[None] * len(dcs) for _ in cfgs]
    pending, floor = [], None
    for p, t, n in cks:
        body = bytes(side[p + 4:p + 4 + n])
        if t == SMod.CHUNK_TABLE:
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
            for ci, c in enumerate(cfgs):
                fits = (SMod.table_fits(tb, c, Bs[ci]) for tb in pending)
                tables[ci][k] = next((f[:2] for f in fits if f is not None and (ignore_crc or O.crc(f[0]) == f[2])), None)
            pending = []
    return cfgs, Bs, tables


def serving(tables_per_cfg, pattern, cfgs, Bs):
    """The probes of the configurations that vote: those that serve the pattern (all without a single usable table among them: none)."""
    got = [(ci, SMod.probed(tables_per_cfg[ci], pattern, c, Bs[ci])) for ci, c in enumerate(cfgs)]
    got = [(ci, p) for ci, p in got if p is not None]
    if not any(t is not None for ci, _ in got for t in tables_per_cfg[ci]):
        return []
    return got


def plan(tables_per_cfg, sizes, pattern, cfgs, Bs):
    """The chunks a search for `pattern` through the sidecar decodes: the AND rule over the configurations that vote."""
    L = len(pattern)
    votes = [SMod.admits(p[0], p[1], sizes, p[2], L, p[3], SMod.overlap(cfgs[ci])) for ci, p in serving(tables_per_cfg, pattern, cfgs, Bs)]
    return SMod.decoded_set(votes, sizes, L)


def usable(tables_per_cfg, patterns, cfgs, Bs):
    """The third statistic: chunks with a usable table of at least one configuration that serves a pattern (0 when none does)."""
    who = set()
    for pat in patterns:
        who.update(ci for ci, _ in serving(tables_per_cfg, pat, cfgs, Bs))
    n = len(tables_per_cfg[0]) if tables_per_cfg else 0
    return sum(any(tables_per_cfg[ci][k] is not None for ci in who) for k in range(n))
