"""The stored record index ("record index blob", include/minlz_hip_record_index_store.h) in numpy: the executable form of the layout.

    ff 06 00 00 "MinLz" 0d                                            stream identifier, block-size value 13
    90 <len24> crc32 <fixed header, 62 B> <directory: nsections x u32>  header chunk
    91 <len24> crc32 <section>                                        one per section (1024 tiles of 65 536 decoded positions)
    20 01 00 00 00                                                    EOF, size 0

pack(D, size, delimiter, bound=None, longest=None) -> bytes; unpack(blob) -> (D, header), or a StoreError whose code is the ABI's; with
`expect` unpack restates the order in which mlz_dev_reader_load_record_index refuses a blob for a handle."""
import struct

import numpy as np

import oracle as O

TILE, SECTION_TILES, SPARSE_MAX, BITMAP = 65536, 1024, 4096, 8192
IDENT = b"\xff\x06\x00\x00MinLz\x0d"
MAGIC = b"MLZRIDX1"
EOF = b"\x20\x01\x00\x00\x00"
FIXED_AT, DIR_AT = 18, 80
BOUND, LONGEST = 1, 2
UNKNOWN = (1 << 64) - 1
ERR_CORRUPT, ERR_UNSUPPORTED, ERR_CRC, ERR_DST_TOO_SMALL, ERR_ARG = 1, 3, 5, 6, 8
FIXED = struct.Struct("<8sIB3xQQQQIIIH")
assert FIXED.size == 62


class StoreError(Exception):
    def __init__(self, code, what):
        Exception.__init__(self, "%s (error %d)" % (what, code))
        self.code = code


def ntiles(size):
    return (size + TILE - 1) // TILE


def nsections(size):
    return (ntiles(size) + SECTION_TILES - 1) // SECTION_TILES


def records(k, size, last_is_delim):
    return k + 1 if size > 0 and not last_is_delim else k


def payload_bytes(c):
    return BITMAP if c > SPARSE_MAX else (c + 1) // 2 * 4


def frame(type_, body):
    """A chunk whose body starts with the masked CRC32C of the rest."""
    n = len(body) + 4
    return bytes([type_, n & 0xFF, (n >> 8) & 0xFF, n >> 16]) + struct.pack("<I", O.crc(body)) + body


def binding(chunks):
    """chunks: (decoded length, stored CRC field, chunk type) of every data chunk with bytes, in the handle's order -> (tag, data chunks)."""
    chunks = [c for c in chunks if c[0]]
    return O.crc(b"".join(struct.pack("<IIB", n, crc, t) for n, crc, t in chunks)), len(chunks)


def binding_of(*streams):
    """The binding of a handle over these streams (one: mlz_stream_open_device; more: a set, in order)."""
    out = []
    for s in streams:
        p = 0
        while p + 4 <= len(s):
            t, n = s[p], s[p + 1] | s[p + 2] << 8 | s[p + 3] << 16
            if t == 0x01:
                out.append((n - 4, int.from_bytes(s[p + 4:p + 8], "little"), t))
            elif t in (0x02, 0x03):
                v, shift, q = 0, 0, p + 8
                while True:
                    v |= (s[q] & 0x7F) << shift
                    shift += 7
                    q += 1
                    if s[q - 1] < 0x80:
                        break
                out.append((v, int.from_bytes(s[p + 4:p + 8], "little"), t))
            p += 4 + n
    return binding(out)


def tile_payload(rel):
    """rel: a tile's delimiters minus the tile's start, ascending."""
    if len(rel) > SPARSE_MAX:
        bits = np.zeros(TILE, np.uint8)
        bits[rel] = 1
        return np.packbits(bits, bitorder="little").tobytes()
    return rel.astype("<u2").tobytes() + (b"\0\0" if len(rel) & 1 else b"")


def sections_of(D, size):
    D = np.asarray(D, np.uint64)
    nt = ntiles(size)
    first = np.searchsorted(D, np.arange(nt + 1, dtype=np.uint64) * np.uint64(TILE), side="left")
    out = []
    for s in range(nsections(size)):
        t0, t1 = s * SECTION_TILES, min(nt, (s + 1) * SECTION_TILES)
        cum = (first[t0:t1 + 1] - first[t0]).astype("<u4")
        body = struct.pack("<IIQ", s, t1 - t0, int(first[t0])) + cum.tobytes()
        body += b"".join(tile_payload((D[first[t]:first[t + 1]] - np.uint64(t * TILE)).astype(np.int64)) for t in range(t0, t1))
        out.append(body)
    return out


def head_chunk(flags, delimiter, size, k, N, longest, tag, chunks, lengths, ns=None):
    fixed = FIXED.pack(MAGIC, flags, delimiter, size, k, N, longest, tag, chunks, len(lengths) if ns is None else ns, 0)
    return frame(0x90, fixed + b"".join(struct.pack("<I", n) for n in lengths))


def assemble(head, sections):
    return IDENT + head + b"".join(frame(0x91, s) for s in sections) + EOF


def pack(D, size, delimiter, bound=None, longest=None):
    """D: the delimiters' positions, ascending; bound: (tag, data chunks) of the handle or None (an unbound blob); longest: the longest
    record's length when known."""
    D = np.asarray(D, np.uint64)
    k = len(D)
    assert k == 0 or (int(D[-1]) < size and (np.diff(D.astype(np.int64)) > 0).all())
    N = records(k, size, k > 0 and int(D[-1]) == size - 1)
    secs = sections_of(D, size)
    flags = (BOUND if bound is not None else 0) | (LONGEST if longest is not None else 0)
    tag, chunks = bound if bound is not None else (0, 0)
    return assemble(head_chunk(flags, delimiter, size, k, N, UNKNOWN if longest is None else longest, tag, chunks, [len(s) for s in secs]), secs)


def parse(blob, ignore_crc=False, expect_size=None):
    """The identifier, the header chunk and the directory against len(blob) -> (header dict, [(offset, length) of every section]).
    expect_size: the handle's size, compared where the load compares it (in front of the directory)."""
    if len(blob) < DIR_AT or blob[:10] != IDENT or blob[10] != 0x90:
        raise StoreError(ERR_CORRUPT, "no record index blob")
    magic, flags, delim, size, k, N, longest, tag, chunks, ns, zero = FIXED.unpack(blob[FIXED_AT:DIR_AT])
    if magic != MAGIC:
        raise StoreError(ERR_UNSUPPORTED, "unknown magic")
    len24 = blob[11] | blob[12] << 8 | blob[13] << 16
    if flags & ~3 or blob[FIXED_AT + 13:FIXED_AT + 16] != b"\0\0\0" or zero:
        raise StoreError(ERR_CORRUPT, "flags or padding")
    if size > 1 << 36 or k > size or not (N == k or (N == k + 1 and size > 0)):
        raise StoreError(ERR_CORRUPT, "size, k, N")
    if ns != nsections(size) or len24 != 66 + 4 * ns:
        raise StoreError(ERR_CORRUPT, "sections")
    if (longest > size) if flags & LONGEST else (longest != UNKNOWN):
        raise StoreError(ERR_CORRUPT, "longest")
    if not flags & BOUND and (tag or chunks):
        raise StoreError(ERR_CORRUPT, "an unbound blob with a binding")
    h = dict(flags=flags, delimiter=delim, size=size, k=k, N=N, longest=longest, tag=tag, data_chunks=chunks, nsections=ns)
    if expect_size is not None and size != expect_size:
        raise StoreError(ERR_ARG, "another size")
    head = DIR_AT + 4 * ns
    if len(blob) < head + 5:
        raise StoreError(ERR_CORRUPT, "truncated")
    nt, at, secs = ntiles(size), head, []
    for s in range(ns):
        tiles = min(SECTION_TILES, nt - s * SECTION_TILES)
        n, lo = struct.unpack_from("<I", blob, DIR_AT + 4 * s)[0], 16 + 4 * (tiles + 1)
        if n < lo or n > lo + BITMAP * tiles or n & 3:
            raise StoreError(ERR_CORRUPT, "directory")
        secs.append((at + 8, n))
        at += 8 + n
    if at + 5 != len(blob):
        raise StoreError(ERR_CORRUPT, "the directory does not add up to the blob")
    if not ignore_crc and struct.unpack_from("<I", blob, 14)[0] != O.crc(blob[FIXED_AT:head]):
        raise StoreError(ERR_CRC, "header chunk")
    return h, secs


def unpack(blob, ignore_crc=False, expect=None):
    """-> (D as uint64, header dict).  expect: (size, tag, data chunks) of the handle the blob is loaded into.  The order of the refusals is
    the load's: header, size, directory, header CRC, binding, section CRCs, structure."""
    blob = bytes(blob)
    h, secs = parse(blob, ignore_crc, None if expect is None else expect[0])
    if expect is not None and h["flags"] & BOUND and (h["tag"], h["data_chunks"]) != tuple(expect[1:]):
        raise StoreError(ERR_ARG, "another stream")
    if not ignore_crc:
        for off, n in secs:
            if struct.unpack_from("<I", blob, off - 4)[0] != O.crc(blob[off:off + n]):
                raise StoreError(ERR_CRC, "section")
    for off, n in secs:
        if blob[off - 8] != 0x91 or blob[off - 7] | blob[off - 6] << 8 | blob[off - 5] << 16 != n + 4:
            raise StoreError(ERR_CORRUPT, "section chunk header")
    if blob[-5:] != EOF:
        raise StoreError(ERR_CORRUPT, "EOF chunk")
    size, k, nt = h["size"], h["k"], ntiles(h["size"])
    out, rank = [], 0
    for s, (off, n) in enumerate(secs):
        tiles = min(SECTION_TILES, nt - s * SECTION_TILES)
        no, nti, first = struct.unpack_from("<IIQ", blob, off)
        cum = np.frombuffer(blob, "<u4", tiles + 1, off + 16).astype(np.int64)
        if no != s or nti != tiles:
            raise StoreError(ERR_CORRUPT, "section header")
        if cum[0] != 0 or (np.diff(cum) < 0).any() or (np.diff(cum) > TILE).any():
            raise StoreError(ERR_CORRUPT, "counts")
        if first != rank or first + int(cum[-1]) > k:
            raise StoreError(ERR_CORRUPT, "ranks")
        rank += int(cum[-1])
        p = off + 16 + 4 * (tiles + 1)
        if p + sum(payload_bytes(int(c)) for c in np.diff(cum)) != off + n:
            raise StoreError(ERR_CORRUPT, "payload offsets")
        for i, c in enumerate(np.diff(cum)):
            t, c = s * SECTION_TILES + i, int(c)
            limit = min(TILE, size - t * TILE)
            if c > SPARSE_MAX:
                bits = np.unpackbits(np.frombuffer(blob, np.uint8, BITMAP, p), bitorder="little")
                rel = np.flatnonzero(bits)
                if len(rel) != c or (len(rel) and rel[-1] >= limit):
                    raise StoreError(ERR_CORRUPT, "dense tile")
            else:
                rel = np.frombuffer(blob, "<u2", c, p).astype(np.int64)
                if (np.diff(rel) <= 0).any() or (c and rel[-1] >= limit) or (c & 1 and blob[p + 2 * c:p + 2 * c + 2] != b"\0\0"):
                    raise StoreError(ERR_CORRUPT, "sparse tile")
            out.append(rel.astype(np.uint64) + np.uint64(t * TILE))
            p += payload_bytes(c)
    if rank != k:
        raise StoreError(ERR_CORRUPT, "k")
    D = np.concatenate(out) if out else np.zeros(0, np.uint64)
    if h["N"] != records(k, size, k > 0 and int(D[-1]) == size - 1):
        raise StoreError(ERR_CORRUPT, "N")
    return D, h


def delimiters(data, delimiter):
    return np.flatnonzero(np.frombuffer(data, np.uint8) == delimiter).astype(np.uint64)


def refit(blob, edit):
    """The blob with edit(sections as bytearrays, header dict) applied and every length, directory entry and CRC made again: a corruption
    that is not about the CRC."""
    h, secs = parse(bytes(blob))
    bodies = [bytearray(blob[off:off + n]) for off, n in secs]
    lengths = edit(bodies, h)
    lengths = [len(b) for b in bodies] if lengths is None else lengths
    head = head_chunk(h["flags"], h["delimiter"], h["size"], h["k"], h["N"], h["longest"], h["tag"], h["data_chunks"], lengths, h["nsections"])
    return assemble(head, [bytes(b) for b in bodies])


def reheader(blob, pad=None, **changes):
    """The blob with fields of its fixed header replaced as they are (magic, flags, delimiter, size, k, N, longest, tag, data_chunks,
    nsections, zero; pad: the three bytes behind the delimiter) and the header chunk's CRC made again; nothing is validated."""
    names = ("magic", "flags", "delimiter", "size", "k", "N", "longest", "tag", "data_chunks", "nsections", "zero")
    f = dict(zip(names, FIXED.unpack(blob[FIXED_AT:DIR_AT])))
    head = DIR_AT + 4 * f["nsections"]
    assert set(changes) <= set(names)
    f.update(changes)
    fixed = FIXED.pack(*(f[n] for n in names))
    if pad is not None:
        fixed = fixed[:13] + bytes(pad) + fixed[16:]
    body = fixed + blob[DIR_AT:head]
    return blob[:14] + struct.pack("<I", O.crc(body)) + body + blob[head:]
