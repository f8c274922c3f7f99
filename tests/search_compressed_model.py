"""Compressed block search tables (chunk 0x46, the reference's SPEC_SEARCH.md 2.2 and 2.2.1) in plain Python and numpy: the reader the
library is held against, and the writer the tests need.  A 0x46 chunk carries the fixed fields of a 0x45 chunk (`T M B field R crc`), then
`h0_bs h0_tc`, h0_tc huff0 table descriptions and one record per sub-block of 2^h0_bs bitmap bytes: a table index 0 .. 15 with a uvarint
length and four interleaved Huffman streams, 16 = the bytes themselves, 17 = one byte repeated, 18 = a sparse bit table (uvarint length,
gaps between set bits).  The table descriptions and the streams are RFC 8878 4.2's (direct 4-bit weights or FSE-compressed weights, a
jump table of three 16-bit sizes, four streams read backwards from an end marker); tests/test_search_compressed_model.py pins both
directions of that claim with libzstd.

A configuration here is cfg = (T, M, B, field), as search_model.info_of returns it."""
import heapq

import numpy as np

import oracle as O
from tests import search_model as SM

CHUNK_COMPRESSED = 0x46
RAW, RLE, SPARSE = 16, 17, 18
MAX_TABLES, MAX_SUB = 16, 16
MIN_BS, MAX_BS = 5, 17
MAX_TABLELOG = 11
MAX_WEIGHT = 12          # the largest symbol an FSE weight table may name (RFC 8878: weights 0 .. 12); a table log of 12 is refused later
FSE_MIN_LOG, FSE_MAX_LOG = 5, 6


class Invalid(ValueError):
    """A chunk the reader refuses."""


# ---- varints ----

def put_uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_uvarint(buf, p):
    """-> (value, bytes taken); raises when the bytes end inside it or it runs beyond 64 bits."""
    v = s = 0
    for i in range(10):
        if p + i >= len(buf):
            raise Invalid("a cut uvarint")
        b = buf[p + i]
        if i == 9 and b > 1:
            raise Invalid("uvarint overflow")
        v |= (b & 0x7F) << s
        if b < 0x80:
            return v, i + 1
        s += 7
    raise Invalid("uvarint overflow")


# ---- FSE (RFC 8878 4.1), as far as Huffman weights need it ----

def fse_read_ncount(buf, max_symbol=MAX_WEIGHT, max_log=FSE_MAX_LOG):
    """The table description at the front of buf -> (normalised counts, accuracy log, bytes taken).  A count of -1 is "less than one"."""
    bits = int.from_bytes(bytes(buf), "little")
    avail = 8 * len(buf)
    if avail < 8:
        raise Invalid("FSE table description cut")
    log = (bits & 15) + FSE_MIN_LOG
    if log > max_log:
        raise Invalid("FSE accuracy log %d" % log)
    pos = 4
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    norm, prev0 = [], False
    while remaining > 1 and len(norm) <= max_symbol:
        if prev0:
            n0 = len(norm)
            while (bits >> pos) & 3 == 3:
                n0 += 3
                pos += 2
                if pos > avail:
                    raise Invalid("FSE table description cut")
            n0 += (bits >> pos) & 3
            pos += 2
            if n0 > max_symbol:
                raise Invalid("FSE symbol beyond %d" % max_symbol)
            norm += [0] * (n0 - len(norm))
        mx = 2 * threshold - 1 - remaining
        low = (bits >> pos) & (threshold - 1)
        if low < mx:
            count, pos = low, pos + nb - 1
        else:
            count = (bits >> pos) & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            pos += nb
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
        if pos > avail:
            raise Invalid("FSE table description cut")
    if remaining != 1 or pos > avail:
        raise Invalid("FSE counts do not fill the table")
    return norm, log, (pos + 7) >> 3


def fse_decode_table(norm, log):
    """-> (symbol, bits, base) per state."""
    size = 1 << log
    sym = [0] * size
    nxt = [0] * len(norm)
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = c
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    if pos != 0:
        raise Invalid("FSE spread")
    nbits, base = [0] * size, [0] * size
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nbits[u] = log - (x.bit_length() - 1)
        base[u] = (x << nbits[u]) - size
    return sym, nbits, base


def fse_decode_weights(buf, limit=255):
    """An FSE-compressed weight section (description + two interleaved states read backwards) -> the weights."""
    norm, log, used = fse_read_ncount(buf)
    sym, nbits, base = fse_decode_table(norm, log)
    s = bytes(buf[used:])
    if not s or s[-1] == 0:
        raise Invalid("FSE weight stream without end marker")
    pos = 8 * (len(s) - 1) + s[-1].bit_length() - 1          # bits left below the end marker
    v = int.from_bytes(s, "little") & ((1 << pos) - 1)

    def read(n):
        nonlocal pos
        pos -= n
        if pos >= 0:
            return (v >> pos) & ((1 << n) - 1)
        return ((v << -pos) & ((1 << n) - 1)) if n + pos > 0 else 0    # the bits that exist, zeros below them

    st = [read(log), read(log)]
    if pos < 0:
        raise Invalid("an FSE weight section that ends early")
    out, i = [], 0
    while True:
        if len(out) > limit - 2:
            raise Invalid("too many weights")
        out.append(sym[st[i]])
        st[i] = base[st[i]] + read(nbits[st[i]])
        if pos < 0:                                           # read beyond the stream's first bit: the other state's symbol is the last
            out.append(sym[st[i ^ 1]])
            return out
        i ^= 1


def fse_encode_weights(weights):
    """-> the section's bytes (description + stream), or None where FSE cannot carry them (fewer than two weights)."""
    n = len(weights)
    if n < 2:
        return None
    hist = [0] * (max(weights) + 1)
    for w in weights:
        hist[w] += 1
    log = FSE_MAX_LOG
    size = 1 << log
    present = [s for s, c in enumerate(hist) if c]
    if len(present) == 1:                                     # one value only: a second symbol of probability 1 that never occurs
        spare = 0 if present[0] else 1
        norm = [0] * max(len(hist), spare + 1)
        norm[present[0]], norm[spare] = size - 1, 1
    else:
        norm = [max(1, (c * size + n // 2) // n) if c else 0 for c in hist]
        while sum(norm) != size:
            big = max(range(len(norm)), key=lambda s: norm[s])
            norm[big] += 1 if sum(norm) < size else -1
    # the description
    bits, pos = log - FSE_MIN_LOG, 4
    remaining, threshold, nb = size + 1, size, log + 1
    s = 0
    while remaining > 1:
        count = norm[s] + 1
        mx = 2 * threshold - 1 - remaining
        if count >= threshold:
            count += mx
        if count < mx:
            bits |= count << pos
            pos += nb - 1
        else:
            bits |= count << pos
            pos += nb
        remaining -= norm[s]
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
        s += 1
        if norm[s - 1] == 0 and remaining > 1:
            n0 = s
            while s < len(norm) and norm[s] == 0:
                s += 1
            run = s - n0
            while run >= 3:
                bits |= 3 << pos
                pos += 2
                run -= 3
            bits |= run << pos
            pos += 2
    desc = bits.to_bytes((pos + 7) >> 3, "little")
    # the stream: the decoder's reads in order are init(state 0), init(state 1), then the update behind weight 0, 1, ..., n - 3
    sym, nbits, base = fse_decode_table(norm, log)
    states_of = {}
    for u in range(size):
        states_of.setdefault(sym[u], []).append(u)
    st, reads = [None, None], []                              # reads: (value, bits) from the last one the decoder makes to the first
    for i in range(n - 1, -1, -1):
        c = i & 1
        if st[c] is None:
            st[c] = max(states_of[weights[i]], key=lambda u: nbits[u])      # a final state: its update must run beyond the stream
            assert nbits[st[c]] >= 1
            continue
        t = next(u for u in states_of[weights[i]] if base[u] <= st[c] < base[u] + (1 << nbits[u]))
        reads.append((st[c] - base[t], nbits[t]))
        st[c] = t
    reads.append((st[1], log))
    reads.append((st[0], log))
    acc = tot = 0
    for val, k in reads:                                      # the decoder's last read lies lowest
        acc |= val << tot
        tot += k
    acc |= 1 << tot
    return desc + acc.to_bytes((tot + 8) >> 3, "little")


# ---- the huff0 table description and the 4X streams (RFC 8878 4.2) ----

def read_huff_table(buf, p):
    """A table description at buf[p:] -> (sym, nbits, table log, bytes taken): the decode table of 2^log entries."""
    if p >= len(buf):
        raise Invalid("table description beyond the chunk")
    h = buf[p]
    if h >= 128:
        n = h - 127
        nbytes = (n + 1) // 2
        if p + 1 + nbytes > len(buf):
            raise Invalid("direct weights beyond the chunk")
        w = []
        for i in range(n):
            b = buf[p + 1 + i // 2]
            w.append(b >> 4 if i % 2 == 0 else b & 15)
        used = 1 + nbytes
    else:
        if h == 0 or p + 1 + h > len(buf):
            raise Invalid("FSE weights beyond the chunk")
        w = fse_decode_weights(bytes(buf[p + 1:p + 1 + h]))
        used = 1 + h
    if any(x > MAX_WEIGHT for x in w):
        raise Invalid("weight above %d" % MAX_WEIGHT)
    total = sum((1 << x) >> 1 for x in w)
    if total == 0:
        raise Invalid("no weight")
    log = total.bit_length()                                  # the next power of two above the sum
    if log > MAX_TABLELOG:
        raise Invalid("table log %d" % log)
    rest = (1 << log) - total
    if rest & (rest - 1):
        raise Invalid("weights miss a power of two")
    w = w + [rest.bit_length()]
    if len(w) > 256:
        raise Invalid("more than 256 symbols")
    if sum(1 for x in w if x) < 2:
        raise Invalid("fewer than two symbols")
    sym = np.zeros(1 << log, np.uint8)
    nb = np.zeros(1 << log, np.uint8)
    at = 0
    for wt in range(1, log + 1):
        for s, x in enumerate(w):
            if x == wt:
                span = 1 << (wt - 1)
                sym[at:at + span] = s
                nb[at:at + span] = log + 1 - wt
                at += span
    assert at == 1 << log
    return sym, nb, log, used


def decode_stream(s, count, sym, nb, log):
    """One backward bit stream -> `count` symbols; it must end exactly at its first bit."""
    s = bytes(s)
    if not s or s[-1] == 0:
        raise Invalid("a stream whose last byte is 0")
    sym, nb = sym.tolist(), nb.tolist()
    p = len(s) - 1
    nbit = s[-1].bit_length() - 1
    acc = s[-1] & ((1 << nbit) - 1)
    mask = (1 << log) - 1
    out = bytearray(count)
    for i in range(count):
        while nbit < log and p > 0:
            p -= 1
            acc = (acc << 8) | s[p]
            nbit += 8
        idx = (acc >> (nbit - log)) & mask if nbit >= log else (acc << (log - nbit)) & mask
        out[i] = sym[idx]
        nbit -= nb[idx]
        if nbit < 0:
            raise Invalid("a stream that runs beyond its start")
        acc &= (1 << nbit) - 1
    if p != 0 or nbit != 0:
        raise Invalid("a stream that does not end at its first bit")
    return bytes(out)


def decode_4x(src, n, table):
    """Jump table + four streams -> n bytes."""
    sym, nb, log = table
    if len(src) < 6:
        raise Invalid("no room for a jump table")
    l1, l2, l3 = (src[0] | src[1] << 8), (src[2] | src[3] << 8), (src[4] | src[5] << 8)
    if 6 + l1 + l2 + l3 > len(src):
        raise Invalid("jump-table sizes beyond the sub-block's bytes")
    seg = (n + 3) // 4
    if 3 * seg > n:
        raise Invalid("a sub-block too small for four streams")
    cuts = [6, 6 + l1, 6 + l1 + l2, 6 + l1 + l2 + l3, len(src)]
    counts = [seg, seg, seg, n - 3 * seg]
    return b"".join(decode_stream(src[cuts[i]:cuts[i + 1]], counts[i], sym, nb, log) for i in range(4))


def decode_sparse(src, n):
    """A sparse bit table -> n bytes (SPEC_SEARCH.md 2.2.1)."""
    out = bytearray(n)
    pos = gap = 0
    for b in src:
        gap += b
        if b == 255:
            continue
        pos += gap
        if pos >= 8 * n:
            raise Invalid("a sparse position at or beyond the bit count")
        out[pos >> 3] |= 1 << (pos & 7)
        pos += 1
        gap = 0
    if gap:
        raise Invalid("a sparse table that ends in 255")
    return bytes(out)


def encode_sparse(block):
    bits = np.flatnonzero(np.unpackbits(np.frombuffer(bytes(block), np.uint8), bitorder="little"))
    if not len(bits):
        return b""
    gaps = np.diff(bits, prepend=-1) - 1                     # zeros between a set bit and the one before it
    counts = gaps // 255 + 1                                  # a byte of 255 per full 255, then the rest
    out = np.full(int(counts.sum()), 255, np.uint8)
    out[np.cumsum(counts) - 1] = gaps % 255
    return out.tobytes()


# ---- the reader ----

def fixed_fields(payload, cfg):
    """-> (R, crc, offset of h0_bs) of a payload whose `T M B field` are the configuration's, else raises."""
    T, M, B, field = cfg
    head = bytes([T, M, B]) + bytes(field)
    f = len(head)
    if len(payload) < f + 7 or bytes(payload[:f]) != head:
        raise Invalid("fixed fields")
    return payload[f], int.from_bytes(payload[f + 1:f + 5], "little"), f + 5


def parse_compressed_table(payload, cfg, ignore_crc=False):
    """A 0x46 payload against a configuration -> (R, bitmap), or raises Invalid."""
    payload = bytes(payload)
    T, M, B, field = cfg
    R, crc, p = fixed_fields(payload, cfg)
    bs, tc = payload[p], payload[p + 1]
    p += 2
    if not MIN_BS <= bs <= MAX_BS:
        raise Invalid("h0_bs %d" % bs)
    if tc > MAX_TABLES:
        raise Invalid("h0_tc %d" % tc)
    if B <= R + 3:
        raise Invalid("reductions %d" % R)
    n, sub = 1 << (B - R - 3), 1 << bs
    if n % sub or not 1 <= n // sub <= MAX_SUB:
        raise Invalid("%d bytes in sub-blocks of %d" % (n, sub))
    tables = []
    for _ in range(tc):
        sym, nb, log, used = read_huff_table(payload, p)
        tables.append((sym, nb, log))
        p += used
    out = []
    for _ in range(n // sub):
        if p >= len(payload):
            raise Invalid("chunk ends in front of a sub-block")
        kind = payload[p]
        p += 1
        if kind < 16 or kind == SPARSE:
            if kind < 16 and kind >= tc:
                raise Invalid("table index %d of %d" % (kind, tc))
            ln, used = get_uvarint(payload, p)
            p += used
            if ln > len(payload) - p:
                raise Invalid("a length beyond the chunk")
            src = payload[p:p + ln]
            p += ln
            out.append(decode_sparse(src, sub) if kind == SPARSE else decode_4x(src, sub, tables[kind]))
        elif kind == RAW:
            if sub > len(payload) - p:
                raise Invalid("raw bytes beyond the chunk")
            out.append(payload[p:p + sub])
            p += sub
        elif kind == RLE:
            if p >= len(payload):
                raise Invalid("RLE byte beyond the chunk")
            out.append(payload[p:p + 1] * sub)
            p += 1
        else:
            raise Invalid("kind %d" % kind)
    if p != len(payload):
        raise Invalid("trailing bytes")
    bitmap = b"".join(out)
    if not ignore_crc and O.crc(bitmap) != crc:
        raise Invalid("CRC")
    return R, bitmap


# ---- the writer ----

def code_lengths(hist, limit=MAX_TABLELOG):
    """Huffman code lengths of the symbols with hist > 0 (at least two), none above `limit`: the counts are flattened until the tree fits."""
    hist = np.asarray(hist, np.int64)
    present = np.flatnonzero(hist).tolist()
    assert len(present) >= 2
    shift = 0
    while True:
        heap = [(max(1, int(hist[s]) >> shift), s, (s,)) for s in present]
        heapq.heapify(heap)
        depth = dict.fromkeys(present, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            return depth
        shift += 1


def huff_table(hist, form="auto"):
    """-> (description bytes, code[256], length[256], log).  form: "direct", "fse" or "auto" (direct where it can carry the symbols and
    is not longer)."""
    depth = code_lengths(hist)
    log = max(depth.values())
    w = [0] * 256
    for s, d in depth.items():
        w[s] = log + 1 - d
    last = max(depth)
    listed = w[:last]
    direct = None
    if len(listed) <= 128 and listed:
        body = bytearray((len(listed) + 1) // 2)
        for i, x in enumerate(listed):
            body[i // 2] |= x << 4 if i % 2 == 0 else x
        direct = bytes([127 + len(listed)]) + bytes(body)
    fse = fse_encode_weights(listed)
    if fse is not None:
        fse = bytes([len(fse)]) + fse if len(fse) < 128 else None
    if form == "direct":
        desc = direct
    elif form == "fse":
        desc = fse
    else:
        desc = min((d for d in (direct, fse) if d is not None), key=len, default=None)
    assert desc is not None, "no form of the table description carries these weights"
    code = np.zeros(256, np.uint32)
    length = np.zeros(256, np.uint32)
    at = 0
    for wt in range(1, log + 1):
        for s in range(256):
            if w[s] == wt:
                code[s] = at >> (wt - 1)
                length[s] = log + 1 - wt
                at += 1 << (wt - 1)
    return desc, code, length, log


def encode_stream(data, code, length):
    """The symbols' codes, the first one just below the end marker, as a little-endian byte string."""
    d = np.frombuffer(bytes(data), np.uint8)
    ln = length[d].astype(np.int64)
    total = int(ln.sum()) + 1
    pad = -total % 8
    bits = np.zeros(pad + total, np.uint8)
    bits[pad] = 1
    start = pad + 1 + np.concatenate([[0], np.cumsum(ln)[:-1]])
    within = np.arange(total - 1) - np.repeat(start - pad - 1, ln)
    bits[pad + 1:] = (np.repeat(code[d].astype(np.int64), ln) >> (np.repeat(ln, ln) - 1 - within)) & 1
    return np.packbits(bits)[::-1].tobytes()


def encode_4x(block, code, length):
    n = len(block)
    seg = (n + 3) // 4
    parts = [encode_stream(block[i * seg:(i + 1) * seg if i < 3 else n], code, length) for i in range(4)]
    assert all(len(p) < 65536 for p in parts)
    return b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)


def default_bs(n):
    """The reference's partition: bitmaps up to 32 KiB are one sub-block; up to 512 KiB, 32 KiB sub-blocks; else 64 KiB sub-blocks."""
    if n <= 32 << 10:
        return (n - 1).bit_length()
    return 15 if n <= 512 << 10 else 16


def build_compressed_table(cfg, R, bitmap, h0_bs=None, kinds=None, forms=None, crc=None):
    """-> the 0x46 payload of `bitmap` (2^(B - R - 3) bytes).  kinds: per sub-block "raw", "rle", "sparse", "huff" (a table of its own) or
    ("huff", g) (the table of group g, built over all of the group's sub-blocks); None picks the smallest of them per sub-block, tables
    never shared.  forms: {group or sub-block number: "direct" | "fse"}."""
    T, M, B, field = cfg
    bitmap = bytes(bitmap)
    n = len(bitmap)
    assert n == 1 << (B - R - 3)
    bs = default_bs(n) if h0_bs is None else h0_bs
    sub = 1 << bs
    assert n % sub == 0
    blocks = [bitmap[i:i + sub] for i in range(0, n, sub)]
    forms = forms or {}
    hists = [np.bincount(np.frombuffer(b, np.uint8), minlength=256) for b in blocks]
    if kinds is None:
        kinds = []
        for i, b in enumerate(blocks):
            if np.count_nonzero(hists[i]) == 1:
                kinds.append("rle")
                continue
            sizes = {"raw": sub, "sparse": len(encode_sparse(b)) + 3}
            if sub >= 4:
                desc, code, length, _ = huff_table(hists[i], forms.get(i, "auto"))
                sizes["huff"] = len(desc) + 9 + (int((length[np.frombuffer(b, np.uint8)]).sum()) + 7) // 8 + 3
            kinds.append(min(sizes, key=sizes.get))
    assert len(kinds) == len(blocks)
    groups = {}                                              # table key -> the sub-blocks that use it
    for i, k in enumerate(kinds):
        if k == "huff":
            groups[("own", i)] = [i]
        elif isinstance(k, tuple):
            groups.setdefault(("group", k[1]), []).append(i)
    assert len(groups) <= MAX_TABLES
    tables, index = [], {}
    for key, users in groups.items():
        index[key] = len(tables)
        tables.append(huff_table(sum(hists[i] for i in users), forms.get(key[1], "auto")))
    out = [bytes([T, M, B]) + bytes(field) + bytes([R]) + (O.crc(bitmap) if crc is None else crc).to_bytes(4, "little"), bytes([bs, len(tables)])]
    out += [t[0] for t in tables]
    for i, (k, b) in enumerate(zip(kinds, blocks)):
        if k == "raw":
            out.append(bytes([RAW]) + b)
        elif k == "rle":
            assert b == b[:1] * sub
            out.append(bytes([RLE]) + b[:1])
        elif k == "sparse":
            s = encode_sparse(b)
            out.append(bytes([SPARSE]) + put_uvarint(len(s)) + s)
        else:
            ti = index[("own", i) if k == "huff" else ("group", k[1])]
            s = encode_4x(b, tables[ti][1], tables[ti][2])
            out.append(bytes([ti]) + put_uvarint(len(s)) + s)
    return b"".join(out)


def table_config(body):
    """The configuration a 0x45 / 0x46 payload states -> ((T, M, B, field), offset of R), or None."""
    got = SM.info_of(body)
    if got is None:
        return None
    T, M, B, field = got
    return (T, M, B, field), 3 + len(field)


def recompress_stream(stream, choose=None, **kw):
    """The stream (or sidecar) with its 0x45 chunks rewritten as 0x46, every other byte as it is.  choose(i) -> what stands in place of
    the i-th 0x45 chunk, a sequence of "45" and "46" (default: ("46",)); kw goes to build_compressed_table (a callable value is called
    with i)."""
    stream = bytes(stream)
    out, i = [], 0
    for p, t, n in SM.chunks_of(stream):
        raw = stream[p:p + 4 + n]
        if t != SM.CHUNK_TABLE:
            out.append(raw)
            continue
        body = raw[4:]
        cfg, at = table_config(body)
        R = body[at]
        args = {k: (v(i) if callable(v) else v) for k, v in kw.items()}
        for what in (choose(i) if choose else ("46",)):
            out.append(raw if what == "45" else SM.frame(CHUNK_COMPRESSED, build_compressed_table(cfg, R, body[at + 5:], **args)))
        i += 1
    return b"".join(out)


def compressed_chunks(stream):
    """[(offset of the payload, length)] of the stream's 0x46 chunks."""
    return [(p + 4, n) for p, t, n in SM.chunks_of(bytes(stream)) if t == CHUNK_COMPRESSED]


# ---- the corrupt set: one edit of a valid chunk each ----

def corrupt_set(cfg, R, bitmap):
    """-> [(name, payload)]: every payload must be refused (an error or a CRC mismatch).  `bitmap`: 1 KiB to 64 KiB with at least three
    byte values; the valid chunks (one sub-block each) are built here so that every edit finds its place."""
    T, M, B, field = cfg
    f = 3 + len(field)
    bitmap = bytes(bitmap)
    n = len(bitmap)
    whole = (n - 1).bit_length()
    assert MIN_BS + 5 <= whole < MAX_BS
    huff = build_compressed_table(cfg, R, bitmap, h0_bs=whole, kinds=["huff"])
    huff_fse = build_compressed_table(cfg, R, bitmap, h0_bs=whole, kinds=["huff"], forms={0: "fse"})
    raw = build_compressed_table(cfg, R, bitmap, h0_bs=whole, kinds=["raw"])
    one_bit = bytearray(n)
    one_bit[3] = 0x10
    sparse = build_compressed_table(cfg, R, bytes(one_bit), h0_bs=whole, kinds=["sparse"])
    cases = []

    def put(name, payload):
        cases.append((name, bytes(payload)))

    def with_byte(base, i, v):
        b = bytearray(base)
        b[i] = v
        return b
    d0 = f + 7                                                # the first table description; in `raw` and `sparse` the sub-block's record
    desc_len = read_huff_table(huff, d0)[3]
    rec = d0 + desc_len                                       # the sub-block's record: table index, uvarint, 4X data
    ln, used = get_uvarint(huff, rec + 1)
    data = rec + 1 + used
    put("h0_bs 4", with_byte(raw, f + 5, 4))
    put("h0_bs 18", with_byte(raw, f + 5, 18))
    put("h0_tc 17", with_byte(raw, f + 6, 17))
    put("table index == h0_tc", with_byte(huff, rec, 1))
    put("kind 19", with_byte(raw, d0, 19))
    put("cut uvarint", huff[:rec + 1] + bytes([0x80]))
    put("length beyond the chunk", huff[:rec + 1] + put_uvarint(ln + 1) + huff[data:])
    put("one trailing byte", huff + bytes(1))
    put("stale CRC", with_byte(huff, f + 1, huff[f + 1] ^ 1))
    put("n not divisible by the sub-block size", with_byte(raw, f + 5, whole + 1))
    put("more than 16 sub-blocks", with_byte(raw, f + 5, whole - 5))
    put("weights miss a power of two", huff[:d0] + bytes([127 + 3, 0x22, 0x10]) + huff[rec:])      # weights 2, 2, 1: 5 of 8, and 3 is no power of two
    put("table log 12", huff[:d0] + bytes([127 + 1, 0xc0]) + huff[rec:])
    fse_len = huff_fse[d0]
    assert fse_len < 128
    put("FSE weight section ends early", huff_fse[:d0] + bytes([fse_len - 1]) + huff_fse[d0 + 1:d0 + fse_len] + huff_fse[d0 + 1 + fse_len:])
    put("jump-table sizes beyond the sub-block", with_byte(huff, data + 5, 0xff))
    l1 = huff[data] | huff[data + 1] << 8
    put("stream's last byte 0", with_byte(huff, data + 6 + l1 - 1, 0))
    _, code, length, _ = huff_table(np.bincount(np.frombuffer(bitmap, np.uint8), minlength=256))
    seg = (n + 3) // 4
    short = encode_stream(bitmap[:seg - 1], code, length)     # stream 1 without its last symbol: the decoder's last lookup runs beyond its start
    body = len(short).to_bytes(2, "little") + huff[data + 2:data + 6] + short + huff[data + 6 + l1:]
    put("stream one symbol short", huff[:rec + 1] + put_uvarint(len(body)) + body)
    at_end = b"\xff" * (8 * n // 255) + bytes([8 * n % 255])
    put("sparse position at the bit count", sparse[:d0 + 1] + put_uvarint(len(at_end)) + at_end)
    put("sparse table ends in 255", sparse[:d0 + 1] + put_uvarint(2) + bytes([28, 255]))
    return cases
