"""Plain restatement of the decoder's tile-level classification (DESIGN.md "Tile levels"), and hand-built blocks next to its rule.

The decoder's index pass (dec_index2_kernel + dec_viol_kernel) decides per block:
conformant to one of the three level patterns (the exec pass then runs its tiles level by level), or general (dec_general_kernel,
settled by a team of 1, 2 or 4 workgroups).  A miss there is not an error: it is a schedule under which a tile may read a source tile
that has not been written yet.  This module says, byte range by byte range and in the slow obvious way, what the verdict must be.

- walk(body, dlen): the tokens of a block body, parsed from the format as oracle/minlz_oracle.c decodes it; walk_tokens(body) adds each
  token's stream offset, header length and form.
- apply(ops, dlen): the bytes those tokens produce.
- verdict(ops, dlen): the patterns the block fits, the one the decoder must pick, general or not, and the team size.
- cases(): hand-built blocks (body, expected bytes, intended verdict) around the rule; the intent is stated per (destination tile,
  source tile) pair by each case, so a case that reads one byte more or less than it claims is caught by verdict().

Test helper: no tests here.  The pattern words and the tile size are read from the C sources, not restated.
"""
import os
import re
from collections import namedtuple

import numpy as np

import oracle as O

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "minlz_amd", "csrc")


def _c_constants():
    enc = open(os.path.join(_CSRC, "mlz_encode.hip.inc")).read()
    ker = open(os.path.join(_CSRC, "mlz_kernels.h")).read()
    dec = open(os.path.join(_CSRC, "mlz_decode.hip.inc")).read()
    fast = int(re.search(r"constexpr uint32_t kPatternFast = (0x[0-9A-Fa-f]+)u;", enc).group(1), 16)
    dense = int(re.search(r"#define MLZ_PATTERN_DENSE (0x[0-9A-Fa-f]+)u", enc).group(1), 16)
    three = int(re.search(r"#define MLZ_PATTERN_THREE (0x[0-9A-Fa-f]+)u", enc).group(1), 16)
    tile_log = int(re.search(r"#define MLZ_TILE_LOG (\d+)", ker).group(1))
    seg_log = int(re.search(r"#define MLZ_SEG_LOG (\d+)", dec).group(1))
    return {"three": three, "dense": dense, "fast": fast}, tile_log, seg_log


PATTERNS, TILE_LOG, SEG_LOG = _c_constants()
TILE = 1 << TILE_LOG            # 32 KiB
SEG = 1 << SEG_LOG              # 8 KiB of token stream per index segment
PERIOD = 16                     # 2 bits per tile in a 32-bit word
ORDER = ("three", "dense", "fast")   # block_pattern: the first pattern a block fits


def level(pattern, tile):
    return (PATTERNS[pattern] >> (2 * (tile % PERIOD))) & 3


def may_read(pattern, dst_tile, src_tile):
    """A tile reads itself or tiles of a strictly lower level."""
    return src_tile == dst_tile or level(pattern, src_tile) < level(pattern, dst_tile)


Verdict = namedtuple("Verdict", "fits pattern general team")   # fits: frozenset of pattern names; team: 0 unless general


def team_of_distance(nearest, crosses):
    """team_of: a copy over a tile boundary, or one reading the tile in front: 1; two or three tiles back: 2; else 4."""
    if crosses or nearest == 1:
        return 1
    if nearest in (2, 3):
        return 2
    return 4


def make_verdict(fits, nearest, crosses):
    fits = frozenset(fits)
    pattern = next((p for p in ORDER if p in fits), None)
    general = pattern is None
    return Verdict(fits, pattern, general, team_of_distance(nearest, crosses) if general else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the format (oracle/minlz_oracle.c, mlzo_decode_body)
# ---------------------------------------------------------------------------------------------------------------------------------
Token = namedtuple("Token", "spos hlen form dpos lit off cp")
# spos: stream offset of the token; hlen: its header bytes (tag, length and offset fields; the literal bytes follow them); form: "literal",
# "repeat", "copy1", "copy2", "copy3" or "copy2_lits" (a fused copy3 with literals is "copy3" with lit != b"")


def walk_tokens(body):
    """Yields a Token per token of a block body, as oracle/minlz_oracle.c parses it (off: the effective offset; a repeat's is the one in
    force).  Raises ValueError on a token that runs past the end of the body; says nothing about offsets or the total."""
    b = bytes(body)
    n = len(b)
    s, d, offset = 0, 0, 1   # the initial offset is 1

    def need(k):
        if s + k > n:
            raise ValueError("truncated token at %d" % s)

    def uint(at, k):
        return int.from_bytes(b[at:at + k], "little")

    while s < n:
        t0 = s
        t = b[s]
        kind = t & 3
        lit = b""
        if kind == 0:
            x = t >> 3
            k = 1 if x < 29 else x - 27          # 29: 1 extra byte, 30: 2, 31: 3
            need(k)
            length = x + 1 if x < 29 else uint(s + 1, k - 1) + 30
            s += k
            if t & 4:                            # repeat: a copy at the offset in force
                yield Token(t0, k, "repeat", d, b"", offset, length)
                d += length
                continue
            need(length)
            yield Token(t0, k, "literal", d, b[s:s + length], offset, 0)
            s += length
            d += length
            continue
        if kind == 1:                            # copy1
            form = "copy1"
            need(2)
            length = (t >> 2) & 15
            offset = (uint(s, 2) >> 6) + 1
            s += 2
            if length == 15:
                need(1)
                length = b[s] + 18
                s += 1
            else:
                length += 4
        elif kind == 2:                          # copy2
            form = "copy2"
            need(3)
            length = t >> 2
            offset = uint(s + 1, 2) + 64
            s += 3
            if length <= 60:
                length += 4
            else:
                k = length - 60
                need(k)
                length = uint(s, k) + 64
                s += k
        else:                                    # fused copy2 with literals / copy3
            need(4)
            val = uint(s, 4)
            s += 4
            litlen = (val >> 3) & 3
            if not val & 4:
                form = "copy2_lits"
                length = 4 + ((val >> 5) & 7)
                offset = ((val >> 8) & 0xFFFF) + 64
                s -= 1
                litlen += 1
            else:
                form = "copy3"
                lt = (val >> 5) & 63
                offset = (val >> 11) + 65536
                if lt < 61:
                    length = lt + 4
                else:
                    k = lt - 60
                    need(k)
                    length = uint(s, k) + 64
                    s += k
            need(litlen)
            lit = b[s:s + litlen]
            s += litlen
        yield Token(t0, s - t0 - len(lit), form, d, lit, offset, length)
        d += len(lit) + length


def walk(body, dlen):
    """Yields (dpos, lit, off, cp) per token: output position, literal bytes, effective offset (a repeat's is the one in force) and
    copy length.  Raises ValueError on a body the oracle would reject for its framing."""
    d = 0
    for t in walk_tokens(body):
        yield t.dpos, t.lit, t.off, t.cp
        d = t.dpos + len(t.lit) + t.cp
    if d != dlen:
        raise ValueError("body decodes to %d bytes, not %d" % (d, dlen))


def apply(ops, dlen):
    """The bytes of a token list (a copy with off < cp repeats its window, byte after byte)."""
    out = bytearray(dlen)
    for d, lit, off, cp in ops:
        dc = d + len(lit)
        if dc > dlen:
            raise ValueError("literals at %d run past the block" % d)
        out[d:dc] = lit
        if not cp:
            continue
        if off == 0 or off > dc or dc + cp > dlen:
            raise ValueError("copy at %d: offset %d, length %d" % (dc, off, cp))
        if off >= cp:
            out[dc:dc + cp] = out[dc - off:dc - off + cp]
        else:
            win = bytes(out[dc - off:dc])
            out[dc:dc + cp] = (win * (cp // off + 1))[:cp]
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def verdict(ops, dlen):
    """Every tile a copy writes to reads, for its part of the copy, only itself or tiles of a strictly lower level; an overlapping copy
    (off < cp) reads its whole window [dc - off, dc).  The team: the nearest tile below its own that a copy landing in one tile (and
    reading at most two) reads; a copy whose destination crosses a tile boundary forces team 1."""
    fits = set(ORDER)
    nearest, crosses = None, False
    for d, lit, off, cp in ops:
        if not cp:
            continue
        dc = d + len(lit)
        first, last = dc // TILE, (dc + cp - 1) // TILE
        for kq in range(first, last + 1):
            p0, p1 = max(dc, kq * TILE), min(dc + cp, (kq + 1) * TILE)      # the part of the copy inside tile kq
            a, b = (p0 - off, p1 - off) if off >= cp else (dc - off, dc)    # the bytes that part reads
            src_tiles = range(a // TILE, (b - 1) // TILE + 1)
            for t in src_tiles:
                for p in list(fits):
                    if not may_read(p, kq, t):
                        fits.discard(p)
            if first == last:
                below = [t for t in src_tiles if t < kq]
                if below and len(src_tiles) <= 2:
                    dist = kq - max(below)
                    nearest = dist if nearest is None else min(nearest, dist)
        if last != first:
            crosses = True
    return make_verdict(fits, nearest, crosses)


def block_body(enc):
    """(body, dlen) of an encoded block (0x00, uvarint dlen, body); None for a stored (literal) block."""
    assert enc[0] == 0
    v, shift, i = 0, 0, 1
    while True:
        c = enc[i]
        v |= (c & 0x7F) << shift
        i += 1
        if c < 0x80:
            break
        shift += 7
    return (None, len(enc) - i) if v == 0 else (enc[i:], v)


def encode_block(body, dlen):
    out = bytearray([0])
    v = dlen
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out) + bytes(body)


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-built blocks
# ---------------------------------------------------------------------------------------------------------------------------------
# The filler tokens are laid out with numpy (a 1 MiB block has ~400 000 of them); their bytes are the emitters' (checked here once).
assert O.emit_literal(b"\x07") == b"\x00\x07"
assert O.emit_copy(2000, 8) == bytes([0x12, (2000 - 64) & 0xFF, (2000 - 64) >> 8])
UNIT_COPY = 8    # the filler's copies: (1-byte literal, 8-byte copy) = 9 bytes out of 5 stream bytes (a block's body must be shorter than it)

Case = namedtuple("Case", "name body dlen expected intended")   # expected: bytes; intended: Verdict


class Block:
    """A block written front to back.  Tiles nobody reads into are SLOW to decode (1-byte literals and 8-byte copies inside the tile);
    the tiles that read other tiles are FAST (a short literal, the deciding copy, one long copy of their own bytes): a schedule that
    lets a reader run before its source is done then reads unwritten bytes.  Every tile's bytes are its own (random per tile)."""

    def __init__(self, n_tiles, seed, dlen=None):
        self.dlen = dlen if dlen is not None else n_tiles * TILE
        self.out = np.zeros(self.dlen, dtype=np.uint8)
        self.body = []
        self.body_len = 0
        self.pos = 0
        self.off = 1
        self.rng = np.random.default_rng(seed)
        self.reads = set()        # (destination tile, source tile) pairs the case means to read
        self.crosses = False      # the case means a copy to cross a tile boundary

    # -- intent --
    def intend(self, dst_tile, *src_tiles):
        for t in src_tiles:
            if t != dst_tile:
                self.reads.add((dst_tile, t))

    def intended(self):
        fits = [p for p in ORDER if all(may_read(p, k, t) for k, t in self.reads)]
        below = [k - t for k, t in self.reads]
        return make_verdict(fits, min(below) if below else None, self.crosses)

    # -- tokens --
    def _tok(self, b):
        self.body.append(b)
        self.body_len += len(b)

    def _copy_out(self, dc, off, n):
        if off >= n:
            self.out[dc:dc + n] = self.out[dc - off:dc - off + n]
        else:
            win = self.out[dc - off:dc]
            self.out[dc:dc + n] = np.tile(win, n // off + 1)[:n]

    def lit(self, data):
        data = np.asarray(data, dtype=np.uint8)
        self._tok(O.emit_literal(data))
        self.out[self.pos:self.pos + data.size] = data
        self.pos += data.size

    def lits1(self, n):
        """n one-byte literal tokens of random bytes."""
        r = self.rng.integers(0, 256, n, dtype=np.uint8)
        tok = np.zeros(2 * n, dtype=np.uint8)
        tok[1::2] = r
        self._tok(tok.tobytes())
        self.out[self.pos:self.pos + n] = r
        self.pos += n

    def copy(self, src, n):
        off = self.pos - src
        self._tok(O.emit_copy(off, n))
        self._copy_out(self.pos, off, n)
        self.pos += n
        self.off = off

    def repeat(self, n):
        self._tok(O.emit_repeat(n))
        self._copy_out(self.pos, self.off, n)
        self.pos += n

    def copy_lits(self, three, lits, src, n):
        lits = np.asarray(lits, dtype=np.uint8)
        dc = self.pos + lits.size
        off = dc - src
        self._tok((O.emit_copy_lits3 if three else O.emit_copy_lits2)(lits, off, n))
        self.out[self.pos:dc] = lits
        self._copy_out(dc, off, n)
        self.pos = dc + n
        self.off = off

    def unique(self, n=16):
        self.lit(self.rng.integers(0, 256, n, dtype=np.uint8))

    # -- tiles --
    def slow(self, to):
        """[pos, to), inside the current tile: one-byte literals for the tile's first 2 KiB, then (literal, short copy) pairs reading
        the tile's first KiB."""
        t0 = self.pos // TILE * TILE
        assert to <= t0 + TILE and to >= self.pos
        if self.pos < t0 + 2048:
            self.lits1(min(to, t0 + 2048) - self.pos)
        u = 1 + UNIT_COPY
        k = (to - self.pos) // u
        if k:
            dst = self.pos + u * np.arange(k)
            src = t0 + self.rng.integers(0, 1024 - UNIT_COPY, k)
            off = dst + 1 - src                      # 1025 .. 34 000: copy2
            r = self.rng.integers(0, 256, k, dtype=np.uint8)
            tok = np.zeros((k, 5), dtype=np.uint8)
            tok[:, 1] = r
            tok[:, 2] = ((UNIT_COPY - 4) << 2) | 2
            tok[:, 3] = (off - 64) & 0xFF
            tok[:, 4] = (off - 64) >> 8
            self._tok(tok.tobytes())
            self.out[dst] = r
            for j in range(UNIT_COPY):
                self.out[dst + 1 + j] = self.out[src + j]
            self.pos += u * k
            self.off = int(off[-1])
        if to > self.pos:
            self.lits1(to - self.pos)

    def fast(self, to):
        """[pos, to) inside the current tile as one copy of the tile's own first bytes."""
        t0 = self.pos // TILE * TILE
        assert self.pos > t0 and to <= t0 + TILE
        if to > self.pos:
            self.copy(t0, to - self.pos)

    def fill(self, to, how="slow"):
        while self.pos < to:
            end = min(to, (self.pos // TILE + 1) * TILE)
            if how == "fast" and self.pos % TILE:
                self.fast(end)
            else:
                self.slow(end)

    def pad_stream_to(self, body_pos):
        """Literal tokens until the token stream is body_pos bytes long (2 bytes per 1-byte literal, 3 per 2-byte one)."""
        gap = body_pos - self.body_len
        assert gap >= 0 and gap != 1
        if gap % 2:
            self.lit(self.rng.integers(0, 256, 2, dtype=np.uint8))
            gap -= 3
        self.lits1(gap // 2)
        assert self.body_len == body_pos

    def reader(self, kd, src, n, src_tiles, prefix=16):
        """Tile kd (from its first byte): a short literal, a copy of n bytes from src, the rest one copy of its own bytes."""
        self.fill(kd * TILE)
        assert self.pos == kd * TILE
        if prefix:
            self.unique(prefix)
        self.copy(src, n)
        self.intend(kd, *src_tiles)
        self.fill((kd + 1) * TILE, "fast")

    def case(self, name):
        self.fill(self.dlen)
        body = b"".join(self.body)
        return Case(name, body, self.dlen, self.out.tobytes(), self.intended())


# -- choosing tiles from the pattern words --
def allowed(pattern, kd, lo=0):
    return [s for s in range(max(lo, 0), kd) if may_read(pattern, kd, s)]


def forbidden(pattern, kd, lo=0):
    return [s for s in range(max(lo, 0), kd) if not may_read(pattern, kd, s)]


def _edge_pair(pattern, lo=16, hi=32):
    """A destination tile kd and an allowed source s whose next tile s + 1 (< kd) is forbidden."""
    for kd in range(lo, hi):
        for s in reversed(allowed(pattern, kd, kd - 15)):
            if s + 1 < kd and not may_read(pattern, kd, s + 1):
                return kd, s
    raise AssertionError(pattern)


def _two_allowed(pattern, lo=16, hi=32):
    for kd in range(lo, hi):
        for s in reversed(allowed(pattern, kd, kd - 15)):
            if s + 1 < kd and may_read(pattern, kd, s + 1):
                return kd, s
    raise AssertionError(pattern)


def _only(pattern, lo=1, hi=32, dist=1):
    """A tile kd whose read of kd - dist only `pattern` allows."""
    for kd in range(max(lo, dist), hi):
        if [p for p in ORDER if may_read(p, kd, kd - dist)] == [pattern]:
            return kd
    raise AssertionError(pattern)


def _seed(name):
    return sum((i + 1) * c for i, c in enumerate(name.encode())) & 0xFFFFFF


def named_cases():
    out = []
    T = TILE

    def blk(name, n_tiles=32):
        return Block(n_tiles, _seed(name)), name

    for p in ORDER:
        kd, s = _edge_pair(p)
        b, nm = blk("src_ends_on_allowed_tile_" + p)     # source ends on the last byte of an allowed tile
        b.reader(kd, (s + 1) * T - 4096, 4096, [s])
        out.append(b.case(nm))
        b, nm = blk("src_one_byte_into_forbidden_" + p)  # ... one byte longer
        b.reader(kd, (s + 1) * T - 4096, 4097, [s, s + 1])
        out.append(b.case(nm))
        b, nm = blk("src_allowed_then_forbidden_" + p)
        b.reader(kd, (s + 1) * T - 2048, 4096, [s, s + 1])
        out.append(b.case(nm))
        kd2, s2 = _two_allowed(p)
        b, nm = blk("src_two_allowed_tiles_" + p)
        b.reader(kd2, (s2 + 1) * T - 2048, 4096, [s2, s2 + 1])
        out.append(b.case(nm))

    # destination edges
    kd = 19                                               # three: level 2; tile 16 (level 0) is allowed for it and for tile 20
    b, nm = blk("dst_copy_fills_its_tile")
    b.fill((kd + 1) * T - 3000)
    b.copy(16 * T + 100, 3000)
    b.intend(kd, 16)
    out.append(b.case(nm))
    for tag, src_tile in (("allowed", 16), ("forbidden_for_next", 17)):
        # a copy over the boundary of tiles 19 | 20; its second part is checked against tile 20 (level 1 in three, 2 in dense, 0 in fast)
        b, nm = blk("dst_copy_crosses_tiles_" + tag)
        b.fill((kd + 1) * T - 1000)
        b.copy(src_tile * T + 5000, 3000)
        b.intend(kd, src_tile)
        b.intend(kd + 1, src_tile)
        b.crosses = True
        out.append(b.case(nm))
    for three, dist in ((False, 2), (True, 3)):
        kd = next(k for k in range(18, 32) if level("three", k) > 0 and may_read("three", k, k - dist))
        b, nm = blk("copy_lits%d_start_tile_%d" % (3 if three else 2, kd))
        b.fill(kd * T - 3)
        b.copy_lits(three, b.rng.integers(0, 256, 3, dtype=np.uint8), (kd - dist) * T + 7, 40)   # (lits2 > 11 bytes: + a repeat)
        b.intend(kd, kd - dist)
        b.fill((kd + 1) * T, "fast")
        out.append(b.case(nm))

    # overlapping copies: the window starts one byte inside the tile in front (forbidden for fast / three at kd), or in the tile itself
    for p in ("fast", "three"):
        kd = _only("dense", 16, 32) if p == "three" else next(k for k in range(16, 32) if not may_read("fast", k, k - 1))
        b, nm = blk("overlap_window_one_byte_into_%d" % kd)
        b.fill(kd * T)
        b.unique(16)
        b.copy(kd * T - 1, 1000)                            # off 17 < 1000: reads [kd T - 1, kd T + 16)
        b.intend(kd, kd - 1)
        b.fill((kd + 1) * T, "fast")
        out.append(b.case(nm))
    b, nm = blk("overlap_window_inside_own_tile")
    b.fill(21 * T)
    b.unique(16)
    b.copy(21 * T, 1000)
    b.fill(22 * T, "fast")
    out.append(b.case(nm))

    # period wrap
    b, nm = blk("read_16_tiles_back")
    b.reader(20, 4 * T + 1000, 20000, [4])
    out.append(b.case(nm))
    b, nm = blk("into_tile_16")
    b.reader(16, 15 * T + 100, 8000, [15])
    out.append(b.case(nm))

    # a repeat whose offset was set more than a segment and more than 64 tokens earlier
    kd, s = _edge_pair("three")                             # s allowed for kd, s + 1 forbidden
    for tag in ("allowed", "forbidden"):
        b, nm = blk("repeat_carried_" + tag)
        b.fill(kd * T)
        b.unique(16)
        L = 5000                                             # 5000 one-byte literal tokens: 10 000 stream bytes
        src = s * T + 100 if tag == "allowed" else (s + 1) * T - 64 - L   # the repeat then reads tile s, or exactly from tile s + 1 on
        b.copy(src, 64)
        b.lits1(L)
        b.repeat(3000)
        b.intend(kd, s)
        if tag == "forbidden":
            b.intend(kd, s + 1)
        b.fill((kd + 1) * T, "fast")
        out.append(b.case(nm))

    # pattern selection
    k_fast = _only("fast")
    b, nm = blk("fits_fast_only")
    b.reader(k_fast, (k_fast - 1) * T + 500, 30000, [k_fast - 1])
    b.reader(k_fast + 16, (k_fast + 15) * T + 700, 30000, [k_fast + 15])
    out.append(b.case(nm))
    b, nm = blk("fits_dense_only")                          # 2 reads 1 (fast, dense), 6 reads 2 (dense, three)
    b.reader(2, 1 * T + 300, 20000, [1])
    b.reader(6, 2 * T + 300, 20000, [2])
    out.append(b.case(nm))
    b, nm = blk("fits_three_and_all")
    b.reader(3, 0 * T + 300, 20000, [0])
    b.reader(19, 16 * T + 300, 20000, [16])
    out.append(b.case(nm))
    b, nm = blk("fits_none")
    b.reader(4, 3 * T + 300, 20000, [3])
    out.append(b.case(nm))

    # team sizes: general through a read 16 tiles back, then the nearest read d tiles back
    for d in (1, 2, 3, 4, 5):
        b, nm = blk("team_nearest_%d_back" % d)
        b.reader(24, 8 * T + 100, 10000, [8])
        b.reader(28, (28 - d) * T + 20000, 10000, [28 - d])
        out.append(b.case(nm))
    b, nm = blk("team_crossing_copy")
    b.reader(24, 8 * T + 100, 10000, [8])
    b.fill(27 * T - 500)
    b.copy(20 * T + 100, 1000)
    b.intend(26, 20)
    b.intend(27, 20)
    b.crosses = True
    out.append(b.case(nm))

    # placement: the deciding copy first in its tile, first in a segment of the stream, last in the block
    b, nm = blk("first_token_of_its_tile")
    b.reader(k_fast + 16, (k_fast + 15) * T + 9000, 12000, [k_fast + 15], prefix=0)
    out.append(b.case(nm))
    b, nm = blk("first_token_of_a_segment")
    kd = k_fast + 16
    b.fill(kd * T)
    b.unique(16)
    at = (b.body_len // SEG + 1) * SEG
    b.pad_stream_to(at if at - b.body_len >= 2 else at + SEG)
    b.copy((kd - 1) * T + 2000, 9000)
    b.intend(kd, kd - 1)
    b.fill((kd + 1) * T, "fast")
    out.append(b.case(nm))
    b, nm = blk("last_token_of_the_block")
    b.fill(32 * T - 5000)
    b.copy(30 * T + 100, 5000)
    b.intend(31, 30)
    out.append(b.case(nm))
    return out


def big_cases():
    """8 MiB blocks (256 tiles): conformant to three with reads all over it (the last token of the last tile among them), and a
    general one whose only cross-tile read goes into tile 32 (level 0 again)."""
    T = TILE
    b = Block(256, _seed("big_three"))
    for kd in (17, 35, 70, 101, 150, 199, 230):
        s = max(allowed("three", kd, kd - 15))
        b.reader(kd, s * T + 1234, 25000, [s])
    b.fill(256 * T - 7000)
    b.copy(240 * T + 50, 7000)
    b.intend(255, 240)
    three = b.case("big_three_last_token")
    b = Block(256, _seed("big_tile32"))
    b.reader(32, 31 * T + 4000, 20000, [31])
    return [three, b.case("big_into_tile_32")]


def sweep_cases():
    """Per pattern: one block whose every tile of level > 0 reads its nearest allowed source; and per destination tile mod 16, a block
    in which tile 16 + m reads its nearest forbidden source (whatever the other patterns then say)."""
    T = TILE
    out = []
    for p in ORDER:
        b = Block(32, _seed("sweep_allowed_" + p))
        for kd in range(1, 32):
            ok = allowed(p, kd, kd - 15)
            if ok:
                b.reader(kd, ok[-1] * T + 3000, 6000, [ok[-1]])
        out.append(b.case("sweep_allowed_" + p))
        for m in range(16):
            kd = 16 + m
            bad = forbidden(p, kd, kd - 15)
            if not bad:
                continue
            b = Block(32, _seed("sweep_forbidden_%s_%d" % (p, m)))
            b.reader(kd, bad[-1] * T + 3000, 6000, [bad[-1]])
            out.append(b.case("sweep_forbidden_%s_%d" % (p, m)))
    return out


_CACHE = {}


def cases(kind="named"):
    if kind not in _CACHE:
        _CACHE[kind] = {"named": named_cases, "big": big_cases, "sweep": sweep_cases}[kind]()
    return _CACHE[kind]
