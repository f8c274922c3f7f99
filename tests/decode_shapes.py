"""Designed token streams for the block decoder's internal capacities, and a census that proves what each of them reaches.

The decoder (mlz_decode.hip.inc, mlz_decode_index.hip.inc, mlz_decode_exec.hip.inc, mlz_decode_general.hip.inc) rests on capacities the
format knows nothing about: kept exits and staged token positions per 8 KiB segment of the stream, 64-token rounds, and in the pass for
general blocks a 32 KiB pool of 8-byte slots, a number of prefetched external entries, a ring of three tile images, doubling rounds over
in-tile chains, ready flags taken 64 tiles at a time and teams of settling workgroups.  Natural text reaches few of their edges.

- The constants are read from the C sources by regex, never restated; a regex that no longer matches is an error at import.
- census(body, dlen) says, in plain numpy on top of tile_levels.walk_tokens / verdict, what a block asks of those capacities.
- shape(name) gives a seeded, hand-built general block (body, dlen, facts); facts are predicates over the census that state which capacity
  the block exceeds or meets.  tests/test_decode_shapes.py checks them on the CPU, so a kernel constant that moves makes a fact fail
  instead of silently leaving the path unreached.  Expected bytes always come from the oracle's decoder (expected(name)).

Every shape is a general block: tile 0 is noise in 29-byte literals (tiles 0 .. gap - 1 for the team shapes), the plain tiles after it are
a 16-byte literal, 64 bytes of the tile `gap` tiles back and an overlapping copy of those 80 bytes, so tile 4 reads tile 3 (or, with gap 2 or 4, a tile no level pattern lets it
read) and no pattern fits.

Test helper: no tests here."""
import os
import re
from collections import namedtuple

import numpy as np

import oracle as O
from tests import tile_levels as TL


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' constants
# ---------------------------------------------------------------------------------------------------------------------------------
def _c_constants():
    def text(name):
        return open(os.path.join(TL._CSRC, name)).read()

    def find(src, pattern, what):
        m = re.search(pattern, src)
        if not m:
            raise RuntimeError("tests/decode_shapes.py: cannot find %s in the C sources (pattern %r)" % (what, pattern))
        return m

    ker, dec, idx, gen = text("mlz_kernels.h"), text("mlz_decode.hip.inc"), text("mlz_decode_index.hip.inc"), text("mlz_decode_general.hip.inc")
    c = {}
    c["TILE_LOG"] = int(find(ker, r"#define MLZ_TILE_LOG (\d+)", "MLZ_TILE_LOG").group(1))
    c["SEG_LOG"] = int(find(dec, r"#define MLZ_SEG_LOG (\d+)", "MLZ_SEG_LOG").group(1))
    tile, seg = 1 << c["TILE_LOG"], 1 << c["SEG_LOG"]
    c["EXIT_KEEP"] = int(find(dec, r"constexpr uint32_t kExitKeep = (\d+);", "kExitKeep").group(1))
    c["IDX_STAGE"] = seg // int(find(idx, r"constexpr uint32_t kIdxStage = kSeg / (\d+);", "kIdxStage").group(1))
    c["GEN_EP"] = int(find(gen, r"#define MLZ_GEN_EP (\d+)", "MLZ_GEN_EP").group(1))
    c["GEN_THREADS"] = int(find(gen, r"constexpr int kGenThreads = (\d+);", "kGenThreads").group(1))
    c["EXT_MAX"] = int(find(gen, r"constexpr uint32_t kExtMax = (\d+);", "kExtMax").group(1))
    find(gen, r"constexpr uint32_t kPool = kTile;", "kPool")
    c["POOL"] = tile
    c["ROUND"] = 1 << int(find(gen, r"const uint32_t j_first = rank0 >> (\d+), j_last = r_last >> \1;", "the token round").group(1))
    c["RING_TILES"] = int(find(gen, r"constexpr uint32_t kRing = (\d+) \* kTile;", "kRing").group(1))
    # the overflow rule of role E: ((literal bytes + 31) & ~31) + 8 * entries > kPool
    m = find(gen, r"\(\(shw\[3\] \+ (\d+)\) & ~(\d+)u\) \+ (\d+) \* shw\[1\] > kPool", "the pool's overflow rule")
    if m.group(1) != m.group(2):
        raise RuntimeError("tests/decode_shapes.py: the pool's overflow rule does not round the literal bytes up as expected")
    c["POOL_LIT_ROUND"] = int(m.group(1)) + 1
    c["POOL_SLOT"] = int(m.group(3))
    # the ready flags role S takes per call of ensure(): a wavefront's lanes
    c["FLAG_BATCH"] = int(find(gen, r"const uint32_t upto = notready \? uint32_t\(ctz64\(notready\)\) : (\d+)u;", "the ready-flag batch").group(1))
    return c


K = _c_constants()
assert K["TILE_LOG"] == TL.TILE_LOG and K["SEG_LOG"] == TL.SEG_LOG
TILE, SEG = TL.TILE, TL.SEG
EXIT_KEEP, IDX_STAGE, ROUND = K["EXIT_KEEP"], K["IDX_STAGE"], K["ROUND"]
EXT_MAX, POOL = K["EXT_MAX"], K["POOL"]
PREFETCHED = K["GEN_EP"] * K["GEN_THREADS"]     # external entries of a tile that role S prefetches; the rest take its plain loop
RING = K["RING_TILES"] * TILE
MAX_OFFSET = (2 << 20) + 65535                  # the largest copy3 offset (the format's field)
TAGGY = np.array([0xE8, 0xF0, 0xF8, 0xFF, 0x07, 0x0F, 0xFB, 0x02, 0x01, 0x00], dtype=np.uint8)   # values that long-literal and copy3 tags have


def round_up(x, m):
    return (x + m - 1) // m * m


def pool_need(lit_bytes, ext_entries):
    return round_up(lit_bytes, K["POOL_LIT_ROUND"]) + K["POOL_SLOT"] * ext_entries


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
KINDS = ("lit1", "lit2", "lit3", "copy1", "copy2", "copy3", "copy2_lits", "copy3_lits", "repeat")


def _kind(t):
    """The token forms walk_tokens names, a literal by the bytes of its length field (a literal of < 30 bytes has none: "lit0")."""
    if t.form == "literal":
        return "lit%d" % (t.hlen - 1)
    if t.form == "copy3" and t.lit:
        return "copy3_lits"
    return t.form


class Census:
    """What census() found; see there."""

    def tile_entries(self, tile):
        """(source position, length) of every external entry of a tile, as role E cuts them: a run's entries start every kExtMax bytes."""
        sel = np.nonzero(self.run_tile == tile)[0]
        src, ln = [], []
        for r in sel:
            for q in range(0, int(self.run_len[r]), EXT_MAX):
                src.append(int(self.run_src[r]) + q)
                ln.append(min(EXT_MAX, int(self.run_len[r]) - q))
        return np.array(src, dtype=np.int64), np.array(ln, dtype=np.int64)


def census(body, dlen):
    """What a block body asks of the decoder's capacities.  Raises ValueError where tile_levels.walk does.

    Per tile (arrays of n_tiles):
      tokens       tokens whose output starts in the tile
      lit_bytes    literal bytes in the tile
      ext_entries  external entries.  A byte is external when the position it copies from directly (its own minus the token's offset)
                   lies before the tile's first byte.  Inside one copy token's part of a tile these bytes are one run, the part's first
                   min(part, tile start + offset - part start) bytes; a run of len bytes counts ceil(len / kExtMax) entries.
                   Checked against role E of mlz_decode_general.hip.inc: it clips the copy to the tile [c0, c1), takes e1 = min(c1,
                   tstart + off), n_ext = e1 - c0 and cnt = (n_ext + kExtMax - 1) / kExtMax, and writes entry q with source
                   c0 - off + q * kExtMax and length min(kExtMax, n_ext - q * kExtMax) — the same bytes, the same cut.
      pool_need    round_up(lit_bytes, 32) + 8 * ext_entries, the left side of role E's overflow test against kPool
      chain_depth  the most in-tile copy hops from an output byte to its terminal (a literal or an external byte), by pointer jumping
      chain_end    "lit" or "ext": what the deepest chain of the tile ends in
      src_back     the set of distances, in tiles, from the tile to the tiles its external bytes come from
    Per external run: run_pos, run_src, run_len, run_tile.
    Per 8 KiB segment of the body: seg_starts (token starts) and seg_entry (the offset of the first one; SEG when there is none).
    Per block: max_offset, n_tiles, verdict (tile_levels.verdict: general or not, and the team).
    Per token (dict tok): spos, hlen, dpos, lit, off, cp as arrays, kind as a list of KINDS names."""
    toks = list(TL.walk_tokens(body))
    n = len(toks)
    c = Census()
    spos = np.fromiter((t.spos for t in toks), np.int64, n)
    hlen = np.fromiter((t.hlen for t in toks), np.int64, n)
    dpos = np.fromiter((t.dpos for t in toks), np.int64, n)
    lit = np.fromiter((len(t.lit) for t in toks), np.int64, n)
    off = np.fromiter((t.off for t in toks), np.int64, n)
    cp = np.fromiter((t.cp for t in toks), np.int64, n)
    total = int(dpos[-1] + lit[-1] + cp[-1]) if n else 0
    if total != dlen:
        raise ValueError("body decodes to %d bytes, not %d" % (total, dlen))
    c.tok = {"spos": spos, "hlen": hlen, "dpos": dpos, "lit": lit, "off": off, "cp": cp, "kind": [_kind(t) for t in toks]}
    c.verdict = TL.verdict([(t.dpos, t.lit, t.off, t.cp) for t in toks], dlen)
    c.n_tiles = nt = (dlen + TILE - 1) // TILE
    c.max_offset = int(off[cp > 0].max()) if (cp > 0).any() else 0
    c.tokens = np.bincount(dpos >> TL.TILE_LOG, minlength=nt)

    # per output byte: the position it copies from (-1: a literal), its token
    pos = np.arange(dlen, dtype=np.int32)
    src = np.full(dlen, -1, dtype=np.int32)
    dc = dpos + lit
    first = np.repeat(dc - (np.cumsum(cp) - cp), cp)             # dc - (copy bytes before this token) ...
    at = (np.arange(int(cp.sum()), dtype=np.int64) + first)      # ... + running index = the byte's position
    if (off[cp > 0] > dc[cp > 0]).any():
        raise ValueError("a copy reaches before the block")
    src[at] = (at - np.repeat(off, cp)).astype(np.int32)
    tokid = np.repeat(np.arange(n, dtype=np.int32), lit + cp)
    tile_of = pos >> TL.TILE_LOG
    tstart = tile_of << TL.TILE_LOG
    is_lit = src < 0
    ext = (~is_lit) & (src < tstart)
    c.lit_bytes = np.bincount(tile_of[is_lit], minlength=nt)

    # external runs: maximal inside one token's part of one tile
    prev_same = np.zeros(dlen, dtype=bool)
    prev_same[1:] = ext[:-1] & (tokid[1:] == tokid[:-1]) & (tile_of[1:] == tile_of[:-1])
    start = ext & ~prev_same
    c.run_pos = np.nonzero(start)[0]
    run_id = np.cumsum(start)[ext] - 1
    c.run_len = np.bincount(run_id, minlength=c.run_pos.size)
    c.run_src = src[c.run_pos].astype(np.int64)
    c.run_tile = (c.run_pos >> TL.TILE_LOG)
    c.ext_entries = np.bincount(c.run_tile, weights=(c.run_len + EXT_MAX - 1) // EXT_MAX, minlength=nt).astype(np.int64)
    c.pool_need = np.array([pool_need(int(l), int(e)) for l, e in zip(c.lit_bytes, c.ext_entries)], dtype=np.int64)
    pairs = np.unique(tile_of[ext].astype(np.int64) * (1 << 20) + (tile_of[ext] - (src[ext] >> TL.TILE_LOG)))
    c.src_back = [set() for _ in range(nt)]
    for v in pairs.tolist():
        c.src_back[v >> 20].add(v & 0xFFFFF)

    # in-tile chains: p = the byte one hop on (itself: a terminal), depth = hops from the byte to p; doubled until every p is a terminal
    p = np.where(is_lit | ext, pos, src)
    depth = (p != pos).astype(np.int32)
    while True:
        pp = p[p]
        if np.array_equal(pp, p):
            break
        depth = depth + depth[p]
        p = pp
    c.chain_depth = np.zeros(nt, dtype=np.int64)
    c.chain_end = []
    for t in range(nt):
        a, b = t * TILE, min(dlen, (t + 1) * TILE)
        j = a + int(np.argmax(depth[a:b]))
        c.chain_depth[t] = depth[j]
        c.chain_end.append("lit" if is_lit[p[j]] else "ext")

    nseg = (len(body) + SEG - 1) // SEG
    c.seg_starts = np.bincount(spos >> TL.SEG_LOG, minlength=nseg)
    first_tok = np.searchsorted(spos, np.arange(nseg, dtype=np.int64) * SEG)
    c.seg_entry = np.full(nseg, SEG, dtype=np.int64)
    have = c.seg_starts > 0
    c.seg_entry[have] = spos[first_tok[have]] - np.nonzero(have)[0] * SEG
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------
# tokens laid out with numpy are the emitters' bytes (checked here once)
def _copy2(off, n):
    return bytes([(n - 4) << 2 | 2, (off - 64) & 0xFF, (off - 64) >> 8])


def _copy3(off, n):
    return int(3 | 4 | (n - 4) << 5 | (off - 65536) << 11).to_bytes(4, "little")


assert O.emit_copy(2000, 8) == _copy2(2000, 8) and O.emit_copy(70000, 8) == _copy3(70000, 8) and O.emit_copy(MAX_OFFSET, 64) == _copy3(MAX_OFFSET, 64)
assert O.emit_literal(bytes(29)) == bytes([28 << 3]) + bytes(29) and O.emit_repeat(1) == bytes([4])


class Build:
    """A block body written front to back.  Only positions are tracked; the bytes a body decodes to are the oracle's business."""

    def __init__(self, seed, gap=1):
        self.rng = np.random.default_rng(seed)
        self.gap = gap            # a plain tile reads the tile `gap` tiles back
        self.parts = []
        self.body_len = 0
        self.pos = 0

    def raw(self, b, out):
        b = bytes(b)
        self.parts.append(b)
        self.body_len += len(b)
        self.pos += out

    def noise(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8)

    def lit(self, n, data=None):
        self.raw(O.emit_literal(self.noise(n) if data is None else data), n)

    def lits1(self, n):
        """n one-byte literal tokens."""
        tok = np.zeros(2 * n, dtype=np.uint8)
        tok[1::2] = self.noise(n)
        self.raw(tok.tobytes(), n)

    def copy(self, off, n):
        assert 1 <= off <= self.pos, (off, self.pos)
        self.raw(O.emit_copy(off, n), n)

    def copy_from(self, src, n):
        self.copy(self.pos - src, n)

    def repeat(self, n):
        self.raw(O.emit_repeat(n), n)

    def repeats1(self, n):
        self.raw(O.emit_repeat(1) * n, n)

    def copy_lits(self, three, nlit, off, n):
        assert off <= self.pos + nlit
        self.raw((O.emit_copy_lits3 if three else O.emit_copy_lits2)(self.noise(nlit), off, n), nlit + n)

    def tile(self):
        return self.pos // TILE

    def pad_out_to(self, p):
        """29-byte literals (one-byte headers) and a shorter one until the output is p bytes long."""
        gap = p - self.pos
        assert gap >= 0
        k = gap // 29
        if k:
            tok = np.empty((k, 30), dtype=np.uint8)
            tok[:, 0] = 28 << 3
            tok[:, 1:] = self.noise(29 * k).reshape(k, 29)
            self.raw(tok.tobytes(), 29 * k)
        if gap % 29:
            self.lit(gap % 29)

    def pad_stream_to(self, s):
        """One-byte literal tokens (and one two-byte literal for an odd gap) until the body is s bytes long."""
        gap = s - self.body_len
        assert gap >= 0 and gap != 1, gap
        if gap % 2:
            self.lit(2)
            gap -= 3
        self.lits1(gap // 2)
        assert self.body_len == s

    def next_stream_mark(self, residue, room=2):
        """The next body length that is `residue` mod SEG and at least `room` bytes on (never exactly one byte: it cannot be padded to)."""
        s = self.body_len + room
        s += (residue - s) % SEG
        return s

    def plain(self, upto_tile):
        """Plain tiles up to (not including) tile upto_tile: noise while there is no tile `gap` back, else 16 literal bytes of the tile's own, 64
        bytes of the tile `gap` back (8 entries) and those 80 bytes again and again to the tile's end."""
        assert self.pos % TILE == 0
        while self.pos < upto_tile * TILE:
            if self.tile() < self.gap:
                self.pad_out_to(self.pos + TILE)
            else:
                self.lit(16)
                self.copy(self.gap * TILE, 64)
                self.copy(80, TILE - 80)

    def end_tile(self):
        """The rest of the current tile as one overlapping copy of the tile's own last bytes."""
        rest = -self.pos % TILE
        if 0 < rest < 4:
            self.lit(rest)
        elif rest:
            assert self.pos % TILE
            self.copy(min(80, self.pos % TILE), rest)

    def close(self, min_tiles=6):
        """Ends the tile, then plain tiles until the block has min_tiles and its body is shorter than its output."""
        self.end_tile()
        while self.tile() < min_tiles or self.body_len + 16 >= self.pos:
            self.plain(self.tile() + 1)
        return b"".join(self.parts), self.pos

    # -- the tiles the shapes are about --
    def entries_tile(self, n_ext, lit_bytes, short=0):
        """A whole tile: n_ext copies of 8 bytes (`short` of them of 4) from at least `gap` tiles back, lit_bytes literal bytes (a head and
        one-byte literals in front of the first copies), the rest one overlapping copy inside the tile."""
        assert self.pos % TILE == 0 and self.tile() > self.gap
        head = min(lit_bytes, 16)
        ones = min(n_ext, lit_bytes - head)
        head = lit_bytes - ones
        ext_out = 8 * n_ext - 4 * short
        rest = TILE - ext_out - lit_bytes
        assert rest == 0 or rest >= 4, rest
        if head:
            self.lit(head)
        cl = np.full(n_ext, 8, dtype=np.int64)
        cl[n_ext - short:] = 4
        lone = (np.arange(n_ext) < ones).astype(np.int64)            # a one-byte literal in front of copy i
        off = self.gap * TILE + self.rng.integers(0, 2048, n_ext)    # copy i reads its own place `gap` tiles back, or up to 2 KiB before it
        three = self.gap > 1                                          # offsets of 65 536 and more: copy3
        width = 4 if three else 3
        size = 2 * lone + width
        at = np.cumsum(size) - size
        tok = np.zeros(int(size.sum()), dtype=np.uint8)
        tok[at[lone == 1] + 1] = self.noise(ones)
        h = at + 2 * lone
        if three:
            val = 3 | 4 | (cl - 4) << 5 | (off - 65536) << 11
            for j in range(4):
                tok[h + j] = (val >> (8 * j)) & 0xFF
        else:
            assert off.max() <= 65599
            tok[h] = (cl - 4) << 2 | 2
            tok[h + 1] = (off - 64) & 0xFF
            tok[h + 2] = (off - 64) >> 8
        self.raw(tok.tobytes(), ones + ext_out)
        if rest:
            self.copy(24, rest)
        assert self.pos % TILE == 0

    def sources_tile(self, dists):
        """From the tile's first byte: copies whose sources lie d tiles back for every d of dists, at every residue mod 8 of the source
        address, of 4 .. 16 bytes (entries of 1 .. 8 bytes).  The tile is left open."""
        assert self.pos % TILE == 0
        k = self.tile()
        self.lit(16)
        for d in dists:
            base = (k - d) * TILE + 1000
            for r in range(8):                       # source address residues 0 .. 7; lengths 4 .. 16: last entries of 4 .. 8 and 1 .. 8 bytes
                for n in (4 + r, 9 + r):
                    self.copy_from(base + 8 * int(self.rng.integers(0, 3000)) + r, n)
                self.lits1(1)
        return k


Shape = namedtuple("Shape", "name body dlen facts")


def _seed(name):
    return TL._seed("decode_shapes/" + name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _entries(name, n_ext, lit_bytes, short=0, gap=1, tile=3, min_tiles=7):
    b = Build(_seed(name), gap)
    b.plain(tile)
    b.entries_tile(n_ext, lit_bytes, short)
    body, dlen = b.close(min_tiles)
    return b, body, dlen, tile


def entries_shape(name, n_ext):
    """One tile (tile 3) with exactly n_ext external entries.  Up to 4096 of them the slots fit: above MLZ_GEN_EP * kGenThreads role S runs
    its plain loop behind the prefetched entries, with the slot pool.  4097 entries (4095 of 8 bytes, 2 of 4) overflow the slots: the tile
    is redone packed."""
    full = TILE // EXT_MAX
    if n_ext < full:
        _, body, dlen, k = _entries(name, n_ext, 1000)
    elif n_ext == full:
        _, body, dlen, k = _entries(name, n_ext, 0)
    else:
        assert n_ext == full + 1
        _, body, dlen, k = _entries(name, n_ext, 0, short=2)
    facts = {"tile %d has exactly %d entries" % (k, n_ext): lambda c: c.ext_entries[k] == n_ext,
             "every source is at least a tile back": lambda c: min(c.src_back[k]) >= 1}
    if n_ext <= full:
        facts["the slots fit: pool_need <= kPool"] = lambda c: c.pool_need[k] <= POOL
    else:
        facts["the slots overflow: pool_need > kPool"] = lambda c: c.pool_need[k] > POOL
    if n_ext > PREFETCHED:
        facts["more entries than role S prefetches"] = lambda c: c.ext_entries[k] > PREFETCHED
    else:
        facts["no more entries than role S prefetches"] = lambda c: c.ext_entries[k] <= PREFETCHED
    return Shape(name, body, dlen, facts)


def pool_shape(name, over):
    """pool_need == kPool exactly (3000 entries, 8768 literal bytes), or the smallest value above it: both terms of pool_need are
    multiples of 8, so that is kPool + 8 (3001 entries, 8737 literal bytes, which round up to 8768)."""
    n_ext = 3000
    lit_bytes = POOL - K["POOL_SLOT"] * n_ext
    assert lit_bytes % K["POOL_LIT_ROUND"] == 0 and lit_bytes + 8 * n_ext == TILE
    if over:
        n_ext += 1
        lit_bytes -= K["POOL_LIT_ROUND"] - 1
    _, body, dlen, k = _entries(name, n_ext, lit_bytes)
    want = POOL + (K["POOL_SLOT"] if over else 0)
    return Shape(name, body, dlen, {"tile %d: pool_need == %d" % (k, want): lambda c: c.pool_need[k] == want,
                                    "no more entries than role S prefetches": lambda c: c.ext_entries[k] <= PREFETCHED})


def _sources_facts(k, dists, border_back):
    def lengths(c):
        return set(c.tile_entries(k)[1].tolist())

    def residues(c):
        return set((c.tile_entries(k)[0] % 8).tolist())

    def crossing(c):
        edge = (k - border_back) * TILE
        s, n = c.run_src[c.run_tile == k], c.run_len[c.run_tile == k]
        return bool(((s < edge) & (s + n > edge)).any())

    return {"tile %d reads tiles %s back" % (k, sorted(dists)): lambda c: c.src_back[k] >= set(dists),
            "entry lengths 1 .. 8": lambda c: lengths(c) == set(range(1, 9)),
            "source residues 0 .. 7 mod 8": lambda c: residues(c) == set(range(8)),
            "a source run over the border %d | %d tiles back" % (border_back + 1, border_back): crossing}


def sources_shape(name):
    """Tile 7 reads 1, 2, 3, 4 and 6 tiles back: the ring of the last two tiles, and dst below it.  One source run lies over the border
    between tiles 4 and 5 (the oldest tile in the ring), one ends within 12 bytes of the ring's wrap (the end of tile 5 = 2 x kRing)."""
    b = Build(_seed(name))
    k = 7
    b.plain(k)
    dists = (1, 2, 3, 4, 6)
    b.sources_tile(dists)
    b.copy_from((k - 2) * TILE - 5, 8)          # over the border of tiles k - 3 | k - 2
    b.lits1(1)
    b.copy_from((k - 2) * TILE - 3, 19)
    b.lits1(1)
    for back in (11, 9, 8, 5):                   # sources that end at or just before the ring's wrap
        b.copy_from((k - 1) * TILE - back, min(back, 8))
        b.lits1(1)
    body, dlen = b.close(10)
    facts = _sources_facts(k, dists, 2)
    wrap = (k - 1) * TILE
    assert wrap % RING == 0
    facts["a source in the ring within 12 bytes of its wrap"] = lambda c: bool(((c.tile_entries(k)[0] >= wrap - 11) & (c.tile_entries(k)[0] < wrap)).any())
    return Shape(name, body, dlen, facts)


def max_offsets_shape(name):
    """The largest and smallest offsets of copy3 and copy2, each at the first position where it is valid or in the last tile."""
    b = Build(_seed(name))
    n_tiles = MAX_OFFSET // TILE + 2             # 67 tiles: the last one starts beyond the largest offset
    b.plain(n_tiles - 2)
    b.lit(16)
    b.copy(TILE, 64)
    b.copy(80, MAX_OFFSET - b.pos)
    assert b.pos == MAX_OFFSET and b.tile() == n_tiles - 2
    b.raw(_copy3(MAX_OFFSET, 40), 40)            # the first position where it is valid: it reads the block's first byte
    b.lits1(1)
    b.raw(_copy3(MAX_OFFSET - 1, 64), 64)
    b.lits1(1)
    b.raw(_copy3(65600, 9), 9)
    b.lits1(1)
    b.raw(_copy3(65599, 11), 11)                 # an offset copy2 has as well
    b.lits1(1)
    b.raw(_copy2(64, 64), 64)
    b.lits1(1)
    b.raw(_copy2(65599, 5), 5)
    body, dlen = b.close(n_tiles)

    def has(kind, off):
        return lambda c: any(kk == kind and int(o) == off for kk, o, n in zip(c.tok["kind"], c.tok["off"], c.tok["cp"]) if n)

    facts = {"copy3 at %d" % o: has("copy3", o) for o in (MAX_OFFSET, MAX_OFFSET - 1, 65600, 65599)}
    facts.update({"copy2 at %d" % o: has("copy2", o) for o in (64, 65599)})
    facts["the largest offset reads the block's first byte"] = lambda c: bool(((c.tok["off"] == MAX_OFFSET) & (c.tok["dpos"] == MAX_OFFSET) & (c.tok["cp"] > 0)).any())
    facts["max_offset is the format's largest"] = lambda c: c.max_offset == MAX_OFFSET
    facts["about 2.2 MiB"] = lambda c: c.n_tiles * TILE < 2.3 * (1 << 20)
    return Shape(name, body, dlen, facts)


def chains_shape(name):
    """Tile 3: one literal byte, then 1-byte repeats at offset 1 to the tile's end (a chain through every byte, ending in the literal).
    Tile 4: a 4-byte copy of the previous tile, then 4100 copies of 4 bytes at offset 4, each reading the previous copy's output (ending in
    the external entry).  Tile 5: overlapping copies with periods 1 .. 9 and 63 .. 65."""
    b = Build(_seed(name))
    b.plain(3)
    b.lit(1)
    b.copy(1, 4)
    b.repeats1(TILE - 5)
    assert b.pos == 4 * TILE
    b.copy(TILE, 4)
    b.raw(O.emit_copy(4, 4) * 4100, 4 * 4100)
    b.end_tile()
    periods = list(range(1, 10)) + [63, 64, 65]
    for p in periods:
        b.lit(p)
        b.copy(p, 700 + p)
    body, dlen = b.close(8)

    def overlapping(c):
        tk = c.tok
        got = set(int(o) for o, n, d in zip(tk["off"], tk["cp"], tk["dpos"]) if n > o and d // TILE == 5)
        return got >= set(periods)

    facts = {"tile 3: chain_depth >= 2^14": lambda c: c.chain_depth[3] >= 1 << 14,
             "tile 3: the deepest chain is the whole tile and ends in a literal": lambda c: c.chain_depth[3] == TILE - 1 and c.chain_end[3] == "lit",
             "tile 4: >= 4000 tokens, each reading the one before": lambda c: c.tokens[4] >= 4000 and c.chain_depth[4] >= 4000,
             "tile 4: the deepest chain ends in an external entry": lambda c: c.chain_end[4] == "ext",
             "tile 5: overlapping copies with periods 1 .. 9 and 63 .. 65": overlapping}
    return Shape(name, body, dlen, facts)


def _straddler_tokens(b):
    """kind -> a function that writes one token of that kind at the builder's position."""
    return {"lit1": lambda: b.lit(100), "lit2": lambda: b.lit(1000), "lit3": lambda: b.lit(65600),
            "copy1": lambda: b.copy(100, 12), "copy2": lambda: b.copy(5000, 40), "copy3": lambda: b.copy(70000, 40),
            "copy2_lits": lambda: b.copy_lits(False, 3, 5000, 8), "copy3_lits": lambda: b.copy_lits(True, 2, 70000, 30),
            "repeat": lambda: b.repeat(300)}


def straddlers_shape(name):
    """Every token form over a tile border (its output) and over a segment border (its header bytes); segment entries at kExitKeep - 1,
    kExitKeep and kExitKeep + 1; a repeat as the first token of a tile, of a segment and of a 64-token round."""
    b = Build(_seed(name))
    b.plain(6)
    emit = _straddler_tokens(b)
    for kind in KINDS:
        b.pad_out_to((b.tile() + 1) * TILE - 2)
        emit[kind]()
        b.pad_stream_to(b.next_stream_mark(SEG - 1))
        emit[kind]()
    for x in (EXIT_KEEP - 1, EXIT_KEEP, EXIT_KEEP + 1):   # a literal over a segment border whose end is the segment's first token start
        tok = O.emit_literal(b.noise(300))
        assert x < len(tok)
        b.pad_stream_to(b.next_stream_mark(x - len(tok), room=4))
        b.raw(tok, 300)
        b.lits1(1)
    # repeats: the offset in force comes from the tile / segment / round before
    b.pad_out_to((b.tile() + 1) * TILE + 10)
    b.copy(5000, 8)
    b.pad_out_to((b.tile() + 1) * TILE)
    b.repeat(5)
    b.pad_stream_to(b.next_stream_mark(100))
    b.copy(5000, 8)
    b.pad_stream_to(b.next_stream_mark(0))
    b.repeat(5)
    b.copy(5000, 8)
    ntok = sum(1 for _ in TL.walk_tokens(b"".join(b.parts)))
    b.lits1(-ntok % ROUND)
    b.repeat(5)
    b.lits1(3)
    body, dlen = b.close()

    def out_crosses(kind):
        def f(c):
            tk = c.tok
            end = tk["dpos"] + tk["lit"] + tk["cp"]
            hit = (tk["dpos"] // TILE) != ((end - 1) // TILE)
            return any(h and kk == kind for h, kk in zip(hit, tk["kind"]))
        return f

    def hdr_crosses(kind):
        def f(c):
            tk = c.tok
            hit = (tk["spos"] // SEG) != ((tk["spos"] + tk["hlen"] - 1) // SEG)
            return any(h and kk == kind for h, kk in zip(hit, tk["kind"]))
        return f

    def repeat_first(of):
        def f(c):
            tk = c.tok
            sets = np.array([kk.startswith("copy") for kk in tk["kind"]])
            for i in np.nonzero(np.array([kk == "repeat" for kk in tk["kind"]]))[0]:
                before = np.nonzero(sets[:i])[0]
                if not before.size:
                    continue
                j = before[-1]
                if of == "tile" and tk["dpos"][i] % TILE == 0 and (tk["dpos"][j] + tk["lit"][j]) // TILE == tk["dpos"][i] // TILE - 1:
                    return True
                if of == "segment" and tk["spos"][i] % SEG == 0 and tk["spos"][j] // SEG == tk["spos"][i] // SEG - 1:
                    return True
                if of == "round" and i % ROUND == 0 and j // ROUND == i // ROUND - 1:
                    return True
            return False
        return f

    facts = {}
    for kind in KINDS:
        facts["%s: output over a tile border" % kind] = out_crosses(kind)
        facts["%s: header over a segment border" % kind] = hdr_crosses(kind)
    for x in (EXIT_KEEP - 1, EXIT_KEEP, EXIT_KEEP + 1):
        facts["a segment entered at offset %d" % x] = (lambda x: lambda c: x in set(c.seg_entry.tolist()))(x)
    for of in ("tile", "segment", "round"):
        facts["a repeat first in a %s, offset from the one before" % of] = repeat_first(of)
    return Shape(name, body, dlen, facts)


def _longest_run(mask):
    best = cur = 0
    for m in mask:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return best


def no_token_segments_shape(name):
    """Literal runs of 1.5 to 3 segments of token-like bytes with one short copy between them; no token start falls into the first kExitKeep
    bytes of a segment."""
    b = Build(_seed(name))
    b.plain(6)
    runs = []
    for _ in range(14):
        n = int(b.rng.integers(3 * SEG // 2, 3 * SEG - 8))
        tok_len = len(O.emit_literal(bytes(n)))
        r = (b.body_len + tok_len) % SEG
        if r < EXIT_KEEP + 8 or r > SEG - 16:     # the copy behind the run, or the next run, would start among the kept exits: a longer or shorter run
            n += 2 * EXIT_KEEP if n + 2 * EXIT_KEEP <= 3 * SEG - 8 else -2 * EXIT_KEEP
        b.lit(n, TAGGY[b.rng.integers(0, len(TAGGY), n)])
        runs.append(n)
        b.copy(int(b.rng.integers(1, 60000)), int(b.rng.integers(4, 60)))
    body, dlen = b.close()
    facts = {"literal runs of 1.5 to 3 segments": lambda c: all(3 * SEG // 2 <= n <= 3 * SEG for n in runs) and
             sorted(int(x) for x in c.tok["lit"] if x >= 3 * SEG // 2) == sorted(runs),
             ">= 8 consecutive segments entered at or beyond kExitKeep": lambda c: _longest_run(c.seg_entry >= EXIT_KEEP) >= 8,
             ">= 2 segments without a token start": lambda c: int((c.seg_starts == 0).sum()) >= 2}
    return Shape(name, body, dlen, facts)


def dense_after_sparse_shape(name):
    """An entries_3073 tile (tile 3), a literal of two segments, then three segments' worth of 1-byte repeats (a token per stream byte)."""
    b = Build(_seed(name))
    b.plain(3)
    b.entries_tile(PREFETCHED + 1, 1000)
    b.plain(5)
    b.lit(2 * SEG, TAGGY[b.rng.integers(0, len(TAGGY), 2 * SEG)])
    b.copy(3, 5)
    b.repeats1(3 * SEG)
    body, dlen = b.close(8)

    def dense(c):
        tk = c.tok
        for s in np.nonzero(c.seg_starts > IDX_STAGE)[0]:
            sel = (tk["spos"] >> TL.SEG_LOG) == s
            if (tk["dpos"][sel] // TILE).min() >= 3:
                return True
        return False

    return Shape(name, body, dlen, {"a segment with more than kIdxStage token starts, in tile >= 3": dense,
                                    "tile 3 has %d entries" % (PREFETCHED + 1): lambda c: c.ext_entries[3] == PREFETCHED + 1})


def tiles_shape(name, n_tiles):
    """Exactly n_tiles tiles: noise, then every tile 16 bytes of its own, 64 of the previous tile and their repetition (role S takes the
    ready flags 64 tiles at a time: 65 and 129 tiles need a second and a third batch of one tile)."""
    b = Build(_seed(name))
    b.plain(n_tiles)
    body, dlen = b.close(n_tiles)
    assert n_tiles % K["FLAG_BATCH"] == 1
    return Shape(name, body, dlen, {"exactly %d tiles" % n_tiles: lambda c: c.n_tiles == n_tiles and dlen == n_tiles * TILE,
                                    "every tile reads the one before": lambda c: all(c.src_back[t] == {1} for t in range(1, n_tiles))})


def team_shape(name, gap, shift):
    """sources_ring_and_dst and entries_3073 with no source nearer than `gap` tiles; one source ends `shift` bytes beyond the last byte of
    the tile `gap` back (0: on it; 1: the next smaller team)."""
    b = Build(_seed(name.replace("_sibling", "")), gap)
    k = gap + 3
    b.plain(k)
    b.entries_tile(PREFETCHED + 1, 1000)
    k2 = k + 1
    dists = (2, 3, 4, 5) if gap == 2 else (4, 5, 6)
    b.sources_tile(dists)
    b.copy_from((k2 - dists[1]) * TILE - 5, 8)               # a source run over a tile border, `gap` + 1 | `gap` tiles back
    b.lits1(1)
    b.copy_from((k2 - gap + 1) * TILE - 64 + shift, 64)      # ends on the last allowed byte, or one beyond
    b.lits1(1)
    body, dlen = b.close(k2 + gap + 4)
    team = TL.team_of_distance(gap if shift == 0 else gap - 1, False)
    facts = _sources_facts(k2, dists, dists[1])
    facts["tile %d has %d entries" % (k, PREFETCHED + 1)] = lambda c: c.ext_entries[k] == PREFETCHED + 1
    facts["team %d" % team] = lambda c: c.verdict.team == team
    nearest = gap if shift == 0 else gap - 1
    facts["the nearest source is %d tiles back" % nearest] = lambda c: min(min(s) for s in c.src_back if s) == nearest
    last = (k2 - gap + 1) * TILE
    facts["a source ends %d bytes beyond the tile %d back" % (shift, gap)] = lambda c: bool(((c.run_tile == k2) & (c.run_src + c.run_len == last + shift)).any())
    return Shape(name, body, dlen, facts)


def fuzz_shape(name):
    """Random tokens of every form over 2.3 MiB (72 tiles) behind the plain tiles: offsets drawn up to the whole distance back, so
    far beyond what a block of a few tiles allows, and up to the format's largest."""
    b = Build(_seed(name))
    rng = b.rng
    b.plain(6)
    lits = [1, 2, 3, 5, 17, 29, 30, 31, 70, 300, 5000]
    lens = [4, 5, 8, 11, 12, 18, 19, 33, 64, 65, 300, 3000]
    lens_p = [.12, .10, .12, .08, .08, .08, .06, .10, .08, .06, .08, .04]
    while b.pos < 72 * TILE - 6000:
        kind = int(rng.integers(0, 10))
        if kind < 3:
            b.lit(int(rng.choice(lits)))
        elif kind == 3:
            b.repeat(int(rng.choice([1, 2, 3, 4, 9, 70, 3000])))
        else:
            n = int(rng.choice(lens, p=lens_p))
            hi = [1024, 65599, MAX_OFFSET, 64, MAX_OFFSET][int(rng.integers(0, 5))]
            off = int(rng.integers(1, min(hi, b.pos) + 1))
            fused = rng.random() < 0.3
            if fused and 64 <= off <= 65599:
                b.copy_lits(False, int(rng.integers(1, 5)), off, min(n, 11))
            elif fused and off >= 65536:
                b.copy_lits(True, int(rng.integers(1, 4)), off, min(n, 64))
            else:
                b.copy(off, n)
    body, dlen = b.close(72)
    facts = {"offsets up to the format's largest region": lambda c: c.max_offset > 2_000_000,
             ">= 300 copies from more than 370 000 bytes back": lambda c: int(((c.tok["off"] > 370_000) & (c.tok["cp"] > 0)).sum()) >= 300,
             "more tiles than one batch of ready flags": lambda c: c.n_tiles > K["FLAG_BATCH"],
             "every token form": lambda c: set(c.tok["kind"]) >= set(KINDS) - {"lit3"}}
    return Shape(name, body, dlen, facts)


_MAKERS = {
    "entries_3072": lambda n: entries_shape(n, PREFETCHED),
    "entries_3073": lambda n: entries_shape(n, PREFETCHED + 1),
    "entries_4096": lambda n: entries_shape(n, TILE // EXT_MAX),
    "entries_4097": lambda n: entries_shape(n, TILE // EXT_MAX + 1),
    "pool_full": lambda n: pool_shape(n, False),
    "pool_full_plus_1": lambda n: pool_shape(n, True),
    "sources_ring_and_dst": sources_shape,
    "max_offsets": max_offsets_shape,
    "chains": chains_shape,
    "straddlers": straddlers_shape,
    "no_token_segments": no_token_segments_shape,
    "dense_after_sparse": dense_after_sparse_shape,
    "tiles_65": lambda n: tiles_shape(n, K["FLAG_BATCH"] + 1),
    "tiles_129": lambda n: tiles_shape(n, 2 * K["FLAG_BATCH"] + 1),
    "team2": lambda n: team_shape(n, 2, 0),
    "team2_sibling": lambda n: team_shape(n, 2, 1),
    "team4": lambda n: team_shape(n, 4, 0),
    "team4_sibling": lambda n: team_shape(n, 4, 1),
    "fuzz_far_0": fuzz_shape,
    "fuzz_far_1": fuzz_shape,
    "fuzz_far_2": fuzz_shape,
}
NAMES = tuple(_MAKERS)
_SHAPES, _EXPECTED, _CENSUS = {}, {}, {}


def shape(name):
    if name not in _SHAPES:
        _SHAPES[name] = _MAKERS[name](name)
    return _SHAPES[name]


def expected(name):
    """(code, bytes) of the oracle's decoder for the shape."""
    if name not in _EXPECTED:
        s = shape(name)
        _EXPECTED[name] = O.decode_body(s.body, s.dlen)
    return _EXPECTED[name]


def census_of(name):
    if name not in _CENSUS:
        s = shape(name)
        _CENSUS[name] = census(s.body, s.dlen)
    return _CENSUS[name]


def block(name):
    """The shape behind a block header."""
    s = shape(name)
    return TL.encode_block(s.body, s.dlen)
