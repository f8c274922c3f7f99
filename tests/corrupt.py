"""Format-aware mutations of MinLZ blocks and streams, each with the verdict it is meant to have.

A block mutant is Mutant(name, family, block, claim, keeps_len, ...): `claim` is 0 (a valid block) or the error code the oracle must give
(O.ERR_*).  A valid mutant also says which bytes it decodes to and which tile-level Verdict it has (expected_bytes / expected_verdict),
computed from its token list with tests/tile_levels.py's apply() and verdict(), not from the oracle: tests/test_corrupt.py checks every
claim against O.decode.  keeps_len: the header's dlen equals the sum of the token lengths, so only a check deeper than the total can catch
a corrupt one.

Families (each has valid and corrupt members):
- retarget: a copy gets a new offset (same tile, previous tile, over a tile boundary, a tile the block's pattern forbids, byte 0), valid;
  off = dc + 1 / dc + large, corrupt.
- shift_len: a copy k bytes longer and a later literal k bytes shorter, valid; the last copy k bytes longer, corrupt.
- lit_past_end: the final literal one byte longer with the byte and the header's dlen added, valid; without them, corrupt.
- repeat: a repeat first in the block (offset 1 at dc 0), corrupt; a repeat on a tile boundary, valid.
- cut_append: cut at a token boundary / inside a token, a whole token or 1-3 garbage bytes appended; valid when dlen is fixed with them.
- header: dlen +- 1, dlen > 8 MiB, dlen below the body, stored blocks with a wrong uvarint; a non-minimal uvarint, valid.
- random: bit flips and 4-byte bursts (their claim is the restatement's: walk() and apply() decide).

Streams: stream_mutants(stream) gives (name, bytes) pairs; their verdict is the oracle's (O.stream_decode), asked for by the tests.
Deterministic: every choice comes from a seeded generator.
"""
import bisect
from collections import namedtuple

import numpy as np

import oracle as O
from tests import tile_levels as TL

MAX_OFFSET = (2 << 20) + 65535      # the largest copy3 offset (the format's field)
FAMILIES = ("retarget", "shift_len", "lit_past_end", "repeat", "cut_append", "header", "random")


class Mutant(namedtuple("Mutant", "name family block claim keeps_len ops dlen base_verdict")):
    """ops: the token list of a valid mutant as (dpos, lit, off, cp) (None for a stored block); base_verdict: the source block's."""

    def expected_bytes(self):
        if self.ops is None:
            return _stored_bytes(self.block)
        return TL.apply(self.ops, self.dlen)

    def expected_verdict(self):
        if self.ops is None:
            return TL.make_verdict(TL.ORDER, None, False)
        return TL.verdict(self.ops, self.dlen)


def uvarint_bytes(v, pad=0):
    """uvarint of v; pad > 0 adds that many redundant continuation bytes (a non-minimal encoding binary.Uvarint accepts)."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def _uvarint(b, pos):
    x = s = 0
    for i in range(pos, min(len(b), pos + 10)):
        c = b[i]
        if c < 0x80:
            return x | (c << s), i - pos + 1
        x |= (c & 0x7F) << s
        s += 7
    return None, 0


def _stored_bytes(block):
    _, h = _uvarint(block, 1)
    return bytes(block[1 + h:])


def restate(block):
    """(claim, ops, dlen) of a block per the format (isMinLZ, then the walk): claim 0 with the token list, or an error code."""
    b = bytes(block)
    if len(b) == 1 and b[0] == 0:
        return 0, [], 0
    if not b or b[0] != 0:
        return O.ERR_CORRUPT if not b else O.ERR_UNSUPPORTED, None, 0
    v, h = _uvarint(b, 1)
    if v is None or v > 0xFFFFFFFF:
        return O.ERR_CORRUPT, None, 0
    if v > O.MAX_BLOCK_SIZE:
        return O.ERR_TOO_LARGE, None, 0
    body = b[1 + h:]
    if not body:
        return O.ERR_CORRUPT, None, 0
    if v == 0:
        return 0, None, len(body)
    if v < len(body):
        return O.ERR_CORRUPT, None, 0
    try:
        ops = list(TL.walk(body, v))
        TL.apply(ops, v)
    except ValueError:
        return O.ERR_CORRUPT, None, 0
    return 0, ops, v


class Source:
    """An encoded block parsed once: its header, body, tokens (TL.walk_tokens) and ops."""

    def __init__(self, name, block):
        self.name, self.block = name, bytes(block)
        body, dlen = TL.block_body(self.block)
        self.stored = body is None
        self.dlen = dlen
        self.body = body if body is not None else self.block[-dlen:] if dlen else b""
        self.toks = [] if self.stored else list(TL.walk_tokens(body))
        self.ops = [(t.dpos, t.lit, t.off, t.cp) for t in self.toks]
        self.verdict = TL.make_verdict(TL.ORDER, None, False) if self.stored else TL.verdict(self.ops, dlen)

    def tok_end(self, i):
        return self.toks[i + 1].spos if i + 1 < len(self.toks) else len(self.body)


def _emit(lit, off, cp):
    """Token bytes for literals followed by a copy (either may be empty) — the oracle's emitters."""
    out = O.emit_literal(lit) if lit else b""
    return out + (O.emit_copy(off, cp) if cp else b"")


class _Gen:
    def __init__(self, src, seed, per_kind):
        self.s, self.rng, self.per = src, np.random.default_rng(seed), per_kind
        self.out = []

    def add(self, tag, family, block, claim, keeps_len, ops=None, dlen=None):
        self.out.append(Mutant("%s/%s/%s" % (self.s.name, family, tag), family, bytes(block), claim, keeps_len, ops, dlen, self.s.verdict))

    def block(self, body, dlen=None):
        return b"\x00" + uvarint_bytes(self.s.dlen if dlen is None else dlen) + bytes(body)

    def splice(self, i, j, items, dshift=0):
        """Tokens [i, j) replaced by items: (lit, off | None, cp) tuples (off None: literals and a repeat at the offset in force) or
        source Tokens kept as they are; -> (body, ops).  Later tokens move by dshift output bytes; repeats right after the splice take
        the offset then in force."""
        s = self.s
        new_bytes, new_ops = [], []
        d = s.toks[i].dpos if i < len(s.toks) else s.dlen
        off = s.toks[i - 1].off if i else 1          # the offset in force in front of token i
        for it in items:
            if isinstance(it, TL.Token):
                new_bytes.append(s.body[it.spos:s.tok_end(s.toks.index(it, i, j))])
                if it.form not in ("literal", "repeat"):
                    off = it.off
                new_ops.append((d, it.lit, off, it.cp))
                d += len(it.lit) + it.cp
                continue
            lit, o, cp = it
            if o is None:
                new_bytes.append((O.emit_literal(lit) if lit else b"") + (O.emit_repeat(cp) if cp else b""))
            else:
                new_bytes.append(_emit(lit, o, cp))
                off = o if cp else off
            new_ops.append((d, lit, off, cp))
            d += len(lit) + cp
        after = []
        carry = True
        for t in s.toks[j:]:
            if t.form not in ("literal", "repeat"):
                carry = False
            if not carry and not dshift:
                break
            after.append((t.dpos + dshift, t.lit, off if carry else t.off, t.cp))
        k = j + len(after)
        start = s.toks[i].spos if i < len(s.toks) else len(s.body)
        body = s.body[:start] + b"".join(new_bytes) + s.body[s.tok_end(j - 1) if j else 0:]
        return body, s.ops[:i] + new_ops + after + s.ops[k:]

    def pick(self, idx, n):
        idx = list(idx)
        if len(idx) <= n:
            return idx
        return sorted(self.rng.choice(idx, n, replace=False).tolist())

    # -- families --
    def retarget(self):
        s, T = self.s, TL.TILE
        copies = [i for i, t in enumerate(s.toks) if t.form not in ("literal", "repeat")]
        for i in self.pick(copies, self.per):
            t = s.toks[i]
            dc = t.dpos + len(t.lit)
            k = dc // T
            cand = {"byte0": dc}
            if dc > k * T:
                cand["same_tile"] = dc - k * T
            if k >= 1 and T > t.cp:
                cand["prev_tile"] = dc - ((k - 1) * T + int(self.rng.integers(0, T - t.cp)))
                b = k * T if dc >= k * T + t.cp else (k - 1) * T if k >= 2 else None
                if b is not None and t.cp >= 2:
                    cand["straddle"] = dc - (b - t.cp // 2)
            p = s.verdict.pattern or "three"
            hi = [q for q in range(max(0, k - 15), k) if TL.level(p, q) >= TL.level(p, k)]
            if hi:
                q = hi[int(self.rng.integers(0, len(hi)))]
                cand["forbidden_tile"] = dc - (q * T + int(self.rng.integers(0, max(1, min(T, dc - q * T) - t.cp))))
            for tag, off in sorted(cand.items()):
                if 1 <= off <= min(dc, MAX_OFFSET) and off != t.off:
                    body, ops = self.splice(i, i + 1, [(t.lit, off, t.cp)])
                    if len(body) <= s.dlen:
                        self.add("%s@%d" % (tag, i), "retarget", self.block(body), 0, True, ops, s.dlen)
            for tag, off in (("before_start_1", dc + 1), ("before_start_large", min(dc + 100000, MAX_OFFSET))):
                if dc < off <= MAX_OFFSET:
                    body, _ = self.splice(i, i + 1, [(t.lit, off, t.cp)])
                    if len(body) <= s.dlen:
                        self.add("%s@%d" % (tag, i), "retarget", self.block(body), O.ERR_CORRUPT, True)

    def shift_len(self):
        s = self.s
        lits = [j for j, t in enumerate(s.toks) if t.form == "literal" and len(t.lit) >= 2]
        copies = [i for i, t in enumerate(s.toks) if t.form not in ("literal", "repeat")]
        pairs = []
        for i in copies:
            q = bisect.bisect_right(lits, i + 1)
            if q < len(lits) and s.toks[lits[q]].dpos - s.toks[i].dpos < 1 << 16:
                pairs.append((i, lits[q]))
        for q in self.pick(range(len(pairs)), self.per):
            i, j = pairs[q]
            ti, tj = s.toks[i], s.toks[j]
            kk = int(self.rng.integers(1, min(9, len(tj.lit))))
            items = [(ti.lit, ti.off, ti.cp + kk)] + s.toks[i + 1:j] + [(tj.lit[:-kk], None, 0)]
            body, ops = self.splice(i, j + 1, items)
            self.add("k%d@%d_%d" % (kk, i, j), "shift_len", self.block(body), 0, True, ops, s.dlen)
        if copies:
            i = copies[-1]
            t = s.toks[i]
            body, _ = self.splice(i, i + 1, [(t.lit, t.off, t.cp + 3)], dshift=3)
            self.add("last_copy_past_dlen@%d" % i, "shift_len", self.block(body), O.ERR_CORRUPT, False)

    def lit_past_end(self):
        s = self.s
        if not s.toks or s.toks[-1].form != "literal":
            return
        t = s.toks[-1]
        hdr = O.emit_literal(t.lit + b"\x00")[:-(len(t.lit) + 1)]
        head = s.body[:t.spos] + hdr + t.lit
        self.add("final_literal_plus_1", "lit_past_end", self.block(head), O.ERR_CORRUPT, False)
        ops = s.ops[:-1] + [(t.dpos, t.lit + b"\x5a", t.off, 0)]
        self.add("final_literal_plus_1_with_byte", "lit_past_end", self.block(head + b"\x5a", s.dlen + 1), 0, True, ops, s.dlen + 1)

    def repeat(self):
        s, T = self.s, TL.TILE
        if s.toks and s.toks[0].form == "literal" and len(s.toks[0].lit) > 4:
            t = s.toks[0]
            body, _ = self.splice(0, 1, [(b"", None, 4), (t.lit[4:], None, 0)])
            self.add("first_in_block", "repeat", self.block(body), O.ERR_CORRUPT, True)
        spans = [j for j, t in enumerate(s.toks) if t.form == "literal" and t.dpos // T != (t.dpos + len(t.lit) - 1) // T]
        longs = [j for j, t in enumerate(s.toks) if t.form == "literal" and len(t.lit) >= 6 and j]
        for tag, j in [("after_tile_boundary", j) for j in self.pick(spans, max(1, self.per // 2))] + \
                      [("inside_literal", j) for j in self.pick(longs, max(1, self.per // 2))]:
            t = s.toks[j]
            cut = (t.dpos + len(t.lit) - 1) // T * T - t.dpos if tag == "after_tile_boundary" else 1
            m = min(4, len(t.lit) - cut)
            items = [(t.lit[:cut], None, 0), (b"", None, m)] + ([(t.lit[cut + m:], None, 0)] if cut + m < len(t.lit) else [])
            body, ops = self.splice(j, j + 1, items)
            if len(body) <= s.dlen:
                self.add("%s@%d" % (tag, j), "repeat", self.block(body), 0, True, ops, s.dlen)

    def cut_append(self):
        s = self.s
        n = len(s.toks)
        if n >= 3:
            for i in self.pick(range(1, n), 2):
                t = s.toks[i]
                self.add("cut_at_token@%d" % i, "cut_append", self.block(s.body[:t.spos]), O.ERR_CORRUPT, False)
                if t.spos <= t.dpos:
                    self.add("cut_at_token_fixed@%d" % i, "cut_append", self.block(s.body[:t.spos], t.dpos), 0, True, s.ops[:i], t.dpos)
                if s.tok_end(i) - t.spos >= 2:
                    self.add("cut_inside_token@%d" % i, "cut_append", self.block(s.body[:t.spos + 1]), O.ERR_CORRUPT, False)
        if not s.stored:
            extra = bytes([0x33, 0x44])
            self.add("append_token", "cut_append", self.block(s.body + O.emit_literal(extra)), O.ERR_CORRUPT, False)
            ops = s.ops + [(s.dlen, extra, s.ops[-1][2] if s.ops else 1, 0)]
            self.add("append_token_fixed", "cut_append", self.block(s.body + O.emit_literal(extra), s.dlen + 2), 0, True, ops, s.dlen + 2)
            for g in (1, 2, 3):
                garbage = bytes(self.rng.integers(0, 256, g, dtype=np.uint8))
                c, ops, dl = restate(self.block(s.body + garbage))
                self.add("append_garbage_%d" % g, "cut_append", self.block(s.body + garbage), c, False, ops, dl)

    def header(self):
        s = self.s
        body = s.body
        if s.stored:
            raw = body
            self.add("stored_nonminimal_zero", "header", b"\x00" + uvarint_bytes(0, 1) + raw, 0, False, None, len(raw))
            for tag, v in (("stored_v1", 1), ("stored_v_len", len(raw)), ("stored_v_len_plus_1", len(raw) + 1), ("stored_v_too_large", O.MAX_BLOCK_SIZE + 1)):
                blk = b"\x00" + uvarint_bytes(v) + raw
                c, ops, dl = restate(blk)
                self.add(tag, "header", blk, c, False, ops, dl)
            return
        self.add("dlen_plus_1", "header", self.block(body, s.dlen + 1), O.ERR_CORRUPT, False)
        self.add("dlen_minus_1", "header", self.block(body, s.dlen - 1), O.ERR_CORRUPT, False)
        self.add("dlen_too_large", "header", self.block(body, O.MAX_BLOCK_SIZE + 1), O.ERR_TOO_LARGE, False)
        self.add("dlen_below_body", "header", self.block(body, len(body) - 1), O.ERR_CORRUPT, False)
        for pad in (1, 3):
            self.add("dlen_nonminimal_%d" % pad, "header", b"\x00" + uvarint_bytes(s.dlen, pad) + body, 0, True, s.ops, s.dlen)

    def random(self):
        s = self.s
        blk = bytearray(self.block(s.body))
        h = len(blk) - len(s.body)
        for r in range(max(2, self.per // 2)):
            m = bytearray(blk)
            if r % 2 == 0:
                p = int(self.rng.integers(h, len(m)))
                m[p] ^= 1 << int(self.rng.integers(0, 8))
                tag = "flip@%d" % p
            else:
                p = int(self.rng.integers(h, max(h + 1, len(m) - 4)))
                m[p:p + 4] = bytes(self.rng.integers(0, 256, 4, dtype=np.uint8))
                tag = "burst@%d" % p
            c, ops, dl = restate(m)
            self.add(tag, "random", m, c, False, ops, dl)


def block_mutants(name, block, seed, per_kind=3):
    """The mutants of one encoded block (the source itself not among them)."""
    g = _Gen(Source(name, block), seed, per_kind)
    if not g.s.stored:
        g.retarget()
        g.shift_len()
        g.lit_past_end()
        g.repeat()
        g.random()
    g.cut_append()
    g.header()
    return g.out


def _seed(name):
    return sum((i + 1) * c for i, c in enumerate(name.encode())) & 0xFFFFFF


def cpu_sources():
    """Oracle L1/L2/L3 blocks, stored blocks and a sample of the hand-built cases: (name, block)."""
    from minlz_amd import synth
    out = []
    for kind, gen, size in (("text", synth.text_like, 64 << 10), ("json", synth.json_like, (300 << 10) + 777)):
        src = np.ascontiguousarray(gen(size, seed=size & 0xFFFF)).tobytes()
        for level in (1, 2, 3):
            out.append(("oracle_%s_%d_L%d" % (kind, size, level), O.encode(src, level)))
    for size in (100, 64 << 10):
        raw = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8).tobytes()
        out.append(("stored_%d" % size, b"\x00\x00" + raw))
    named = {c.name: c for c in TL.cases("named")}
    for nm in ("fits_fast_only", "team_nearest_2_back", "repeat_carried_allowed"):
        c = named[nm]
        out.append(("case_" + nm, TL.encode_block(c.body, c.dlen)))
    return out


def mutants_of(sources, per_kind=3):
    out = []
    for name, block in sources:
        out += block_mutants(name, block, _seed(name), per_kind)
    return out


_CACHE = {}


def cpu_mutants():
    if "cpu" not in _CACHE:
        _CACHE["cpu"] = mutants_of(cpu_sources())
    return _CACHE["cpu"]


# ---------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------
Chunk = namedtuple("Chunk", "off type clen")   # off: the chunk header's offset in the stream


def chunks(stream):
    out, p = [], 0
    while p + 4 <= len(stream):
        t = stream[p]
        n = stream[p + 1] | stream[p + 2] << 8 | stream[p + 3] << 16
        out.append(Chunk(p, t, n))
        p += 4 + n
    return out


def _set_len(b, c, n):
    b[c.off + 1:c.off + 4] = n.to_bytes(3, "little")


def stream_mutants(stream, seed=1):
    """(name, bytes) for one valid stream of several data chunks: single faults in every framing field, and two-fault streams (an early
    chunk with a bad CRC or a bad body, then a later framing error, an oversized chunk or a cut)."""
    s = bytes(stream)
    cs = chunks(s)
    data = [c for c in cs if c.type in (0x01, 0x02, 0x03)]
    eof = [c for c in cs if c.type == 0x20][-1]
    rng = np.random.default_rng(seed)
    out = []

    def mut(name, f):
        b = bytearray(s)
        f(b)
        out.append((name, bytes(b)))

    first, last = data[0], data[-1]
    comp = next(c for c in data if c.type in (0x02, 0x03))
    for c, tag in ((first, "first"), (last, "last"), (comp, "comp")):
        mut("len_plus_1_" + tag, lambda b, c=c: _set_len(b, c, c.clen + 1))
        mut("len_minus_1_" + tag, lambda b, c=c: _set_len(b, c, c.clen - 1))
        mut("len_3_" + tag, lambda b, c=c: _set_len(b, c, 3))
        mut("len_huge_" + tag, lambda b, c=c: _set_len(b, c, 0xFFFFFF))
        for t in (0x00, 0x03, 0x05, 0x80, 0xFE):
            mut("type_%02x_%s" % (t, tag), lambda b, c=c, t=t: b.__setitem__(c.off, t))
        mut("crc_" + tag, lambda b, c=c: b.__setitem__(c.off + 5, b[c.off + 5] ^ 0x10))
    # the block uvarint of a compressed chunk: +-1, above the block size, non-minimal (the chunk grows a byte)
    v, h = _uvarint(s, comp.off + 8)
    for tag, nv in (("plus_1", v + 1), ("minus_1", v - 1), ("over_block", (1 << 23) + 1), ("zero", 0)):
        def f(b, nv=nv):
            enc = uvarint_bytes(nv)
            b[comp.off + 8:comp.off + 8 + h] = enc
            _set_len(b, comp, comp.clen - h + len(enc))
        mut("uvarint_" + tag, f)
    # EOF size
    ev, eh = _uvarint(s, eof.off + 4)
    for tag, nv in (("plus_1", ev + 1), ("minus_1", ev - 1)):
        def f(b, nv=nv):
            enc = uvarint_bytes(nv)
            b[eof.off + 4:eof.off + 4 + eh] = enc
            b[eof.off + 1] = len(enc)
        mut("eof_" + tag, f)
    mut("eof_len_11", lambda b: b.__setitem__(eof.off + 1, 11))
    mut("eof_empty", lambda b: b.__setitem__(slice(eof.off, len(b)), b"\x20\x00\x00\x00"))
    # padding / skippable chunks, valid and cut
    out.append(("pad_chunk", s + b"\xfe\x05\x00\x00" + bytes(5)))
    out.append(("pad_chunk_cut", s + b"\xfe\x05\x00\x00" + bytes(3)))
    out.append(("pad_3_bytes", s + bytes(3)))
    out.append(("reserved_skippable_before_eof", s[:eof.off] + b"\x80\x02\x00\x00ab" + s[eof.off:]))
    # truncation: at a chunk boundary, inside a header, inside a body, inside the EOF chunk
    for c in data[1:] + [eof]:
        out.append(("cut_at_%d" % c.off, s[:c.off]))
    for c in (first, last):
        out.append(("cut_in_header_%d" % c.off, s[:c.off + 2]))
        out.append(("cut_in_body_%d" % c.off, s[:c.off + 4 + c.clen // 2]))
    out.append(("cut_in_eof", s[:-1]))
    # a token byte of a compressed chunk's body
    for r in range(3):
        p = int(rng.integers(comp.off + 8 + h, comp.off + 4 + comp.clen))
        mut("body_%d" % p, lambda b, p=p: b.__setitem__(p, b[p] ^ 0xFF))
    # a stored chunk claiming more than a block, in a stream cut short: the size is checked before the bytes are read (ErrTooLarge)
    for c in [c for c in data if c.type == 0x01][:1]:
        b = bytearray(s[:c.off + 4 + 100])
        _set_len(b, c, (1 << 20) + 5)
        out.append(("uncompressed_too_large_cut", bytes(b)))
    # two faults: early chunk bad (CRC or body), later framing error / too large / cut
    body_p = first.off + 4 + first.clen // 2
    early = (("crc", lambda b: b.__setitem__(first.off + 5, b[first.off + 5] ^ 0x01)),
             ("body", lambda b: b.__setitem__(body_p, b[body_p] ^ 0xFF)))
    for etag, ef in early:
        late = (("cut_last", lambda b: b.__delitem__(slice(last.off + 4 + last.clen // 2, len(b)))),
                ("len_huge_last", lambda b: _set_len(b, last, 0xFFFFFF)),
                ("type_00_last", lambda b: b.__setitem__(last.off, 0x00)),
                ("eof_wrong", lambda b: b.__setitem__(eof.off + 4, b[eof.off + 4] ^ 0x01)),
                ("uncompressed_too_large_last", lambda b: (b.__setitem__(last.off, 0x01), _set_len(b, last, (1 << 20) + 5))))
        for ltag, lf in late:
            b = bytearray(s)
            lf(b)     # the later fault first: it may cut the stream, the early one is in front of it
            ef(b)
            out.append(("two_%s_then_%s" % (etag, ltag), bytes(b)))
    return out


def stream_verdict(stream, max_out):
    """(code, bytes) of the oracle's Reader."""
    try:
        return 0, O.stream_decode(stream, max_out)
    except O.OracleError as e:
        return e.code, None
