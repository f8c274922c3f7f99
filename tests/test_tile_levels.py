"""The restatement of the decoder's tile-level classification (tests/tile_levels.py) pinned on the CPU: its token walker against the
oracle's decoder, and every hand-built case against its own claim (bytes the oracle agrees with, and the verdict the case means)."""
import numpy as np
import pytest

import oracle as O
from minlz_amd import synth
from tests import tile_levels as TL
from tests.util import load_zip


def _ops_bytes(enc):
    body, dlen = TL.block_body(enc)
    return TL.apply(TL.walk(body, dlen), dlen)


def test_pattern_words_are_the_documented_levels():
    # DESIGN.md "Tile levels" / mlz_encode.hip.inc: fast 0 1 2 3 ..., dense 0 1 2 3 1 2 3 2 3 1 2 3 2 3 2 3, three 0 1 1 2 1 2 2 2 1 2 2 2 1 2 2 2
    assert [TL.level("fast", t) for t in range(16)] == [0, 1, 2, 3] * 4
    assert [TL.level("dense", t) for t in range(16)] == [0, 1, 2, 3, 1, 2, 3, 2, 3, 1, 2, 3, 2, 3, 2, 3]
    assert [TL.level("three", t) for t in range(16)] == [0, 1, 1, 2, 1, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 2]
    assert TL.TILE == 32768 and all(TL.level(p, t) == TL.level(p, t + 16) for p in TL.ORDER for t in range(16))
    # the issue's examples: tile 7 reading tile 6 is legal only under fast; 6 <- 2 with 2 <- 1 only under dense
    assert [p for p in TL.ORDER if TL.may_read(p, 7, 6)] == ["fast"]
    assert [p for p in TL.ORDER if TL.may_read(p, 6, 2) and TL.may_read(p, 2, 1)] == ["dense"]


def test_rule_by_hand():
    T = TL.TILE
    v = TL.verdict([(5, b"", 1, 10)], 64)                                     # a run inside tile 0
    assert v == TL.Verdict(frozenset(TL.ORDER), "three", False, 0)
    v = TL.verdict([(7 * T, b"", 1, 100)], 32 * T)                            # window one byte into tile 6
    assert v.fits == {"fast"} and v.pattern == "fast"
    v = TL.verdict([(7 * T + 20, b"", 10, 100)], 32 * T)                      # window inside tile 7 only
    assert v.fits == frozenset(TL.ORDER)
    v = TL.verdict([(4 * T, b"", T, 100)], 32 * T)                            # 4 <- 3: no pattern, team 1
    assert v == TL.Verdict(frozenset(), None, True, 1)
    v = TL.verdict([(20 * T, b"", 16 * T, 100)], 32 * T)                      # 16 back only: team 4
    assert v == TL.Verdict(frozenset(), None, True, 4)
    v = TL.verdict([(20 * T, b"", 16 * T, 100), (23 * T, b"", 2 * T + 200, 100)], 32 * T)   # + 2 back: team 2
    assert v.team == 2
    v = TL.verdict([(20 * T, b"", 16 * T, 100), (26 * T - 10, b"", 6 * T, 100)], 32 * T)    # + a copy over 25 | 26: team 1
    assert v.team == 1


def test_walker_on_the_golden_block(twain, twain_mzb):
    assert _ops_bytes(twain_mzb) == twain == O.decode(twain_mzb)


@pytest.mark.parametrize("kind", ["text", "json", "random"])
@pytest.mark.parametrize("size", [(32 << 10) + 1, 64 << 10, 96 << 10, 1 << 20, 3 << 20])
def test_walker_on_oracle_blocks(kind, size):
    data = {"text": synth.text_like, "json": synth.json_like}.get(kind)
    src = data(size, seed=size & 0xFFFF) if data else np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
    src = np.ascontiguousarray(src).tobytes()
    for level in (0, 1, 2, 3):
        enc = O.encode(src, level)
        body, dlen = TL.block_body(enc)
        if body is None:                                   # stored block: no tokens
            assert level == 0 or kind == "random"
            continue
        e, ref = O.decode_body(body, dlen)
        assert e == 0 and ref == src
        assert TL.apply(TL.walk(body, dlen), dlen) == ref, (kind, size, level)


def test_walker_on_the_block_corpus():
    # fuzz/block-corpus-dec.zip: mostly corrupt blocks.  The walker must accept exactly the bodies the oracle accepts, with its bytes.
    ok = rejected = 0
    for name, enc in load_zip("block-corpus-dec.zip"):
        try:
            body, dlen = TL.block_body(enc)
        except (IndexError, AssertionError):
            continue                                       # not a MinLZ block header
        if body is None or dlen > O.MAX_BLOCK_SIZE:
            continue
        e, want = O.decode_body(body, dlen)
        try:
            got = TL.apply(TL.walk(body, dlen), dlen)
        except ValueError:
            got = None
        assert (got is None) == (e != 0), name
        if got is not None:
            assert got == want, name
            ok += 1
        else:
            rejected += 1
    assert ok + rejected >= 50


def test_walker_rejects_a_truncated_body():
    body = O.emit_literal(b"abcd") + O.emit_copy(4, 8)
    assert TL.apply(TL.walk(body, 12), 12) == b"abcdabcdabcd"
    with pytest.raises(ValueError):
        list(TL.walk(body[:-1], 12))


def _all_cases():
    return [("named", c.name) for c in TL.cases("named")] + [("big", c.name) for c in TL.cases("big")] + [("sweep", c.name) for c in TL.cases("sweep")]


@pytest.mark.parametrize("kind,name", _all_cases())
def test_built_case_is_what_it_claims(kind, name):
    c = next(c for c in TL.cases(kind) if c.name == name)
    assert O.decode_body(c.body, c.dlen) == (0, c.expected)
    assert len(c.body) < c.dlen and O.decode(TL.encode_block(c.body, c.dlen)) == c.expected   # a valid block, not only a valid body
    ops = list(TL.walk(c.body, c.dlen))
    assert TL.apply(ops, c.dlen) == c.expected
    assert TL.verdict(ops, c.dlen) == c.intended


def test_case_set_covers_the_issue():
    named = {c.name: c.intended for c in TL.cases("named")}
    # team sizes by nearest read: 1, 2, 3, 4, 5 tiles back and a copy over a tile boundary
    assert [named["team_nearest_%d_back" % d].team for d in (1, 2, 3, 4, 5)] + [named["team_crossing_copy"].team] == [1, 2, 2, 4, 4, 1]
    assert named["fits_fast_only"].fits == {"fast"} and named["fits_dense_only"].fits == {"dense"}
    assert named["fits_three_and_all"].fits == frozenset(TL.ORDER) and named["fits_none"].general
    picked = {v.pattern for v in named.values()}
    assert {"three", "dense", "fast", None} <= picked
    big = TL.cases("big")
    assert [c.dlen for c in big] == [8 << 20, 8 << 20] and [c.intended.general for c in big] == [False, True]
