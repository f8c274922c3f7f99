"""The designed decoder inputs of tests/decode_shapes.py proved on the CPU: every shape is a valid general block whose bytes the oracle and
the restated token walk agree on, and every fact it claims about the decoder's capacities holds under the census.  The GPU tests
(tests/test_gpu_decode_shapes.py) then only have to compare bytes: what the inputs reach is shown here."""
import numpy as np
import pytest

import oracle as O
from tests import decode_shapes as DS
from tests import tile_levels as TL


def test_constants_are_the_kernels():
    # what the shapes are built around (read from the C sources; the values the kernels have today)
    assert (DS.TILE, DS.SEG, DS.EXIT_KEEP, DS.IDX_STAGE, DS.ROUND) == (32768, 8192, 256, 4096, 64)
    assert (DS.PREFETCHED, DS.EXT_MAX, DS.POOL, DS.RING) == (3072, 8, 32768, 3 * 32768)
    assert DS.pool_need(1, 1) == 40 and DS.pool_need(32, 0) == 32 and DS.pool_need(33, 2) == 80


def test_census_by_hand():
    T = DS.TILE
    rng = np.random.default_rng(1)
    # tile 0: 40 000 literal bytes run into tile 1; tile 1: a copy of 20 bytes from tile 0 (3 entries: 8, 8, 4), an overlapping copy at offset 3
    # reading it (in-tile), a copy over the border 1 | 2 from 100 back (in-tile on both sides), a copy of 9 bytes from tile 0 in tile 2
    body = O.emit_literal(rng.integers(0, 256, 40000, dtype=np.uint8)) + O.emit_copy(39000, 20) + O.emit_copy(3, 30) + \
        O.emit_literal(bytes(2 * T - 40050 - 10)) + O.emit_copy(100, 30) + O.emit_copy(2 * T, 9)
    dlen = 2 * T + 20 + 9
    assert O.decode_body(body, dlen)[0] == 0
    c = DS.census(body, dlen)
    assert c.n_tiles == 3 and c.tokens.tolist() == [1, 4, 1]
    assert c.lit_bytes.tolist() == [T, 40000 - T + 2 * T - 40050 - 10, 0]
    assert c.ext_entries.tolist() == [0, 3, 3 + 2]          # tile 2: the border copy's 20 bytes there read tile 1 (8 + 8 + 4), then 9 bytes (8 + 1)
    assert c.run_len.tolist() == [20, 20, 9] and c.run_src.tolist() == [1000, 2 * T - 100, 20]
    assert c.tile_entries(1)[1].tolist() == [8, 8, 4] and c.tile_entries(1)[0].tolist() == [1000, 1008, 1016]
    assert c.pool_need.tolist() == [T, DS.round_up(int(c.lit_bytes[1]), 32) + 24, 24 + 16]
    assert c.chain_depth.tolist() == [0, 10, 0]              # 30 bytes at offset 3: the last byte is ten hops from the external bytes
    assert c.chain_end[1] == "ext"
    assert c.src_back == [set(), {1}, {1, 2}]
    assert c.seg_starts.tolist()[:1] == [1] and c.seg_entry[0] == 0 and c.seg_entry[1] == DS.SEG and c.seg_starts[1] == 0
    assert c.max_offset == 2 * T


OVERFLOWS = ("entries_4097", "pool_full_plus_1")
UNPLANNED = ("straddlers", "no_token_segments", "fuzz_far_0", "fuzz_far_1", "fuzz_far_2")
BEYOND_PREFETCH = ("entries_3073", "entries_4096", "entries_4097", "dense_after_sparse", "team2", "team2_sibling", "team4", "team4_sibling")


@pytest.mark.parametrize("name", DS.NAMES)
def test_shape_is_what_it_claims(name):
    s = DS.shape(name)
    code, want = DS.expected(name)
    assert code == 0
    assert s.dlen <= 3 << 20 or name == "tiles_129"
    ops = list(TL.walk(s.body, s.dlen))
    assert TL.apply(ops, s.dlen) == want
    assert len(s.body) < s.dlen and O.decode(DS.block(name)) == want        # a valid block, not only a valid body
    c = DS.census_of(name)
    assert c.verdict == TL.verdict(ops, s.dlen) and c.verdict.general
    assert c.n_tiles >= 6 and c.lit_bytes[0] == DS.TILE and c.tokens[0] == (DS.TILE + 28) // 29    # noise in 29-byte literals, then >= 5 tiles
    # the slots overflow (the tile is redone packed) and role S's plain loop runs exactly where a shape is built for it, in one tile
    # (a tile that is nearly all literals overflows with a handful of entries: the literal-heavy shapes have such tiles as a by-product,
    #  and the random ones have what they happen to have)
    if name not in UNPLANNED:
        assert int((c.pool_need > DS.POOL).sum()) == (1 if name in OVERFLOWS else 0)
        assert int((c.ext_entries > DS.PREFETCHED).sum()) == (1 if name in BEYOND_PREFETCH else 0)
    failed = [k for k, holds in s.facts.items() if not holds(c)]
    assert not failed, failed
    assert s.facts


def test_shapes_cover_the_teams():
    teams = {n: DS.census_of(n).verdict.team for n in DS.NAMES}
    assert (teams["team2"], teams["team2_sibling"], teams["team4"], teams["team4_sibling"]) == (2, 1, 4, 2)
    assert all(t == 1 for n, t in teams.items() if not n.startswith("team"))


def test_a_moved_constant_is_noticed():
    # the facts are about the constants, not about today's numbers: the same census against another capacity fails them
    c = DS.census_of("entries_3073")
    s = DS.shape("entries_3073")
    assert all(f(c) for f in s.facts.values())
    old = DS.PREFETCHED
    DS.PREFETCHED = old + 1024
    try:
        assert not all(f(c) for f in s.facts.values())
    finally:
        DS.PREFETCHED = old
