"""The rule the encoder's table of kernel variants must keep: a block's bytes depend on the block, the level and the options alone — not
on what else is in its batch, and not on which launch of the group served it.  A group launches the match kernel once per block class
present (blocks of at least 1 MiB, smaller ones), with another instantiation per class, level and far-table setting, and LevelBalanced has
one more for groups whose blocks all fit a tile (mlz_hip.hip: the selection of the match launches).  The four batches below — everything,
the blocks of at most one tile, the small blocks of several tiles, the big blocks — reach every row of that selection at every leg, and
each block of each batch must come out as it does when it is encoded alone."""
import pytest

import minlz_amd as mz
import oracle as O
from minlz_amd import synth

pytestmark = pytest.mark.gpu

TILE, BIG = 32768, 1 << 20
# both classes, the class border and the tile border
SIZES = [0, 1, 20_000, TILE, 40_000, 65_536, 300_000, BIG - 1, BIG, BIG + 77]

# (level, option, value): the option is set for the leg and put back to its default, 1, afterwards
LEGS = [(mz.LevelSuperFast, None, None), (mz.LevelFastest, mz.OPT_ENCODE_FAR, 0), (mz.LevelFastest, mz.OPT_ENCODE_FAR, 1),
        (mz.LevelBalanced, mz.OPT_L2_FREE, 0), (mz.LevelBalanced, mz.OPT_L2_FREE, 1)]


@pytest.fixture(scope="module")
def blocks():
    # (the generators make at least one byte: the empty block is the empty string)
    return [(synth.json_like(n, seed=500 + i) if i & 1 else synth.text_like(n, seed=500 + i)).tobytes() if n else b"" for i, n in enumerate(SIZES)]


@pytest.mark.parametrize("level,opt,value", LEGS, ids=["superfast", "fastest-far0", "fastest-far1", "balanced-levels", "balanced-free"])
def test_a_block_is_encoded_the_same_in_any_batch(ctx, blocks, level, opt, value):
    assert [len(b) for b in blocks] == SIZES
    if opt is not None:
        ctx.set_option(opt, value)
    try:
        alone = [mz.Encode(b, level, ctx) for b in blocks]
        for b, e in zip(blocks, alone):
            assert O.decode(e, guard=64) == b
        batches = {"all": blocks,
                   "one tile at most": [b for b in blocks if len(b) <= TILE],
                   "small, several tiles": [b for b in blocks if TILE < len(b) < BIG],
                   "big": [b for b in blocks if len(b) >= BIG]}
        assert sum(len(v) for v in batches.values()) == 2 * len(blocks)
        for name, batch in batches.items():
            want = [alone[blocks.index(b)] for b in batch]
            got = mz.encode_batch(batch, level, ctx)
            assert [len(g) for g in got] == [len(w) for w in want], name
            assert got == want, name
    finally:
        if opt is not None:
            ctx.set_option(opt, 1)
