"""The far-table build's workgroup placement (far_place, mlz_encode.hip.inc): far_build_kernel runs on a one-dimensional grid and derives
(block, epoch, slice) from the workgroup number, eight (block, epoch) groups at a time, padded to a multiple of eight.  A slice that is
lost, built twice over another or written into the wrong table changes the encoder's matches, so the check is the bytes: every block of
every batch must be the block the CPU model predicts (tests/encode_legs.py; the device is never the reference).

The batches are chosen for the group counts Q = blocks x epochs the map can get wrong: 1, 3 (less than eight), 8 (exactly eight, two
ways), 9 and 17 (one more than a multiple of eight), blocks of unequal length whose shorter ones have empty epochs, and both block
classes in one batch (two far launches).  LevelFastest has 4 slices per table, LevelBalanced with tile levels 8.

The same kernel reads whole tiles with 16-byte loads and a block's last tile window by window; the last batch puts a block's end 8 and 7
bytes behind a tile border, on either side of what the whole-tile path asks for, at both levels (windows every 4th and every 2nd byte).

Not vacuous: for every block above one tile the model's body with far tables differs from its body without them."""
import functools

import pytest

import minlz_amd as mz
from minlz_amd import synth
from tests import encode_cases as EC
from tests import encode_legs as EL

pytestmark = pytest.mark.gpu

MIB = 1 << 20
A, B, C4, C8 = MIB + 5, 2 * MIB + 4097, 4 * MIB + 1, 8 * MIB

# (name, [(length, seed), ...]): blocks of one length in a batch differ in their seed, so a table that lands at another block shows
BATCHES = [
    ("a-q1", [(A, 0)]),
    ("b-q3", [(A, s) for s in range(3)]),
    ("c-q8", [(B, s) for s in range(4)]),
    ("d-q9-empty-epochs", [(C4, 0), (A, 0), (B, 0)]),
    ("e-q17", [(A, s) for s in range(17)]),
    ("f-q8-8MiB", [(C8, 0), (A, 1)]),
    ("g-both-classes", [(64 * 1024 + 3, 0), (3 * MIB, 0)]),
    # the whole-tile path's own border: a last whole tile with exactly the 8 spare bytes it asks for, with 7, and a short last tile
    ("h-spare-bytes", [(2 * MIB + 8, 0), (2 * MIB + 7, 1), (MIB + EL.TILE + 12, 2)]),
]


@functools.lru_cache(maxsize=None)
def _case(n, seed):
    data = synth.enwik_like(n, seed)
    data.setflags(write=False)
    return EC.Case("enwik_like(%d, %d)" % (n, seed), data)


ALL_KEYS = tuple(sorted({k for _, blocks in BATCHES for k in blocks}))


@functools.lru_cache(maxsize=None)
def _bodies(leg, keys=ALL_KEYS):
    """The model's body per (length, seed), computed once per leg for all the batches together."""
    return dict(zip(keys, EL.model_bodies([_case(*k) for k in keys], leg)))


def _check(ctx, leg, blocks, keys=ALL_KEYS):
    level, opt, value = EL.leg_settings(leg)
    cases = [_case(*k) for k in blocks]
    want = [EL.block_of(c.data, _bodies(leg, keys)[k]) for c, k in zip(cases, blocks)]
    ctx.set_option(opt, value)
    try:
        got = mz.encode_batch([c.data for c in cases], level, ctx)
    finally:
        ctx.set_option(opt, 1)
    bad = ["block %d %s: %d bytes, the model's has %d" % (i, c.name, len(g), len(w)) for i, (c, g, w) in enumerate(zip(cases, got, want)) if g != w]
    assert not bad, "%s: %d of %d blocks\n%s" % (leg, len(bad), len(cases), "\n".join(bad))


def test_far_tables_change_the_bytes():
    """What makes the comparisons below a test of the tables: without them the model writes another body for every block above a tile."""
    far1, far0 = _bodies("fastest-far1"), _bodies("fastest-far0")
    same = [k for k in far1 if k[0] > EL.TILE and far1[k] == far0[k]]
    assert not same, same
    assert all(len(far1[k]) < len(far0[k]) for k in far1 if k[0] >= MIB)


@pytest.mark.parametrize("name,blocks", BATCHES, ids=[b[0] for b in BATCHES])
def test_fastest_batches_match_the_model(ctx, name, blocks):
    _check(ctx, "fastest-far1", blocks)


@pytest.mark.parametrize("name,blocks", [BATCHES[3], BATCHES[7]], ids=[BATCHES[3][0], BATCHES[7][0]])
def test_balanced_levels_eight_slices(ctx, name, blocks):
    _check(ctx, "balanced-levels", blocks, tuple(blocks))
