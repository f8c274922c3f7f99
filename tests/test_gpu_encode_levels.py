"""The encoder's five kernel configurations on the edge inputs of tests/encode_cases.py.  Per configuration ("leg": LevelSuperFast,
LevelFastest without and with far tables, LevelBalanced with and without tile levels) every block must be

- the block the CPU model predicts (tools/encmodel2 at run2.params_for: tests/test_encode_model.py pins that expected value without a
  GPU), header and all, or the stored block where the layout decides so (encode_legs.is_stored restates its comparison);
- within MaxEncodedLen and decoded by the oracle back to the input;
- the same bytes in one batch of all the test's cases (blocks of at most a tile, small ones and big ones side by side: every match
  launch of the group runs) as alone;
- decoded by the GPU back to the input, in one batch and alone, the decoder taking the path the restatement of the tile levels
  (tests/tile_levels.py) says: never the general one at the four level-bound legs — a block that left its levels would still round-trip,
  three times slower —, and the general one with a team of 4 where LevelBalanced without levels reads another tile."""
import numpy as np
import pytest

import minlz_amd as mz
import oracle as O
from tests import encode_cases as EC
from tests import encode_legs as EL
from tests.tile_levels_gpu import check_single

pytestmark = pytest.mark.gpu

LEGS = EL.model().LEGS


def _first_diff(a, b):
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    k = min(x.size, y.size)
    d = np.flatnonzero(x[:k] != y[:k])
    return int(d[0]) if d.size else k


def _check_leg(ctx, leg, cases):
    level, opt, value = EL.leg_settings(leg)
    inputs = [c.data.tobytes() for c in cases]
    want = [EL.block_of(c.data, body) for c, body in zip(cases, EL.model_bodies(cases, leg))]
    if opt is not None:
        ctx.set_option(opt, value)
    try:
        alone = [mz.Encode(c.data, level, ctx) for c in cases]
        batch = mz.encode_batch([c.data for c in cases], level, ctx)
    finally:
        if opt is not None:
            ctx.set_option(opt, 1)
    bad = []
    for c, src, enc, w, b in zip(cases, inputs, alone, want, batch):
        if len(enc) > mz.MaxEncodedLen(len(src)):
            bad.append("%s %s: %d bytes, MaxEncodedLen %d" % (leg, c.name, len(enc), mz.MaxEncodedLen(len(src))))
        try:
            if O.decode(enc, guard=64) != src:
                bad.append("%s %s: the oracle decodes other bytes" % (leg, c.name))
        except O.OracleError as e:
            bad.append("%s %s: %s" % (leg, c.name, e))
        if enc != w:
            bad.append("%s %s: block of %d bytes, the model's has %d (%s), first differing byte %d"
                       % (leg, c.name, len(enc), len(w), "stored" if w[:2] == b"\x00\x00" else "compressed", _first_diff(enc, w)))
        if b != enc:
            bad.append("%s %s: in the batch %d bytes, alone %d, first differing byte %d" % (leg, c.name, len(b), len(enc), _first_diff(b, enc)))
    assert not bad, "%d of %d cases\n%s" % (len({m.split(":")[0] for m in bad}), len(cases), "\n".join(bad[:40]))

    assert mz.decode_batch(alone, ctx) == inputs
    if leg != "balanced-free":
        assert ctx.general_blocks() == 0, leg
    general = []
    for c, src, enc in zip(cases, inputs, alone):
        if EL.levels_checked(len(src)):
            v = check_single(ctx, enc, src, (leg, c.name))
            if v.general:
                general.append((c.name, v.team))
    return general


@pytest.mark.parametrize("leg", LEGS)
def test_small_and_corpus_blocks(ctx, leg):
    general = _check_leg(ctx, leg, EC.small_cases() + EC.corpus_cases())
    if leg == "balanced-free":
        assert general and all(team == 4 for _, team in general), general
    else:
        assert not general, general


@pytest.mark.parametrize("leg", LEGS)
def test_large_blocks(ctx, leg):
    _check_leg(ctx, leg, EC.large_cases())
