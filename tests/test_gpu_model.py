"""The device encoder against its CPU model (tools/encmodel2: a sequential statement of exactly the match + serialize
kernels' algorithm, test infrastructure like the oracle): block bodies must be byte-identical at every one of the encoder's
five kernel configurations (run2.LEGS), for both block classes (>= 1 MiB: 12-bit near tables; smaller: 13-bit, far tables
sized by the block).  The edge inputs are in tests/test_gpu_encode_levels.py; these are the plain text and JSON blocks."""
import numpy as np
import pytest

import minlz_amd as mz
from minlz_amd import synth
from tests import encode_legs as EL

pytestmark = pytest.mark.gpu

# (level 20 = LevelBalanced WITH the tile levels of rounds 1-3: option 14 = 0; level 10 = LevelFastest without far tables: option 2 = 0)
LEG_OF = {1: "fastest-far1", 2: "balanced-free", 20: "balanced-levels", -1: "superfast", 10: "fastest-far0"}


@pytest.fixture(scope="module")
def model():
    return EL.model()  # compiles the model with g++ on import


def _body(enc):
    assert enc[0] == 0
    h = 1
    while enc[h] & 0x80:
        h += 1
    return bytes(enc[h + 1:])


@pytest.mark.parametrize("level", list(LEG_OF))
def test_device_output_equals_the_model(ctx, model, level):
    leg = LEG_OF[level]
    lv, opt, value = EL.leg_settings(leg)
    if opt is not None:
        ctx.set_option(opt, value)
    try:
        _check_model(ctx, model, lv, leg)
    finally:
        if opt is not None:
            ctx.set_option(opt, 1)


def _check_model(ctx, model, lv, leg):
    rng = np.random.default_rng(9)
    mix = np.concatenate([synth.text_like(200000, 4), rng.integers(0, 256, 100000, dtype=np.uint8), synth.json_like(150000, 5)])
    cases = [synth.text_like(100000, 7), synth.text_like((1 << 20) + 77, 8), mix, synth.json_like(3 << 20, 2),
             synth.text_like(64 << 10, 3), synth.text_like((128 << 10) + 5, 6), synth.json_like(300000, 9), synth.text_like(700000, 10)]
    for a in cases:
        a = np.ascontiguousarray(a)
        enc = mz.Encode(a, lv, ctx)
        assert _body(enc) == model.model_body(a, leg), (leg, a.size)
    # one batch with blocks of every size class (far tables of different sizes side by side)
    encs = mz.encode_batch([np.ascontiguousarray(a) for a in cases], lv, ctx)
    for a, enc in zip(cases, encs):
        assert _body(enc) == model.model_body(np.ascontiguousarray(a), leg), (leg, a.size, "batch")
