"""The expected value of tests/test_gpu_encode_levels.py, pinned without a GPU: the CPU model of the match + serialize kernels
(tools/encmodel2) over the edge inputs of tests/encode_cases.py, at the parameters of each of the encoder's five kernel configurations
(run2.params_for).  The model alone must write streams the oracle decodes back to the input, streams that keep the tile levels their
level promises, and it must compress most of the inputs — otherwise the GPU comparison would be one of stored blocks."""
import pytest

import oracle as O
from tests import encode_cases as EC
from tests import encode_legs as EL
from tests import tile_levels as TL

LEGS = EL.model().LEGS


@pytest.mark.parametrize("leg", LEGS)
def test_model_on_edge_inputs(leg):
    cases = EC.small_cases() + EC.corpus_cases() + EC.large_cases()
    bodies = EL.model_bodies(cases, leg)
    bad, general, big, compressed = [], [], 0, 0
    for c, body in zip(cases, bodies):
        n = c.data.size
        # round trip.  (The model never declines: a piece that does not beat one literal run is written as that run, so every body decodes,
        # the ones the layout then replaces by a stored block included; run2.model_body checks the output bound.)
        code, dec = O.decode_body(body, n)
        if code != 0 or dec != c.data.tobytes():
            bad.append("%s: the oracle decodes the body with code %d%s" % (c.name, code, ", other bytes" if code == 0 else ""))
            continue
        stored = EL.is_stored(n, len(body))
        if n > 64:
            big += 1
            compressed += not stored
        if EL.levels_checked(n):
            v = TL.verdict(TL.walk(body, n), n)
            if v.general:
                general.append((c.name, v.team, stored))
    assert not bad, "\n".join(bad)
    if leg == "balanced-free":
        assert all(team == 4 for _, team, _ in general), general   # far sources lie at least four tiles back (MLZ_OPT_L2_GAP)
        assert any(not stored for _, _, stored in general), "no block of the list is a general one: the GPU test's team-4 assertion would be vacuous"
    else:
        assert not general, general
    assert 4 * compressed >= 3 * big, (leg, compressed, big)
