"""GPU side of tests/tile_levels.py, shared by the tests that decode blocks of real encoders and compare the decoder's counters with the
restated verdict.

Test helper: no tests here."""
import minlz_amd as mz
from tests import tile_levels as TL


def check_single(ctx, enc, want, what):
    """Decodes one block alone: the bytes must be `want`, and the counters of general blocks (mlz_get_counter 2) and of the team size (6)
    what tile_levels.verdict() says of the block's body.  Returns the verdict."""
    assert mz.decode_batch([enc], ctx) == [want], what
    body, dlen = TL.block_body(enc)
    v = TL.verdict(TL.walk(body, dlen), dlen) if body is not None else TL.make_verdict(TL.ORDER, None, False)
    assert (ctx.general_blocks(), ctx.general_team()) == (int(v.general), v.team), (what, v)
    return v
