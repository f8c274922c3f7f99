"""The encoder's five kernel configurations ("legs": tools/encmodel2/run2.py names them and gives the CPU model's parameters for each)
and the block the model predicts for an input — the expected value of tests/test_encode_model.py (the model alone, no GPU) and of
tests/test_gpu_encode_levels.py (the kernels against it).

Test helper: no tests here."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

from tests import tile_levels as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = TL.TILE
LEVELS_MAX = (1 << 20) + 77      # the largest block whose body is walked by the restatement of the tile levels (pure Python)
MIN_NON_LITERAL = 16             # kMinNonLiteralBlock (mlz_format.h)

_run2 = None


def model():
    """tools/encmodel2/run2 (compiles the model with g++ on its first import)."""
    global _run2
    if _run2 is None:
        sys.path.insert(0, os.path.join(ROOT, "tools", "encmodel2"))
        import run2
        _run2 = run2
    return _run2


def leg_settings(leg):
    """(level, option, value): the option is set for the leg and put back to its default, 1, afterwards."""
    import minlz_amd as mz
    return {"superfast": (mz.LevelSuperFast, None, None),
            "fastest-far0": (mz.LevelFastest, mz.OPT_ENCODE_FAR, 0),
            "fastest-far1": (mz.LevelFastest, mz.OPT_ENCODE_FAR, 1),
            "balanced-levels": (mz.LevelBalanced, mz.OPT_L2_FREE, 0),
            "balanced-free": (mz.LevelBalanced, mz.OPT_L2_FREE, 1)}[leg]


def is_stored(n, body_len):
    """The layout's decision (encode_gather2_kernel, mlz_encode2.hip.inc:801-802, and encode_layout_kernel, mlz_encode.hip.inc:537-538):
    stored <=> n < kMinNonLiteralBlock or total > n - (n >> 5) - 6 — a strict '>' against the reference's dstLimit, not 'not shorter
    than the input'."""
    return n < MIN_NON_LITERAL or body_len > n - (n >> 5) - 6


def uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def block_of(data, body):
    """The block the encoder must write for `data` when its token stream is `body`: 00 uvarint(n) body, the stored block 00 00 data
    where the layout decides so, 00 for the empty block."""
    n = data.size
    if n == 0:
        return b"\x00"
    if is_stored(n, len(body)):
        return b"\x00\x00" + data.tobytes()
    return b"\x00" + uvarint(n) + body


def model_bodies(cases, leg, threads=None):
    """The model's token stream per case (the calls run side by side: ctypes releases the interpreter lock, and the model keeps no state
    between blocks)."""
    run2 = model()
    with ThreadPoolExecutor(max_workers=threads or min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda c: run2.model_body(c.data, leg), cases))


def levels_checked(n):
    """Blocks whose tile-level verdict the tests restate: more than one tile, and small enough for the walk in Python."""
    return TILE < n <= LEVELS_MAX


def body_verdict(enc):
    """tile_levels.verdict of an encoded block; a stored block conforms to every pattern."""
    body, dlen = TL.block_body(enc)
    return TL.verdict(TL.walk(body, dlen), dlen) if body is not None else TL.make_verdict(TL.ORDER, None, False)
