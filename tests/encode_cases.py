"""Named edge inputs of the block encoder, one list for every test that feeds it hostile data: runs, overlapping copies of period 1-5,
matches that end on a tile or piece border, offsets next to the 2 MiB + 65535 maximum, blocks of 0-17 bytes and blocks that cross the
2 MiB far-table epoch (MLZ_EPOCH_LOG = 21).  Every input is deterministic (seeded by its name) and contiguous np.uint8; the name goes
into assertion messages.

Test helper: no tests here.  small_cases(), large_cases() and corpus_cases() return lists of Case; each list is built once."""
import zlib
from collections import namedtuple

import numpy as np

from minlz_amd import synth
from tests.util import load_zip

Case = namedtuple("Case", "name data")

MIB = 1 << 20
MAX_OFFSET = 2 * MIB + 65535          # kMaxCopy3Offset
SMALL_SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 100, 4096, 32767, 32768, 32769, 65535, 65536, 65537, 131072, 300000, MIB - 1, MIB, MIB + 77]
PERIODS = [1, 2, 3, 4, 5, 7, 63, 64, 65]
PATTERN_SIZES = [16, 17, 100, 4096, 65535, 65536, 65537, 65549, 70000, 131072, 300000]
LARGE_OFFSETS = [65536, 65600, 200000, MIB, 2 * MIB + 65535, 3 * MIB]
LARGE_SIZES = [2 * MIB - 1, 2 * MIB + 32768 + 5, 4 * MIB + 1, 8 * MIB]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def alphabet(name, n, letters):
    return _rng(name).integers(0, letters, size=n, dtype=np.uint8)


def period(name, n, p):
    return np.tile(_rng(name).integers(0, 256, size=p, dtype=np.uint8), n // p + 1)[:n].copy()


def farflip(name, n):
    """A random chunk of n / 7 bytes tiled 8 times, with n / 64 single-bit flips."""
    rng = _rng(name)
    d = np.tile(rng.integers(0, 256, size=max(n // 7, 1), dtype=np.uint8), 8)[:n].copy()
    k = n // 64
    d[rng.integers(0, max(n, 1), size=k)] ^= (1 << rng.integers(0, 8, size=k)).astype(np.uint8)
    return d


def maxoff(name, n):
    """A random chunk three bytes shorter than the largest offset, tiled: every copy reaches almost as far back as the format allows."""
    chunk = _rng(name).integers(0, 256, size=MAX_OFFSET - 3, dtype=np.uint8)
    return np.tile(chunk, n // chunk.size + 1)[:n].copy()


def _case(name, data):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    data.setflags(write=False)
    return Case(name, data)


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _small():
    out = []
    for n in SMALL_SIZES:
        for letters in (2, 4):
            name = "alphabet%d/%d" % (letters, n)
            out.append(_case(name, alphabet(name, n, letters)))
        for p in PERIODS:
            name = "period%d/%d" % (p, n)
            out.append(_case(name, period(name, n, p)))
        name = "farflip/%d" % n
        out.append(_case(name, farflip(name, n)))
    for pat in synth.PATTERNS:
        for n in PATTERN_SIZES:
            out.append(_case("%s/%d" % (pat, n), synth.pattern(pat, n)))
    for o in LARGE_OFFSETS:
        out.append(_case("large_offset/%d" % o, synth.large_offset(o + 5000, o)))
    return out


def _large():
    out = []
    for n in LARGE_SIZES:
        name = "alphabet4/%d" % n
        out.append(_case(name, alphabet(name, n, 4)))
        name = "period65/%d" % n
        out.append(_case(name, period(name, n, 65)))
        name = "farflip/%d" % n
        out.append(_case(name, farflip(name, n)))
        if n >= 4 * MIB:
            name = "maxoff/%d" % n
            out.append(_case(name, maxoff(name, n)))
    out.append(_case("zeros/%d" % (8 * MIB), np.zeros(8 * MIB, dtype=np.uint8)))
    return out


def _corpus():
    return [_case("enc_regressions/" + label, np.frombuffer(blob, dtype=np.uint8)) for label, blob in load_zip("enc_regressions.zip")]


def small_cases():
    """Blocks of 0 bytes to 3 MiB + 5000: every size class, the tile, piece and class borders."""
    return _once("small", _small)


def large_cases():
    """Blocks of 2 MiB - 1 to 8 MiB: they cross the far-table epoch."""
    return _once("large", _large)


def corpus_cases():
    """The members of tests/golden/enc_regressions.zip."""
    return _once("corpus", _corpus)
