"""The device-resident Reader's chunk walk without a GPU: tools/stream_walk_check.cpp restates the region algorithm of
minlz_amd/csrc/mlz_stream_walk.hip.inc on the host and runs the library's own record and running-state code (mlz_stream_walk.h) on what it
finds; its verdict and decoded prefix must be the host Reader's chunk walk's (mlz_stream_decoded_len / _prefix_len) for valid streams, for
every mutant of tests/corrupt.py's stream_mutants, for cuts at every length near the chunk borders and for the stream of many tiny chunks."""
import struct
from collections import Counter

import numpy as np
import pytest

from minlz_amd import _lib
from tests import corrupt as CM
from tests import stream_device_cases as SC
from tests.search_host import build_checker



@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    program = build_checker(tmp_path_factory, "stream_walk_check.cpp")
    return lambda streams: [tuple(int(v) for v in line.split()) for line in program([struct.pack("<Q", len(s)) + s for s in streams])[0]]


def _host(s):
    a = np.frombuffer(s, dtype=np.uint8)
    L = _lib.lib()
    p = a.ctypes.data if a.size else None
    return L.mlz_stream_decoded_len(p, a.size), L.mlz_stream_decoded_prefix_len(p, a.size)


def _compare(checker, named):
    got = checker([s for _, s in named])
    assert len(got) == len(named)
    bad = ["%s: walk %s, host Reader %s" % (n, g[:2], _host(s)) for (n, s), g in zip(named, got) if g[:2] != _host(s)]
    assert not bad, "\n".join(bad[:20])
    return got


def test_exported():
    L = _lib.lib()
    assert L.mlz_stream_decoded_len_device and L.mlz_stream_decode_device


def test_valid_streams(checker):
    cases = SC.valid_streams_cpu()
    got = _compare(checker, [(n, s) for n, s, _ in cases])
    for (n, s, d), g in zip(cases, got):
        assert g[0] == len(d), n


@pytest.mark.parametrize("bs,count,codes", [(1 << 20, 65, {0: 3, 1: 41, 2: 3, 3: 6, 5: 12}), (64 << 10, 125, {0: 3, 1: 96, 2: 2, 3: 6, 5: 18})])
def test_mutants(checker, bs, count, codes):
    s = SC.oracle_stream(bs)
    d = SC.data_mix()
    muts = CM.stream_mutants(s)
    assert len(muts) == count
    got = _compare(checker, muts)
    # the oracle's Reader: its framing verdicts are the walk's; CRC and body errors (found by the decode) are not the walk's to find
    want = Counter()
    for (name, b), g in zip(muts, got):
        code = CM.stream_verdict(b, len(d) + 16)[0]
        want[code] += 1
        if g[0] < 0:
            assert code != 0, name
        elif code not in (0, 1, 5):
            assert False, "%s: the oracle says %d, the walk found no framing error" % (name, code)
    assert dict(want) == codes


def test_cuts(checker):
    """A stream cut at every length around its chunk borders (and the first 64 lengths): stubs, truncated chunks, a clean end."""
    s = SC.oracle_stream(64 << 10)
    cs = CM.chunks(s)
    cuts = set(range(0, 64))
    for c in cs[:6] + cs[-4:]:
        cuts.update(range(max(c.off - 3, 0), min(c.off + 16, len(s) + 1)))
    cuts.update(range(4096 - 8, 4096 + 8))
    cuts.update(range((256 << 10) - 8, (256 << 10) + 8))
    _compare(checker, [("cut_%d" % k, s[:k]) for k in sorted(cuts)])


def test_many_tiny_chunks(checker):
    s, d = SC.tiny_chunks()
    sb, _ = SC.tiny_chunks(break_crc=True)
    got = _compare(checker, [("tiny", s), ("tiny_crc", sb), ("tiny_cut", s[:len(s) - 7]), ("tiny_odd_cut", s[:400_001])])
    assert got[0][0] == len(d) and got[0][2] == 200 + 2   # identifier, the data chunks, EOF: no skippable chunk in the table
