"""The device-resident Reader's chunk walk without a GPU: tools/stream_walk_check.cpp restates the region algorithm of
minlz_amd/csrc/mlz_stream_walk.hip.inc on the host and runs the library's own record and running-state code (mlz_stream_walk.h) on what it
finds; its verdict and decoded prefix must be the host Reader's chunk walk's (mlz_stream_decoded_len / _prefix_len) for valid streams, for
every mutant of tests/corrupt.py's stream_mutants, for cuts at every length near the chunk borders and for the stream of many tiny chunks.

The host Reader runs the same step, record and state code (stream_parse), so that comparison checks the region algorithm against the
straight walk; the rules themselves are held against the oracle's Reader in test_mutants.  The tool also runs the host Reader's walk
over its exact-size copy of every stream, and every case goes through the plain build and the build under AddressSanitizer and UBSan
(a stand-alone program, nothing preloaded): neither walk reads a byte past the stream's end."""
import struct
from collections import Counter

import numpy as np
import pytest

from minlz_amd import _lib
from tests import corrupt as CM
from tests import search_host as H
from tests import stream_device_cases as SC

SRC = "stream_walk_check.cpp"


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


@pytest.fixture(scope="module")
def checker(programs):
    """streams -> per stream (result, prefix, table entries, host result, host prefix); the sanitized build must print the same."""
    return lambda streams: [tuple(int(v) for v in line.split()) for line in H.both(programs, [struct.pack("<Q", len(s)) + s for s in streams])]


def test_sanitized_build_links(programs):
    if programs[1] is None:
        pytest.skip("this g++ does not link the sanitizer runtimes: " + H.LINK_ERROR[SRC][-300:])


def _host(s):
    a = np.frombuffer(s, dtype=np.uint8)
    L = _lib.lib()
    p = a.ctypes.data if a.size else None
    return L.mlz_stream_decoded_len(p, a.size), L.mlz_stream_decoded_prefix_len(p, a.size)


def _compare(checker, named):
    """The region walk (columns 0, 1) and the tool's host Reader walk (3, 4) against the library's host Reader."""
    got = checker([s for _, s in named])
    assert len(got) == len(named)
    bad = ["%s: walk %s, tool's host Reader %s, host Reader %s" % (n, g[:2], g[3:5], _host(s)) for (n, s), g in zip(named, got) if not g[:2] == g[3:5] == _host(s)]
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


# (oracle code, the host walk's result or "ok" for >= 0) -> single-fault mutants, per block size: a change in the mutator cannot empty a class unnoticed
TALLY = {1 << 20: {(0, "ok"): 3, (2, -2): 3, (3, -3): 6, (1, "ok"): 2, (1, -1): 33, (1, -3): 1, (5, "ok"): 7},
         64 << 10: {(0, "ok"): 3, (2, -2): 2, (3, -3): 6, (1, "ok"): 1, (1, -1): 94, (1, -3): 1, (5, "ok"): 8}}


@pytest.mark.parametrize("bs,count,codes", [(1 << 20, 65, {0: 3, 1: 41, 2: 3, 3: 6, 5: 12}), (64 << 10, 125, {0: 3, 1: 96, 2: 2, 3: 6, 5: 18})])
def test_mutants(checker, bs, count, codes):
    s = SC.oracle_stream(bs)
    d = SC.data_mix()
    muts = CM.stream_mutants(s)
    assert len(muts) == count
    got = _compare(checker, muts)
    # the oracle's Reader: its framing verdicts are the walk's; CRC and body errors (found by the decode) are not the walk's to find
    want = Counter()
    verdicts = {}
    for (name, b), g in zip(muts, got):
        verdicts[name] = CM.stream_verdict(b, len(d) + 16)
        code = verdicts[name][0]
        want[code] += 1
        if g[0] < 0:
            assert code != 0, name
        elif code not in (0, 1, 5):
            assert False, "%s: the oracle says %d, the walk found no framing error" % (name, code)
    assert dict(want) == codes
    # The host walk against the oracle, an independent judge, for every single-fault mutant: a clean stream has the oracle's length; too
    # large (2) and unsupported (3) are framing verdicts and exact; corrupt (1) and CRC (5) may be the decode's to find, so the walk may
    # pass — or report a framing error of its own, because a body error in front of a framing error wins in the oracle.
    seen = Counter()
    for name, b in muts:
        if name.startswith("two_"):
            continue
        code, data = verdicts[name]
        walk = _host(b)[0]
        seen[(code, "ok" if walk >= 0 else walk)] += 1
        if code == 0:
            assert walk == len(data), name
        elif code in (2, 3):
            assert walk == -code, name
        if walk >= 0:
            assert code in (0, 1, 5), name
        else:
            assert code != 0, name
    assert dict(seen) == TALLY[bs]


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
