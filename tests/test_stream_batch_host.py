"""The batch calls over many streams in HBM without a GPU: tools/stream_batch_check.cpp runs the lane walk, its step cap and the verdict
code of minlz_amd/csrc/mlz_stream_batch.h (what walk_batch_kernel and the batch decode run) over streams laid BACK TO BACK in one buffer.
Every stream's verdict and decoded prefix must be the host Reader's chunk walk's (mlz_stream_decoded_len / _prefix_len) of that stream
alone: the next stream of the batch lies right behind it, so a byte read past a stream's end changes a verdict here."""
import struct
from collections import Counter

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib
from tests import corrupt as CM
from tests import stream_batch_cases as BC
from tests import stream_device_cases as SC
from tests.search_host import LINK_ERROR, build_checker

SRC = "stream_batch_check.cpp"
WALK_STEPS = 4096   # kBatchWalkSteps


def _checker(tmp_path_factory, sanitized):
    program = build_checker(tmp_path_factory, SRC, sanitized=sanitized)
    assert program is not None, LINK_ERROR.get(SRC)

    def walk(streams):
        buf, spans = BC.back_to_back(streams)
        records = [struct.pack("<Q", len(spans))] + [struct.pack("<QQ", o, n) for o, n in spans] + [struct.pack("<Q", len(buf)) + buf]
        return [tuple(int(v) for v in line.split()) for line in program(records, ["walk"])[0]]
    walk.verdicts = lambda text: [int(v) for line in program([text.encode()], ["verdicts"])[0] for v in line.split()]
    return walk


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _checker(tmp_path_factory, False)


@pytest.fixture(scope="module")
def checker_san(tmp_path_factory):
    """The same program under the address and undefined-behaviour sanitizers: stand-alone, nothing preloaded."""
    return _checker(tmp_path_factory, True)


def _host(s):
    a = np.frombuffer(s, dtype=np.uint8)
    L = _lib.lib()
    p = a.ctypes.data if a.size else None
    return L.mlz_stream_decoded_len(p, a.size), L.mlz_stream_decoded_prefix_len(p, a.size)


def _compare(run, named):
    got = run([s for _, s in named])
    assert len(got) == len(named)
    bad = ["%s: batch walk %s, host Reader %s" % (n, g[:2], _host(s)) for (n, s), g in zip(named, got) if g[:2] != _host(s)]
    assert not bad, "\n".join(bad[:20])
    return got


def test_exported():
    L = _lib.lib()
    assert L.mlz_stream_decoded_len_batch_device and L.mlz_stream_decode_batch_device and L.mlz_stream_encode_batch_device


def test_valid_streams(checker):
    cases = SC.valid_streams_cpu()
    s, d = SC.with_skippables()
    cases.append(("skippables_again", s, d))
    got = _compare(checker, [(n, s) for n, s, _ in cases])
    for (n, s, d), g in zip(cases, got):
        assert g[0] == len(d) and g[3] == 0, n


def test_tiny_streams(checker):
    """An empty stream and streams of 1, 3 and 4 bytes, between whole ones: a stub, a header with nothing behind it."""
    whole = BC.small_stream()
    named = [("whole", whole), ("no_bytes", b""), ("one", whole[:1]), ("three", whole[:3]), ("four", whole[:4]), ("empty_stream", O.stream_encode(b"", 1, BC.BS)),
             ("no_bytes_2", b""), ("one_ff", b"\xff"), ("four_eof", b"\x20\x00\x00\x00"), ("four_pad", b"\xfe\x00\x00\x00"), ("whole_2", whole)]
    got = _compare(checker, named)
    assert got[0][0] == got[-1][0] == len(BC.small_data())
    assert [g[2] for g in got[1:5]] == [0, 1, 1, 1]


def test_mutants(checker):
    d = BC.small_data()
    muts = BC.small_mutants()
    types = {c.type for c in CM.chunks(BC.small_stream())}
    assert 0x01 in types and 0x02 in types            # stream_mutants needs a stored and a compressed chunk
    assert len(muts) == BC.MUTANT_COUNT
    got = _compare(checker, muts)
    want = Counter()
    for (name, b), g in zip(muts, got):
        code = CM.stream_verdict(b, len(d) + 16)[0]
        want[code] += 1
        assert g[3] == 0, name
        if g[0] < 0:
            assert code != 0, name
        elif code not in (0, 1, 5):   # CRC and body errors are the decode's to find, not the walk's
            assert False, "%s: the oracle says %d, the walk found no framing error" % (name, code)
    assert dict(want) == BC.MUTANT_CODES
    assert all(want[c] > 0 for c in (0, 1, 2, 3, 5))


def test_mutants_sanitized(checker_san):
    """Every mutant in one batch through the sanitizer build: no byte outside the buffer is read, whatever the lengths claim."""
    _compare(checker_san, BC.small_mutants())


def test_cuts(checker):
    """The stream cut at every length around its chunk borders (and the first 64 lengths), all cuts in one batch."""
    s = BC.small_stream()
    cs = CM.chunks(s)
    cuts = set(range(0, 64))
    for c in cs:
        cuts.update(range(max(c.off - 3, 0), min(c.off + 16, len(s) + 1)))
    cuts.update(range(len(s) - 8, len(s) + 1))
    _compare(checker, [("cut_%d" % k, s[:k]) for k in sorted(cuts)])


def test_long_stream_alone_is_flagged(checker):
    s, d = SC.tiny_chunks()
    sb, _ = SC.tiny_chunks(break_crc=True)
    whole = BC.small_stream()
    named = [("whole", whole), ("tiny", s), ("whole_2", whole), ("tiny_crc", sb), ("tiny_cut", s[:len(s) - 7]), ("empty", b"")]
    got = _compare(checker, named)
    assert [g[3] for g in got] == [0, 1, 0, 1, 1, 0]
    assert got[1][0] == len(d) and got[1][2] == 200 + 2   # identifier, the data chunks, EOF


def test_step_cap_is_exact(checker):
    """A stream of exactly the cap's number of chunk headers stays with the lane; one more makes it long."""
    def stream(headers):
        return SC.stream_id(4 << 10) + SC.frame(0x80, b"") * (headers - 2) + SC.eof(0)
    got = _compare(checker, [("at_cap", stream(WALK_STEPS)), ("over_cap", stream(WALK_STEPS + 1)), ("under_cap", stream(WALK_STEPS - 1))])
    assert [g[3] for g in got] == [0, 1, 0] and all(g[0] == 0 for g in got)


def test_verdicts_from_jobs(checker):
    """Hand-made per-chunk results: a body error in stream 3, a CRC error in chunk 0 of stream 5 and a later body error in it."""
    n_streams, per, size = 8, 4, 1000
    lines = [str(n_streams)]
    for i in range(n_streams):
        lines.append("%d %d" % (per * size, per))
        for j in range(per):
            got, crc_got = size, 77
            if (i, j) == (3, 2):
                got = -1
            if (i, j) == (5, 0):
                crc_got = 78
            if (i, j) == (5, 3):
                got = size - 1
            lines.append("1 %d %d 1 %d 77" % (got, size, crc_got))
    out = checker.verdicts("\n".join(lines) + "\n")
    assert out == [per * size] * 3 + [-1] + [per * size] + [-5] + [per * size] * 2
    # a framing error behind good chunks stays; a chunk's error in front of it wins; a stored chunk has no decode result; no CRC check: no CRC error
    out = checker.verdicts("4\n-3 1\n1 10 10 1 5 5\n-3 1\n1 10 10 1 5 6\n7 1\n0 -9 7 1 5 5\n7 1\n1 7 7 0 5 6\n")
    assert out == [-3, -5, 7, 7]
