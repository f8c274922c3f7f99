"""The record index without a GPU: tools/stream_record_index_check.cpp runs the rules the calls share with their kernels
(minlz_amd/csrc/mlz_stream_record_index.h: the exact 16-byte mask, lane, step and tile ranks, N from k and the last byte, the span rule, the
lower-bound rule) as plain loops, plain and under AddressSanitizer and UBSan, and tests/record_index_model.py says what must come out.  A
second check does not rest on the model: the records are data.split(delimiter) with one trailing empty piece dropped."""
import shutil
import struct

import numpy as np
import pytest

from minlz_amd import _lib
from tests import record_index_model as IM
from tests import search_host as H
from tests.search_host import both

SRC = "stream_record_index_check.cpp"
SHIFTS = (0, 5, 15)
NEW_SYMBOLS = ["mlz_dev_reader_index_records", "mlz_dev_reader_record_count", "mlz_dev_reader_record_spans", "mlz_dev_reader_read_records",
               "mlz_dev_reader_record_numbers", "mlz_dev_reader_record_range"]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def idx_case(data, delim, pos=(), shift=0):
    return struct.pack("<IIIQQ", 1, delim[0], shift, len(data), len(pos)) + bytes(data) + np.asarray(pos, np.uint64).tobytes()


def parse(line):
    head, _, rest = line.partition(":")
    D, spans, nums = rest.split("|")
    N, k, tiles = (int(v) for v in head.split())
    return dict(N=N, k=k, tiles=tiles, D=[int(v) for v in D.split()], spans=[tuple(int(v) for v in s.split(":")) for s in spans.split()],
                numbers=[IM.NO_RECORD if v == "-" else int(v) for v in nums.split()])


def positions(data, delim):
    """Where the numbers are asked: the starts of records, their last bytes, the delimiters, the last byte, the size and beyond."""
    start, length = IM.spans(data, delim)
    pos = set(start[:50].tolist()) | set((start + np.maximum(length, 1) - 1)[:50].tolist()) | set(IM.delimiters(data, delim)[:50].tolist())
    pos |= {0, max(len(data) - 1, 0), len(data), len(data) + 1, 1 << 40}
    return sorted(pos)


def check(checkers, cases):
    """cases: (data, delim); every case runs at three misalignments of the buffer -> the parsed results at misalignment 0."""
    recs = [idx_case(d, dl, positions(d, dl), s) for d, dl in cases for s in SHIFTS]
    lines = both(checkers, recs)
    assert len(lines) == len(recs)
    out = []
    for ci, (data, delim) in enumerate(cases):
        N, k = IM.count(data, delim)
        start, length = IM.spans(data, delim)
        pos = positions(data, delim)
        want_no, _ = IM.numbers(data, delim, pos)
        for si, s in enumerate(SHIFTS):
            got = parse(lines[ci * len(SHIFTS) + si])
            what = "case %d: %d bytes, delimiter %#x, shift %d" % (ci, len(data), delim[0], s)
            assert (got["N"], got["k"]) == (N, k), what
            assert got["tiles"] == (s + len(data) + 65535) // 65536 if len(data) else got["tiles"] == 0, what
            assert got["D"] == IM.delimiters(data, delim).tolist(), what
            assert got["spans"] == list(zip(start.tolist(), length.tolist())), what
            assert got["numbers"] == want_no, what
            if si == 0:
                out.append(got)
    return out


def test_sanitized_build_links(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizer runtimes: " + H.LINK_ERROR[SRC][-300:])
    assert shutil.which("g++")


def test_exported():
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert getattr(L, s) and s in _lib.SYMBOLS


def test_word_mask_is_exact(checkers):
    assert both(checkers, [struct.pack("<I", 2)]) == ["words %d ok" % (1 << 24)]


NL = b"\n"


def test_edges(checkers):
    res = check(checkers, [
        (b"", NL),                          # empty data
        (b"\n", NL),                        # one byte, a delimiter
        (b"x", NL),                         # ... and not
        (b"\nabc\ndef", NL),                # begins with a delimiter, ends without one
        (b"abc\ndef\n", NL),                # ends with one
        (b"abc\ndef", NL),
        (b"a\n\nb\n\n\nc\n\n", NL),         # doubled delimiters
        (b"no delimiter at all, in more than sixteen bytes", NL),
        (b"\n" * 100, NL),                  # every byte a delimiter
        (b"\n" * 16, NL),
    ])
    assert [(r["N"], r["k"]) for r in res] == [(0, 0), (1, 1), (1, 0), (3, 2), (2, 2), (2, 1), (7, 7), (1, 0), (100, 100), (16, 16)]
    assert res[3]["spans"] == [(0, 0), (1, 3), (5, 3)] and res[6]["spans"] == [(0, 1), (2, 0), (3, 1), (5, 0), (6, 0), (7, 1), (9, 0)]
    assert res[8]["spans"] == [(i, 0) for i in range(100)]


@pytest.mark.parametrize("at", [(15,), (16,), (17,), (15, 16, 17), (65535,), (65536,), (65537,), (65535, 65536, 65537), (0, 15, 16, 65535, 65536, 131071)])
def test_delimiters_at_block_and_tile_borders(checkers, at):
    d = bytearray(b"abcdefghijklmnopqrstuvwxyz" * 5042)[:131072]
    for a in at:
        d[a] = 10
    (r,) = check(checkers, [(bytes(d), NL)])
    assert r["D"] == list(at) and r["N"] == len(at) + (0 if at[-1] == len(d) - 1 else 1)


def test_every_byte_a_delimiter_over_tiles(checkers):
    """The densest case: 16 hits per lane and step, 65 536 per tile, over a tile border and a ragged tail."""
    n = 65536 + 4096 + 33
    (r,) = check(checkers, [(b"," * n, b",")])
    assert r["N"] == r["k"] == n


@pytest.mark.parametrize("delim", [0x00, 0x0A, 0x80, 0xFF])
def test_exact_mask(checkers, delim):
    """delimiter ^ 1 directly behind and in front of a hit, and delimiter ^ 0x80: what a zero-byte test with a borrow or without the high
    bit miscounts."""
    d, n1, n80 = bytes([delim]), bytes([delim ^ 1]), bytes([delim ^ 0x80])
    unit = d + n1 + n1 + d + n80 + n1 + d + d + n1 + n80 + n80 + d + n1
    data = (unit * 40 + n1 * 7 + d + n1 + n80 * 3) * 3
    rng = np.random.default_rng(delim)
    noise = bytes(np.frombuffer(d + n1 + n80 + bytes([delim ^ 0x7f]), np.uint8)[rng.integers(0, 4, 5000)])
    res = check(checkers, [(data, d), (noise, d), (n1 * 300, d), (n80 * 300, d), ((n1 + d) * 150, d), ((d + n1) * 150, d)])
    assert res[2]["k"] == 0 and res[3]["k"] == 0 and res[4]["k"] == 150 and res[5]["N"] == 151


@pytest.mark.parametrize("alphabet", [b"ab\n", b"abcdefgh \n\n", b"\n\n\nx", bytes(range(256))])
def test_split(checkers, alphabet):
    """Not through the model: the records are data.split(delimiter) with one trailing empty piece dropped."""
    rng = np.random.default_rng(len(alphabet))
    cases = []
    for n in (1, 7, 16, 17, 300, 3000, 70000):
        cases.append((bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)]), NL))
    lines = both(checkers, [idx_case(d, dl, (), s) for d, dl in cases for s in SHIFTS])
    for ci, (data, _) in enumerate(cases):
        pieces = data.split(NL)
        if pieces[-1] == b"":
            pieces.pop()
        for si in range(len(SHIFTS)):
            got = parse(lines[ci * len(SHIFTS) + si])
            assert got["N"] == len(pieces)
            assert [data[o:o + n] for o, n in got["spans"]] == pieces
            assert all(o == 0 or data[o - 1:o] == NL for o, _ in got["spans"])


def test_model_ranges_and_reads():
    """The model's own words for record_range and read, on a line that can be counted by hand."""
    data = b"a\n\nbcd\nef"
    assert IM.count(data, NL) == (4, 3)
    assert IM.record_range(data, NL, 0, 4) == (0, 9) and IM.record_range(data, NL, 1, 2) == (2, 4) and IM.record_range(data, NL, 2, 0) == (3, 0)
    assert IM.record_range(data, NL, 4, 0) == (9, 0) and IM.record_range(data, NL, 3, 2) is None
    assert IM.read(data, NL, [3, 1, 0, 3]) == (b"efaef", [0, 2, 2, 3, 5])
    assert IM.numbers(data, NL, [0, 1, 2, 3, 8, 9]) == ([0, 0, 1, 2, 3, IM.NO_RECORD], 5)
