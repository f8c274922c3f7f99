"""mlz_dev_reader_search_records without a GPU: tools/stream_records_check.cpp runs the rules the call shares with its kernels
(minlz_amd/csrc/mlz_stream_records.h: the window of an occurrence and the merge, the bounds as a wavefront finds them, the opening rule, the
cut at the caps) as plain loops, plain and under AddressSanitizer and UBSan, and tests/records_model.py says what must come out.  A second
check does not rest on the model: with a reach of at least the longest record the records are the lines that hold the pattern."""
import shutil
import struct

import numpy as np
import pytest

from minlz_amd import _lib
from tests import records_model as RM
from tests import search_host as H
from tests.search_host import both

SRC = "stream_records_check.cpp"
BIG = 1 << 40


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def rec_case(data, pat, delim, W, rec_cap=BIG, dst_cap=BIG, shift=0):
    return struct.pack("<IIIIIQQQ", 1, len(pat), W, delim[0], shift, rec_cap, dst_cap, len(data)) + pat + data


def parse(line):
    head, _, rest = line.partition(":")
    recs, _, wins = rest.partition("|")
    R, nbytes, occ, flagged, k, written, nw, wbytes = (int(v) for v in head.split())
    return dict(R=R, totals=(R, nbytes, occ, flagged), k=k, written=written, nw=nw, wbytes=wbytes,
                recs=[tuple(int(v) for v in r.split(":")) for r in recs.split()], wins=[tuple(int(v) for v in w.split(":")) for w in wins.split()])


def check(checkers, cases):
    """cases: (data, pat, delim, W, rec_cap, dst_cap); every case runs at three misalignments of the window buffer."""
    shifts = (0, 5, 15)
    lines = both(checkers, [rec_case(*c, shift=s) for c in cases for s in shifts])
    assert len(lines) == len(cases) * len(shifts)
    for ci, c in enumerate(cases):
        data, pat, delim, W, rec_cap, dst_cap = c
        want = RM.result(data, pat, delim, W, rec_cap, dst_cap)
        recs, _ = RM.records(data, pat, delim, W)
        wins = RM.windows(len(data), RM.occurrences(data, pat), len(pat), W)
        for si in range(len(shifts)):
            got = parse(lines[ci * len(shifts) + si])
            what = "case %d: %r in %d bytes, W %d, caps %d / %d" % (ci, pat, len(data), W, rec_cap, dst_cap)
            assert got["totals"] == want["totals"], what
            assert got["recs"] == recs, what
            assert got["k"] == want["k"] and got["written"] == len(want["dst"]), what
            assert got["wins"] == [(lo, hi - lo) for lo, hi in wins] and got["nw"] == len(wins) and got["wbytes"] == sum(hi - lo for lo, hi in wins), what
    return [RM.result(*c) for c in cases]


def test_sanitized_build_links(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizer runtimes: " + H.LINK_ERROR[SRC][-300:])
    assert shutil.which("g++")


def test_exported():
    L = _lib.lib()
    assert L.mlz_dev_reader_search_records and "mlz_dev_reader_search_records" in _lib.SYMBOLS


N = b"needle"
FILL = bytes(range(ord("a"), ord("z") + 1)) * 200   # no delimiter, no needle


def test_edges_of_the_stream(checkers):
    res = check(checkers, [
        (N + b" first\nmiddle\nlast " + N, N, b"\n", 64, BIG, BIG),        # an occurrence at 0 and at the last possible position
        (N, N, b"\n", 1, BIG, BIG),                                           # the stream is the pattern
        (FILL[:300] + N + FILL[:500], N, b"\n", RM.DEFAULT_REACH, BIG, BIG),               # no delimiter at all: one record, the stream, no flag
        (FILL[:300] + N + FILL[:500], N, b"\n", 100, BIG, BIG),               # ... and cut on both sides
        (b"\n" + N + b"\n", N, b"\n", 8, BIG, BIG),                           # the delimiter as first and as last byte
        (b"\n\n" + N + b"\n\n" + FILL[:20] + b"\n\n" + N + N + b"\n\n", N, b"\n", 50, BIG, BIG),   # doubled delimiters
        (FILL[:100] + b"\n" + FILL[:30] + N, N, b"\n", 64, BIG, BIG),         # ends without a delimiter
    ])
    assert res[0]["R"] == 2 and res[0]["rec_off"] == [0, 20] and res[0]["flags"] == [0, 0]
    assert res[2]["R"] == 1 and res[2]["flags"] == [0] and len(res[2]["dst"]) == 806
    assert res[3]["flags"] == [3] and len(res[3]["dst"]) == 206
    assert res[5]["R"] == 2 and res[5]["totals"][2] == 3


def test_occurrences_in_one_record(checkers):
    res = check(checkers, [
        (b"x\n" + N + b" and " + N + b"\ny\n", N, b"\n", 64, BIG, BIG),                     # two
        (b"x\n" + N + b" and " + N + b" and " + N + b"\ny\n" + N + b"\n", N, b"\n", 64, BIG, BIG),   # three, then one
        (b"b\naaaa\nb", b"aa", b"\n", 16, BIG, BIG),                                          # overlapping occurrences
        (b"aaaa", b"aa", b"\n", 1, BIG, BIG),
        (b"aaaaaaaaaaaa", b"aa", b"\n", 2, BIG, BIG),                                         # ... whose reach moves s with every occurrence
    ])
    assert res[0]["R"] == 1 and res[0]["totals"][2] == 2
    assert res[1]["R"] == 2 and res[1]["totals"][2] == 4
    assert res[2]["R"] == 1 and res[2]["totals"][2] == 3 and res[2]["dst"] == b"aaaa"


@pytest.mark.parametrize("a,b", [(40, 90), (90, 40), (70, 70), (0, 33), (33, 0), (1100, 2300)])
def test_reach_against_the_record_length(checkers, a, b):
    """A record of a bytes, the pattern and b bytes between two delimiters: the reach at, one below and one above every length that matters."""
    rec = FILL[:a] + N + FILL[5:5 + b]
    data = FILL[:2500] + b"\n" + rec + b"\n" + FILL[:2500]
    ws = sorted({w for base in (a, b, len(rec), 1) for w in (base - 1, base, base + 1, base + 2) if 1 <= w})
    res = check(checkers, [(data, N, b"\n", w, BIG, BIG) for w in ws])
    seen = set()
    for w, r in zip(ws, res):
        want = (0 if w >= a + 1 else 1) | (0 if w >= b + 1 else 2)
        assert r["flags"] == [want], (w, a, b)
        seen.add(want)
        if want == 0:
            assert r["dst"] == rec and r["rec_off"] == [2501]
    assert 0 in seen and (3 in seen or not (a and b))


def test_one_long_record_gives_two(checkers):
    rec = FILL[:50] + N + FILL[:194] + N + FILL[:44]
    data = b"head\n" + rec + b"\ntail"
    res = check(checkers, [
        (data, N, b"\n", 40, BIG, BIG),      # different s: two records, cut
        (data, N, b"\n", 120, BIG, BIG),     # ... that overlap
        (data, N, b"\n", 260, BIG, BIG),     # equal s (the delimiter): one record
    ])
    assert res[0]["R"] == 2 and res[0]["flags"] == [3, 3]
    assert res[1]["R"] == 2 and res[1]["rec_off"][1] < res[1]["rec_off"][0] + res[1]["rec_start"][1]
    assert res[2]["R"] == 1 and res[2]["dst"] == rec and res[2]["flags"] == [0]


def test_record_takes_the_later_end(checkers):
    """Two occurrences with one s where only the later one reaches the delimiter behind them."""
    rec = b"ab" + N + FILL[:12] + N + FILL[:10]
    far = b"ab" + N + FILL[:12] + N + FILL[:40]
    res = check(checkers, [(FILL[:100] + b"\n" + r + b"\n" + FILL[:100], N, b"\n", 24, BIG, BIG) for r in (rec, far)])
    assert res[0]["R"] == 1 and res[0]["totals"][2] == 2 and res[0]["dst"] == rec and res[0]["flags"] == [0]
    assert res[1]["R"] == 1 and res[1]["flags"] == [2] and res[1]["dst"] == far[:50]


def test_windows_touch_or_miss(checkers):
    W = 30
    for gap, nw in ((2 * W, 1), (2 * W + 1, 2), (2 * W - 1, 1)):
        data = FILL[:200] + N + FILL[:gap] + N + FILL[:200]
        (r,) = check(checkers, [(data, N, b"\n", W, BIG, BIG)])
        assert len(RM.windows(len(data), RM.occurrences(data, N), len(N), W)) == nw
        assert r["R"] == 2


def test_caps(checkers):
    lines = [b"one " + N, N + b" two two", b"none", b"three " + N + b" three", N]
    data = b"\n".join(lines) + b"\n"
    hits = [ln for ln in lines if N in ln]
    ends = np.cumsum([len(h) for h in hits]).tolist()
    cases = [(data, N, b"\n", 64, rc, BIG) for rc in (0, 1, 2, len(hits), len(hits) + 1)]
    cases += [(data, N, b"\n", 64, BIG, e + d) for e in ends for d in (-1, 0, 1)]
    cases += [(data, N, b"\n", 64, 0, 0), (data, N, b"\n", 64, 2, ends[0]), (data, N, b"\n", 64, 1, ends[2])]
    res = check(checkers, cases)
    assert [r["k"] for r in res[:5]] == [0, 1, 2, 4, 4]
    assert [r["k"] for r in res[5:17]] == [0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
    assert [r["k"] for r in res[17:]] == [0, 1, 1]
    assert all(r["R"] == 4 and r["totals"] == (4, ends[-1], 4, 0) for r in res)
    assert res[17]["dst"] == b"" and res[17]["rec_start"] == [0]


@pytest.mark.parametrize("alphabet", [b"ab\n", b"abcdefgh \n\n", bytes(range(256))])
def test_lines_that_hold_the_pattern(checkers, alphabet):
    """Not through the model: with a reach of at least the longest record the records are the lines that hold the pattern, with their offsets."""
    rng = np.random.default_rng(len(alphabet))
    cases, want = [], []
    for n in (1, 7, 300, 3000):
        data = bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])
        for plen in (1, 2, 3):
            pat = bytes(b for b in data[n // 3:] if b != 10)[:plen] or b"a"
            lines = data.split(b"\n")
            offs = np.cumsum([0] + [len(ln) + 1 for ln in lines]).tolist()
            W = max(len(ln) for ln in lines) + 1
            cases.append((data, pat, b"\n", W, BIG, BIG))
            want.append([(o, ln) for o, ln in zip(offs, lines) if pat in ln])
    out = both(checkers, [rec_case(*c) for c in cases])
    for c, w, line in zip(cases, want, out):
        got = parse(line)
        assert got["R"] == len(w) and got["totals"][3] == 0
        assert [(s, c[0][s:e]) for s, e, _ in got["recs"]] == w
