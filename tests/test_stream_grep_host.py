"""The grep over the record index without a GPU: tools/stream_grep_check.cpp runs the rules the call shares with its kernels
(minlz_amd/csrc/mlz_stream_grep.h: the mark rule with the narrowed bisection against the full one, the tail mask, the context rule from the
two scans, ranks, the cap cut and the byte sums) as plain loops, plain and under AddressSanitizer and UBSan, and tests/grep_model.py —
bytes.split and set arithmetic — says what must come out."""
import shutil
import struct

import numpy as np
import pytest

from minlz_amd import _lib
from tests import grep_model as GM
from tests import record_index_model as IM
from tests import search_host as H
from tests.search_host import both

SRC = "stream_grep_check.cpp"
NL = b"\n"
INVERT = 16
BIG = 1 << 40


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def occurrences(data, pattern):
    out, at = [], data.find(pattern)
    while at >= 0:
        out.append(at)
        at = data.find(pattern, at + 1)
    return out


def grep_case(data, pattern, invert, before, after, rec_cap, tile=16384):
    D = IM.delimiters(data, NL)
    pos = occurrences(data, pattern)
    return (struct.pack("<IIIQQQQQQ", 1, INVERT if invert else 0, tile, len(data), len(D), len(pos), before, after, rec_cap) + D.astype(np.uint64).tobytes() +
            np.asarray(pos, np.uint64).tobytes())


def parse(line):
    head, _, rest = line.partition(":")
    no, kinds = rest.split("|")
    R, S, written, nbytes, atomics = (int(v) for v in head.split())
    return dict(totals=(R, S, written, nbytes), atomics=atomics, numbers=[int(v) for v in no.split()], kinds=[int(v) for v in kinds.split()])


def build(N, selected, ends_with_delim=True, hot=1):
    """N records of 0 .. 2 filler bytes; the selected ones hold `hot` occurrences of b"x".  Without a closing delimiter the last record
    must have a byte, or it would not exist."""
    sel = set(selected)
    recs = [b"q" * (r % 3) + (b"x" * hot if r in sel else b"") for r in range(N)]
    if N and not ends_with_delim and not recs[-1]:
        recs[-1] = b"q"
    data = NL.join(recs) + (NL if N and ends_with_delim else b"")
    assert len(GM.records(data, NL)) == N
    return data


def check(checkers, cases):
    """cases: (data, invert, before, after, rec_cap) -> the parsed results, each compared whole with the model."""
    lines = both(checkers, [grep_case(d, b"x", inv, b, a, cap) for d, inv, b, a, cap in cases])
    assert len(lines) == len(cases)
    out = []
    for line, (d, inv, b, a, cap) in zip(lines, cases):
        got, want = parse(line), GM.result(d, NL, [b"x"], inv, b, a, cap)
        what = "N %d, invert %s, before %d, after %d, cap %d" % (want["N"], inv, b, a, cap)
        assert got["totals"] == want["totals"], what
        assert got["numbers"] == want["numbers"] and got["kinds"] == want["kinds"], what
        assert got["atomics"] == len(want["M"]), what
        out.append(got)
    return out


def test_sanitized_build_links(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizer runtimes: " + H.LINK_ERROR[SRC][-300:])
    assert shutil.which("g++")


def test_exported():
    L = _lib.lib()
    assert getattr(L, "mlz_dev_reader_grep_records") and "mlz_dev_reader_grep_records" in _lib.SYMBOLS


def test_smears_and_tail_mask(checkers):
    assert both(checkers, [struct.pack("<I", 2)]) == ["smear ok"]


def selections(N):
    """Selected records at 0, 31, 32, 63 and N - 1 (as far as they exist), alone and together; none; every record."""
    marks = [r for r in (0, 31, 32, 63, N - 1) if 0 <= r < N]
    sets = [[], list(range(N)), sorted(set(marks))] + [[r] for r in sorted(set(marks))]
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


@pytest.mark.parametrize("N", [0, 1, 31, 32, 33, 64, 65])
def test_small_counts(checkers, N):
    """Every context size against every selection, with and without invert (N % 32 == 0 and == 1 among them), both stream endings."""
    cases = []
    for sel in selections(N):
        for ends in (True, False):
            d = build(N, sel, ends)
            for inv in (False, True):
                for reach in (0, 1, 3, 31, 32, 33, N, BIG):
                    cases += [(d, inv, reach, 0, BIG), (d, inv, 0, reach, BIG), (d, inv, reach, reach, BIG)]
    check(checkers, cases)


def test_contexts_touch_overlap_and_run_off_the_ends(checkers):
    d = build(200, [2, 10, 14, 15, 40, 47, 100, 133, 197])
    cases = [(d, False, 3, 3, BIG),       # 10 and 14: touch (11..13 | 11..13); 14 and 15 neighbours; 2 and 197 run off both ends
             (d, False, 3, 4, BIG),       # 40 and 47: 41..44 | 44..46 overlap in 44
             (d, False, 2, 2, BIG),       # 40 and 47 apart: 43 and 44 stay out
             (d, False, 33, 0, BIG), (d, False, 0, 33, BIG), (d, False, 64, 64, BIG), (d, False, 1000, 1000, BIG)]
    res = check(checkers, cases)
    assert 43 not in res[2]["numbers"] and 44 not in res[2]["numbers"] and 44 in res[1]["numbers"] and res[0]["numbers"][:6] == [0, 1, 2, 3, 4, 5]
    assert res[6]["totals"][0] == 200 and sum(res[6]["kinds"]) == 9


def test_the_cut_at_the_cap(checkers):
    d = build(100, [5, 50, 95], hot=3)
    R = GM.result(d, NL, [b"x"], False, 2, 2)["R"]
    assert R == 15
    res = check(checkers, [(d, False, 2, 2, cap) for cap in (0, 1, R - 1, R, R + 1, BIG)] + [(d, True, 0, 0, cap) for cap in (0, 7, 97, 98)])
    assert [len(r["numbers"]) for r in res] == [0, 1, R - 1, R, R, R, 0, 7, 97, 97]
    assert res[0]["totals"][2] == 0 and res[3]["totals"][2] == res[3]["totals"][3] > 0


def test_many_records(checkers):
    """70 000 records: 69 words per lane and a ragged last slab; a hot record (one atomic for thousands of occurrences); tiles of several
    sizes, so that the narrowed bisection sees tiles with one record, with many and with none."""
    N = 70000
    rng = np.random.default_rng(5)
    sparse = sorted(set(rng.integers(0, N, 40).tolist()) | {0, 31, 32, 63, N - 1})
    d = build(N, sparse)
    hot = build(N, [7, 40000], hot=3000)
    every = build(N, range(N))
    none = build(N, [])
    cases = [(d, False, 0, 0, BIG), (d, True, 0, 0, BIG), (d, False, 3, 3, BIG), (d, False, 33, 31, BIG), (d, False, N, N, BIG), (d, False, BIG, 0, 100),
             (d, True, 1, 0, 5000), (hot, False, 1, 1, BIG), (every, False, 0, 0, BIG), (every, True, 5, 5, BIG), (none, False, 5, 5, BIG), (none, True, 0, 0, BIG),
             (none, True, BIG, BIG, 70001)]
    res = check(checkers, cases)
    assert res[7]["atomics"] == 2 and res[8]["totals"][:2] == (N, N) and res[9]["totals"][0] == 0 and res[11]["totals"][:2] == (N, N)
    lines = both(checkers, [grep_case(hot, b"x", False, 0, 0, BIG, tile) for tile in (1, 7, 4096, 1 << 20)])
    assert [parse(ln)["numbers"] for ln in lines] == [[7, 40000]] * 4


def test_model_by_hand():
    """The model's own words on lines that can be counted by hand."""
    data = b"ab\n\ncab\nzz\nb\n\nlast"
    assert GM.records(data, NL) == [b"ab", b"", b"cab", b"zz", b"b", b"", b"last"]
    r = GM.result(data, NL, [b"ab"])
    assert (r["M"], r["numbers"], r["kinds"], r["totals"]) == ([0, 2], [0, 2], [1, 1], (2, 2, 5, 5))
    r = GM.result(data, NL, [b"ab", b"zz"], invert=True)
    assert r["S"] == [1, 4, 5, 6] and r["totals"] == (4, 4, 5, 5)          # the empty records are selected under invert
    r = GM.result(data, NL, [b"zz"], before=1, after=2, rec_cap=3)
    assert (r["C"], r["numbers"], r["kinds"], r["totals"]) == ([2, 3, 4, 5], [2, 3, 4], [0, 1, 0], (4, 1, 6, 6))
    assert GM.result(data, NL, [], invert=True)["R"] == 7 and GM.result(data, NL, [])["R"] == 0
    assert GM.result(b"", NL, [b"x"], invert=True)["totals"] == (0, 0, 0, 0)
    assert GM.lines(data, NL, [2, 3, 4]) == (b"cabzzb", [0, 3, 5, 6])
