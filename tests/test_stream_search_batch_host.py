"""mlz_stream_search_batch_device without a GPU: tools/stream_search_batch_check.cpp runs the host code the call shares with its kernels
(minlz_amd/csrc/mlz_stream_search_batch.h: the virtual positions, batch_stream_of, the tiles' streams, the count rule; mlz_stream_search.h:
the layout, the pattern index and the scan rule of one tile) and the Python model (tests/search_batch_model.py) says what must come out:
every stream's own brute-force pairs as triples in (stream, position, pattern) order, the streams' counts and the presence rows."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from minlz_amd import _lib
from tests import search_batch_model as BM
from tests import search_host as H
from tests.test_stream_search_many_host import LENGTHS, _pattern_sets, _two_letter, rec_patterns

SRC = "stream_search_batch_check.cpp"
GROUPS = [1, 50, 1000, 20000]


HEADER = "minlz_hip_search_batch.h"


def test_exported(tmp_path):
    """The library exports the symbol; include/minlz_hip_search_batch.h declares it and nothing else, with as many parameters as its entry in
    _lib.ABI_EXT has argument types; the header compiles as C99 on its own (it includes minlz_hip.h), as cgo would compile it."""
    L = _lib.lib()
    assert L.mlz_stream_search_batch_device
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == ["mlz_stream_search_batch_device"]
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert restype is _lib.i64 and len(argtypes) == params.count(",") + 1 == 18 and name not in _lib.ABI
    src = tmp_path / "client.c"
    src.write_text('#include "%s"\nint main(void) { return mlz_stream_search_batch_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == -MLZ_ERR_ARG ? 0 : 1; }\n' % HEADER)
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (n_patterns == 0 is refused before any device call: no GPU is needed)


def rec_batch(chunk_sizes, pats, datas, group_bytes):
    """chunk_sizes: per stream its chunks' decoded sizes; datas: per stream its bytes."""
    assert all(sum(c) == len(d) for c, d in zip(chunk_sizes, datas))
    out = [struct.pack("<IIQ", len(chunk_sizes), len(pats), group_bytes)]
    for c in chunk_sizes:
        out.append(struct.pack("<I", len(c)) + np.asarray(c, np.uint64).tobytes())
    return b"".join(out) + rec_patterns(pats) + b"".join(datas)


def parse(line, n_patterns):
    head, _, rest = line.partition(":")
    total, tiles, groups, bad_tiles = (int(v) for v in head.split())
    trip, counts, rows = rest.split("|")
    triples = [tuple(int(x) for x in v.split(":")) for v in trip.split()]
    rows = [[int(w, 16) for w in r.split(",")] for r in rows.split()]
    present = [{p for p in range(n_patterns) if (row[p >> 5] >> (p & 31)) & 1} for row in rows]
    return dict(total=total, tiles=tiles, groups=groups, bad_tiles=bad_tiles, triples=triples, counts=[int(v) for v in counts.split()], present=present)


def _random_case(rng, pats, n=None, big=9000, nck_max=8):
    lmin, lmax = min(len(p) for p in pats), max(len(p) for p in pats)
    small = [0, 1, max(0, lmin - 1), lmin, max(1, lmax - 1), lmax]
    n = int(rng.integers(1, 9)) if n is None else n
    chunk_sizes = []
    for i in range(n):
        kind = rng.integers(0, 4)
        if kind == 0:                                                           # a stream of 0, 1, lmin - 1, lmin, lmax - 1 or lmax bytes
            s = int(rng.choice(small))
            chunk_sizes.append([s] if s or rng.random() < 0.5 else [])
        elif kind == 1:                                                         # ... in several tiny chunks
            chunk_sizes.append(rng.choice([0, 1, 2, 5], int(rng.integers(1, 6))).tolist())
        else:                                                                   # a large one
            chunk_sizes.append(rng.choice(small + [100, 700, big], int(rng.integers(1, nck_max))).tolist())
    datas = []
    for c in chunk_sizes:
        d = bytearray(_two_letter(rng, sum(c)))
        for p in pats:
            if len(p) > 7 and len(d) >= len(p):                                 # long ones are planted: two letters alone would never hold them
                for _ in range(2):
                    o = int(rng.integers(0, len(d) - len(p) + 1))
                    d[o:o + len(p)] = p
        datas.append(bytes(d))
    group = int(rng.choice(GROUPS))
    return rec_batch(chunk_sizes, pats, datas, group), BM.result(datas, pats), (n, lmin, lmax, group, len(pats))


def _border_cases(rng):
    """Stream i ends with the first half of a pattern and stream i + 1 starts with the second half: not found.  The same bytes across a
    chunk border inside one stream: found.  Filler letters that no pattern holds, so every occurrence is a designed one."""
    out = []
    for L, h in ((2, 1), (3, 1), (3, 2), (7, 3), (16, 8), (40, 39), (256, 1), (256, 128), (256, 255)):
        p = _two_letter(rng, L)
        others = [_two_letter(rng, 1), p[:h], p[h:]]                            # (the halves themselves are patterns too: they are found where they lie)
        pats = [p] + [q for q in others if q]
        fill = lambda k: bytes(rng.integers(99, 101, k, dtype=np.uint8))        # 'c', 'd'
        a, b = p[:h], p[h:]
        long_a, long_b = fill(5000) + a, b + fill(5000)
        streams = [
            ([len(long_a)], long_a), ([len(long_b)], long_b),                   # long neighbours
            ([len(a)], a), ([len(b)], b),                                       # the halves alone: one-byte neighbours where h or L - h is 1
            ([], b""),                                                          # an empty stream between two halves
            ([len(a)], a), ([], b""), ([0], b""), ([len(b)], b),
            ([300 + len(a), len(b) + 300], fill(300) + p + fill(300)),          # across a chunk border inside one stream: found
            ([len(a), len(b)], p),                                              # ... a stream that is nothing but the pattern, in two chunks
            ([300, len(a), 0, len(b), 7], fill(300) + p + fill(7)),             # ... with an empty chunk in the border
        ]
        for group in GROUPS:
            cs, ds = [s[0] for s in streams], [s[1] for s in streams]
            want = BM.result(ds, pats)
            # the designed answer, apart from the model: pattern 0 occurs in the last three streams only, once each
            assert [c for c in (sum(1 for t in want["triples"] if t[0] == i and t[2] == 0) for i in range(len(ds)))] == [0] * 9 + [1, 1, 1]
            out.append((rec_batch(cs, pats, ds, group), want, (len(ds), min(map(len, pats)), L, group, len(pats))))
    return out


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(41)
    recs, want, meta = [], [], []

    def add(r, w, m):
        recs.append(r); want.append(w); meta.append(m)
    for pats in _pattern_sets(rng):                                             # the sets of the layout test: mixed lengths, prefixes, duplicates
        for _ in range(2):
            add(*_random_case(rng, pats))
    pats = [_two_letter(rng, int(L)) for L in rng.choice([2, 3, 7, 16], 4096)]  # one set of 4096 patterns
    add(*_random_case(rng, pats, n=5, big=700, nck_max=5))
    for c in _border_cases(rng):
        add(*c)
    return recs, want, meta


def _check(lines, want, meta):
    assert len(lines) == len(want)
    several = 0
    for line, w, m in zip(lines, want, meta):
        got = parse(line, m[4])
        assert got["bad_tiles"] == 0, m                                          # no tile's [gpos, gpos + hi_end) holds a hole byte
        assert got["total"] == w["total"] and got["triples"] == w["triples"], m
        assert got["counts"] == w["counts"] and got["present"] == w["present"], m
        several += got["groups"] > 2
    return several


def test_batch_layout_finds_what_brute_force_finds_per_stream(tmp_path_factory, cases):
    """Streams of 0, 1, lmin - 1, lmin, lmax - 1 and lmax bytes next to large ones, groups of 1 to 20000 bytes (streams cross many group
    borders, and many streams share a group), dense two-letter data, the layout test's pattern sets and one of 4096 patterns, the designed
    stream borders: triples in (stream, position, pattern) order, each once; counts from the prefix; presence by tile_stream."""
    recs, want, meta = cases
    lines = H.build_checker(tmp_path_factory, SRC)(recs)[0]
    assert _check(lines, want, meta) > 40
    assert len(recs) > 250 and sum(w["total"] for w in want) > 20000 and max(m[4] for m in meta) == 4096
    assert {m[1] for m in meta} >= {1, 2, 3, 7} and {m[2] for m in meta} >= set(LENGTHS[3:])
    assert any(0 in w["counts"] and max(w["counts"]) > 100 for w in want)


def test_batch_layout_under_the_sanitizers(tmp_path_factory, cases):
    """The check tool built once with -fsanitize=address,undefined, on the same case file: no read outside the staged bytes of a tile, the
    pattern blob, the index or the n + 1 virtual bases."""
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    recs, want, meta = cases
    lines, err = run(recs)
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check(lines, want, meta)
