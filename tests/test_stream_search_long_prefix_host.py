"""The rules of the long-prefix search tables (table type 4) and of the search's plan over them without a GPU:
tools/stream_search_check.cpp runs the shared header minlz_amd/csrc/mlz_stream_search.h on the host (record kinds 10 and 11) and
tests/search_long_prefix_tables.py is the same specification in Python, written separately.  The two must agree, and the decoded set must
hold every chunk with a byte of a true occurrence."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from minlz_amd.api import search_long_prefix_config
from tests import search_cases as SC
from tests import search_long_prefix_cases as LC
from tests import search_long_prefix_tables as SL
from tests import search_prefix_tables as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sscl") / "ssc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "stream_search_check.cpp")], check=True)

    def run(records):
        path = exe.parent / "cases.bin"
        with open(path, "wb") as f:
            for r in records:
                f.write(r)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=900, check=True)
        os.unlink(path)
        return r.stdout.splitlines()
    return run


def rec_stream(stream, pattern, flags=0):
    return struct.pack("<IQII", 10, len(stream), len(pattern), flags) + stream + pattern


def rec_groups(M, field, pattern):
    return struct.pack("<IIII", 11, M, len(pattern), len(field)) + bytes(field) + pattern


def parse_stream_line(line):
    head, _, rest = line.partition(":")
    return tuple(int(v) for v in head.split()), [int(v) for v in rest.split()]      # (T, M, B, usable, ng, t_min, gsize), the plan


def test_exported():
    L = _lib.lib()
    assert L.mlz_stream_bound_long_prefix and L.mlz_stream_encode_gather_device_long_prefix
    assert {"mlz_stream_bound_long_prefix", "mlz_stream_encode_gather_device_long_prefix"} <= set(_lib.SYMBOLS)
    assert C.sizeof(_lib.SearchLongPrefix) == 264


def cfg(prefix=LC.USER, m=6, e=3, k=None, reserved=(0, 0, 0, 0)):
    c = _lib.SearchLongPrefix()
    c.match_len, c.extras, c.prefix_len = m, e, len(prefix) if k is None else k
    for i, v in enumerate(reserved):
        c.reserved[i] = v
    for i, v in enumerate(prefix):
        c.prefix[i] = v
    return c


def test_bound_and_arguments_on_the_host():
    """mlz_stream_bound_long_prefix needs no device: the sizes and every -MLZ_ERR_ARG case of the configuration."""
    L = _lib.lib()
    for bs in (4 << 10, 64 << 10, 2 << 20, 8 << 20):
        n = 3 * bs + 5
        B = SL.table_bits(bs)
        for idx in (0, 1):
            plain = L.mlz_stream_bound(n, bs, idx)
            for K in (1, 8, 9, 256):
                got = L.mlz_stream_bound_long_prefix(n, bs, idx, C.byref(cfg(b"x" * K)))
                assert got == plain + (7 + 2 + K) + 4 * (12 + 2 + K + max(32, 1 << (B - 3))), (bs, K)
    assert L.mlz_stream_bound_long_prefix(0, 4096, 0, C.byref(cfg())) == L.mlz_stream_bound(0, 4096, 0) + 7 + 2 + 8
    ok = [cfg(m=0, e=10), cfg(m=8, e=8), cfg(m=1, e=15), cfg(m=6, e=0), cfg(b"x" * 256), cfg(b"x")]
    for c in ok:
        assert L.mlz_stream_bound_long_prefix(1000, 4096, 0, C.byref(c)) > 0
    bad = [cfg(k=0), cfg(k=257), cfg(k=65535), cfg(m=9), cfg(m=200, e=0), cfg(m=8, e=9), cfg(m=0, e=11), cfg(m=2, e=15), cfg(m=1, e=16), cfg(e=255),
           cfg(reserved=(1, 0, 0, 0)), cfg(reserved=(0, 0, 0, 7))]
    for i, c in enumerate(bad):
        assert L.mlz_stream_bound_long_prefix(1000, 4096, 0, C.byref(c)) == -8, i
    assert L.mlz_stream_bound_long_prefix(1000, 4096, 0, None) == -8
    for flags in (4, 4 | 6 << 8, 6 << 8, 1 | 4):
        assert L.mlz_stream_bound_long_prefix(1000, 4096, flags, C.byref(cfg())) == -8
    assert L.mlz_stream_bound_long_prefix(1000, 1000, 0, C.byref(cfg())) == -8
    # the existing calls keep refusing type 4
    c4 = _lib.SearchTables()
    c4.table_type, c4.match_len = 4, 6
    assert L.mlz_stream_bound_tables(1000, 4096, 0, C.byref(c4)) == -8


def test_python_configuration():
    c = search_long_prefix_config(0, LC.USER, 3)
    assert (c.match_len, c.extras, c.prefix_len, bytes(c.prefix[:8]), bytes(c.reserved)) == (0, 3, 8, LC.USER, bytes(4))
    for args in ((6, b"", 0), (6, b"x" * 257, 0), (9, b"x", 0), (-1, b"x", 0), (6, b"x", 11), (0, b"x", 11), (6, b"x", 16), (6, b"x", -1)):
        with pytest.raises(ValueError):
            search_long_prefix_config(*args)


def test_groups_against_the_model(checker):
    rng = np.random.default_rng(31)
    prefixes = [b"a", b"aa", b"abab", b"ab", b"abc", b"abcabcab", b"abcabcabc", bytes(rng.choice(np.frombuffer(b"ab", np.uint8), 40)),
                bytes(rng.choice(np.frombuffer(b"abc", np.uint8), 200))]
    assert sorted({len(p) for p in prefixes}) == [1, 2, 3, 4, 8, 9, 40, 200]
    recs, want = [], []

    def add(M, E, pfx, pat):
        field = SL.field_of(pfx, E)
        recs.append(rec_groups(M, field, pat))
        G, t_min = SL.groups(pat, M, field)
        want.append(((t_min, E + 1) if G else None, [i + len(pfx) for i in G]))      # (t_min and the group size matter only where there is a group)
    for M in (1, 2, 4, 6, 8):
        for E in sorted({0, 3, 15 - M, 16 - M if M > 1 else 15}):
            for pfx in prefixes:
                K = len(pfx)
                for L in (1, K, K + M + E - 1, K + M + E, K + M + E + 1, 2 * K + M + E + 5, 100, 256):
                    if not 1 <= L <= 256:
                        continue
                    fill = bytes(rng.choice(np.frombuffer(b"abz", np.uint8), L))
                    add(M, E, pfx, fill)
                    b = bytearray(fill)                       # the prefix planted at 0, in the middle and where it is too late for a group
                    for o in (0, L // 2, L - K - M - E, L - K - M - E + 1):
                        if 0 <= o <= L - K:
                            b[o:o + K] = pfx
                            add(M, E, pfx, bytes(b))
    add(6, 3, b"aa", b"aaa" + b"z" * 9)          # two overlapping groups: i = 0 and 1
    add(6, 3, b"abab", b"zababab" + b"q" * 9)    # ... of a self-overlapping prefix, t_min = 0
    add(6, 0, b"a", b"a" * 256)                  # the most groups: 250
    add(1, 0, b"a", b"a" * 256)                  # 255
    got = []
    for line in checker(recs):
        head, _, rest = line.partition(":")
        t_min, gsize = (int(v) for v in head.split())
        W = [int(v) for v in rest.split()]
        got.append(((t_min, gsize) if W else None, W))
    assert got == want
    counts = [len(w) for _, w in want]
    assert 0 in counts and 1 in counts and 2 in counts and 255 in counts and {0, 1} == {t[0] for t, _ in want if t}
    assert want[-4] == ((1, 4), [2, 3]) and want[-3] == ((0, 4), [5, 7])


CONFIGS = [(LC.USER, 6, 3), (LC.USER, 6, 0), (b'":"', 8, 8), (b'"user":"u', 1, 15), (b", ", 4, 0), (b'"id":"', 2, 14)]


def _spliced(kind, bs, nblk, M, E, pfx, tail=777, level=1, **kw):
    d, pats = LC.designed(kind, bs, nblk, tail, M, E, pfx)
    field = SL.field_of(pfx, E)
    B = SL.table_bits(bs)
    sp, tables = SL.splice(O.stream_encode(d, level, bs), d, M, B, field, **kw)
    assert O.stream_decode(sp, len(d)) == d
    return d, pats, sp, tables, (4, M, B, field)


def _check_patterns(checker, d, sp, pats, what, model_stream=None):
    """The checker's plan over `sp` is the model's, and it holds every chunk with a byte of an occurrence."""
    T, M, B, field, tables = SL.read_tables(sp if model_stream is None else model_stream)
    sizes = [n for n, _ in SL.data_grid(sp)]
    everything = [k for k in range(len(sizes)) if sizes[k]]
    lines = checker([rec_stream(sp, p) for _, p in pats])
    n_tables = sum(t is not None for t in tables)
    out = {}
    for (name, p), line in zip(pats, lines):
        head, got = parse_stream_line(line)
        assert got == SL.plan(tables, sizes, p, T, M, B, field), (what, name)
        assert head[3] == SL.usable_tables(tables, p, T, M, field), (what, name, head)
        if T == 4:
            G, t_min = SL.groups(p, M, field)
            assert head[:3] == (T, M, B) and head[4] == (len(G) if n_tables else 0), (what, name, head)
            if G and n_tables:
                assert head[5:] == (t_min, field[1] + 1), (what, name, head)
            else:
                assert got == everything, (what, name)
        touched = SL.chunks_touched(sizes, SL.brute(d, p), len(p))
        assert touched <= set(got), (what, name, sorted(touched - set(got)))
        if not name.startswith("absent"):
            assert touched, (what, name)
        out[name] = (head, got)
    return out


@pytest.mark.parametrize("pfx,M,E", CONFIGS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_spliced_streams_decoded_set_holds_every_occurrence(checker, kind, pfx, M, E):
    bs, nblk = 64 << 10, 8
    d, pats, sp, tables, cfg4 = _spliced(kind, bs, nblk, M, E, pfx)
    res = _check_patterns(checker, d, sp, pats + SC.patterns(d, M, bs), (kind, pfx, M, E))
    everything = list(range(nblk + 1))
    assert res["late"][1] == everything and res["late"][0][3:5] == (0, 0)
    assert res["prefix_only"][1] == everything and res["prefix_only"][0][3:5] == (0, 0)
    n_tables = sum(t is not None for t in tables)
    if n_tables:
        assert res["p0"][0][4:6] == (1, 1) and res["inside"][0][4:6] == (1, 0) and res["two_groups"][0][4:6] == (2, 1)
    if M + E >= 6 and n_tables == nblk + 1:
        assert {0, 1} <= set(res["two_groups"][1]) and {1, 2} <= set(res["straddle"][1]) and {2, 3} <= set(res["ends_on_last"][1])
        assert len(res["absent_keyed"][1]) <= 2
    # MLZ_SEARCH_NO_TABLES
    head, got = parse_stream_line(checker([rec_stream(sp, pats[0][1], 1)])[0])
    assert head[3:5] == (0, 0) and got == everything


@pytest.mark.parametrize("bs,nblk,level", [(4 << 10, 40, 1), (1 << 20, 4, 2), (2 << 20, 4, 1)])
def test_other_block_sizes_and_levels(checker, bs, nblk, level):
    d, pats, sp, tables, cfg4 = _spliced("json_like", bs, nblk, 6, 3, LC.USER, level=level, skip=(2,))
    assert tables[2] is None and sum(t is not None for t in tables) == nblk
    _check_patterns(checker, d, sp, pats, (bs, level))


def test_user_prefix_figures(checker):
    """json_like, seed 2, 16 x 64 KiB + 777, prefix '"user":"', M = 6, E = 3: the set bits, the fold and the admitted chunks."""
    bs, nblk = 64 << 10, 16
    d = synth.json_like(bs * nblk + 777, 2).tobytes()
    field = SL.field_of(LC.USER, 3)
    sp, tables = SL.splice(O.stream_encode(d, 1, bs), d, 6, 16, field)
    assert all(t is not None for t in tables)
    for k in range(nblk):
        bits = len(set(SL.indexed_hashes(d[k * bs:(k + 1) * bs], d[(k + 1) * bs:(k + 1) * bs + 32], 16, 6, field).tolist()))
        assert 500 <= bits <= 900, (k, bits)
        assert tables[k][1] == 3 and len(tables[k][0]) == 1024, (k, tables[k][1])
    share = sum(12 + len(field) + len(t[0]) for t in tables) / len(d)
    assert share < 0.02
    head, got = parse_stream_line(checker([rec_stream(sp, LC.ABSENT_USER)])[0])
    assert head == (4, 6, 16, nblk + 1, 1, 0, 4) and len(got) <= 2
    at = d.find(LC.USER, 5 * bs + 1000)
    present = d[at - 3:at + 19]
    head, got = parse_stream_line(checker([rec_stream(sp, present)])[0])
    assert SL.chunks_touched([bs] * nblk + [777], SL.brute(d, present), 22) <= set(got) and len(got) < nblk


def test_table_verdicts(checker):
    """An info chunk with M + E = 17 or a field cut short: the stream has no configuration.  A table whose extras or one prefix byte differ
    and a type 2 table in a type 4 stream: that chunk has no table.  The plan stays the model's and holds every occurrence."""
    bs, nblk, M, E = 64 << 10, 6, 8, 8
    d, pats, sp, tables, (T, _, B, field) = _spliced("json_like", bs, nblk, M, E, LC.USER)
    K = len(LC.USER)
    sizes = [n for n, _ in SL.data_grid(sp)]
    everything = list(range(nblk + 1))
    assert all(t is not None for t in tables)
    base = _check_patterns(checker, d, sp, pats, "base")
    assert base["p0"][1] != everything
    ilen = 4 + 3 + 2 + K
    assert sp[10:10 + ilen] == SL.info_chunk(M, B, field)
    # M + E = 17 (in the info chunk alone, and in every chunk)
    bad_field = bytes([K - 1, 9]) + LC.USER
    every = SL.splice(O.stream_encode(d, 1, bs), d, M, B, bad_field)[0]
    for name, b in (("info E + 1", sp[:10] + SL.info_chunk(M, B, bad_field) + sp[10 + ilen:]), ("E = 9 everywhere", every),
                    ("short field", sp[:10] + SL.frame(SL.CHUNK_INFO, bytes([T, M, B]) + field[:5]) + sp[10 + ilen:]),
                    ("no extras byte", sp[:10] + SL.frame(SL.CHUNK_INFO, bytes([T, M, B, K - 1])) + sp[10 + ilen:])):
        assert O.stream_decode(b, len(d)) == d, name
        assert SL.read_tables(b)[0] is None, name
        res = _check_patterns(checker, d, b, pats, name)
        assert all(got == everything and head[:5] == (0, 0, 0, 0, 0) for head, got in res.values()), name
    # one table patched: its extras, one prefix byte; replaced by a type 2 table
    tabs = [c for c in SL.chunks_of(sp) if c[1] == SL.CHUNK_TABLE]
    p0 = dict(pats)["p0"]
    skipped = next(k for k in range(1, nblk) if k not in base["p0"][1])
    off, _, tn = tabs[skipped]
    t2 = list(tables); t2[skipped] = None
    tab2, R2 = SP.build_table(d[skipped * bs:(skipped + 1) * bs], d[(skipped + 1) * bs:(skipped + 1) * bs + 8], B, M, SP.mask_of(2, b"::::::::"))
    for name, b in (("extras", sp[:off + 8] + bytes([E - 1]) + sp[off + 9:]), ("prefix byte", sp[:off + 9 + 3] + b"t" + sp[off + 9 + 4:]),
                    ("last prefix byte", sp[:off + 9 + K - 1] + b"'" + sp[off + 9 + K:]),
                    ("type 2 table", sp[:off] + SP.table_chunk(tab2, R2, 2, M, B, b"::::::::") + sp[off + 4 + tn:])):
        assert O.stream_decode(b, len(d)) == d, name
        assert SL.read_tables(b)[4] == t2, name
        res = _check_patterns(checker, d, b, pats, name)
        assert res["p0"][0][3] == nblk and skipped in res["p0"][1], name
    # ... and with the right table behind the wrong one: found
    b = sp[:off] + SP.table_chunk(tab2, R2, 2, M, B, b"::::::::") + sp[off:]
    assert SL.read_tables(b)[4] == tables and _check_patterns(checker, d, b, pats, "both") == base


def test_the_two_models_agree_for_one_prefix_byte():
    """K = 1, E = 0 is table type 2 with that one value: the same table bytes and R for every block."""
    bs, nblk = 64 << 10, 8
    d = synth.json_like(bs * nblk, 3).tobytes()
    for M in (1, 2, 6, 8):
        for v in (b":", b'"', b"e"):
            field = SL.field_of(v, 0)
            mask = SP.mask_of(2, v * 8)
            for k in range(nblk):
                blk = d[k * bs:(k + 1) * bs]
                follow = d[(k + 1) * bs:(k + 1) * bs + 8] if k + 1 < nblk else None
                assert SL.build_table(blk, follow, 16, M, field) == SP.build_table(blk, follow, 16, M, mask), (M, v, k)


def test_model_block_rules():
    """The indexed starts, written out: block borders, the last block's limit and a prefix that would run beyond the stream's end."""
    f = SL.field_of(b"ab", 1)              # K = 2, M = 3, E = 1: the last block indexes the starts 0 .. n - 6
    M = 3
    assert SL.indexed_starts(b"zzzzzzzab", b"cdefgh", M, f) == [7]
    assert SL.indexed_starts(b"zzzzzzzza", b"bcdefg", M, f) == [8]                 # the prefix straddles the border: it belongs to this block
    assert SL.indexed_starts(b"bzzzzzzzz", b"zzzzzz", M, f) == []                  # ... and not to the next one
    assert SL.indexed_starts(b"zzzabcdef", None, M, f) == [3] and SL.indexed_starts(b"zzzzabcde", None, M, f) == []
    assert SL.indexed_starts(b"abcde", None, M, f) == [] and SL.indexed_starts(b"abcdef", None, M, f) == [0]
    assert SL.indexed_starts(b"aaaa", b"aaaaaa", M, SL.field_of(b"aa", 1)) == [0, 1, 2, 3]
    assert SL.indexed_starts(b"zzz\0", b"", M, SL.field_of(b"\0\0", 1)) == []      # zeros beyond the end are no prefix bytes
    assert SL.indexed_starts(b"zzz\0", b"\0", M, SL.field_of(b"\0\0", 1)) == [3]
    # the windows of a start near the end take zeros beyond the stream
    h = SL.indexed_hashes(b"zzzzzzzab", b"c", 16, M, f)
    want = SL.hash_windows(np.frombuffer(b"c\0\0\0", np.uint8), 16, M)
    assert h.tolist() == want.tolist()
