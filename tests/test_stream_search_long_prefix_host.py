"""The rules of the long-prefix search tables (table type 4) and of the search's plan over them without a GPU:
tools/stream_search_check.cpp runs the shared header minlz_amd/csrc/mlz_stream_search.h on the host (record kinds 10 and 11) and
tests/search_model.py is the same specification in Python, written separately.  The two must agree, and the decoded set must
hold every chunk with a byte of a true occurrence."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from minlz_amd.api import search_long_prefix_config
from tests import search_cases as SC
from tests import search_long_prefix_cases as LC
from tests import search_model as SMod
from tests.search_host import build_checker, parse_stream_line, rec_groups, rec_stream


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    run = build_checker(tmp_path_factory, "stream_search_check.cpp")
    return lambda records: run(records)[0]


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
        B = SMod.table_bits(bs)
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
        cfg4 = SMod.config(4, M, pfx, E)
        recs.append(rec_groups(M, cfg4[2], pat))
        G, t_min = SMod.groups(pat, cfg4)
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
    field = SMod.config(4, M, pfx, E)[2]
    B = SMod.table_bits(bs)
    sp, tables = SMod.splice(O.stream_encode(d, level, bs), d, (4, M, field), B, **kw)
    assert O.stream_decode(sp, len(d)) == d
    return d, pats, sp, tables, (4, M, B, field)


def _check_patterns(checker, d, sp, pats, what, model_stream=None):
    """The checker's plan over `sp` is the model's, and it holds every chunk with a byte of an occurrence."""
    cfg, B, tables = SMod.read_tables(sp if model_stream is None else model_stream)
    T, M, field = cfg or (None, None, b"")
    sizes = [n for n, _ in SMod.data_grid(sp)]
    everything = [k for k in range(len(sizes)) if sizes[k]]
    lines = checker([rec_stream(10, sp, p) for _, p in pats])
    n_tables = sum(t is not None for t in tables)
    out = {}
    for (name, p), line in zip(pats, lines):
        head, got = parse_stream_line(line)
        assert got == SMod.plan(tables, sizes, p, cfg, B), (what, name)
        assert head[3] == SMod.usable_tables(tables, p, cfg), (what, name, head)
        if T == 4:
            G, t_min = SMod.groups(p, cfg)
            assert head[:3] == (T, M, B) and head[4] == (len(G) if n_tables else 0), (what, name, head)
            if G and n_tables:
                assert head[5:] == (t_min, field[1] + 1), (what, name, head)
            else:
                assert got == everything, (what, name)
        touched = SMod.chunks_touched(sizes, SMod.brute(d, p), len(p))
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
    head, got = parse_stream_line(checker([rec_stream(10, sp, pats[0][1], 1)])[0])
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
    cfg4 = SMod.config(4, 6, LC.USER, 3)
    field = cfg4[2]
    sp, tables = SMod.splice(O.stream_encode(d, 1, bs), d, cfg4, 16)
    assert all(t is not None for t in tables)
    for k in range(nblk):
        bits = len(set(SMod.indexed_hashes(cfg4, d[k * bs:(k + 1) * bs], d[(k + 1) * bs:(k + 1) * bs + 32], 16).tolist()))
        assert 500 <= bits <= 900, (k, bits)
        assert tables[k][1] == 3 and len(tables[k][0]) == 1024, (k, tables[k][1])
    share = sum(12 + len(field) + len(t[0]) for t in tables) / len(d)
    assert share < 0.02
    head, got = parse_stream_line(checker([rec_stream(10, sp, LC.ABSENT_USER)])[0])
    assert head == (4, 6, 16, nblk + 1, 1, 0, 4) and len(got) <= 2
    at = d.find(LC.USER, 5 * bs + 1000)
    present = d[at - 3:at + 19]
    head, got = parse_stream_line(checker([rec_stream(10, sp, present)])[0])
    assert SMod.chunks_touched([bs] * nblk + [777], SMod.brute(d, present), 22) <= set(got) and len(got) < nblk


def test_table_verdicts(checker):
    """An info chunk with M + E = 17 or a field cut short: the stream has no configuration.  A table whose extras or one prefix byte differ
    and a type 2 table in a type 4 stream: that chunk has no table.  The plan stays the model's and holds every occurrence."""
    bs, nblk, M, E = 64 << 10, 6, 8, 8
    d, pats, sp, tables, (T, _, B, field) = _spliced("json_like", bs, nblk, M, E, LC.USER)
    K = len(LC.USER)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    everything = list(range(nblk + 1))
    assert all(t is not None for t in tables)
    base = _check_patterns(checker, d, sp, pats, "base")
    assert base["p0"][1] != everything
    ilen = 4 + 3 + 2 + K
    assert sp[10:10 + ilen] == SMod.info_chunk((4, M, field), B)
    # M + E = 17 (in the info chunk alone, and in every chunk)
    bad_field = bytes([K - 1, 9]) + LC.USER
    every = SMod.splice(O.stream_encode(d, 1, bs), d, (4, M, bad_field), B)[0]
    for name, b in (("info E + 1", sp[:10] + SMod.info_chunk((4, M, bad_field), B) + sp[10 + ilen:]), ("E = 9 everywhere", every),
                    ("short field", sp[:10] + SMod.frame(SMod.CHUNK_INFO, bytes([T, M, B]) + field[:5]) + sp[10 + ilen:]),
                    ("no extras byte", sp[:10] + SMod.frame(SMod.CHUNK_INFO, bytes([T, M, B, K - 1])) + sp[10 + ilen:])):
        assert O.stream_decode(b, len(d)) == d, name
        assert SMod.read_tables(b)[0] is None, name
        res = _check_patterns(checker, d, b, pats, name)
        assert all(got == everything and head[:5] == (0, 0, 0, 0, 0) for head, got in res.values()), name
    # one table patched: its extras, one prefix byte; replaced by a type 2 table
    tabs = [c for c in SMod.chunks_of(sp) if c[1] == SMod.CHUNK_TABLE]
    p0 = dict(pats)["p0"]
    skipped = next(k for k in range(1, nblk) if k not in base["p0"][1])
    off, _, tn = tabs[skipped]
    t2 = list(tables); t2[skipped] = None
    tab2, R2 = SMod.build_table((2, M, b"::::::::"), d[skipped * bs:(skipped + 1) * bs], d[(skipped + 1) * bs:(skipped + 1) * bs + 8], B)
    for name, b in (("extras", sp[:off + 8] + bytes([E - 1]) + sp[off + 9:]), ("prefix byte", sp[:off + 9 + 3] + b"t" + sp[off + 9 + 4:]),
                    ("last prefix byte", sp[:off + 9 + K - 1] + b"'" + sp[off + 9 + K:]),
                    ("type 2 table", sp[:off] + SMod.table_chunk((2, M, b"::::::::"), B, tab2, R2) + sp[off + 4 + tn:])):
        assert O.stream_decode(b, len(d)) == d, name
        assert SMod.read_tables(b)[2] == t2, name
        res = _check_patterns(checker, d, b, pats, name)
        assert res["p0"][0][3] == nblk and skipped in res["p0"][1], name
    # ... and with the right table behind the wrong one: found
    b = sp[:off] + SMod.table_chunk((2, M, b"::::::::"), B, tab2, R2) + sp[off:]
    assert SMod.read_tables(b)[2] == tables and _check_patterns(checker, d, b, pats, "both") == base


def test_the_two_models_agree_for_one_prefix_byte():
    """K = 1, E = 0 is table type 2 with that one value: the same table bytes and R for every block."""
    bs, nblk = 64 << 10, 8
    d = synth.json_like(bs * nblk, 3).tobytes()
    for M in (1, 2, 6, 8):
        for v in (b":", b'"', b"e"):
            cfg4, cfg2 = SMod.config(4, M, v, 0), SMod.config(2, M, v)
            for k in range(nblk):
                blk = d[k * bs:(k + 1) * bs]
                follow = d[(k + 1) * bs:(k + 1) * bs + 8] if k + 1 < nblk else None
                assert SMod.build_table(cfg4, blk, follow, 16) == SMod.build_table(cfg2, blk, follow, 16), (M, v, k)


def test_model_block_rules():
    """The indexed starts, written out: block borders, the last block's limit and a prefix that would run beyond the stream's end."""
    f = SMod.config(4, 3, b"ab", 1)             # K = 2, M = 3, E = 1: the last block indexes the starts 0 .. n - 6
    assert SMod.indexed_starts(f, b"zzzzzzzab", b"cdefgh") == [7]
    assert SMod.indexed_starts(f, b"zzzzzzzza", b"bcdefg") == [8]                 # the prefix straddles the border: it belongs to this block
    assert SMod.indexed_starts(f, b"bzzzzzzzz", b"zzzzzz") == []                  # ... and not to the next one
    assert SMod.indexed_starts(f, b"zzzabcdef", None) == [3] and SMod.indexed_starts(f, b"zzzzabcde", None) == []
    assert SMod.indexed_starts(f, b"abcde", None) == [] and SMod.indexed_starts(f, b"abcdef", None) == [0]
    assert SMod.indexed_starts(SMod.config(4, 3, b"aa", 1), b"aaaa", b"aaaaaa") == [0, 1, 2, 3]
    assert SMod.indexed_starts(SMod.config(4, 3, b"\0\0", 1), b"zzz\0", b"") == []      # zeros beyond the end are no prefix bytes
    assert SMod.indexed_starts(SMod.config(4, 3, b"\0\0", 1), b"zzz\0", b"\0") == [3]
    # the windows of a start near the end take zeros beyond the stream
    h = SMod.indexed_hashes(f, b"zzzzzzzab", b"c", 16)
    want = SMod.hash_windows(np.frombuffer(b"c\0\0\0", np.uint8), 16, 3)
    assert h.tolist() == want.tolist()
