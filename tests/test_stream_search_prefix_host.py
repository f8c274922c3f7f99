"""The rules of the prefix search tables (table types 2 and 3) and of the search's plan over them without a GPU:
tools/stream_search_check.cpp runs the shared header minlz_amd/csrc/mlz_stream_search.h on the host (record kinds 6 to 9) and
tests/search_model.py is the same specification in Python, written separately.  The two must agree, and the decoded set must hold
every chunk with a byte of a true occurrence."""
import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib
from tests import search_cases as SC
from tests import search_model as SMod
from tests import search_prefix_cases as PC
from tests.search_host import build_checker, parse_stream_line, rec_reduce, rec_rule, rec_stream, rec_windows

TYPES = (1, 2, 3)        # what a search of record kind 6 knows


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    run = build_checker(tmp_path_factory, "stream_search_check.cpp")
    return lambda records: run(records)[0]


def test_exported():
    L = _lib.lib()
    assert L.mlz_stream_bound_tables and L.mlz_stream_encode_gather_device_tables
    assert {"mlz_stream_bound_tables", "mlz_stream_encode_gather_device_tables"} <= set(_lib.SYMBOLS)


def test_bound_and_arguments_on_the_host():
    """mlz_stream_bound_tables needs no device: the sizes and every -MLZ_ERR_ARG case of the configuration."""
    L = _lib.lib()
    import ctypes as C

    def cfg(T, m=6, n=1, reserved=0):
        c = _lib.SearchTables()
        c.table_type, c.match_len, c.n_prefix, c.reserved = T, m, n, reserved
        return c
    for bs in (4 << 10, 64 << 10, 8 << 20):
        n = 3 * bs + 5
        B = SMod.table_bits(bs)
        plain = L.mlz_stream_bound(n, bs, 0)
        assert L.mlz_stream_bound_tables(n, bs, 0, None) == plain and L.mlz_stream_bound_tables(n, bs, 5, None) == L.mlz_stream_bound(n, bs, 5)
        for T, f in ((1, 0), (2, 8), (3, 32)):
            assert L.mlz_stream_bound_tables(n, bs, 0, C.byref(cfg(T))) == plain + 7 + f + 4 * (12 + f + max(32, 1 << (B - 3)))
        assert L.mlz_stream_bound_tables(n, bs, 0, C.byref(cfg(1))) == L.mlz_stream_bound(n, bs, 4)
    bad = [cfg(0), cfg(4), cfg(2, m=9), cfg(2, n=0), cfg(2, n=9), cfg(3, reserved=1), cfg(1, m=200)]
    for c in bad:
        assert L.mlz_stream_bound_tables(1000, 4096, 0, C.byref(c)) == -8
    for flags in (4, 4 | 6 << 8, 6 << 8, 1 | 4):
        assert L.mlz_stream_bound_tables(1000, 4096, flags, C.byref(cfg(2))) == -8
    assert L.mlz_stream_bound_tables(1000, 4096, 1, C.byref(cfg(2, n=8))) > 0 and L.mlz_stream_bound_tables(1000, 4096, 0, C.byref(cfg(3, n=77))) > 0
    assert L.mlz_stream_bound_tables(1000, 1000, 0, C.byref(cfg(2))) == -8


def test_windows_against_the_model(checker):
    rng = np.random.default_rng(21)
    recs, want = [], []
    for case in range(300):
        L = int(rng.choice([1, 2, 5, 6, 7, 9, 16, 40, 256]))
        M = int(rng.integers(1, 9))
        pset = bytes(rng.choice(256, int(rng.choice([0, 1, 3, 8, 9, 100])), replace=False).astype(np.uint8))
        T, field = SMod.field_of(pset)
        if case % 7 == 0:
            T, field = 1, b""
        pat = bytes(rng.choice(np.frombuffer(pset + b"ab", np.uint8), L)) if case % 2 else bytes(rng.integers(0, 256, L, dtype=np.uint8))
        recs.append(rec_windows(T, M, field, pat))
        W, t_min = SMod.windows(pat, (T, M, field))
        want.append((t_min if W else None, W))      # (t_min matters only where there is a window)
    got = []
    for line in checker(recs):
        head, _, rest = line.partition(":")
        W = [int(v) for v in rest.split()]
        got.append((int(head) if W else None, W))
    assert got == want
    assert any(not w for _, w in want) and any(len(w) == 1 for _, w in want) and {0, 1, None} == {t for t, _ in want}


def test_rule_on_generated_vectors(checker):
    rng = np.random.default_rng(12)
    recs, want = [], []
    for case in range(600):
        n = int(rng.integers(1, 40))
        L = int(rng.choice([2, 5, 7, 16, 100, 256]))
        nw = int(rng.integers(1, L))
        t_min = int(rng.integers(0, 2))
        a = rng.integers(0, nw + 1, n)
        s = rng.integers(0, nw + 1, n)
        full = rng.random(n) < 0.3          # no usable table, or every window present
        a[full] = nw
        s[a == nw] = nw
        sizes = rng.choice([0, 1, 3, L - 1, L, 4096, 65536], n)
        recs.append(rec_rule(a, s, sizes, nw, L, t_min))
        want.append(SMod.decoded_set([SMod.admits(a.tolist(), s.tolist(), sizes.tolist(), nw, L, t_min)], sizes.tolist(), L))
    got = [[int(v) for v in line.split()] for line in checker(recs)]
    assert got == want
    # t_min = 1 is the type 1 rule, as Appendix B.4.1 writes it
    def type1_rule(a, s, sizes, nw, L):
        n, take = len(sizes), set()
        for k in range(n):
            if not sizes[k]:
                continue
            cand = a[k] == nw
            if not cand and k + 1 < n:
                s_next = nw if sizes[k + 1] < L else s[k + 1]
                cand = max(1, nw - s_next) <= min(a[k], nw - 1)
            if cand:
                take.add(k)
                need, j = L - 1, k + 1
                while need > 0 and j < n:
                    if sizes[j]:
                        take.add(j)
                    need -= sizes[j]
                    j += 1
        return sorted(take)
    for case in range(100):
        n, L = int(rng.integers(1, 20)), 16
        nw = int(rng.integers(1, L))
        a, s = rng.integers(0, nw + 1, n), rng.integers(0, nw + 1, n)
        s[a == nw] = nw
        sizes = rng.choice([0, 3, L, 4096], n)
        assert SMod.decoded_set([SMod.admits(a.tolist(), s.tolist(), sizes.tolist(), nw, L, 1)], sizes.tolist(), L) == type1_rule(a.tolist(), s.tolist(), sizes.tolist(), nw, L)


def _spliced(kind, bs, nblk, M, pset, tail=777, level=1):
    d, pats = PC.designed(kind, bs, nblk, tail, M, pset)
    T, field = SMod.field_of(pset)
    B = SMod.table_bits(bs)
    sp, tables = SMod.splice(O.stream_encode(d, level, bs), d, (T, M, field), B)
    assert O.stream_decode(sp, len(d)) == d
    return d, pats, sp, tables, (T, M, B, field)


def _check_patterns(checker, d, sp, tables, cfg, pats, what):
    T, M, B, field = cfg
    sizes = [n for n, _ in SMod.data_grid(sp)]
    lines = checker([rec_stream(6, sp, p) for _, p in pats])
    n_tables = sum(t is not None for t in tables)
    for (name, p), line in zip(pats, lines):
        head, got = parse_stream_line(line)
        W, t_min = SMod.windows(p, (T, M, field))
        assert got == SMod.plan(tables, sizes, p, (T, M, field), B), (what, name)
        assert head[:3] == (T, M, B) and head[3] == SMod.usable_tables(tables, p, (T, M, field)) and head[4] == (len(W) if n_tables else 0), (what, name, head)
        if W and n_tables:
            assert head[5] == t_min, (what, name)
        else:
            assert got == [k for k in range(len(sizes)) if sizes[k]], (what, name)
        touched = SMod.chunks_touched(sizes, SMod.brute(d, p), len(p))
        assert touched <= set(got), (what, name, sorted(touched - set(got)))
        if not name.startswith("absent"):
            assert touched, (what, name)
    return dict(zip((n for n, _ in pats), (parse_stream_line(l) for l in lines)))


@pytest.mark.parametrize("set_name", sorted(PC.SETS))
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("M", [1, 2, 4, 6, 8])
def test_spliced_streams_decoded_set_holds_every_occurrence(checker, kind, M, set_name):
    bs, nblk = 64 << 10, 8
    d, pats, sp, tables, cfg = _spliced(kind, bs, nblk, M, PC.SETS[set_name])
    assert all(t is not None for t in tables)
    res = _check_patterns(checker, d, sp, tables, cfg, pats + SC.patterns(d, M, bs), (kind, M, set_name))
    assert res["one_window"][0][4] == 1 and res["unusable"][0][3:5] == (0, 0)
    assert res["border_short"][0][4:] == (SMod.windows(dict(pats)["border_short"], (*cfg[:2], cfg[3]))[0].__len__(), 0)
    if M > 1:
        assert res["late_prefix"][0][3:5] == (0, 0)
    no = parse_stream_line(checker([rec_stream(6, sp, pats[0][1], 1)])[0])
    assert no[0][3:5] == (0, 0) and no[1] == list(range(nblk + 1))


@pytest.mark.parametrize("M", [1, 2, 4, 6, 8])
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 40), (1 << 20, 3), (8 << 20, 2)])
def test_every_block_size(checker, bs, nblk, M):
    """Block sizes 4 KiB (B = 12) to 8 MiB (B = 23); the set alternates with M."""
    set_name = sorted(PC.SETS)[M % 2]
    d, pats, sp, tables, cfg = _spliced("json_like", bs, nblk, M, PC.SETS[set_name], tail=300)
    assert sum(t is not None for t in tables) >= nblk
    _check_patterns(checker, d, sp, tables, cfg, pats + SC.patterns(d, M, bs)[-5:], (bs, M, set_name))


def test_table_verdicts(checker):
    """A table whose prefix field differs from the info chunk's, a type 3 table in a type 2 stream, a type 4 info chunk and a truncated
    field: the chunk, or the stream, counts as having no table."""
    bs, nblk, M = 64 << 10, 6, 6
    d, pats, sp, tables, cfg = _spliced("json_like", bs, nblk, M, PC.SETS["json4"])
    T, _, B, field = cfg
    assert T == 2 and len(field) == 8
    sizes = [n for n, _ in SMod.data_grid(sp)]
    p = pats[0][1]
    everything = list(range(nblk + 1))

    def run(stream, flags=0):
        return parse_stream_line(checker([rec_stream(6, bytes(stream), p, flags)])[0])
    base = run(sp)
    assert base[0][3] == nblk + 1 and base[1] == SMod.plan(tables, sizes, p, (T, M, field), B) and len(base[1]) < nblk + 1
    skipped = next(k for k in range(1, nblk) if k not in base[1])
    tabs = [c for c in SMod.chunks_of(sp) if c[1] == SMod.CHUNK_TABLE]
    off = tabs[skipped][0]
    # the field of one table differs (the CRC, over the table bytes, still holds): with and without the CRC check
    b = bytearray(sp)
    b[off + 4 + 3 + 1] ^= 0x01
    t2 = list(tables); t2[skipped] = None
    for flags in (0, 2):
        got = run(b, flags)
        assert got[0][3] == nblk and skipped in got[1] and got[1] == SMod.plan(t2, sizes, p, (T, M, field), B)
        assert SMod.read_tables(bytes(b), bool(flags), TYPES)[2] == t2
    # a type 3 table in front of that chunk, valid in itself
    T3, f3 = SMod.field_of(PC.SETS["nonalnum"])
    tab3, R3 = SMod.build_table((T3, M, f3), d[skipped * bs:(skipped + 1) * bs], d[(skipped + 1) * bs:(skipped + 1) * bs + 8], B)
    old_len = 4 + tabs[skipped][2]
    b = sp[:off] + SMod.table_chunk((T3, M, f3), B, tab3, R3) + sp[off + old_len:]
    assert O.stream_decode(b, len(d)) == d
    got = run(b)
    assert got[0][3] == nblk and skipped in got[1] and SMod.read_tables(b, types=TYPES)[2] == t2
    # ... and behind it the right one: found
    b = sp[:off] + SMod.table_chunk((T3, M, f3), B, tab3, R3) + sp[off:]
    assert run(b) == base and SMod.read_tables(b, types=TYPES)[2] == tables
    # a type 4 info chunk, a field cut short, a type 2 info chunk over type 1 tables: no configuration / no table
    for name, mutate in (("type 4", lambda s: s[:14] + b"\x04" + s[15:]),
                         ("short field", lambda s: s[:10] + SMod.frame(SMod.CHUNK_INFO, bytes([T, M, B]) + field[:5]) + s[10 + 4 + 11:])):
        b = mutate(sp)
        assert O.stream_decode(b, len(d)) == d, name
        got = run(b)
        assert got[0][3:5] == (0, 0) and got[1] == everything, name
        assert SMod.read_tables(b, types=TYPES)[0] is None, name
    # the empty type 3 mask: a valid configuration that serves no pattern
    T0, f0 = SMod.field_of(b"")
    assert T0 == 3 and f0 == bytes(32)
    sp0, tables0 = SMod.splice(O.stream_encode(d, 1, bs), d, (T0, M, f0), B)
    assert all(t == (bytes(32), B - 8) for t in tables0)
    got = run(sp0)
    assert got[0][:5] == (3, M, B, 0, 0) and got[1] == everything


def test_reduce_rule_with_the_prefix_limit(checker):
    rng = np.random.default_rng(4)
    recs, want, seen = [], [], set()
    for B, fill in ((8, 0.0), (8, 0.05), (8, 0.2), (12, 0.004), (12, 0.05), (12, 0.3), (16, 0.01), (16, 0.04), (16, 0.72), (20, 0.001), (13, 0.0)):
        bits = rng.random(1 << B) < fill
        pops, cur = [], bits
        for r in range(B - 8 + 1):
            pops.append(int(cur.sum()))
            half = len(cur) // 2
            cur = cur[:half] | cur[half:]
        for limit in (10, 25):
            recs.append(rec_reduce(B, pops, limit))
            t = bits
            if int(t.sum()) * 100 // (1 << B) > 70:
                want.append((0, 0))
                continue
            R = 0
            while len(t) // 8 >= 64:
                half = len(t) // 2
                m = t[:half] | t[half:]
                if int(m.sum()) * 100 > half * limit:
                    break
                t, R = m, R + 1
            want.append((len(t) // 8, R))
        seen.add(want[-2] != want[-1])
    got = [tuple(int(v) for v in line.split()) for line in checker(recs)]
    assert got == want and seen == {True, False}


@pytest.mark.parametrize("set_name", sorted(PC.SETS))
@pytest.mark.parametrize("kind", SC.KINDS)
def test_designated_input_skips_most_chunks(kind, set_name):
    """128 x 64 KiB, M = 6, the needle '"id":"' + 10 random bytes in blocks 3 and 64 and across 126|127: the rule decodes a handful of chunks."""
    T, field = SMod.field_of(PC.SETS[set_name])
    for seed in (1, 2, 3):
        bs, nblk, M = 64 << 10, 128, 6
        d, nd, at = PC.planted_id(kind, bs, nblk, seed)
        B = SMod.table_bits(bs)
        tables = []
        for k in range(nblk):
            t, R = SMod.build_table((T, M, field), d[k * bs:(k + 1) * bs], d[(k + 1) * bs:(k + 1) * bs + 8] if k + 1 < nblk else None, B)
            tables.append(None if t is None else (t, R))
        got = SMod.plan(tables, [bs] * nblk, nd, (T, M, field), B)
        print(kind, set_name, seed, len(got), got)
        assert {3, 64, 126, 127} <= set(got) and len(got) <= 12
