"""mlz_dev_reader_search_many without a GPU: tools/stream_search_many_check.cpp runs the host code the call shares with its kernels
(minlz_amd/csrc/mlz_stream_search.h: the marking form of the decoded-set rule, the layout for patterns of several lengths, the pattern
index and the scan rule of one tile) and the Python model of the table types (tests/search_model.py) says what must come out: the union of the
patterns' plans, and every pair (position, pattern) of a brute-force search over the taken chunks, in order, each once."""
import struct

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from tests import search_cases as SC
from tests import search_host as H
from tests import search_long_prefix_cases as LC
from tests import search_model as SMod
from tests import search_prefix_cases as PC

SRC = "stream_search_many_check.cpp"
NO_TABLE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    run = H.build_checker(tmp_path_factory, SRC)
    return lambda records: run(records)[0]


def rec_patterns(pats):
    return np.asarray([len(p) for p in pats], np.uint32).tobytes() + b"".join(pats)


def rec_plan(T, M, B, field, sizes, tables, pats):
    out = [struct.pack("<IIIIIII", 1, T, M, B, len(field), len(sizes), len(pats)), bytes(field), np.asarray(sizes, np.uint64).tobytes()]
    for t in tables:
        out.append(struct.pack("<II", NO_TABLE, 0) if t is None else struct.pack("<II", t[1], len(t[0])) + t[0])
    return b"".join(out) + rec_patterns(pats)


def rec_layout(sizes, jobs, pats, data, group_bytes):
    return (struct.pack("<IIIIQQ", 2, len(sizes), len(jobs), len(pats), group_bytes, len(data)) + np.asarray(sizes, np.uint64).tobytes() +
            np.asarray(jobs, np.uint32).tobytes() + rec_patterns(pats) + data)


def rec_index(pats):
    return struct.pack("<II", 3, len(pats)) + rec_patterns(pats)


def parse_plan(line):
    head, _, rest = line.partition(":")
    served, unserved = (int(v) for v in head.split())
    return served, unserved, [int(v) for v in rest.split()]


def test_exported():
    L = _lib.lib()
    assert L.mlz_dev_reader_search_many and "mlz_dev_reader_search_many" in _lib.SYMBOLS


# ---- the union plan ----

def _configs(kind, M):
    """(name, T, M, B, field, sizes, tables, [(name, pattern)], plan(pattern), served(pattern)) over spliced 12 x 64 KiB streams, one per table family."""
    bs, nblk, tail = 64 << 10, 12, 777
    B = SMod.table_bits(bs)
    d = getattr(synth, kind)(bs * nblk + tail, 2).tobytes()
    cfg = SMod.config(1, M)
    sp, tables = SMod.splice(O.stream_encode(d, 1, bs), d, cfg, B)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    use = any(t is not None for t in tables)
    yield ("type 1", 1, M, B, b"", sizes, tables, SC.patterns(d, M, bs),
           lambda p, cfg=cfg, tables=tables, sizes=sizes, use=use: SMod.plan(tables, sizes, p, cfg, B, use_tables=use), lambda p: len(p) >= M)
    for sname, pset in PC.SETS.items():
        T, field = SMod.field_of(pset)
        cfg = (T, M, field)
        d2, pats = PC.designed(kind, bs, nblk, tail, M, pset)
        sp, tables = SMod.splice(O.stream_encode(d2, 1, bs), d2, cfg, B)
        sizes = [n for n, _ in SMod.data_grid(sp)]
        yield ("type %d %s" % (T, sname), T, M, B, field, sizes, tables, pats + SC.patterns(d2, M, bs),
               lambda p, cfg=cfg, tables=tables, sizes=sizes: SMod.plan(tables, sizes, p, cfg, B),
               lambda p, cfg=cfg: bool(SMod.windows(p, cfg)[0]) if len(p) >= M else False)
    cfg = SMod.config(4, M, LC.USER, 3)
    d4, pats = LC.designed(kind, bs, nblk, tail, M, 3, LC.USER)
    sp, tables = SMod.splice(O.stream_encode(d4, 1, bs), d4, cfg, B)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    yield ("type 4", 4, M, B, cfg[2], sizes, tables, pats + SC.patterns(d4, M, bs),
           lambda p, cfg=cfg, tables=tables, sizes=sizes: SMod.plan(tables, sizes, p, cfg, B), lambda p, cfg=cfg: bool(SMod.groups(p, cfg)[0]))


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("M", [1, 6, 8])
def test_union_plan_is_the_union_of_the_models_plans(checker, kind, M):
    recs, want, what = [], [], []
    for name, T, M_, B, field, sizes, tables, pats, plan, served in _configs(kind, M):
        everything = [k for k in range(len(sizes)) if sizes[k]]
        plans = {n: plan(p) for n, p in pats}
        ok = [(n, p) for n, p in pats if served(p)]
        bad = [(n, p) for n, p in pats if not served(p)]
        assert ok, name
        has_tables = any(t is not None for t in tables)
        lists = [ok, ok[:1], ok[-2:] + ok[:2] + ok[:1]]                # all served ones; one; a few, with a duplicate
        lists += [[pp] + ok[:3] for pp in bad[:1]] + [ok[:2] + [pp] for pp in bad[-1:]]   # one unserved pattern in the list: everything
        if M > 1 and T == 1:
            lists.append(ok + [("short", ok[0][1][:M - 1])])
        for lst in lists:
            recs.append(rec_plan(T, M_, B, field, sizes, tables, [p for _, p in lst]))
            u = sorted(set().union(*[set(plans[n] if n in plans else everything) for n, _ in lst]))
            n_bad = sum(1 for _, p in lst if not served(p))
            if n_bad:
                assert u == everything, (name, [n for n, _ in lst])
            want.append((len(lst) - n_bad, n_bad, u))
            what.append((kind, M, name, [n for n, _ in lst]))
        if has_tables and M >= 6 and T == 1:   # the union is a real selection: the absent needle alone decodes less than everything
            assert len(plans["absent"]) < len(everything), name
    lines = checker(recs)
    assert len(lines) == len(want)
    for line, w, m in zip(lines, want, what):
        assert parse_plan(line) == w, m


def test_one_short_pattern_marks_every_nonempty_chunk(checker):
    """Chunk sizes with zeros among them, real tables of a 6 x 64 KiB stream on the others."""
    bs, M = 64 << 10, 6
    d = synth.json_like(bs * 6, 3).tobytes()
    B, cfg = SMod.table_bits(bs), SMod.config(1, M)
    sp, tables = SMod.splice(O.stream_encode(d, 1, bs), d, cfg, B)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    sizes2 = [sizes[0], 0, sizes[1], sizes[2], 0, 0, sizes[3], sizes[4], sizes[5]]
    tables2 = [tables[0], None, tables[1], tables[2], None, None, tables[3], tables[4], tables[5]]
    absent = bytes(SC.needle(16, 99))
    want_absent = SMod.plan(tables2, sizes2, absent, cfg, B)
    lines = checker([rec_plan(1, M, B, b"", sizes2, tables2, [absent]), rec_plan(1, M, B, b"", sizes2, tables2, [absent, d[100:105]]),
                     rec_plan(1, M, B, b"", sizes2, tables2, [absent, d[3 * bs - 8:3 * bs + 8]])])
    assert parse_plan(lines[0]) == (1, 0, want_absent) and len(want_absent) < 6
    assert parse_plan(lines[1]) == (1, 1, [0, 2, 3, 6, 7, 8])
    both = sorted(set(want_absent) | set(SMod.plan(tables2, sizes2, d[3 * bs - 8:3 * bs + 8], cfg, B)))
    assert parse_plan(lines[2]) == (2, 0, both) and {3, 6} <= set(both)   # (chunks 3 and 6 are neighbours in the data: the empty ones hold nothing)


# ---- the layout, the index and the scan rule ----

LENGTHS = [1, 2, 3, 7, 16, 40, 256]


def _two_letter(rng, n):
    return bytes(rng.integers(97, 99, n, dtype=np.uint8))


def _layout_case(rng, pats, case, nck=None, big=9000):
    lmin, lmax = min(len(p) for p in pats), max(len(p) for p in pats)
    nck = int(rng.integers(1, 30)) if nck is None else nck
    sizes = rng.choice([0, 1, 2, 5, max(1, lmin - 1), lmin, max(1, lmax - 1), lmax, 100, 700, big], nck).tolist()
    d = bytearray(_two_letter(rng, sum(sizes)))
    for p in pats:
        if len(p) > 7 and len(d) >= len(p):                                     # long ones are planted, some of them over each other's ends
            for _ in range(3):
                o = int(rng.integers(0, len(d) - len(p) + 1))
                d[o:o + len(p)] = p
    d = bytes(d)
    full = case % 2 == 0
    jobs = [k for k in range(nck) if sizes[k] and (full or rng.random() < 0.6)]
    group = int(rng.choice([1, 50, 1000, 20000]))
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    taken = np.zeros(len(d) + 1, dtype=bool)
    for k in jobs:
        taken[starts[k]:starts[k + 1]] = True
    ok = {}                                                                     # per length: the positions whose bytes all lie in taken chunks
    pairs = []
    for i, p in enumerate(pats):
        L = len(p)
        if L not in ok:
            c = np.concatenate([[0], np.cumsum(~taken[:len(d)])])
            ok[L] = (c[L:] - c[:len(c) - L]) == 0 if len(d) >= L else np.zeros(0, dtype=bool)
        pairs += [(q, i) for q in SMod.brute(d, p) if ok[L][q]]
    pairs.sort()
    return rec_layout(sizes, jobs, pats, d, group), pairs, (nck, lmin, lmax, group, full, len(pats))


def _pattern_sets(rng):
    """The sets of the layout test: mixed lengths, one pattern a prefix of another, duplicates."""
    sets = []
    for case in range(90):
        n = int(rng.integers(1, 9))
        lens = rng.choice(LENGTHS, n).tolist()
        sets.append([_two_letter(rng, L) if L <= 7 else bytes(rng.integers(0, 256, L, dtype=np.uint8)) for L in lens])
    for case in range(20):                                                      # prefixes of one another, every length class from one string
        base = _two_letter(rng, 256)
        sets.append([base[:L] for L in rng.permutation(LENGTHS).tolist()] + [base[:2]])
    for case in range(10):                                                      # duplicates
        a, b = _two_letter(rng, 3), _two_letter(rng, 16)
        sets.append([a, b, a, a, b, _two_letter(rng, 1)])
    return sets


@pytest.fixture(scope="module")
def layout_cases():
    rng = np.random.default_rng(23)
    recs, want, meta = [], [], []
    for case, pats in enumerate(_pattern_sets(rng)):
        r, w, m = _layout_case(rng, pats, case)
        recs.append(r); want.append(w); meta.append(m)
    # 4096 patterns: lengths 2 .. 40 over two letters (so many are equal and many are prefixes of others), few chunks
    for case, lens in enumerate(([2, 3, 7, 16], [7, 16, 40], [1, 16])):
        pats = [_two_letter(rng, int(L)) for L in rng.choice(lens, 4096)]
        r, w, m = _layout_case(rng, pats, case, nck=12, big=700)
        recs.append(r); want.append(w); meta.append(m)
    return recs, want, meta


def _check_layout_lines(lines, want, meta):
    several_groups = 0
    for line, w, m in zip(lines, want, meta):
        head, _, rest = line.partition(":")
        count, tiles, groups, scratch_max = (int(v) for v in head.split())
        got = [tuple(int(x) for x in v.split(":")) for v in rest.split()]
        assert got == w and count == len(w), m
        several_groups += groups > 2
    return several_groups


def test_layout_with_mixed_lengths_finds_what_brute_force_finds(checker, layout_cases):
    """search_layout (lengths lmin .. lmax), search_many_index and the scan rule executed on the host: small groups, so that runs of neighbouring chunks cross
    many group borders, chunks shorter than the shortest and the longest pattern (carried bytes then come from more than one group back),
    gaps between runs; the pairs in (position, pattern) order, each once."""
    recs, want, meta = layout_cases
    lines = checker(recs)
    assert len(lines) == len(want)
    assert _check_layout_lines(lines, want, meta) > 40
    assert sum(len(w) for w in want) > 20000 and max(m[5] for m in meta) == 4096
    assert {m[1] for m in meta} >= {1, 2, 3, 7} and {m[2] for m in meta} >= {7, 16, 40, 256}


def test_layout_under_the_sanitizers(tmp_path_factory, layout_cases):
    """The check tool built once with -fsanitize=address,undefined, on the same case file: no read outside the staged bytes of a tile,
    the pattern blob or the index."""
    # (the runtimes linked statically: a stand-alone program that needs nothing of its environment)
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    recs, want, meta = layout_cases
    lines, err = run(recs + [rec_index([b"ab", b"abc", b"b"])])
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check_layout_lines(lines[:-1], want, meta)


def _key(p, m, hb):
    v = int.from_bytes(p[:m], "little")
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - hb)


def test_index_holds_every_pattern_once_in_its_bucket(checker):
    rng = np.random.default_rng(31)
    sets = []
    for lmin in (1, 2, 3, 4, 9):
        for n in (1, 2, 255, 256, 257, 1000, 4096):
            lens = [lmin] + rng.choice([L for L in (lmin, lmin + 1, 16, 256)], n - 1).tolist()
            alpha = 256 if n > 300 else 3
            sets.append((lmin, [bytes(rng.integers(0, alpha, int(L), dtype=np.uint8)) for L in rng.permutation(lens)]))
    lines = checker([rec_index(p) for _, p in sets])
    for (lmin, pats), line in zip(sets, lines):
        head, _, rest = line.partition(":")
        m, hb, gmin, gmax = (int(v) for v in head.split())
        heads, _, order = rest.partition("|")
        heads, order = [int(v) for v in heads.split()], [int(v) for v in order.split()]
        n = len(pats)
        assert (m, gmin, gmax) == (min(4, lmin), lmin, max(len(p) for p in pats))
        assert hb == min(12, max(8, (n - 1).bit_length())) and len(heads) == (1 << hb) + 1
        assert heads[0] == 0 and heads[-1] == n and all(a <= b for a, b in zip(heads, heads[1:]))
        assert sorted(order) == list(range(n))                                   # every pattern exactly once
        for b in range(1 << hb):
            ent = order[heads[b]:heads[b + 1]]
            assert ent == sorted(ent) and all(_key(pats[i], m, hb) == b for i in ent), (lmin, n, b)
