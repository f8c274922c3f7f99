"""The rules of the block search tables and of mlz_dev_reader_search's plan without a GPU: tools/stream_search_check.cpp runs the shared
header minlz_amd/csrc/mlz_stream_search.h (the hash, a table chunk's checks, the probe, the rule that picks the chunks to decode, the
writer's reduction rule) on the host, with the kernels' hops over the chunk headers as plain loops, and tests/search_model.py is the same
specification in Python, written separately.  The two must agree, and the decoded set must hold every chunk with a byte of a true occurrence."""
import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from tests import search_cases as SC
from tests import search_model as SMod
from tests.search_host import build_checker, parse_stream_line, rec_hash, rec_layout, rec_reduce, rec_rule, rec_stream


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    run = build_checker(tmp_path_factory, "stream_search_check.cpp")
    return lambda records: run(records)[0]


def type1(M):
    return SMod.config(1, M)


def test_exported():
    L = _lib.lib()
    assert L.mlz_dev_reader_search and "mlz_dev_reader_search" in _lib.SYMBOLS


def test_hash_against_python_integers(checker):
    rng = np.random.default_rng(5)
    triples = []
    for M in range(1, 9):
        for B in sorted({8, 12, 15, 16, 17, 20, 23}):
            vals = [0, (1 << 64) - 1, 0x0123456789ABCDEF] + [int(v) for v in rng.integers(0, 1 << 63, 20, dtype=np.uint64) * 2 + 1]
            triples += [(v, B, M) for v in vals]
    assert (2 in {M for _, _, M in triples}) and {15, 16} <= {B for _, B, M in triples if M == 2}
    got = [int(v) for v in checker([rec_hash(triples)])[0].split()]
    want = [SMod.hash_value(v, B, M) for v, B, M in triples]
    assert got == want
    # bytes beyond M do not enter; the vectorised model agrees with the integer one
    buf = rng.integers(0, 256, 300, dtype=np.uint8)
    for M in range(1, 9):
        for B in (8, 15, 16, 23):
            hv = SMod.hash_windows(buf, B, M)
            for i in (0, 7, len(hv) - 1):
                v = int.from_bytes(buf[i:i + M].tobytes(), "little")
                assert int(hv[i]) == SMod.hash_value(v, B, M) == SMod.hash_value(v | (0xAB << (8 * M)) if M < 8 else v, B, M)
            assert int(hv.max()) < (1 << B)


def test_rule_on_generated_vectors(checker):
    rng = np.random.default_rng(11)
    recs, want = [], []
    for case in range(400):
        n = int(rng.integers(1, 40))
        L = int(rng.choice([1, 5, 6, 7, 16, 100, 256]))
        M = int(rng.integers(1, min(L, 8) + 1))
        nw = L - M + 1
        a = rng.integers(0, nw + 1, n)
        s = rng.integers(0, nw + 1, n)
        full = rng.random(n) < 0.3          # no usable table, or every window present
        a[full] = nw
        s[a == nw] = nw
        sizes = rng.choice([0, 1, 3, L - 1 if L > 1 else 1, L, 4096, 65536], n)
        recs.append(rec_rule(a, s, sizes, nw, L))
        want.append(SMod.decoded_set([SMod.admits(a.tolist(), s.tolist(), sizes.tolist(), nw, L, 1)], sizes.tolist(), L))
    got = [[int(v) for v in line.split()] for line in checker(recs)]
    assert got == want


def _spliced(kind, bs, nblk, M, seed=2, tail=777, level=1):
    d = getattr(synth, kind)(bs * nblk + tail, seed).tobytes()
    s = O.stream_encode(d, level, bs)
    B = SMod.table_bits(bs)
    sp, tables = SMod.splice(s, d, type1(M), B)
    assert O.stream_decode(sp, len(d)) == d
    return d, sp, tables, B


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("M", [1, 2, 4, 6, 8])
def test_spliced_streams_decoded_set_holds_every_occurrence(checker, kind, M):
    bs, nblk = 64 << 10, 12
    d, sp, tables, B = _spliced(kind, bs, nblk, M)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    assert any(t is not None for t in tables) or M <= 2
    pats = SC.patterns(d, M, bs)
    lines = checker([rec_stream(3, sp, p) for _, p in pats] + [rec_stream(3, sp, p, 1) for _, p in pats[:2]])
    assert {len(p) for _, p in pats} >= {1, max(1, M - 1), M, M + 1, 16, 256}
    for (name, p), line in zip(pats, lines):
        (gM, gB, usable), got = parse_stream_line(line)
        want = SMod.plan(tables, sizes, p, type1(M), B)
        assert got == want, (kind, M, name)
        if len(p) >= M and usable:
            assert (gM, gB, usable) == (M, B, sum(t is not None for t in tables))
        touched = SMod.chunks_touched(sizes, SMod.brute(d, p), len(p))
        assert touched <= set(got), (kind, M, name, sorted(touched - set(got)))
        if name != "absent":
            assert touched
    for line in lines[len(pats):]:
        assert parse_stream_line(line)[1] == list(range(len(sizes)))


def test_real_tables_every_block_size(checker):
    """Block sizes 4 KiB (B = 12) to 8 MiB (B = 23), a short last block, an incompressible block in the middle (stored: no table)."""
    for bs, nblk in ((4 << 10, 40), (1 << 20, 3), (8 << 20, 2)):
        d = bytearray(synth.text_like(bs * nblk + 300, 7).tobytes())
        d[bs:2 * bs] = synth.random_bytes(bs, seed=3).tobytes()
        d = bytes(d)
        M, B = 6, SMod.table_bits(bs)
        sp, tables = SMod.splice(O.stream_encode(d, 1, bs), d, type1(M), B)
        sizes = [n for n, _ in SMod.data_grid(sp)]
        assert tables[1] is None and tables[0] is not None and sizes[-1] == 300
        pats = [d[bs // 2:bs // 2 + 16], d[2 * bs - 8:2 * bs + 8], d[-20:], d[bs + 100:bs + 116], bytes(SC.needle(16, 5))]
        lines = checker([rec_stream(3, sp, p) for p in pats])
        for p, line in zip(pats, lines):
            _, got = parse_stream_line(line)
            assert got == SMod.plan(tables, sizes, p, type1(M), B)
            assert SMod.chunks_touched(sizes, SMod.brute(d, p), len(p)) <= set(got)
        absent = parse_stream_line(lines[-1])[1]
        assert {1, 2} <= set(absent)   # the stored block has no table: it and the chunk behind it are always decoded


def test_broken_and_foreign_tables_count_as_none(checker):
    bs, nblk, M = 64 << 10, 6, 6
    d, sp, tables, B = _spliced("json_like", bs, nblk, M)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    p = bytes(SC.needle(16, 8))
    base = parse_stream_line(checker([rec_stream(3, sp, p)])[0])
    assert base[0][2] == sum(t is not None for t in tables) == nblk + 1 and base[1] == SMod.plan(tables, sizes, p, type1(M), B)
    cks = [c for c in SMod.chunks_of(sp) if c[1] == SMod.CHUNK_TABLE]
    off = cks[2][0]
    flipped = bytearray(sp)
    flipped[off + 12 + 5] ^= 0x10          # a table bit; the CRC is now stale
    t2 = list(tables); t2[2] = None
    got = parse_stream_line(checker([rec_stream(3, bytes(flipped), p)])[0])
    assert got[0][2] == nblk and got[1] == SMod.plan(t2, sizes, p, type1(M), B) and 2 in got[1]
    tb = bytearray(tables[2][0]); tb[5] ^= 0x10
    t3 = list(tables); t3[2] = (bytes(tb), tables[2][1])
    got = parse_stream_line(checker([rec_stream(3, bytes(flipped), p, 2)])[0])
    assert got[0][2] == nblk + 1 and got[1] == SMod.plan(t3, sizes, p, type1(M), B)
    for mutate in ("type", "M", "B", "R", "0x46"):
        b = bytearray(sp)
        if mutate == "0x46":
            b[off] = 0x46
        else:
            b[off + 4 + ("type", "M", "B", "R").index(mutate)] += 1
        got = parse_stream_line(checker([rec_stream(3, bytes(b), p, 2)])[0])
        assert got[0][2] == nblk and 2 in got[1], mutate
    # no info chunk, a pattern shorter than M: every chunk is decoded
    noinfo = sp[:10] + sp[17:]
    head, got = parse_stream_line(checker([rec_stream(3, noinfo, p)])[0])
    assert (head[2], got) == (0, list(range(nblk + 1)))
    head, got = parse_stream_line(checker([rec_stream(3, sp, p[:M - 1])])[0])
    assert (head[2], got) == (0, list(range(nblk + 1)))


def test_reduce_rule_agrees_with_the_model(checker):
    rng = np.random.default_rng(3)
    recs, want = [], []
    for B, fill in ((8, 0.0), (8, 0.2), (12, 0.01), (12, 0.3), (16, 0.05), (16, 0.69), (16, 0.72), (20, 0.001), (13, 0.0)):
        bits = rng.random(1 << B) < fill
        pops, cur = [], bits
        for r in range(B - 8 + 1):
            pops.append(int(cur.sum()))
            half = len(cur) // 2
            cur = cur[:half] | cur[half:]
        recs.append(rec_reduce(B, pops))
        blk_bits = np.packbits(bits, bitorder="little").tobytes()
        # the model's fold on the same bits
        t = bits
        if int(t.sum()) * 100 // (1 << B) > 70:
            want.append((0, 0))
            continue
        R = 0
        while len(t) // 8 >= 64:
            half = len(t) // 2
            m = t[:half] | t[half:]
            if int(m.sum()) * 100 > half * 25:
                break
            t, R = m, R + 1
        want.append((len(t) // 8, R))
        assert len(blk_bits) == (1 << B) // 8
    got = [tuple(int(v) for v in line.split()) for line in checker(recs)]
    assert got == want
    assert (0, 0) in want and any(r == B - 8 for (_, r), (B, _) in zip(want, ((8, 0), (8, 0), (12, 0), (12, 0), (16, 0), (16, 0), (16, 0), (20, 0), (13, 0))))


@pytest.mark.parametrize("kind", SC.KINDS)
def test_designated_input_skips_most_chunks(kind):
    """128 x 64 KiB, M = 6, a random 16-byte needle in blocks 3 and 64 and across 126|127: the rule decodes a handful of chunks."""
    for seed in (1, 2, 3):
        bs, nblk, M = 64 << 10, 128, 6
        d, nd, at = SC.planted(kind, bs, nblk, 16, seed)
        B = SMod.table_bits(bs)
        tables = []
        for k in range(nblk):
            t, R = SMod.build_table(type1(M), d[k * bs:(k + 1) * bs], d[(k + 1) * bs:(k + 1) * bs + 8] if k + 1 < nblk else None, B)
            tables.append(None if t is None else (t, R))
        got = SMod.plan(tables, [bs] * nblk, nd, type1(M), B)
        print(kind, seed, len(got), got)
        assert {3, 64, 126, 127} <= set(got) and len(got) <= 12


def test_scratch_layout_finds_what_brute_force_finds(checker):
    """search_layout executed on the host: small groups, so that runs of neighbouring chunks cross many group borders, chunks shorter than
    the pattern (a run's carried bytes then come from more than one group back), gaps between runs; ascending positions, each once."""
    rng = np.random.default_rng(17)
    recs, want, meta = [], [], []
    for case in range(120):
        nck = int(rng.integers(1, 30))
        L = int(rng.choice([1, 2, 3, 7, 16, 40, 256]))
        sizes = rng.choice([0, 1, 2, 5, L - 1 if L > 1 else 1, L, 100, 700, 9000], nck).tolist()
        d = bytearray(rng.integers(97, 99, sum(sizes), dtype=np.uint8).tobytes())      # two letters: many occurrences of short patterns
        pat = bytes(rng.integers(97, 99, L, dtype=np.uint8)) if L <= 7 else bytes(rng.integers(0, 256, L, dtype=np.uint8))
        for _ in range(6):
            if len(d) >= L:
                o = int(rng.integers(0, len(d) - L + 1))
                d[o:o + L] = pat
        d = bytes(d)
        full = case % 2 == 0
        jobs = [k for k in range(nck) if sizes[k] and (full or rng.random() < 0.6)]
        group = int(rng.choice([1, 50, 1000, 20000]))
        recs.append(rec_layout(sizes, jobs, pat, d, group))
        # what a search of the taken runs can find: occurrences whose bytes all lie in taken chunks
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        taken = np.zeros(len(d) + 1, dtype=bool)
        for k in jobs:
            taken[starts[k]:starts[k + 1]] = True
        want.append([p for p in SMod.brute(d, pat) if taken[p:p + L].all()])
        meta.append((nck, L, group, full))
    lines = checker(recs)
    several_groups = 0
    for line, w, m in zip(lines, want, meta):
        head, _, rest = line.partition(":")
        count, tiles, groups, scratch_max = (int(v) for v in head.split())
        assert [int(v) for v in rest.split()] == w and count == len(w), m
        several_groups += groups > 2
    assert several_groups > 40 and sum(len(w) for w in want) > 1000
