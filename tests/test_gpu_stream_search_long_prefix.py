"""Search tables with a long prefix and extra matches (table type 4) written by the device-resident Writer
(mlz_stream_encode_gather_device_long_prefix, HipCtx.stream_encode_gather_device(search_long_prefix=...)) and used by the pattern search
(mlz_dev_reader_search), against tests/search_model.py: the specification in plain Python.  The Writer's stream must be the
table-less stream of the same call with the model's chunks spliced in; a search must return what a brute-force search of the decoded bytes
returns and decode exactly the chunks the model's plan names."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, synth
from tests import search_cases as SC
from tests import search_long_prefix_cases as LC
from tests import search_model as SMod
from tests import search_prefix_cases as PC
from tests.search_gpu import Searcher, data_for, first_difference, gather, on_device

pytestmark = pytest.mark.gpu

MLZ_ERR_ARG = 8
FILL = ord("a")
ME = [(6, 0), (6, 3), (8, 8), (1, 15)]


def writer_case(ctx, d, bs, M, E, pfx, add_index=False, cuts=None, what=""):
    """-> (stream, tables): the Writer's stream, equal to the model's splice of the table-less stream of the same call."""
    cuts = [0] + list(cuts or []) + [len(d)]
    ranges = [d[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    off = gather(ctx, ranges, bs, add_index)
    on = gather(ctx, ranges, bs, add_index, search_match_len=M, search_long_prefix=pfx, search_extras=E)
    field, B = SMod.config(4, M, pfx, E)[2], SMod.table_bits(bs)
    want, tables = SMod.splice(off, d, (4, M, field), B, index=add_index)
    what = "%s bs=%d K=%d M=%d E=%d index=%s ranges=%d" % (what, bs, len(pfx), M, E, add_index, len(ranges))
    assert len(on) == len(want) and on == want, what + ": lengths %d / %d, first difference at %d" % (len(on), len(want), first_difference(on, want))
    assert SMod.read_tables(on) == ((4, M, field), B, tables), what
    assert mz.stream_decode(on, ctx=ctx) == d and O.stream_decode(on, len(d)) == d, what
    return on, tables


def popcount(table):
    return int(np.unpackbits(np.frombuffer(table, np.uint8)).sum())


# ---- Writer: whole streams ----

@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 50), (64 << 10, 9), (1 << 20, 2), (2 << 20, 2)])
def test_writer_stream_is_the_models(ctx, kind, bs, nblk):
    d = data_for(kind, bs, nblk, 1234)
    configs = [(LC.USER if kind == "json_like" else b"the ", 6, 3)] + ([(b"e ", 8, 8)] if bs == 64 << 10 else [])
    for pfx, M, E in configs:
        for add_index in ((False, True) if bs == 64 << 10 else (bs == 2 << 20,)):
            on, tables = writer_case(ctx, d, bs, M, E, pfx, add_index, what=kind)
            grid = SMod.data_grid(on)
            assert grid[1][1] == 0x01 and tables[1] is None and grid[-1][0] == 1234       # the incompressible block: stored, no table; a ragged tail
            assert sum(t is not None for t in tables) == len(tables) - 1
            assert any(popcount(t[0]) for t in tables if t is not None)


# ---- Writer: hand-built blocks ----

def prefix_of(K):
    """K bytes that occur only where they are planted: no letter, and only the first byte is '<'."""
    return (b"<" + b"-" * (K - 2) + b">")[:K] if K > 1 else b"<"


def tag(i):
    """8 letters that name plant i."""
    return bytes(98 + ((i * 7919 + 13 * j * (i + 1)) >> (2 * j)) % 25 for j in range(8))


def hand_built(sizes, plants, pfx, fill=FILL):
    """Blocks of one filler byte with the prefix at the stream positions `plants`, each followed by letters that name it (the letters are
    written first, so that a neighbouring plant's prefix stays)."""
    d = bytearray([fill]) * sum(sizes)
    K = len(pfx)
    for i, g in enumerate(plants):
        t = tag(i)[:max(0, len(d) - g - K)]
        d[g + K:g + K + len(t)] = t
    for g in plants:
        p = pfx[:max(0, len(d) - g)]
        d[g:g + len(p)] = p
    return bytes(d)


def indexed_by_rule(sizes, g, K, M, E):
    """Whether the rule, written out, indexes a prefix planted at stream position g: every start of a block with a block behind it, the
    starts up to n - K - M - E of the last block."""
    starts = np.concatenate([[0], np.cumsum(sizes)])
    k = int(np.searchsorted(starts, g, side="right")) - 1
    p, n = g - int(starts[k]), sizes[k]
    return k, (g + K <= int(starts[-1])) and (k + 1 < len(sizes) or p <= n - K - M - E)


def single_plant(ctx, bs, sizes, g, pfx, M, E):
    """One plant: exactly the model's bits, E + 1 at the most, in exactly the table of the block where the prefix starts."""
    K, B = len(pfx), SMod.table_bits(bs)
    zero = (bytes(32), B - 8)
    d = hand_built(sizes, [g], pfx)
    on, tables = writer_case(ctx, d, bs, M, E, pfx, what="plant at %d" % g)
    k, indexed = indexed_by_rule(sizes, g, K, M, E)
    assert all(t in (zero, None) for i, t in enumerate(tables) if i != k), g
    starts = np.concatenate([[0], np.cumsum(sizes)])
    follow = d[starts[k + 1]:starts[k + 1] + K - 1 + M + E] if k + 1 < len(sizes) else None
    hashes = set(SMod.indexed_hashes(SMod.config(4, M, pfx, E), d[starts[k]:starts[k + 1]], follow, B).tolist())
    assert bool(hashes) == indexed, (g, "the model and the rule, written out, disagree")
    if not indexed:
        assert tables[k] in (zero, None), g
    else:
        tab, R = tables[k]
        folded = {h & ((1 << (B - R)) - 1) for h in hashes}
        assert 1 <= popcount(tab) == len(folded) <= E + 1, g
        assert all((tab[h >> 3] >> (h & 7)) & 1 for h in folded), g
    return tables


@pytest.mark.parametrize("K", [1, 8, 9, 256])
def test_hand_built_block_edges(ctx, K):
    """64 KiB blocks: a prefix with 1 and K - 1 bytes in front of a border, one that ends on a block's last byte, one that starts on a
    block's first byte, the last indexed start of the last block and the first one behind it, plants across a lane's 8 positions and a
    sweep of 8192 — all together, and alone where a neighbour could hide a mistake."""
    bs, tail = 64 << 10, 1000
    sizes = [bs, bs, bs, tail]
    end = 3 * bs + tail
    pfx = prefix_of(K)
    for M, E in ME:
        W = M + E
        edges = [bs - 1, bs - (K - 1) if K > 1 else bs - 2, 2 * bs - K, 2 * bs, end - K - W, end - K - W + 1]
        plants = edges + [0, 6, 7, 8, 8190, 8191, 8192, bs + 8191, 3 * bs - 1, 3 * bs, end - K, end - 1]
        d = hand_built(sizes, sorted(set(plants)), pfx)
        on, tables = writer_case(ctx, d, bs, M, E, pfx, add_index=(M == 6), what="hand-built")
        assert all(t is not None for t in tables[:3])
        for g in edges + ([7, 8191] if (M, E) == (6, 3) else []):
            single_plant(ctx, bs, sizes, g, pfx, M, E)


def test_hand_built_parts_and_slices(ctx):
    """1 MiB blocks (several workgroups take parts of at least 64 KiB of a block) and 2 MiB blocks (B = 21: two slices of the table, each
    in a workgroup of its own): prefixes around every 64 KiB step and around the steps of a split into 2 .. 32 equal parts; one byte long
    (every neighbouring start) and nine bytes long (across the step)."""
    for bs, nblk in ((1 << 20, 2), (2 << 20, 2)):
        sizes = [bs] * nblk + [5000]
        steps = set(range(64 << 10, bs + 1, 64 << 10))
        for parts in (2, 3, 5, 8, 16, 32):
            per = -(-(-(-bs // parts)) // 8) * 8              # the starts 0 .. bs - 1 in `parts` shares, rounded up to 8
            steps.update(p * per for p in range(1, parts) if p * per < bs)
        dense = {m + o for m in steps for o in (-2, -1, 0) if m + o < bs} | {bs + m - 1 for m in steps} | {0, bs - 1, nblk * bs - 1, nblk * bs + 4999 - 10}
        d = hand_built(sizes, sorted(dense), b"<")
        on, tables = writer_case(ctx, d, bs, 6, 3, b"<", what="parts, K = 1")
        assert all(t is not None for t in tables) and tables[0][1] < SMod.table_bits(bs) - 8
        across = {m - 4 for m in steps} | {bs + m - 8 for m in steps if m < bs} | {bs - 9, nblk * bs - 1}
        d = hand_built(sizes, sorted(across), prefix_of(9))
        on, tables = writer_case(ctx, d, bs, 8, 8, prefix_of(9), what="parts, K = 9")
        assert all(t is not None for t in tables) and tables[0][1] < SMod.table_bits(bs) - 8
    single_plant(ctx, 1 << 20, [1 << 20, 1 << 20, 5000], (1 << 20) - 4, prefix_of(9), 6, 3)
    single_plant(ctx, 2 << 20, [2 << 20, 2 << 20, 5000], (1 << 20) + (64 << 10) - 3, prefix_of(9), 6, 3)


@pytest.mark.parametrize("K", [1, 8, 9, 256])
def test_hand_built_short_blocks(ctx, K):
    """A last block shorter than K + M + E (it indexes nothing), and a next block shorter than the overlap: prefix and windows of the block
    in front of it run through it, the windows into zeros beyond the stream's end."""
    bs = 4096
    pfx = prefix_of(K)
    for M, E in ((6, 3), (1, 15)):
        for t in sorted({1, 2, K - 1, K, K + M + E - 1} - {0}):
            sizes = [bs, bs, t]
            plants = [bs - (K + 1) // 2, 2 * bs - K, 2 * bs]                # across the first border, up to the second, behind it
            d = hand_built(sizes, plants, pfx)
            on, tables = writer_case(ctx, d, bs, M, E, pfx, what="short last block of %d" % t)
            assert tables[2] in (None, (bytes(32), 4))                     # (a last block of a few bytes may be stored)
            assert tables[1] != (bytes(32), 4)
            # the same bytes as two ranges: the short block comes by value
            assert writer_case(ctx, d, bs, M, E, pfx, cuts=[2 * bs])[0] == on
            for g in (2 * bs - K, 2 * bs - 1):
                single_plant(ctx, bs, sizes, g, pfx, M, E)
    # a prefix of zero bytes does not run into the zeros beyond the stream's end
    d = bytearray([FILL]) * (2 * bs + 1)
    d[2 * bs - 2:] = bytes(3)
    on, tables = writer_case(ctx, bytes(d), bs, 6, 3, bytes(4), what="zeros")
    assert tables[1] in (None, (bytes(32), 4))
    on, tables = writer_case(ctx, bytes(d), bs, 6, 3, bytes(3), what="zeros")
    assert tables[1] is not None and popcount(tables[1][0]) == 1


def test_self_overlapping_prefix(ctx):
    """`aaaa` with the prefix `aa`: every position starts a prefix."""
    bs = 4096
    for M, E in ME:
        d = bytes([FILL]) * (3 * bs + 100)
        on, tables = writer_case(ctx, d, bs, M, E, b"aa", what="all a")
        d = hand_built([bs, bs, bs, 100], [5, bs - 2, 2 * bs + 7, 3 * bs + 60], b"aaaa", fill=ord("b"))
        writer_case(ctx, d, bs, M, E, b"aa", what="aaaa")
        writer_case(ctx, d, bs, M, E, b"abab", what="abab")
    d = (b"ab" * (bs // 2 + 1000))[:2 * bs + 333]
    writer_case(ctx, d, bs, 6, 3, b"abab", what="abab everywhere")


@pytest.mark.parametrize("K", [2, 8, 256])
def test_writer_several_ranges(ctx, K):
    """A cut inside a prefix, a cut directly behind a prefix, three ranges with an empty middle range, a last range of 3 bytes: the bytes
    behind a range travel by value, across as many ranges as it takes, and every split gives the one-range stream."""
    bs = 64 << 10
    pfx = prefix_of(K) if K != 8 else LC.USER
    for M, E in ((6, 3), (1, 15)):
        for g in (2 * bs - K // 2, 2 * bs - K):                       # the cut at 2 * bs: inside the prefix, directly behind it
            d = bytearray(data_for("json_like", bs, 4, 3, random_block=None))
            d[g:g + K] = pfx
            d[4 * bs - K + 1:4 * bs + 1] = pfx                         # ... and a prefix that ends in the last range of 3 bytes
            d = bytes(d)
            one, _ = writer_case(ctx, d, bs, M, E, pfx)
            two, _ = writer_case(ctx, d, bs, M, E, pfx, True, cuts=[2 * bs])
            assert len(two) > len(one)
            for cuts in ([2 * bs], [2 * bs, 2 * bs], [2 * bs, 4 * bs], [bs, bs, 2 * bs, 2 * bs, 4 * bs, 4 * bs], [0, 2 * bs, 4 * bs]):
                assert writer_case(ctx, d, bs, M, E, pfx, cuts=cuts)[0] == one, cuts


# ---- Writer: arguments ----

def test_writer_arguments(ctx):
    L = _lib.lib()
    bs = 64 << 10
    d = synth.json_like(100_000, 2).tobytes()
    src = on_device([d])[0]
    sp, sl = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(len(d))
    out = torch.full((400_000,), 0x5A, dtype=torch.uint8, device="cuda")

    def cfg(prefix=LC.USER, m=6, e=3, k=None, reserved=(0, 0, 0, 0)):
        c = _lib.SearchLongPrefix()
        c.match_len, c.extras, c.prefix_len = m, e, len(prefix) if k is None else k
        for i, v in enumerate(reserved):
            c.reserved[i] = v
        for i, v in enumerate(prefix):
            c.prefix[i] = v
        return c

    def call(flags, c, cap=None):
        return L.mlz_stream_encode_gather_device_long_prefix(ctx.handle, 1, bs, flags, C.byref(c) if c is not None else None, sp, sl, 1, out.data_ptr(),
                                                             out.numel() if cap is None else cap)
    bad = [None, cfg(k=0), cfg(k=257), cfg(m=9), cfg(m=8, e=9), cfg(m=0, e=11), cfg(m=1, e=16), cfg(reserved=(0, 1, 0, 0)), cfg(reserved=(0, 0, 0, 255))]
    for c in bad:
        assert call(0, c) == -MLZ_ERR_ARG
    for flags in (4, 4 | 6 << 8, 3 << 8, 1 | 4):
        assert call(flags, cfg()) == -MLZ_ERR_ARG
    assert (out.cpu().numpy() == 0x5A).all()
    n = call(1, cfg(m=0))
    assert n > 0 and out[:n].cpu().numpy().tobytes() == gather(ctx, [d], bs, True, search_match_len=6, search_long_prefix=LC.USER, search_extras=3)        # match_len 0 = 6
    assert out[10:17].cpu().numpy().tobytes() == bytes([0x44, 3 + 2 + 8, 0, 0, 4, 6, 16]) and out[17:27].cpu().numpy().tobytes() == bytes([7, 3]) + LC.USER
    n = call(0, cfg(b"x" * 256, m=8, e=8))
    assert n > 0 and out[10:14].cpu().numpy().tobytes() == bytes([0x44, (3 + 258) & 255, (3 + 258) >> 8, 0])
    small = L.mlz_stream_bound_long_prefix(len(d), bs, 0, C.byref(cfg())) - 1
    assert small > 0 and call(0, cfg(), small) == -6                                                  # MLZ_ERR_DST_TOO_SMALL
    ptr = [src.data_ptr()], [len(d)], out.data_ptr(), out.numel()
    for kw in (dict(search_long_prefix=LC.USER), dict(search_match_len=6, search_long_prefix=LC.USER, search_prefix=b":"), dict(search_match_len=6, search_extras=3),
               dict(search_match_len=6, search_long_prefix=b""), dict(search_match_len=6, search_long_prefix=b"x" * 257),
               dict(search_match_len=8, search_long_prefix=b"x", search_extras=9), dict(search_match_len=9, search_long_prefix=b"x")):
        with pytest.raises(ValueError):
            ctx.stream_encode_gather_device(1, bs, False, *ptr, **kw)
    # the existing call keeps refusing type 4
    c4 = _lib.SearchTables()
    c4.table_type, c4.match_len = 4, 6
    assert L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, 0, C.byref(c4), sp, sl, 1, out.data_ptr(), out.numel()) == -MLZ_ERR_ARG
    assert gather(ctx, [b""], 4096, False, search_match_len=6, search_long_prefix=LC.USER, search_extras=3) == gather(ctx, [b""], 4096, False)             # an empty stream: no header, no info chunk


# ---- search ----

def check_search(sr, stream, d, pattern, what, cap=None, ignore_crc=False):
    want = SMod.brute(d, pattern)
    plan, sizes, usable = SMod.plan_of_stream(stream, pattern, ignore_crc)
    cap = len(want) + 3 if cap is None else cap
    total, pos, stats = sr(pattern, cap, ignore_crc=ignore_crc)
    assert total == len(want) and pos == want[:cap], what
    assert stats == (len(sizes), len(plan), usable), (what, stats, plan)
    assert SMod.chunks_touched(sizes, want, len(pattern)) <= set(plan), what
    total, pos, all_stats = sr(pattern, cap, ignore_crc=ignore_crc, no_tables=True)
    assert total == len(want) and pos == want[:cap] and all_stats == (len(sizes), sum(1 for n in sizes if n), 0), what + " (no tables)"
    return stats


@pytest.mark.parametrize("pfx,M,E", [(LC.USER, 6, 3), (LC.USER, 6, 0), (b'":"', 8, 8), (b'"user":"u', 1, 15)])
def test_search_over_the_writers_streams(ctx, pfx, M, E):
    bs, nblk = 64 << 10, 8
    d, pats = LC.designed("json_like", bs, nblk, 777, M, E, pfx)
    stream = gather(ctx, [d], bs, True, search_match_len=M, search_long_prefix=pfx, search_extras=E)
    assert SMod.read_tables(stream)[:2] == (SMod.config(4, M, pfx, E), 16)
    sr = Searcher(ctx, stream)
    try:
        res = {name: check_search(sr, stream, d, p, "K=%d M=%d E=%d %s" % (len(pfx), M, E, name)) for name, p in pats + SC.patterns(d, M, bs)}
        everything = (nblk + 1, nblk + 1, 0)
        assert res["late"] == everything and res["prefix_only"] == everything and res["absent"] == everything
        for name in ("p0", "inside", "two_groups", "straddle", "ends_on_last", "natural", "natural_inside", "absent_keyed"):
            assert res[name][2] == nblk + 1, name                        # the tables served the pattern
        if M >= 6:
            for name in ("p0", "inside", "two_groups", "straddle", "ends_on_last"):
                assert res[name][1] < nblk + 1, name
            assert res["absent_keyed"][1] <= 2
        # small caps
        frequent = b'","user":"user_'
        want = SMod.brute(d, frequent)
        assert len(want) > 100
        for cap in (0, 1, 7, len(want) - 1):
            check_search(sr, stream, d, frequent, "cap %d" % cap, cap=cap)
    finally:
        sr.close()


def test_search_foreign_streams(ctx):
    """Model-spliced streams of other writers: oracle level 1 and 2 blocks, a chunk without a table in the middle, stored chunks with tables."""
    bs, M, E = 64 << 10, 6, 3
    field = SMod.config(4, M, LC.USER, E)[2]
    d, pats = LC.designed("json_like", bs, 8, 777, M, E, LC.USER)
    r = bytearray(synth.random_bytes(3 * bs, seed=2).tobytes() + d[:2 * bs])
    r[bs + 100:bs + 100 + len(pats[0][1])] = pats[0][1]                      # an occurrence inside a stored chunk
    r = bytes(r)
    cases = []
    for level, obs in ((1, bs), (2, 1 << 20)):
        cases.append(("oracle L%d" % level, SMod.splice(O.stream_encode(d, level, obs), d, (4, M, field), SMod.table_bits(obs))[0], d))
    cases.append(("a table-less chunk in the middle", SMod.splice(O.stream_encode(d, 1, bs), d, (4, M, field), 16, skip=(4,))[0], d))
    cases.append(("stored chunks", SMod.splice(O.stream_encode(r, 1, bs), r, (4, M, field), 16, stored_too=True)[0], r))
    for name, stream, data in cases:
        assert O.stream_decode(stream, len(data)) == data, name
        sr = Searcher(ctx, stream)
        try:
            for pname, p in pats + [("random", r[bs + 5:bs + 21])]:
                check_search(sr, stream, data, p, "%s / %s" % (name, pname))
            if name.startswith("a table-less"):
                st = check_search(sr, stream, data, dict(pats)["p0"], name)
                assert st[2] == 8 and st[1] >= 2
        finally:
            sr.close()


def test_search_table_verdicts(ctx):
    """One table whose extras, or one prefix byte, differ from the info chunk's: its chunk is table-less.  An info chunk with M + E = 17 or
    a field cut short: the stream has no configuration.  The result is exact in every case."""
    bs, nblk, M, E = 64 << 10, 8, 8, 8
    K = len(LC.USER)
    d, pats = LC.designed("json_like", bs, nblk, 777, M, E, LC.USER)
    stream = gather(ctx, [d], bs, False, search_match_len=M, search_long_prefix=LC.USER, search_extras=E)
    (T, _, field), B, tables = SMod.read_tables(stream)
    p = dict(pats)["p0"]
    plan = SMod.plan_of_stream(stream, p)[0]
    skipped = next(k for k in range(1, nblk) if k not in plan)
    off = [c for c in SMod.chunks_of(stream) if c[1] == SMod.CHUNK_TABLE][skipped][0]
    t2 = list(tables); t2[skipped] = None
    for name, b in (("extras", stream[:off + 8] + bytes([E - 1]) + stream[off + 9:]), ("prefix byte", stream[:off + 9 + K - 1] + b"'" + stream[off + 9 + K:])):
        assert SMod.read_tables(b)[2] == t2
        sr = Searcher(ctx, b)
        try:
            for ignore in (False, True):
                st = check_search(sr, b, d, p, name, ignore_crc=ignore)
                assert st[2] == nblk and st[1] >= len(plan) + 1
            for pname, q in pats:
                check_search(sr, b, d, q, name + " / " + pname)
        finally:
            sr.close()
    ilen = 4 + 3 + 2 + K
    for name, b in (("M + E = 17", stream[:10] + SMod.info_chunk((4, M, bytes([K - 1, 9]) + LC.USER), B) + stream[10 + ilen:]),
                    ("short field", stream[:10] + SMod.frame(SMod.CHUNK_INFO, bytes([4, M, B]) + field[:5]) + stream[10 + ilen:])):
        assert SMod.read_tables(b)[0] is None
        sr = Searcher(ctx, b)
        try:
            assert check_search(sr, b, d, p, name)[1:] == (nblk + 1, 0)
        finally:
            sr.close()


@pytest.mark.parametrize("kind", SC.KINDS)
def test_designated_input_decodes_a_handful(ctx, kind):
    """128 x 64 KiB, prefix '"id":"', M = 6, E = 3, the needle '"id":"' + 10 random bytes at three places, one across a border: the library
    decodes exactly the chunks the model plans, 12 at the most (measured: 6 in every case, each of the 3 candidates and the chunk behind it)."""
    for seed in (1, 2, 3):
        bs, nblk = 64 << 10, 128
        d, nd, at = PC.planted_id(kind, bs, nblk, seed)
        stream = gather(ctx, [d], bs, False, search_match_len=6, search_long_prefix=LC.ID, search_extras=3)
        sr = Searcher(ctx, stream)
        try:
            st = check_search(sr, stream, d, nd, "%s seed %d" % (kind, seed))
            print(kind, seed, "decoded", st[1], "of", st[0], "tables", st[2], "stream", len(stream))
            assert st[0] == nblk and st[1] <= 12
            assert sorted(set(SMod.brute(d, nd)) & set(at)) == sorted(at)
        finally:
            sr.close()


def test_user_prefix_absent_pattern(ctx):
    """json_like, seed 2, 16 x 64 KiB + 777, prefix '"user":"', M = 6, E = 3: an absent record pattern decodes 2 chunks at the most, and
    the tables are about 1.6 % of the input."""
    bs, nblk = 64 << 10, 16
    d = synth.json_like(bs * nblk + 777, 2).tobytes()
    plain = gather(ctx, [d], bs, False)
    stream = gather(ctx, [d], bs, False, search_match_len=6, search_long_prefix=LC.USER, search_extras=3)
    print("tables", len(stream) - len(plain), "bytes of", len(d))
    sr = Searcher(ctx, stream)
    try:
        st = check_search(sr, stream, d, LC.ABSENT_USER, "absent")
        print("absent: decoded", st[1], "of", st[0])
        assert st[0] == nblk + 1 and st[2] == nblk + 1 and st[1] <= 2
        at = d.find(LC.USER, 5 * bs + 1000)
        st = check_search(sr, stream, d, d[at - 3:at + 19], "present")
        assert st[1] < nblk + 1
    finally:
        sr.close()
