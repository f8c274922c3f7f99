"""Search tables with byte prefixes (table types 2 and 3) written by the device-resident Writer (mlz_stream_encode_gather_device_tables,
HipCtx.stream_encode_gather_device(search_prefix=...)) and used by the pattern search (mlz_dev_reader_search), against
tests/search_model.py: the specification in plain Python.  The Writer's stream must be the table-less stream of the same call with
the model's chunks spliced in; a search must return what a brute-force search of the decoded bytes returns and decode exactly the chunks
the model's plan names."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, synth
from tests import search_cases as SC
from tests import search_model as SMod
from tests import search_prefix_cases as PC
from tests.search_gpu import Searcher, data_for, first_difference, gather, on_device

pytestmark = pytest.mark.gpu

TYPES = (1, 2, 3)       # these tests read a stream's tables as a searcher that knows the types 1 to 3

MLZ_ERR_ARG = 8
FILL = ord("a")          # in neither prefix set


def writer_case(ctx, d, bs, M, pset, add_index, cuts=None, what=""):
    """-> (stream, tables): the Writer's stream, equal to the model's splice of the table-less stream of the same call."""
    cuts = [0] + list(cuts or []) + [len(d)]
    ranges = [d[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    off = gather(ctx, ranges, bs, add_index)
    on = gather(ctx, ranges, bs, add_index, search_match_len=M, search_prefix=pset)
    T, field = SMod.field_of(pset)
    B = SMod.table_bits(bs)
    want, tables = SMod.splice(off, d, (T, M, field), B, index=add_index)
    what = "%s bs=%d M=%d T=%d index=%s ranges=%d" % (what, bs, M, T, add_index, len(ranges))
    assert len(on) == len(want) and on == want, what + ": lengths %d / %d, first difference at %d" % (len(on), len(want), first_difference(on, want))
    assert SMod.read_tables(on, types=TYPES) == ((T, M, field), B, tables), what
    assert mz.stream_decode(on, ctx=ctx) == d and O.stream_decode(on, len(d)) == d, what
    return on, tables


# ---- Writer: whole streams ----

@pytest.mark.parametrize("set_name", sorted(PC.SETS))
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 50), (64 << 10, 9), (1 << 20, 4), (8 << 20, 2)])
def test_writer_stream_is_the_models(ctx, kind, bs, nblk, set_name):
    d = data_for(kind, bs, nblk, 1234)
    on, tables = writer_case(ctx, d, bs, 6, PC.SETS[set_name], add_index=(bs in (64 << 10, 8 << 20)), what=kind)
    grid = SMod.data_grid(on)
    assert grid[1][1] == 0x01 and tables[1] is None and grid[-1][0] == 1234       # the incompressible block: stored, no table; a ragged tail
    assert sum(t is not None for t in tables) == len(tables) - 1


@pytest.mark.parametrize("M", [1, 2, 6, 8])
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 50), (64 << 10, 9)])
def test_writer_every_match_length(ctx, M, bs, nblk):
    d = data_for("json_like", bs, nblk, 1234)
    for set_name in sorted(PC.SETS):
        writer_case(ctx, d, bs, M, PC.SETS[set_name], add_index=(M % 2 == 0), what=set_name)


@pytest.mark.parametrize("M", [1, 6, 8])
def test_writer_several_ranges(ctx, M):
    """Two ranges, and three with the middle one empty: a range's last block indexes the window that lies in the next range's first M bytes."""
    bs = 64 << 10
    d = bytearray(data_for("json_like", bs, 4, 3, random_block=None))
    d[2 * bs - 1] = PC.PFX                                     # the last byte in front of the cut is a prefix byte
    d = bytes(d)
    for pset in PC.SETS.values():
        one, _ = writer_case(ctx, d, bs, M, pset, False)
        two, _ = writer_case(ctx, d, bs, M, pset, True, cuts=[2 * bs])
        assert writer_case(ctx, d, bs, M, pset, False, cuts=[2 * bs, 2 * bs])[0] == one
        assert writer_case(ctx, d, bs, M, pset, False, cuts=[2 * bs, 4 * bs])[0] == one      # a last range of 3 bytes: shorter than the overlap
        assert len(two) > len(one)


def test_type_1_through_the_new_call_is_the_flag_path(ctx):
    L = _lib.lib()
    bs = 64 << 10
    d = data_for("text_like", bs, 5, 99)
    src = on_device([d])[0]
    sp, sl = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(len(d))
    for M in (0, 1, 6, 8):
        for idx in (0, 1):
            want = gather(ctx, [d], bs, bool(idx), search_match_len=M)
            cfg = _lib.SearchTables()
            cfg.table_type, cfg.match_len = 1, M
            cap = L.mlz_stream_bound_tables(len(d), bs, idx, C.byref(cfg))
            assert cap == L.mlz_stream_bound(len(d), bs, idx | 4 | M << 8)
            dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            n = L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, idx, C.byref(cfg), sp, sl, 1, dst.data_ptr(), cap)
            assert n == len(want) and dst[:n].cpu().numpy().tobytes() == want, (M, idx)
            # without a configuration: the existing call
            n = L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, idx | 4 | M << 8, None, sp, sl, 1, dst.data_ptr(), cap)
            assert n == len(want) and dst[:n].cpu().numpy().tobytes() == want, (M, idx)
    plain = gather(ctx, [d], bs, False)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    assert L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, 0, None, sp, sl, 1, dst.data_ptr(), L.mlz_stream_bound(len(d), bs, 0)) == len(plain)
    assert dst[:len(plain)].cpu().numpy().tobytes() == plain


# ---- Writer: hand-built blocks ----

def tag(i):
    """8 letters that name plant i."""
    return bytes(97 + ((i * 7919 + 13 * j * (i + 1)) >> (2 * j)) % 26 for j in range(8))


def hand_built(sizes, plants):
    """Blocks of one filler byte (`sizes`: the bytes per block) with single prefix bytes at the stream positions `plants`, each followed by
    letters that name it (written first, so that a neighbouring plant's prefix byte stays)."""
    d = bytearray([FILL]) * sum(sizes)
    for i, g in enumerate(plants):
        t = tag(i)[:max(0, len(d) - g - 1)]
        d[g + 1:g + 1 + len(t)] = t
    for g in plants:
        d[g] = PC.PFX
    return bytes(d)


def indexed_by_rule(sizes, plants, M):
    """How many plants the rule indexes: the position behind plant g is q = g + 1 - (its block's start), within 1 .. n (a block that is not
    the last) or 1 .. n - M (the last)."""
    starts = np.concatenate([[0], np.cumsum(sizes)])
    cnt = 0
    for g in plants:
        k = int(np.searchsorted(starts, g, side="right")) - 1
        q, n = g + 1 - int(starts[k]), sizes[k]
        cnt += q <= (n if k + 1 < len(sizes) else n - M)
    return cnt


def hand_case(ctx, bs, sizes, plants, M, pset=b":"):
    assert all(s == bs for s in sizes[:-1]) and len(set(plants)) == len(plants)
    d = hand_built(sizes, plants)
    on, tables = writer_case(ctx, d, bs, M, pset, False, what="hand-built")
    T, field = SMod.field_of(pset)
    B = SMod.table_bits(bs)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    n_idx = sum(len(SMod.indexed_hashes((T, M, field), d[starts[k]:starts[k + 1]], d[starts[k + 1]:starts[k + 1] + 8] if k + 1 < len(sizes) else None, B)) for k in range(len(sizes)))
    assert n_idx == indexed_by_rule(sizes, plants, M), "the model and the rule, written out, disagree"
    return d, on, tables


@pytest.mark.parametrize("M", [1, 6, 8])
def test_hand_built_block_edges(ctx, M):
    """64 KiB blocks: a prefix byte as a block's last byte (a middle block: position n, in the next block's bytes; the last block: nothing),
    as its first byte, at the end of a lane's 8 positions and of a sweep of 8192, and around the last block's limit n - M."""
    bs, tail = 64 << 10, 1000
    sizes = [bs, bs, bs, tail]
    end = 3 * bs + tail
    plants = [bs - 1, 2 * bs - 1, 2 * bs, 0, 6, 7, 8, 8190, 8191, 8192, bs + 8191, 3 * bs - 1, end - 1, end - M - 1, end - M, end - M - 2, 3 * bs]
    d, on, tables = hand_case(ctx, bs, sizes, sorted(set(plants)), M)
    assert all(t is not None for t in tables)
    # every plant alone, at the places where a neighbour could hide a mistake
    for g in (bs - 1, 0, 7, 8191, end - M - 1, end - M):
        d1, _, t1 = hand_case(ctx, bs, sizes, [g], M)
        k = min(g // bs, 3)
        others = [t for i, t in enumerate(t1) if i != k]
        assert all(t == (bytes(32), 8) for t in others), g
        indexed = indexed_by_rule(sizes, [g], M)
        assert (t1[k] != (bytes(32), 8)) == bool(indexed), g
        if indexed:
            assert sum(bin(b).count("1") for b in t1[k][0]) == 1, g


def test_hand_built_parts_and_slices(ctx):
    """1 MiB blocks (several workgroups take parts of at least 64 KiB of a block) and 2 MiB blocks (B = 21: two slices of the table, each
    in a workgroup of its own): prefix bytes around every 64 KiB step and around the steps of a split into 2 .. 32 equal parts."""
    for bs, nblk in ((1 << 20, 2), (2 << 20, 2)):
        sizes = [bs] * nblk + [5000]
        plants = set()
        for m in range(64 << 10, bs + 1, 64 << 10):
            plants.update((m - 2, m - 1, m, bs + m - 1))
        for parts in (2, 3, 5, 8, 16, 32):
            per = -(-(-(-(bs + 1) // parts)) // 8) * 8          # the positions 0 .. bs in `parts` shares, rounded up to 8
            plants.update(p * per + o for p in range(1, parts) for o in (-2, -1, 0) if p * per < bs)
        plants.update((0, bs - 1, nblk * bs - 1, nblk * bs + 4999))
        d, on, tables = hand_case(ctx, bs, sizes, sorted(plants), 6)
        assert all(t is not None for t in tables) and tables[0][1] < SMod.table_bits(bs) - 8


@pytest.mark.parametrize("M", [2, 6, 8])
def test_hand_built_short_next_block(ctx, M):
    """A prefix byte as the last byte in front of a last block of 1 .. M - 1 bytes: its window takes zeros beyond the stream's end."""
    bs = 4096
    for t in range(1, M):
        sizes = [bs, bs, t]
        d, on, tables = hand_case(ctx, bs, sizes, [bs - 1, 2 * bs - 1], M)
        assert tables[1] != (bytes(32), 4) and tables[2] in (None, (bytes(32), 4))      # (a last block of a few bytes may be stored)
        # the same bytes as two ranges: the short block comes by value
        assert writer_case(ctx, d, bs, M, b":", False, cuts=[2 * bs])[0] == on


def test_hand_built_empty_tables(ctx):
    """No prefix byte in a block, and the empty type 3 mask: the zero table of 32 bytes with R = B - 8, which lets a searcher skip the block."""
    bs = 64 << 10
    d = hand_built([bs, bs, 500], [bs + 5])
    on, tables = writer_case(ctx, d, bs, 6, b":", False)
    assert tables[0] == tables[2] == (bytes(32), 8) and tables[1] != tables[0]
    text = data_for("text_like", bs, 3, 500)
    on, tables = writer_case(ctx, text, bs, 6, b"", True)
    assert SMod.read_tables(on, types=TYPES)[0][0] == 3 and on[10:17] == bytes([0x44, 35, 0, 0, 3, 6, 16]) and on[17:49] == bytes(32)
    assert tables == [(bytes(32), 8), None, (bytes(32), 8), (bytes(32), 8)]               # (block 1 is incompressible: stored, no table)
    sr = Searcher(ctx, on)
    try:
        check_search(sr, on, text, text[2 * bs + 100:2 * bs + 116], "empty mask")
    finally:
        sr.close()


# ---- Writer: arguments ----

def test_writer_arguments(ctx):
    L = _lib.lib()
    bs = 64 << 10
    d = synth.text_like(100_000, 2).tobytes()
    src = on_device([d])[0]
    sp, sl = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(len(d))
    out = torch.full((400_000,), 0x5A, dtype=torch.uint8, device="cuda")

    def cfg(T, m=6, n=1, reserved=0):
        c = _lib.SearchTables()
        c.table_type, c.match_len, c.n_prefix, c.reserved = T, m, n, reserved
        c.prefix[0] = PC.PFX
        return c

    def call(flags, c):
        return L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, flags, C.byref(c) if c is not None else None, sp, sl, 1, out.data_ptr(), out.numel())
    for c in (cfg(0), cfg(4), cfg(255), cfg(2, m=9), cfg(2, n=0), cfg(2, n=9), cfg(1, reserved=1), cfg(3, reserved=7)):
        assert call(0, c) == -MLZ_ERR_ARG and L.mlz_stream_bound_tables(len(d), bs, 0, C.byref(c)) == -MLZ_ERR_ARG
    for flags in (4, 4 | 6 << 8, 3 << 8, 1 | 4):
        assert call(flags, cfg(2)) == -MLZ_ERR_ARG and L.mlz_stream_bound_tables(len(d), bs, flags, C.byref(cfg(2))) == -MLZ_ERR_ARG
    assert (out.cpu().numpy() == 0x5A).all()
    n = call(1, cfg(2, m=0))
    assert n > 0 and out[:n].cpu().numpy().tobytes() == gather(ctx, [d], bs, True, search_match_len=6, search_prefix=b":")        # match_len 0 = 6
    assert call(0, cfg(3, n=200)) > 0                                                                # n_prefix is ignored outside type 2
    c8 = cfg(2, n=8)
    for i, v in enumerate(b":,\" ={}["):
        c8.prefix[i] = v
    n = call(0, c8)
    assert n > 0 and out[17:25].cpu().numpy().tobytes() == b":,\" ={}["                             # the values in the order given
    small = L.mlz_stream_bound_tables(len(d), bs, 0, C.byref(cfg(2))) - 1
    assert small > 0 and L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, bs, 0, C.byref(cfg(2)), sp, sl, 1, out.data_ptr(), small) == -6   # MLZ_ERR_DST_TOO_SMALL
    with pytest.raises(ValueError):
        ctx.stream_encode_gather_device(1, bs, False, [src.data_ptr()], [len(d)], out.data_ptr(), out.numel(), search_prefix=b":")
    # the existing calls return what they did
    for b2 in (4 << 10, 64 << 10, 8 << 20):
        n2, B = 3 * b2 + 5, SMod.table_bits(b2)
        assert L.mlz_stream_bound(n2, b2, 4) == L.mlz_stream_bound(n2, b2, 0) + 7 + 4 * (12 + max(32, 1 << (B - 3)))
    assert gather(ctx, [b""], 4096, False, search_match_len=6, search_prefix=b":") == gather(ctx, [b""], 4096, False)                 # an empty stream: no header, no info chunk


# ---- search ----

def check_search(sr, stream, d, pattern, what, cap=None, ignore_crc=False):
    want = SMod.brute(d, pattern)
    cfg, B, tables = SMod.read_tables(stream, ignore_crc, TYPES)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    plan = SMod.plan(tables, sizes, pattern, cfg, B)
    cap = len(want) + 3 if cap is None else cap
    total, pos, stats = sr(pattern, cap, ignore_crc=ignore_crc)
    assert total == len(want) and pos == want[:cap], what
    assert stats == (len(sizes), len(plan), SMod.usable_tables(tables, pattern, cfg)), (what, stats, plan)
    assert SMod.chunks_touched(sizes, want, len(pattern)) <= set(plan), what
    total, pos, all_stats = sr(pattern, cap, ignore_crc=ignore_crc, no_tables=True)
    assert total == len(want) and pos == want[:cap] and all_stats == (len(sizes), sum(1 for n in sizes if n), 0), what + " (no tables)"
    return stats


@pytest.mark.parametrize("set_name,M", [("json4", 6), ("nonalnum", 6), ("json4", 1), ("nonalnum", 8), ("json4", 2)])
def test_search_over_the_writers_streams(ctx, set_name, M):
    bs, nblk = 64 << 10, 8
    pset = PC.SETS[set_name]
    d, pats = PC.designed("json_like", bs, nblk, 777, M, pset)
    stream = gather(ctx, [d], bs, True, search_match_len=M, search_prefix=pset)
    T, field = SMod.field_of(pset)
    assert SMod.read_tables(stream, types=TYPES)[:2] == ((T, M, field), 16)
    sr = Searcher(ctx, stream)
    try:
        res = {name: check_search(sr, stream, d, p, "%s M=%d %s" % (set_name, M, name)) for name, p in pats + SC.patterns(d, M, bs)}
        assert res["unusable"][1:] == (nblk + 1, 0) and res["one_window"][2] == nblk + 1
        if M >= 6:
            assert res["one_window"][1] < nblk + 1 and res["border_last"][1] < nblk + 1 and res["absent_keyed"][1] <= 2
        # a small cap
        frequent = b'","user":"user_'
        want = SMod.brute(d, frequent)
        assert len(want) > 100
        for cap in (1, 7, len(want) - 1):
            check_search(sr, stream, d, frequent, "cap %d" % cap, cap=cap)
    finally:
        sr.close()


def test_search_foreign_streams(ctx):
    """Model-spliced streams of other writers: oracle level 1 and 2 blocks, stored chunks with tables, a chunk without a table in the middle."""
    bs, M = 64 << 10, 6
    pset = PC.SETS["json4"]
    T, field = SMod.field_of(pset)
    d, pats = PC.designed("json_like", bs, 8, 777, M, pset)
    r = synth.random_bytes(3 * bs, seed=2).tobytes() + d[:2 * bs]
    cases = []
    for level, obs in ((1, bs), (2, 1 << 20)):
        cases.append(("oracle L%d" % level, SMod.splice(O.stream_encode(d, level, obs), d, (T, M, field), SMod.table_bits(obs))[0], d))
    cases.append(("a table-less chunk in the middle", SMod.splice(O.stream_encode(d, 1, bs), d, (T, M, field), 16, skip=(4,))[0], d))
    T3, field3 = SMod.field_of(PC.SETS["nonalnum"])
    cases.append(("type 3", SMod.splice(O.stream_encode(d, 1, bs), d, (T3, M, field3), 16)[0], d))
    cases.append(("stored chunks", SMod.splice(O.stream_encode(r, 1, bs), r, (T, M, field), 16, stored_too=True)[0], r))
    for name, stream, data in cases:
        assert O.stream_decode(stream, len(data)) == data, name
        sr = Searcher(ctx, stream)
        try:
            for pname, p in pats + [("random", r[bs + 5:bs + 21])]:
                check_search(sr, stream, data, p, "%s / %s" % (name, pname))
            if name.startswith("a table-less"):
                st = check_search(sr, stream, data, dict(pats)["one_window"], name)
                assert st[2] == 8 and st[1] >= 2
        finally:
            sr.close()


def test_search_patched_prefix_field(ctx):
    """One table whose prefix field differs from the info chunk's: its chunk is table-less, the result is still exact."""
    bs, nblk, M = 64 << 10, 8, 6
    pset = PC.SETS["json4"]
    d, pats = PC.designed("json_like", bs, nblk, 777, M, pset)
    stream = gather(ctx, [d], bs, False, search_match_len=M, search_prefix=pset)
    cfg, B, tables = SMod.read_tables(stream, types=TYPES)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    p = dict(pats)["one_window"]
    plan = SMod.plan(tables, sizes, p, cfg, B)
    skipped = next(k for k in range(1, nblk) if k not in plan)
    tabs = [c for c in SMod.chunks_of(stream) if c[1] == SMod.CHUNK_TABLE]
    b = bytearray(stream)
    b[tabs[skipped][0] + 4 + 3 + 7] ^= 0x20
    b = bytes(b)
    t2 = list(tables); t2[skipped] = None
    assert SMod.read_tables(b, types=TYPES)[2] == t2
    sr = Searcher(ctx, b)
    try:
        for ignore in (False, True):
            st = check_search(sr, b, d, p, "patched field", ignore_crc=ignore)
            assert st[2] == nblk and st[1] >= len(plan) + 1
        for name, q in pats:
            check_search(sr, b, d, q, "patched field / " + name)
    finally:
        sr.close()
    # a type 4 info chunk: the stream has no configuration
    b = stream[:14] + b"\x04" + stream[15:]
    sr = Searcher(ctx, b)
    try:
        assert check_search(sr, b, d, p, "type 4 info")[1:] == (nblk + 1, 0)
    finally:
        sr.close()


@pytest.mark.parametrize("set_name", sorted(PC.SETS))
@pytest.mark.parametrize("kind", SC.KINDS)
def test_designated_input_decodes_a_handful(ctx, kind, set_name):
    """128 x 64 KiB, M = 6, the needle '"id":"' + 10 random bytes: the library decodes exactly the chunks the model plans, 12 at the most."""
    pset = PC.SETS[set_name]
    for seed in (1, 2, 3):
        bs, nblk = 64 << 10, 128
        d, nd, at = PC.planted_id(kind, bs, nblk, seed)
        stream = gather(ctx, [d], bs, False, search_match_len=6, search_prefix=pset)
        sr = Searcher(ctx, stream)
        try:
            st = check_search(sr, stream, d, nd, "%s %s seed %d" % (kind, set_name, seed))
            print(kind, set_name, seed, "decoded", st[1], "of", st[0], "tables", st[2], "stream", len(stream))
            assert st[0] == nblk and st[1] <= 12
            assert sorted(set(SMod.brute(d, nd)) & set(at)) == sorted(at)
        finally:
            sr.close()
