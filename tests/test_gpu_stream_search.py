"""Block search tables written by the device-resident Writer (MLZ_STREAM_SEARCH_TABLES on mlz_stream_encode_gather_device) and the pattern
search over streams in HBM (mlz_dev_reader_search, DeviceReader.search, DeviceStream.search), against tests/search_model.py: the
specification in plain Python.  The Writer's stream must be the flag-off stream of the same call with the model's chunks spliced in; a
search must return what a brute-force search of the decoded bytes returns and decode exactly the chunks the model's plan rule names."""
import io

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, stream as S, synth
from tests import search_cases as SC
from tests import search_model as SMod
from tests.search_gpu import Searcher, data_for, gather

pytestmark = pytest.mark.gpu

TYPES = (1,)            # these tests read a stream's tables as a searcher that knows type 1 alone

MLZ_ERR_ARG = 8


def check_stream(ctx, stream, d, bs, M, add_index, what):
    """Every reader returns the original bytes."""
    assert mz.stream_decode(stream, ctx=ctx) == d, what
    assert O.stream_decode(stream, len(d)) == d, what
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    out = torch.empty(len(d) + 1, dtype=torch.uint8, device="cuda")
    assert ctx.stream_decode_device(t.data_ptr(), t.numel(), out.data_ptr(), len(d)) == len(d), what
    assert out[:len(d)].cpu().numpy().tobytes() == d, what
    with ctx.stream_open_device(t.data_ptr(), t.numel()) as rd:
        assert rd.size == len(d)
        o, n = 2 * bs - 100, min(bs + 300, len(d) - (2 * bs - 100))
        assert rd.read([(o, n, 0)], out.data_ptr(), n) == n and out[:n].cpu().numpy().tobytes() == d[o:o + n], what
    if add_index:
        rs = S.ReadSeeker(stream, backend=S.HipBackend(ctx))
        for o in (0, bs - 5, 2 * bs + 17, len(d) - 40):
            assert rs.ReadAt(60, o) == d[o:o + 60], (what, o)


def writer_case(ctx, kind, bs, nblk, M, add_index, parts=1, mctx=None):
    d = data_for(kind, bs, nblk, 1234)
    cut = [0] + [((nblk * i) // parts) * bs for i in range(1, parts)] + [len(d)]
    ranges = [d[cut[i]:cut[i + 1]] for i in range(parts)]
    c = mctx or ctx
    off = gather(c, ranges, bs, add_index)
    on = gather(c, ranges, bs, add_index, search_match_len=M)
    B = SMod.table_bits(bs)
    want, tables = SMod.splice(off, d, SMod.config(1, M), B, index=add_index)
    what = "%s bs=%d M=%d index=%s parts=%d" % (kind, bs, M, add_index, parts)
    assert len(on) == len(want), what
    assert on == want, what + ": first difference at %d" % next(i for i in range(len(on)) if on[i] != want[i])
    grid = SMod.data_grid(on)
    assert grid[1][1] == 0x01 and tables[1] is None and grid[-1][0] == 1234, what   # the incompressible block: stored, no table; a short last block
    assert sum(t is not None for t in tables) >= (len(tables) // 2 if M >= 4 else 0), what
    assert SMod.read_tables(on, types=TYPES)[2] == tables
    check_stream(ctx, on, d, bs, M, add_index, what)
    return on, d, tables


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 50), (64 << 10, 9), (1 << 20, 4), (8 << 20, 2)])
def test_writer_stream_is_the_models(ctx, kind, bs, nblk):
    writer_case(ctx, kind, bs, nblk, 6, add_index=(bs in (64 << 10, 8 << 20)))


@pytest.mark.parametrize("M", [1, 2, 4, 6, 8])
@pytest.mark.parametrize("bs,nblk", [(4 << 10, 30), (1 << 20, 3)])
def test_writer_every_match_length(ctx, M, bs, nblk):
    writer_case(ctx, "json_like", bs, nblk, M, add_index=(M % 2 == 0))


def test_writer_default_match_length_and_index_both_ways(ctx):
    d = data_for("text_like", 64 << 10, 40, 99, random_block=None)
    for idx in (False, True):
        a, b = gather(ctx, [d], 64 << 10, idx, search_match_len=0), gather(ctx, [d], 64 << 10, idx, search_match_len=6)
        assert a == b and a[10:17] == bytes([0x44, 3, 0, 0, 1, 6, 16])


def test_writer_several_ranges_on_two_contexts(ctx):
    m = mz.Context(devices=[0, 0])
    try:
        for bs, nblk, parts in ((64 << 10, 12, 3), (1 << 20, 4, 2), (4 << 10, 40, 4)):
            for M in (6, 8):
                writer_case(ctx, "enwik_like", bs, nblk, M, add_index=True, parts=parts, mctx=m)
        # an empty range between two others, and a last range shorter than the overlap
        bs = 64 << 10
        d = data_for("text_like", bs, 4, 3)
        off = gather(m, [d[:2 * bs], b"", d[2 * bs:4 * bs], d[4 * bs:]], bs, False)
        on = gather(m, [d[:2 * bs], b"", d[2 * bs:4 * bs], d[4 * bs:]], bs, False, search_match_len=6)
        assert on == SMod.splice(off, d, SMod.config(1, 6), 16)[0]
    finally:
        m.close()


def test_writer_arguments(ctx):
    L = _lib.lib()
    d = np.frombuffer(synth.text_like(100_000, 2).tobytes(), np.uint8)
    dst = np.empty(300_000, np.uint8)
    assert L.mlz_stream_encode(ctx.handle, 1, 64 << 10, 4, d.ctypes.data, d.size, dst.ctypes.data, dst.size) == -MLZ_ERR_ARG
    assert L.mlz_stream_encode(ctx.handle, 1, 64 << 10, 0, d.ctypes.data, d.size, dst.ctypes.data, dst.size) > 0
    for m in range(9, 16):
        assert L.mlz_stream_bound(1000, 4096, 4 | m << 8) == -MLZ_ERR_ARG
        t = torch.from_numpy(d.copy()).cuda()
        out = torch.empty(400_000, dtype=torch.uint8, device="cuda")
        with pytest.raises(mz.MinLZError) as e:
            ctx.stream_encode_gather_device(1, 64 << 10, False, [t.data_ptr()], [t.numel()], out.data_ptr(), out.numel(), search_match_len=m)
        assert int(str(e.value).split()[2]) == MLZ_ERR_ARG
    for bs in (4 << 10, 64 << 10, 8 << 20):
        n = 3 * bs + 5
        B = SMod.table_bits(bs)
        assert L.mlz_stream_bound(n, bs, 4) == L.mlz_stream_bound(n, bs, 0) + 7 + 4 * (12 + max(32, 1 << (B - 3)))
    assert gather(ctx, [b""], 4096, False, search_match_len=6) == gather(ctx, [b""], 4096, False)   # an empty stream: no header, no info chunk


# ---- search ----

def check_search(sr, stream, d, pattern, what, cap=None, ignore_crc=False):
    want = SMod.brute(d, pattern)
    cfg, B, tables = SMod.read_tables(stream, ignore_crc, TYPES)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    plan = SMod.plan(tables, sizes, pattern, cfg, B, use_tables=any(t is not None for t in tables))
    cap = len(want) + 3 if cap is None else cap
    total, pos, stats = sr(pattern, cap, ignore_crc=ignore_crc)
    assert total == len(want) and pos == want[:cap], what
    usable = sum(t is not None for t in tables) if cfg is not None and len(pattern) >= cfg[1] else 0
    assert stats == (len(sizes), len(plan), usable), what
    assert SMod.chunks_touched(sizes, want, len(pattern)) <= set(plan), what
    total, pos, all_stats = sr(pattern, cap, ignore_crc=ignore_crc, no_tables=True)
    assert total == len(want) and pos == want[:cap] and all_stats == (len(sizes), sum(1 for n in sizes if n), 0), what + " (no tables)"
    return stats   # (of the search with tables)


def search_data(bs, nblk, tail, M, seed=5):
    """Text with a needle planted inside a block, across two blocks and ending in the short last block, and a run of 'a' over a border."""
    d = bytearray(synth.text_like(bs * nblk + tail, seed).tobytes())
    nd = bytes(SC.needle(16, seed))
    for o in (2 * bs + 1000, 4 * bs - 7, len(d) - 16):
        d[o:o + 16] = nd
    d[5 * bs - 20:5 * bs + 30] = b"a" * 50
    big = bytes(SC.needle(256, seed + 1))
    d[6 * bs - 100:6 * bs + 156] = big
    d[bs + 77:bs + 77 + 256] = big
    return bytes(d), nd, big


def pattern_set(d, nd, big, M, bs):
    pats = [("planted", nd), ("aaaa", b"aaaa"), ("L256", big), ("absent", bytes(SC.needle(16, 77))), ("L1", d[3 * bs + 5:3 * bs + 6]), ("L1_rare", b"\x00")]
    if M > 1:
        pats.append(("L_M-1", nd[:M - 1]))
    pats += [("L_M", nd[:M]), ("L_M+1", nd[:M + 1]), ("border_M", d[bs - M // 2:bs - M // 2 + M])]
    return pats


@pytest.mark.parametrize("M", [1, 2, 6, 8])
def test_search_over_the_writers_streams(ctx, M):
    bs = 64 << 10
    d, nd, big = search_data(bs, 9, 500, M)
    stream = gather(ctx, [d], bs, True, search_match_len=M)
    sr = Searcher(ctx, stream)
    try:
        for name, p in pattern_set(d, nd, big, M, bs):
            check_search(sr, stream, d, p, "M=%d %s" % (M, name))
        # cap below the total, cap = 0 with NULL
        want = SMod.brute(d, b"aaaa")
        assert len(want) >= 47
        for cap in (1, 5, len(want) - 1, len(want)):
            check_search(sr, stream, d, b"aaaa", "cap %d" % cap, cap=cap)
        total, pos, _ = sr(b"aaaa", 0, null=True)
        assert total == len(want) and pos == []
        # the tensor front end
        with shard.HipTensorCodec(ctx).open_stream(sr.t) as ds:
            t, total = ds.search(nd, 2)
            assert total == 3 and t.dtype == torch.int64 and t.is_cuda and t.cpu().tolist() == SMod.brute(d, nd)[:2]
    finally:
        sr.close()


def test_search_streams_without_tables_and_foreign_streams(ctx):
    bs = 64 << 10
    d, nd, big = search_data(bs, 9, 500, 6)
    cases = [("flag off", gather(ctx, [d], bs, False))]
    w = io.BytesIO()
    wr = S.Writer(w, level=1, block_size=bs, concurrency=4, backend=S.HipBackend(ctx))
    for a, b in ((0, 100), (100, 3 * bs + 7), (3 * bs + 7, 3 * bs + 9), (3 * bs + 9, len(d))):   # short interior blocks, one shorter than the pattern
        wr.Write(d[a:b])
        wr.Flush()
    wr.Close()
    cases.append(("python writer with Flush", w.getvalue()))
    for level, obs in ((1, bs), (2, 1 << 20)):
        o = O.stream_encode(d, level, obs)
        cases.append(("oracle L%d" % level, o))
        cases.append(("oracle L%d spliced" % level, SMod.splice(o, d, SMod.config(1, 6), SMod.table_bits(obs))[0]))
    # (the block in front of the 2-byte block gets a table that saw those 2 bytes and zeros: a writer that looks at the next chunk alone)
    cases.append(("python writer spliced, stored chunks too", SMod.splice(w.getvalue(), d, SMod.config(1, 6), 16, stored_too=True, next_chunk_only=True)[0]))
    r = synth.random_bytes(3 * bs, seed=2).tobytes() + d[:2 * bs]
    cases.append(("stored chunks spliced", SMod.splice(O.stream_encode(r, 1, bs), r, SMod.config(1, 6), 16, stored_too=True)[0]))
    for name, stream in cases:
        data = r if name.startswith("stored") else d
        assert O.stream_decode(stream, len(data)) == data, name
        sr = Searcher(ctx, stream)
        try:
            for pname, p in pattern_set(data, nd, big, 6, bs)[:6] + [("random", r[bs + 5:bs + 21])]:
                check_search(sr, stream, data, p, "%s / %s" % (name, pname))
        finally:
            sr.close()
    for empty in (b"", O.stream_encode(b"", 1, bs)):
        sr = Searcher(ctx, empty)
        try:
            assert sr(b"abc", 4) == (0, [], (0, 0, 0)) and sr(b"abc", 0, null=True, no_tables=True) == (0, [], (0, 0, 0))
        finally:
            sr.close()


def test_search_many_chunks_cross_group_borders(ctx):
    """More than one 64 MiB group of decoded chunks, runs of neighbouring chunks that cross the group border."""
    bs = 1 << 20
    base = synth.json_like(8 << 20, 9).tobytes()
    d = bytearray(base * 18)[:(140 << 20) + 321]
    nd = bytes(SC.needle(40, 12))
    for o in (5, (64 << 20) - 20, (64 << 20) - 40, (64 << 20), (128 << 20) - 1, len(d) - 40):
        d[o:o + 40] = nd
    d = bytes(d)
    stream = gather(ctx, [d], bs, False, search_match_len=6)
    sr = Searcher(ctx, stream)
    try:
        st = check_search(sr, stream, d, nd, "many chunks")
        assert st[1] <= 20
        check_search(sr, stream, d, b'": ', "frequent", cap=1000)
    finally:
        sr.close()


@pytest.mark.parametrize("kind", SC.KINDS)
def test_designated_input_decodes_a_handful(ctx, kind):
    for seed in (1, 2, 3):
        bs, nblk = 64 << 10, 128
        d, nd, at = SC.planted(kind, bs, nblk, 16, seed)
        stream = gather(ctx, [d], bs, False, search_match_len=6)
        sr = Searcher(ctx, stream)
        try:
            st = check_search(sr, stream, d, nd, "%s seed %d" % (kind, seed))
            print(kind, seed, "decoded", st[1], "of", st[0], "tables", st[2])
            assert st[0] == nblk and st[1] <= 12
            assert sorted(set(SMod.brute(d, nd)) & set(at)) == sorted(at)
        finally:
            sr.close()


def test_broken_table_and_broken_chunks(ctx):
    bs, nblk = 64 << 10, 16
    d, nd, at = SC.planted("text_like", bs, nblk, 16, 2)
    stream = gather(ctx, [d], bs, False, search_match_len=6)
    cfg, B, tables = SMod.read_tables(stream, types=TYPES)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    plan = SMod.plan(tables, sizes, nd, cfg, B)
    assert len(plan) < nblk - 2
    skipped = next(k for k in range(nblk) if k not in plan)
    tabs = [c for c in SMod.chunks_of(stream) if c[1] == SMod.CHUNK_TABLE]
    datas = [c for c in SMod.chunks_of(stream) if c[1] in (1, 2, 3)]
    assert len(tabs) == nblk
    # a table with one more bit set and its old CRC: table-less with the CRC check, used without it
    b = bytearray(stream)
    p = tabs[skipped][0] + 12
    i = next(i for i in range(32) if b[p + i] != 0xFF)
    b[p + i] |= (~b[p + i] & 0xFF) & -(~b[p + i] & 0xFF)
    b = bytes(b)
    sr = Searcher(ctx, b)
    try:
        st = check_search(sr, b, d, nd, "flipped table bit")
        assert st[2] == nblk - 1 and st[1] >= len(plan) + 1
        st = check_search(sr, b, d, nd, "flipped table bit, ignore_crc", ignore_crc=True)
        assert st[2] == nblk
        st = check_search(sr, b, d, nd, "flipped table bit, again with the check")
        assert st[2] == nblk - 1
    finally:
        sr.close()
    # a corrupt chunk the plan skips goes unnoticed; a corrupt chunk it needs gives its error
    for k, want_err in ((skipped, False), (plan[0], True)):
        b = bytearray(stream)
        b[datas[k][0] + 5] ^= 0x40          # the chunk's CRC
        sr = Searcher(ctx, bytes(b))
        try:
            if want_err:
                with pytest.raises(mz.ErrCRC):
                    sr(nd, 10)
                assert sr(nd, 10, ignore_crc=True)[:2] == (3, SMod.brute(d, nd))
                with pytest.raises(mz.ErrCRC):
                    sr(nd, 10, no_tables=True)
            else:
                assert sr(nd, 10)[:2] == (3, SMod.brute(d, nd))
                with pytest.raises(mz.ErrCRC):
                    sr(nd, 10, no_tables=True)
        finally:
            sr.close()
    b = bytearray(stream)
    body = datas[plan[0]]
    b[body[0] + 8 + 3 + 40:body[0] + 8 + 3 + 60] = b"\xff" * 20   # token bytes of a needed chunk
    sr = Searcher(ctx, bytes(b))
    try:
        with pytest.raises(mz.MinLZError):
            sr(nd, 10)
    finally:
        sr.close()


def test_search_arguments(ctx):
    L = _lib.lib()
    stream = O.stream_encode(b"hello hello hello", 1, 4096)
    sr = Searcher(ctx, stream)
    try:
        out = torch.zeros(4, dtype=torch.int64, device="cuda")
        host = np.zeros(4, np.uint64)
        h = sr.rd.handle
        pat = b"x" * 300
        assert L.mlz_dev_reader_search(h, None, 0, pat, 0, out.data_ptr(), 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(h, None, 0, pat, 257, out.data_ptr(), 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(h, None, 0, None, 3, out.data_ptr(), 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(h, None, 0, pat, 3, None, 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(h, None, 0, pat, 3, host.ctypes.data, 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(None, None, 0, pat, 3, out.data_ptr(), 4, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_search(h, None, 0, b"hello", 5, out.data_ptr(), 4, None) == 3 and out.cpu().tolist() == [0, 6, 12, 0]
        assert L.mlz_dev_reader_search(h, None, 0, b"llo h", 5, None, 0, None) == 2
        assert L.mlz_dev_reader_search(h, None, 0, pat, 256, out.data_ptr(), 4, None) == 0
    finally:
        sr.close()
