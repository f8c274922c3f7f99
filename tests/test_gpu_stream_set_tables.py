"""mlz_stream_open_batch_device_tables (Context.stream_open_batch_device(tables=True), HipTensorCodec.open_streams(tables=True)) on the GPU: a set
of streams whose searches and greps prune by every stream's inline search tables.  Every test compares the tabled set with the plain set of
the same streams (all outputs equal), with Python over the decoded bytes (what is found), with the model's plan (tests/set_tables_model.py:
stats[1] and mlz_dev_reader_set_tables_info) and with no_tables=True (the plain set's decoded count).  Every output buffer has a guard band."""
import re

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import api, shard, synth
from tests import corrupt as CM
from tests import regex_model as RM
from tests import regex_prune_model as RP
from tests import search_model as SMod
from tests import set_tables_model as M
from tests import stream_batch_cases as BC
from tests import stream_set_model as SS
from tests.search_gpu import gather
from tests.test_gpu_stream_search_batch import Batch
from tests.test_gpu_stream_search_batch_prune import needle, put, single_tabled

pytestmark = pytest.mark.gpu

MLZ_ERR_ARG = 8
GUARD, SENT = 8, -0x5A5A5A5A5A5A5A5B
NL = 10


def _buf(n, dtype):
    sent = {torch.int64: SENT, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}[dtype]
    return torch.full((n + GUARD,), sent, dtype=dtype, device="cuda"), sent


def _clean(t, sent, k):
    torch.cuda.synchronize()
    o = t.cpu().numpy()
    assert (o[k:] == sent).all(), "written beyond the results"
    return o[:k].tolist()


def g_search(rd, pat, cap, **kw):
    out, s = _buf(cap, torch.int64)
    total, st = rd.search(pat, out.data_ptr() if cap else None, cap, **kw)
    return (total, _clean(out, s, min(total, cap))), st


def g_many(rd, pats, cap, **kw):
    pos, s64 = _buf(cap, torch.int64)
    which, s32 = _buf(cap, torch.int32)
    counts, _ = _buf(len(pats), torch.int64)
    total, st = rd.search_many(pats, counts.data_ptr(), pos.data_ptr() if cap else None, which.data_ptr() if cap else None, cap, **kw)
    k = min(total, cap)
    return (total, _clean(pos, s64, k), _clean(which, s32, k), _clean(counts, s64, len(pats))), st


def g_records(rd, pat, rec_cap, dst_cap, **kw):
    data, s8 = _buf(dst_cap, torch.uint8)
    off, s64 = _buf(rec_cap, torch.int64)
    start, _ = _buf(rec_cap + 1, torch.int64)
    flags, _ = _buf(rec_cap, torch.uint8)
    total, totals, st = rd.search_records(pat, b"\n", data.data_ptr() if dst_cap else None, dst_cap, off.data_ptr() if rec_cap else None, start.data_ptr() if rec_cap else None,
                                          flags.data_ptr() if rec_cap else None, rec_cap, **kw)
    torch.cuda.synchronize()
    assert (data.cpu().numpy()[dst_cap:] == s8).all() and (off.cpu().numpy()[rec_cap:] == s64).all() and (start.cpu().numpy()[rec_cap + 1:] == s64).all()
    k = min(total, rec_cap)
    return (total, totals, off.cpu().numpy()[:k].tolist(), bytes(data.cpu().numpy()[:int(start[k]) if rec_cap else 0])), st


def g_grep(rd, pats, cap, regex=False, **kw):
    nums, s64 = _buf(cap, torch.int64)
    kinds, s8 = _buf(cap, torch.uint8)
    call = rd.grep_regex if regex else rd.grep_records
    R, totals, st = call(pats, nums.data_ptr() if cap else None, kinds.data_ptr() if cap else None, cap, **kw)
    k = min(R, cap)
    return (R, totals, _clean(nums, s64, k), _clean(kinds, s8, k)), st


class Pair:
    """The tabled set and the plain set of the same batch, side by side: both(call, ...) runs the guarded call on each, asserts equal outputs
    and that no_tables on the tabled set decodes what the plain set does -> (outputs, the tabled set's stats, the plain set's)."""

    def __init__(self, ctx, streams):
        self.ctx, self.b = ctx, Batch(streams)
        self.tab, self.res = ctx.stream_open_batch_device(self.b.src, self.b.spans, tables=True)
        self.plain, res = ctx.stream_open_batch_device(self.b.src, self.b.spans)
        assert res == self.res and self.tab.size == self.plain.size and self.tab.stream_bases() == self.plain.stream_bases()

    def both(self, call, *a, off=True, **kw):
        got, st = call(self.tab, *a, **kw)
        counters = (self.ctx.counter(10), self.ctx.counter(11), self.ctx.counter(14))
        want, sp = call(self.plain, *a, **kw)
        assert got == want, (call.__name__, a[1:], kw)
        assert st[0] == sp[0] and counters[0] == st[1] and counters[1] == st[2]
        if off:
            got2, st2 = call(self.tab, *a, no_tables=True, **kw)
            assert got2 == want and st2[1] == sp[1]
        assert np.array_equal(self.b.t.cpu().numpy(), self.b.image), "the input was modified"
        self.counter14 = counters[2]
        return got, st, sp

    def index(self):
        assert self.tab.index_records(b"\n")[0] == self.plain.index_records(b"\n")[0]

    def info(self):
        return self.tab.set_tables_info()[:6]

    def close(self):
        self.tab.close()
        self.plain.close()


def brute_many(data, pats):
    pairs = sorted((p, i) for i, pat in enumerate(pats) for p in SMod.brute(data, pat))
    return len(pairs), [p for p, _ in pairs], [i for _, i in pairs], [len(SMod.brute(data, pat)) for pat in pats]


def lines(n, seed, bs=None):
    """JSON-like bytes of about n bytes that end with a newline and hold no byte above 0x7f."""
    d = bytearray(synth.json_like(n, seed).tobytes())
    d[-1] = NL
    return bytes(d)


# ---- a. a mixed set of 70 streams ----

def test_mixed_set(ctx):
    BS = 4096
    kinds = [dict(search_match_len=6)] * 51 + [dict(search_match_len=4)] * 4 + [dict(search_match_len=6, search_prefix=b'":')] * 4 + \
            [dict(search_match_len=4, search_long_prefix=b'":', search_extras=2)] * 4 + [dict(search_match_len=5)] * 2
    hd = b'":'
    inside, border, absent = needle(11, 16, hd), needle(12, 16, hd), needle(13, 16, hd)
    ends = [needle(14, 16, hd), needle(15, 16, hd), needle(16, 16, hd)]
    pats = [inside, border, absent] + ends
    datas = [synth.json_like(5 * BS + 37 * k + 11, 300 + k).tobytes() for k in range(len(kinds))]
    datas[3] = put(datas[3], 2 * BS + 700, inside)
    datas[53] = put(datas[53], BS + 99, inside)
    datas[7] = put(datas[7], 3 * BS - 5, border)
    datas[57] = put(datas[57], 2 * BS - 9, border)
    for at, near, p in ((20, 1, ends[0]), (30, 5, ends[1]), (40, 15, ends[2])):                  # 1, M - 1 and L - 1 bytes on the near side of a stream's end
        datas[at] = datas[at][:-near] + p[:near]
        datas[at + 1] = p[near:] + datas[at + 1][16 - near:]
    streams = [gather(ctx, [d], BS, k % 2 == 0, **kw) for k, (d, kw) in enumerate(zip(datas, kinds))]
    extra = [synth.json_like(3 * BS, 400).tobytes(), b"", put(synth.json_like(BS // 2, 401).tobytes(), 100, inside), synth.random_bytes(2 * BS + 50, seed=9).tobytes()]
    datas += extra
    streams += [O.stream_encode(extra[0], 1, BS), O.stream_encode(b"", 1, BS), gather(ctx, [extra[2]], BS, search_match_len=6), gather(ctx, [extra[3]], BS, search_match_len=6)]
    assert [t for _, t in SMod.data_grid(streams[-1])][0] == 0x01                              # the stored-block stream
    whole = gather(ctx, [datas[0]], BS, search_match_len=6)
    cut = whole[:[c for c in CM.chunks(whole) if c.type in (1, 2, 3)][-2].off + 4 + 30]          # a framing error: left out of the set
    datas.append(b"")
    streams.append(cut)
    assert len(streams) == 70
    healthy = [True] * 69 + [False]
    concat = b"".join(datas)
    m = M.plan(streams, datas, pats, healthy)
    assert 0 < m["decoded"] < m["nck"] / 2 and m["nck"] > 256, "a wrong input: the model's plan must decode some and fewer than half of the chunks: %r" % ((m["decoded"], m["nck"]),)
    p = Pair(ctx, streams)
    try:
        assert p.res[-1] < 0 and all(r == len(d) for r, d in zip(p.res[:-1], datas))
        assert p.info() == (0,) * 6                                                            # nothing of the tables before the first search
        want = brute_many(concat, pats)
        assert want[3][:2] == [3, 2] and want[3][2] == 0 and want[3][3:] == [1, 1, 1]
        got, st, sp = p.both(g_many, pats, want[0] + 3)
        assert got == want and sp[1] == sp[0] == m["nck"] and sp[2] == 0
        assert st[1] == m["decoded"] and p.info() == m["info"] and st[2] == m["info"][3] and st[3] == m["unserved"] == 0
        assert m["info"][0] == 5 and m["info"][5] == sum(1 for d in datas if d) - 1
        got, st, _ = p.both(g_many, pats, 0)
        assert got[0] == want[0] and got[3] == want[3] and st[1] == m["decoded"]
        for pat in (inside, ends[2], absent):
            m1 = M.plan(streams, datas, [pat], healthy)
            got, st, _ = p.both(g_search, pat, 8)
            hits = SMod.brute(concat, pat)
            assert got == (len(hits), hits) and st[1] == m1["decoded"] and p.info() == m1["info"], pat
        # a pattern no class serves: every chunk, and nothing pruned
        m0 = M.plan(streams, datas, [b"\x81\x82"], healthy)
        got, st, _ = p.both(g_search, b"\x81\x82", 4)
        assert st[1] == m0["decoded"] == sp[1] and p.info() == m0["info"] and m0["info"][1] == 0
        p.index()
        got, st, _ = p.both(g_records, inside, 8, 1 << 16)
        assert got[0] == 3 and st[1] == M.plan(streams, datas, [inside], healthy)["decoded"]
    finally:
        p.close()


# ---- b, c. grep ----

def grep_want(concat, pats, invert=False):
    recs = SS.records(concat, NL)
    return [i for i, r in enumerate(recs) if any(q in r for q in pats) != invert]


def grep_batch(ctx, joined):
    BS = 64 << 10
    pats = [needle(21), needle(22)]
    datas = [lines(20000 + 300 * k, 500 + k) for k in range(70)]
    for k, pat in ((5, pats[0]), (33, pats[0]), (61, pats[1])):
        datas[k] = put(datas[k], 7000 + k, pat)
    if joined:
        # 10 | 11: the record runs on, and a needle lies in it on the far side; 40 | 41: a needle straddles the border
        datas[10] = datas[10][:-1] + b"x"
        datas[11] = put(datas[11], 3, pats[0])
        assert NL not in datas[11][:40]
        datas[40] = datas[40][:-7] + pats[1][:7]
        datas[41] = pats[1][7:] + datas[41][9:]
        assert NL not in datas[40][-40:] and NL not in datas[41][:40]
    # the batch Writer writes them, tables and all, in one call
    src, spans = BC.back_to_back(datas)
    out, at = shard.HipTensorCodec(ctx).encode_streams(torch.from_numpy(np.frombuffer(src, np.uint8).copy()).cuda(), spans, 1, BS, search_match_len=6)
    o = out.cpu().numpy()
    streams = [o[a:a + n].tobytes() for a, n in at]
    assert streams[5] == gather(ctx, [datas[5]], BS, search_match_len=6) and all(len(SMod.data_grid(s)) == 1 for s in streams)
    return pats, datas, streams


def test_grep_streams_that_end_with_the_delimiter(ctx):
    pats, datas, streams = grep_batch(ctx, False)
    concat = b"".join(datas)
    m = M.plan(streams, datas, pats, records=True)
    p = Pair(ctx, streams)
    try:
        p.index()
        assert p.tab.stream_records()[1] == 0
        sel = grep_want(concat, pats)
        assert len(sel) == 3
        got, st, sp = p.both(g_grep, pats, len(sel) + 4)
        assert got[0] == len(sel) and got[2] == sel and got[3] == [1] * 3 and sp[1] == sp[0] == 70
        alone = sum(single_tabled(ctx, p.b, i, pats)[2][1] for i in range(70))
        assert st[1] == m["decoded"] == alone and 3 <= alone < 35, (st, m["decoded"], alone)
        assert p.info() == m["info"] and m["info"][5] == 0 and m["info"][1] == 70 and st[2] == m["info"][3] > 60
        got, st, _ = p.both(g_grep, pats, 0)
        assert got[0] == 3 and st[1] == m["decoded"]
        got, st, _ = p.both(g_grep, pats, 64, before=2, after=2)
        assert got[0] > 3 and [n for n, k in zip(got[2], got[3]) if k] == sel
        inv = grep_want(concat, pats, True)
        got, st, _ = p.both(g_grep, pats, len(inv) + 4, invert=True)
        assert got[2] == inv
        got, st, _ = p.both(g_grep, pats, 8, ignore_case=True)
        assert got[2] == sel and st[1] == M.plan(streams, datas, pats, records=True, fold=True)["decoded"]
    finally:
        p.close()
    # the tensor layer: grep and grep_streams on a tabled set against the plain set
    codec = shard.HipTensorCodec(ctx)
    buf, spans = BC.back_to_back(streams, 3)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    with codec.open_streams(t, spans, tables=True) as a, codec.open_streams(t, spans) as c:
        assert a.tables and not c.tables and a.tables_info()[:6] == (0,) * 6
        y = c.grep_streams(pats)
        x = a.grep_streams(pats)
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and x[0].tolist() == [5, 33, 61]
        assert ctx.counter(10) == m["decoded"] and a.tables_info()[:6] == m["info"]
        x, y = a.grep(pats), c.grep(pats)
        assert x[0] == y[0] == 3 and all(torch.equal(u, v) for u, v in zip(x[1:], y[1:]))
        a.grep_streams(pats, no_tables=True)
        assert ctx.counter(10) == 70


def test_grep_with_two_joined_streams(ctx):
    pats, datas, streams = grep_batch(ctx, True)
    concat = b"".join(datas)
    m = M.plan(streams, datas, pats, records=True)
    p = Pair(ctx, streams)
    try:
        p.index()
        assert p.tab.stream_records()[1] == 2
        sel = grep_want(concat, pats)
        assert len(sel) == 5
        got, st, sp = p.both(g_grep, pats, 16)
        assert got[2] == sel and st[1] == m["decoded"] < 35 and p.info() == m["info"] and m["info"][5] == 2
        # rule a alone would leave the two streams in front of the borders out
        assert {10, 40} <= set(m["take"]) and {11, 41} <= set(m["take"])
        mp = M.plan(streams, datas, pats)
        got, st, _ = p.both(g_many, pats, 16)
        assert got == brute_many(concat, pats) and st[1] == mp["decoded"] and p.info() == mp["info"] and mp["info"][5] == 69
    finally:
        p.close()


# ---- d. grep -E, pruned ----

def test_grep_regex_pruned(ctx):
    BS = 4096
    lit = needle(31)
    datas = [lines(5 * BS + 50 * k, 600 + k) for k in range(12)]
    for k in (2, 6, 9):
        datas[k] = put(datas[k], 2 * BS + 100 + k, lit)
    streams = [gather(ctx, [d], BS, search_match_len=6) for d in datas]
    concat = b"".join(datas)
    flat = [n for s in streams for n, _ in SMod.data_grid(s)]
    assert all(flat)                                                                          # (widen's chunks all hold bytes)
    mr = M.plan(streams, datas, [lit], records=True)
    p = Pair(ctx, streams)
    try:
        p.index()
        # a literal in 3 streams; no literal; a literal that holds the delimiter (it can match inside no record)
        chunks = [(o, n) for o, n in zip(np.cumsum([0] + flat[:-1]).tolist(), flat)]
        rec_spans, number = RP.spans(concat, b"\n")
        wide = RP.widen(chunks, set(mr["take"]), rec_spans, number)
        for expr, pruned in ((re.escape(lit) + b"[^x]", True), (b"^$", False), (b"\\}\n\\{", False)):
            want = RM.result(concat, b"\n", expr)["numbers"]
            with api.Regex(expr) as rx:
                got, st, sp = p.both(g_grep, rx, len(want) + 4, regex=True, prune=True)
            assert got[2] == want and sp[1] == sp[0], expr
            if pruned:
                # the plan, and the plan widened to whole records over the handle's chunk list: exactly what is decoded
                assert len(want) == 3 and st[3] == len(mr["take"]) and st[1] == len(wide) and 0 < len(wide) < st[0], (st, len(mr["take"]), len(wide))
            elif expr == b"^$":
                assert st[1] == st[0]                                                          # no literal: every chunk
            else:
                assert st[1] == 0                                                              # its one literal can lie inside no record: nothing is decoded
    finally:
        p.close()
    codec = shard.HipTensorCodec(ctx)
    buf, spans = BC.back_to_back(streams, 3)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    with codec.open_streams(t, spans, tables=True) as a, codec.open_streams(t, spans) as c:
        y = c.grep_streams_regex(re.escape(lit), prune=True)
        x = a.grep_streams_regex(re.escape(lit), prune=True)
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and x[0].tolist() == [2, 6, 9]
        assert ctx.counter(10) == len(wide)
        assert a.grep_regex(re.escape(lit), prune=True)[0] == c.grep_regex(re.escape(lit), prune=True)[0] == 3


# ---- e, f. compressed tables, stale tables ----

def table_of_untaken(stream, kind, taken):
    """The first table chunk of type `kind` that stands in front of a data chunk the plan does not take."""
    k, last = 0, None
    for c in CM.chunks(stream):
        if c.type == kind:
            last = c
        elif c.type in (1, 2, 3):
            if last is not None and k not in taken:
                return last
            k, last = k + 1, None
    raise AssertionError("a wrong input: every chunk with such a table is taken")


def test_compressed_and_stale_tables(ctx):
    BS = 64 << 10                                                                            # (sparse data: the Writer writes 0x46 only where that is smaller)
    pat = needle(41)
    datas = [put(bytes(6 * BS + 10 * k), 2 * BS - 8, pat) for k in range(6)]
    plain45 = [gather(ctx, [d], BS, search_match_len=6) for d in datas]
    packed = [gather(ctx, [d], BS, search_match_len=6, search_compress=True) for d in datas]
    n46 = sum(1 for s in packed for c in CM.chunks(s) if c.type == 0x46)
    assert n46 > 0
    m45, m46 = M.plan(plain45, datas, [pat]), M.plan(packed, datas, [pat])
    assert m46["take"] == m45["take"] and m46["info"][4] == n46 and m45["info"][4] == 0 and m46["info"][3] == m45["info"][3]
    concat = b"".join(datas)
    hits = SMod.brute(concat, pat)
    p = Pair(ctx, packed)
    try:
        got, st, _ = p.both(g_search, pat, 16)
        assert got == (len(hits), hits) and st[1] == m46["decoded"] < st[0] and p.info() == m46["info"] and p.counter14 == n46
        expanded = p.tab.set_tables_info()[6]
        assert expanded == n46
        got, st, _ = p.both(g_search, pat, 16)
        assert st[1] == m46["decoded"] and p.tab.set_tables_info()[6] == expanded              # the second search expands nothing
    finally:
        p.close()
    # one 0x46 chunk with a flipped payload byte is passed over: its block is admitted
    bad = bytearray(packed[2])
    ck = table_of_untaken(packed[2], 0x46, m46["per"][2])
    bad[ck.off + 4 + ck.clen - 3] ^= 0x41
    broken = packed[:2] + [bytes(bad)] + packed[3:]
    mb = M.plan(broken, datas, [pat])
    assert mb["info"][3] == m46["info"][3] - 1 and mb["decoded"] > m46["decoded"]                  # (the admitted block, and the one that holds the bytes behind it)
    p = Pair(ctx, broken)
    try:
        got, st, _ = p.both(g_search, pat, 16)
        assert got == (len(hits), hits) and st[1] == mb["decoded"] and p.info() == mb["info"]
    finally:
        p.close()
    # f. a stale 0x45 CRC in one stream: that chunk is admitted; under MLZ_STREAM_IGNORE_CRC the table is used
    stale = bytearray(plain45[4])
    t3 = table_of_untaken(plain45[4], 0x45, m45["per"][4])
    stale[t3.off + 4 + 4] ^= 0x10
    batch = plain45[:4] + [bytes(stale)] + plain45[5:]
    ms, mi = M.plan(batch, datas, [pat]), M.plan(batch, datas, [pat], ignore_crc=True)
    assert ms["decoded"] > m45["decoded"] and mi["take"] == m45["take"]
    p = Pair(ctx, batch)
    try:
        got, st, _ = p.both(g_search, pat, 16)
        assert got == (len(hits), hits) and st[1] == ms["decoded"] and p.info() == ms["info"]
        got, st, _ = p.both(g_search, pat, 16, ignore_crc=True)
        assert got == (len(hits), hits) and st[1] == mi["decoded"] and p.info() == mi["info"]
    finally:
        p.close()


# ---- g. the plain open, refusals, empty sets ----

def test_plain_open_refusals_and_empty_sets(ctx):
    BS = 4096
    pat = needle(51)
    datas = [put(synth.json_like(3 * BS, 800 + k).tobytes(), BS + 5, pat) for k in range(3)]
    streams = [gather(ctx, [d], BS, search_match_len=6) for d in datas]
    p = Pair(ctx, streams)
    try:
        nck = sum(len(SMod.data_grid(s)) for s in streams)
        (total, _), st = g_search(p.plain, pat, 8)
        assert total == 3 and st[:3] == (nck, nck, 0)
        with pytest.raises(mz.MinLZError) as e:
            p.plain.set_tables_info()
        assert "error %d" % MLZ_ERR_ARG in str(e.value)
        cfg = api.search_config(1, 6)
        room = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        for call in (lambda: p.tab.build_sidecar([cfg], room.data_ptr(), room.numel()), lambda: p.tab.attach_sidecar(room.data_ptr(), 64),
                     lambda: p.tab.extract_sidecar(room.data_ptr(), room.numel())):
            with pytest.raises(mz.MinLZError) as e:
                call()
            assert e.value.code == api.ERR_UNSUPPORTED
        off, n = p.b.spans[0]
        one = ctx.stream_open_device(p.b.src + off, n)
        try:
            with pytest.raises(mz.MinLZError) as e:
                one.set_tables_info()
            assert "error %d" % MLZ_ERR_ARG in str(e.value)
        finally:
            one.close()
    finally:
        p.close()
    rd, res = ctx.stream_open_batch_device(None, [], tables=True)
    try:
        assert res == [] and rd.size == 0 and g_search(rd, pat, 4)[0] == (0, []) and rd.set_tables_info()[:6] == (0,) * 6
    finally:
        rd.close()
    p = Pair(ctx, [O.stream_encode(b"", 1, BS), gather(ctx, [b""], BS, search_match_len=6)])
    try:
        got, st, _ = p.both(g_search, pat, 4)
        assert got == (0, []) and st[1] == 0
        got, st, _ = p.both(g_many, [pat, b"ab"], 4)
        assert got[0] == 0
    finally:
        p.close()
