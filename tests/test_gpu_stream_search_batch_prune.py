"""mlz_stream_search_batch_device_pruned (Context.stream_search_batch_device(prune=True), HipTensorCodec.search_streams(prune=True)) on the GPU: a
batch of streams in HBM searched for many patterns, only the chunks decoded that the streams' inline block search tables cannot rule out.
Every result is compared with the model (tests/search_batch_prune_model.py: brute force per stream for what is found, search_model.plan per
stream for what is decoded), with the unpruned call on the same batch and, for healthy streams, with open_stream + search_many with tables on
that stream alone.  The guarded buffers and the comparisons are those of tests/test_gpu_stream_search_batch.py, run through a context whose
batch search prunes."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from tests import corrupt as CM
from tests import search_batch_prune_model as PM
from tests import search_model as SMod
from tests import stream_batch_cases as BC
from tests.search_gpu import gather
from tests.test_gpu_stream_search_batch import Batch, check, needles, plant

pytestmark = pytest.mark.gpu

MLZ_ERR_CORRUPT, MLZ_ERR_CRC, MLZ_ERR_ARG = 1, 5, 8
IGNORE_CRC, SEARCH_TABLES, NO_TABLES, IGNORE_CASE = 2, 4, 8, 32
BS = 64 << 10
PLAN_BYTES = 16                                                                        # mlz_get_counter 16


class Pruned:
    """The context with the batch search pruned: what Batch.search and check call goes to mlz_stream_search_batch_device_pruned."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def stream_search_batch_device(self, *a, **kw):
        r = self._ctx.stream_search_batch_device(*a, prune=True, **kw)
        self.home = self._ctx.counter(PLAN_BYTES)                                      # the bytes the call's plan brought to the host
        return r


def needle(seed, L=16, head=b""):
    """Random bytes above 0x7f behind `head`: no letter and no prefix byte among them."""
    return head + bytes(np.random.default_rng(seed).integers(128, 256, L - len(head), dtype=np.uint8))


def json_data(k, nblk=5, bs=BS):
    return synth.json_like(nblk * bs + 100 * k, 92 + k).tobytes()


def put(d, o, p):
    return d[:o] + p + d[o + len(p):]


def single_tabled(ctx, b, i, pats, **kw):
    """open_stream on stream i alone + search_many WITH tables -> (total, the pairs, stats)."""
    off, n = b.spans[i]
    rd = ctx.stream_open_device(b.src + off if n else None, n)
    try:
        total, _ = rd.search_many(pats, None, None, None, 0, **kw)
        pos = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
        which = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        total2, stats = rd.search_many(pats, None, pos.data_ptr() if total else None, which.data_ptr() if total else None, total, **kw)
        torch.cuda.synchronize()
        assert total2 == total
        return total, list(zip(pos.cpu().numpy()[:total].tolist(), which.cpu().numpy()[:total].tolist())), stats
    finally:
        rd.close()


def within_the_bound(p, n, nck, rounds=None):
    """The traffic of the last call through the pruning context p: at most 32 bytes per stream and one per data chunk; with `rounds` CRC
    rounds exactly 16 bytes of key and one of class verdict per stream, a word per round and a byte per chunk."""
    assert 16 * n <= p.home <= 32 * n + nck, (p.home, n, nck)
    if rounds is not None:
        assert p.home == 17 * n + 4 * rounds + nck, (p.home, n, nck, rounds)


def against_the_model(got, streams, pats, what, healthy=None, **kw):
    """stats 0, 1, 4 .. 7 of a pruned call against the model's plan -> the model."""
    m = PM.plan(streams, pats, healthy=healthy, **kw)
    print(what, "model: decoded", m["decoded"], "tabbed", m["tabbed"], "skipped", m["skipped"], "classes", m["classes"], "whole", m["whole"], "plans", m["plans"])
    st = got["stats"]
    assert len(st) == 8 and st[0] == sum(len(s) for s in m["sizes"] if s is not None), what
    assert (st[4], st[5], st[6], st[7]) == (m["tabbed"], m["skipped"], m["classes"], m["whole"]), what
    return m


def same_outputs(a, b):
    return all(a[k] == b[k] for k in ("total", "res", "stream_counts", "pattern_counts", "present", "triples"))


# ---- 1. a mixed batch ----

def test_mixed_batch(ctx):
    inside, across, absent = needle(1), needle(2), needle(3)
    kinds = [dict(search_match_len=6), dict(search_match_len=4), dict(search_match_len=6, search_prefix=b'":'), dict(search_match_len=4, search_long_prefix=b'":', search_extras=2)]
    # the needles start with '":' so that every configuration serves them
    pats = [b'":' + inside[2:], b'":' + across[2:], b'":' + absent[2:]]
    datas, streams = [], []
    for k, kw in enumerate(kinds):
        d = put(put(json_data(k), 2 * BS - 8, pats[1]), 4 * BS + 1000 + k, pats[0])
        datas.append(d)
        streams.append(gather(ctx, [d], BS, k % 2 == 0, **kw))
    for k in range(3):                                                                # type 1, M = 6 again: streams that hold none of the needles
        d = synth.json_like(2 * BS, 70 + k).tobytes()
        datas.append(d)
        streams.append(gather(ctx, [d], BS, search_match_len=6))
    plain = put(json_data(7, 3), BS - 5, pats[1])
    datas += [plain, b"", put(json_data(8, 1)[:BS // 2], 700, pats[0]), synth.random_bytes(2 * BS + 50, seed=9).tobytes()]
    streams += [O.stream_encode(plain, 1, BS), O.stream_encode(b"", 1, BS), gather(ctx, [datas[-2]], BS, search_match_len=6), gather(ctx, [datas[-1]], BS, search_match_len=6)]
    assert [t for _, t in SMod.data_grid(streams[-1])][0] == 0x01                       # the stored-block stream
    b = Batch(streams)
    p = Pruned(ctx)
    got, want = check(p, b, datas, pats, "mixed, pruned", singles=[])
    within_the_bound(p, len(streams), got["stats"][0], rounds=2)                        # (a round that checks every table, and one that finds nothing left)
    assert ctx.counter(10) == got["stats"][1] and ctx.counter(11) == got["stats"][4] and ctx.counter(14) == 0
    m = against_the_model(got, streams, pats, "mixed")
    unpruned = b.search(ctx, pats, want["total"] + 3)
    assert same_outputs(got, unpruned) and unpruned["stats"][1] == unpruned["stats"][0]
    decoded = 0
    for i, d in enumerate(datas):
        total, pairs, st = single_tabled(ctx, b, i, pats)
        assert total == want["counts"][i] and [(i, q, p) for q, p in pairs] == [t for t in want["triples"] if t[0] == i], i
        assert st[1] == len(m["plans"][i]), (i, st, m["plans"][i])
        decoded += st[1]
    assert got["stats"][1] == decoded == m["decoded"] < got["stats"][0]
    assert got["stats"][5] > 0 and got["stats"][2] == 0 and got["stats"][3] == 1
    assert want["pattern_counts"] == [5, 5, 0]
    # under MLZ_STREAM_IGNORE_CRC: the same plan and the same answers
    got2, _ = check(p, b, datas, pats, "mixed, ignore_crc", flags=IGNORE_CRC, singles=[], model=want)
    assert got2["stats"] == got["stats"]
    within_the_bound(p, len(streams), got["stats"][0], rounds=0)


# ---- 2. unserved patterns and folding ----

def test_unserved_patterns_and_folding(ctx):
    ident = b"\x81K\x93\xa7\xf2q\xc5\x88\xd4V\x9e\xb1\xe3\xf7\x8a\x90"                 # three letters, at most two in a window of 6
    d0 = put(put(put(json_data(0), 1000, ident), 2 * BS - 5, ident.lower()), 2 * BS + 500, ident.upper())
    d1 = json_data(1)
    datas = [d0, d1, put(json_data(2, 3), 100, ident)]
    streams = [gather(ctx, [d], BS, search_match_len=6) for d in datas[:2]] + [O.stream_encode(datas[2], 1, BS)]
    b = Batch(streams)
    p = Pruned(ctx)
    # a pattern shorter than M: its class is decoded whole
    got, _ = check(p, b, datas, [ident, ident[:5]], "a short pattern", singles=[])
    m = against_the_model(got, streams, [ident, ident[:5]], "a short pattern")
    assert got["stats"][7] == 3 and got["stats"][1] == got["stats"][0] == m["decoded"]
    # the same id alone prunes
    got, want = check(p, b, datas, [ident], "the id", singles=[])
    m = against_the_model(got, streams, [ident], "the id")
    assert got["stats"][1] == m["decoded"] < got["stats"][0] and want["counts"] == [1, 0, 1]
    # MLZ_SEARCH_IGNORE_CASE: all three cases are found, and the plan is the single-stream flagged plan
    got, want = check(p, b, datas, [ident], "the id, folded", flags=IGNORE_CASE, singles=[], fold=True)
    m = against_the_model(got, streams, [ident], "the id, folded", fold=True)
    assert want["counts"] == [3, 0, 1] and got["stats"][1] == m["decoded"] < got["stats"][0]
    for i in range(3):
        total, _, st = single_tabled(ctx, b, i, [ident], ignore_case=True)
        assert total == want["counts"][i] and st[1] == len(m["plans"][i])
    # with folding, a six-letter word decodes every chunk
    got, _ = check(p, b, datas, [b"stream"], "a word, folded", flags=IGNORE_CASE, singles=[], fold=True)
    m = against_the_model(got, streams, [b"stream"], "a word, folded", fold=True)
    assert got["stats"][1] == got["stats"][0] and got["stats"][7] == 3


# ---- 3. classes ----

def test_classes(ctx):
    kinds = [dict(search_match_len=6), dict(search_match_len=4), dict(search_match_len=6, search_prefix=b'"'), dict(search_match_len=6, search_prefix=b'":,{}[] \n'),
             dict(search_match_len=4, search_long_prefix=b'":', search_extras=2), dict(search_match_len=5)]
    pat = needle(4, 16, b'":')
    datas = [put(json_data(k), 2 * BS - 8, pat) for k in range(6)]
    streams = [gather(ctx, [d], BS, **kw) for d, kw in zip(datas, kinds)]
    p = Pruned(ctx)
    b = Batch(streams)
    got, want = check(p, b, datas, [pat], "six classes", singles=[])
    m = against_the_model(got, streams, [pat], "six classes")
    assert got["stats"][6] == 6 and got["stats"][7] == 2 and m["pruning"] == [True] * 4 + [False] * 2
    full = [sum(1 for v in s if v) for s in m["sizes"]]
    assert got["stats"][1] == m["decoded"] and [len(x) for x in m["plans"]][4:] == full[4:] and all(len(x) < f for x, f in zip(m["plans"][:4], full[:4]))
    # reordered: other streams are the first four classes
    order = [5, 4, 3, 2, 1, 0]
    b2 = Batch([streams[i] for i in order])
    got2, _ = check(p, b2, [datas[i] for i in order], [pat], "six classes, reversed", singles=[])
    m2 = against_the_model(got2, [streams[i] for i in order], [pat], "six classes, reversed")
    assert got2["stats"][1] == m2["decoded"] and m2["pruning"] == [True] * 4 + [False] * 2 and got2["stats"][6] == 6
    assert [len(x) for x in m2["plans"]][4:] == [full[1], full[0]]
    # aliases: the same source span named twice, among others
    b3 = Batch(streams[:2])
    b3.spans = [b3.spans[0], b3.spans[1], b3.spans[0], b3.spans[0], b3.spans[1]]
    ali = [0, 1, 0, 0, 1]
    got3, _ = check(p, b3, [datas[i] for i in ali], [pat], "aliases", singles=[])
    m3 = against_the_model(got3, [streams[i] for i in ali], [pat], "aliases")
    assert got3["stats"][1] == m3["decoded"] < got3["stats"][0] and got3["stats"][6] == 2


# ---- 4. errors in one batch ----

def _table_chunks(stream):
    return [c for c in CM.chunks(stream) if c.type == 0x45]


def _data_chunks(stream):
    return [c for c in CM.chunks(stream) if c.type in (1, 2, 3)]


def test_errors_in_one_batch(ctx):
    pat = needle(5)
    datas = [put(json_data(k), 2 * BS - 8, pat) for k in range(4)]
    streams = [gather(ctx, [d], BS, search_match_len=6) for d in datas]
    plans = PM.plan(streams, [pat])["plans"]
    assert all(1 in x and 2 in x and 3 not in x for x in plans)
    p = Pruned(ctx)
    # a framing error keeps the walk's code; a corrupt TAKEN chunk gives its stream's code and a second pass; the others are intact
    cut = streams[1][:_data_chunks(streams[1])[-2].off + 4 + 300]                      # inside the last full data chunk's body
    taken = bytearray(streams[2])
    ck = _data_chunks(streams[2])[2]
    taken[ck.off + 4 + ck.clen // 2] ^= 0x5A
    taken = bytes(taken)
    codes = {1: CM.stream_verdict(cut, 6 * BS)[0], 2: CM.stream_verdict(taken, 6 * BS)[0]}
    assert codes[1] != 0 and codes[2] in (MLZ_ERR_CORRUPT, MLZ_ERR_CRC)
    batch = [streams[0], cut, taken, streams[3]]
    b = Batch(batch)
    got, want = check(p, b, [datas[0], None, None, datas[3]], [pat], "errors", codes=codes, singles=[])
    assert got["stats"][2] == 1 and got["stats"][3] == 2 and want["counts"] == [1, 0, 0, 1]
    m = PM.plan(batch, [pat], healthy=[True, False, True, True])
    assert got["stats"][1] == m["decoded"] + sum(len(x) for i, x in enumerate(m["plans"]) if i in (0, 3))   # the second pass decodes the healthy streams' plans again
    # the same corruption in a PRUNED chunk goes unnoticed
    pruned = bytearray(streams[2])
    ck = _data_chunks(streams[2])[3]
    pruned[ck.off + 4 + ck.clen // 2] ^= 0x5A
    pruned = bytes(pruned)
    assert CM.stream_verdict(pruned, 6 * BS)[0] in (MLZ_ERR_CORRUPT, MLZ_ERR_CRC)
    b = Batch([streams[0], pruned, streams[3]])
    got, want = check(p, b, [datas[0], datas[2], datas[3]], [pat], "a corrupt pruned chunk", singles=[])
    against_the_model(got, [streams[0], streams[2], streams[3]], [pat], "a corrupt pruned chunk")
    assert got["stats"][2] == 0 and got["stats"][3] == 1 and want["counts"] == [1, 1, 1]
    unpruned = b.search(ctx, [pat], 8)
    assert unpruned["res"][1] < 0                                                      # (the unpruned call decodes it and reports it)
    # a table with a flipped CRC: its chunk is decoded; under IGNORE_CRC the table is used
    stale = bytearray(streams[0])
    t3 = _table_chunks(streams[0])[3]
    stale[t3.off + 4 + 4] ^= 0x10
    stale = bytes(stale)
    b = Batch([stale, streams[3]])
    got, _ = check(p, b, [datas[0], datas[3]], [pat], "a stale table", singles=[])
    within_the_bound(p, 2, got["stats"][0], rounds=2)                                  # (the second round locates the stale table's chunk again and finds no other table)
    m = against_the_model(got, [stale, streams[3]], [pat], "a stale table")
    assert 3 in m["plans"][0] and got["stats"][1] == m["decoded"] and got["stats"][4] == m["tabbed"] == len(_table_chunks(stale)) - 1 + len(_table_chunks(streams[3]))
    got, _ = check(p, b, [datas[0], datas[3]], [pat], "a stale table, ignore_crc", flags=IGNORE_CRC, singles=[])
    m = against_the_model(got, [stale, streams[3]], [pat], "a stale table, ignore_crc", ignore_crc=True)
    assert 3 not in m["plans"][0] and got["stats"][1] == m["decoded"]
    # a table chunk cut short of its block does not fit: the table's chunk header states fewer bytes, a padding chunk takes the rest
    short = bytearray(streams[0])
    n = t3.clen - 20
    short[t3.off + 1:t3.off + 4] = bytes([n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF])
    short[t3.off + 4 + n:t3.off + 4 + n + 4] = bytes([0xFE, 16, 0, 0])
    short = bytes(short)
    assert O.stream_decode(short, len(datas[0]) + 1) == datas[0]
    b = Batch([short, streams[3]])
    got, _ = check(p, b, [datas[0], datas[3]], [pat], "a short table", singles=[])
    m = against_the_model(got, [short, streams[3]], [pat], "a short table")
    assert 3 in m["plans"][0] and got["stats"][1] == m["decoded"]


# ---- 5. no tables and 0x46 tables ----

def test_no_tables_and_compressed_tables(ctx):
    pats = [needle(6), needle(7, 7)]
    datas = [plant(json_data(k, 3), pats, BS, k) for k in range(3)]
    p = Pruned(ctx)
    plain = Batch([O.stream_encode(d, 1, BS) for d in datas])
    got, want = check(p, plain, datas, pats, "no tables", singles=[])
    assert p.home == 16 * 3                                                            # (the keys alone: no class, no plan)
    unpruned = plain.search(ctx, pats, want["total"] + 3)
    assert same_outputs(got, unpruned) and got["stats"][:4] == unpruned["stats"] and got["stats"][4:] == (0, 0, 0, 3)
    tabled = Batch([gather(ctx, [d], BS, search_match_len=6) for d in datas])
    got, _ = check(p, tabled, datas, pats, "NO_TABLES", flags=NO_TABLES, singles=[], model=want)
    assert p.home == 0
    unpruned = tabled.search(ctx, pats, want["total"] + 3)
    assert same_outputs(got, unpruned) and got["stats"][:4] == unpruned["stats"] and got["stats"][4:] == (0, 0, 0, 0) and got["stats"][1] == got["stats"][0]
    # a stream whose tables all became 0x46 is decoded whole and brings no table; its neighbour prunes
    sparse = put(put(bytes(4 * BS), BS + 70, pats[0]), 3 * BS - 3, pats[1])
    packed = gather(ctx, [sparse], BS, search_match_len=6, search_compress=True)
    kinds = [c.type for c in CM.chunks(packed)]
    assert kinds.count(0x46) > 0 and kinds.count(0x45) == 0 and kinds.count(0x44) == 1
    one = put(json_data(0), 2 * BS - 8, pats[0])
    streams = [packed, gather(ctx, [one], BS, search_match_len=6)]
    b = Batch(streams)
    got, _ = check(p, b, [sparse, one], pats, "compressed tables", singles=[])
    m = against_the_model(got, streams, pats, "compressed tables")
    assert m["plans"][0] == [0, 1, 2, 3] and got["stats"][4] == len(_table_chunks(streams[1])) and got["stats"][1] == m["decoded"] < got["stats"][0]


# ---- 6. arguments ----

def test_arguments(ctx):
    pats = needles(7)
    datas = [plant(json_data(k, 2), pats, BS, k) for k in range(2)]
    b = Batch([gather(ctx, [d], BS, search_match_len=6) for d in datas])
    L = _lib.lib()
    n, cap = 2, 16
    blob, lens = b"".join(pats), (C.c_uint32 * len(pats))(*[len(p) for p in pats])
    out_count = (C.c_int64 * n)(*([123] * n))
    stats = (C.c_uint64 * 8)(*([77] * 8))
    outs = {k: torch.full((64,), v, dtype=t, device="cuda") for k, v, t in (("sc", 1, torch.int64), ("pc", 2, torch.int64), ("pr", 3, torch.int32), ("hs", 4, torch.int32),
                                                                          ("hp", 5, torch.int64), ("hw", 6, torch.int32))}
    arr = lambda spans: (_lib.BlockDesc * len(spans))(*[_lib.BlockDesc(o, ln, 0, 0) for o, ln in spans])

    def call(flags=0, src=None, spans=None, count=None, blob=blob, lens=lens, npat=len(pats), cap=cap, **ptr):
        p = {k: t.data_ptr() for k, t in outs.items()}
        p.update(ptr)
        spans = b.spans if spans is None else spans
        return L.mlz_stream_search_batch_device_pruned(ctx.handle, None, flags, b.src if src is None else src, arr(spans), len(spans) if count is None else count, blob, lens, npat,
                                                       out_count, p["sc"], p["pc"], p["pr"], p["hs"], p["hp"], p["hw"], cap, stats)
    host = np.zeros(4096, np.uint8)
    many = (C.c_uint32 * 4097)(*([1] * 4097))
    refused = [
        call(npat=0), call(blob=b"x" * 4097, lens=many, npat=4097),
        call(blob=b"ab", lens=(C.c_uint32 * 2)(0, 2), npat=2), call(blob=b"x" * 258, lens=(C.c_uint32 * 2)(257, 1), npat=2),
        call(hs=None), call(hp=None), call(hw=None),
        call(sc=host.ctypes.data), call(pc=host.ctypes.data), call(pr=host.ctypes.data), call(hp=host.ctypes.data),
        call(src=b.image.ctypes.data + 37),
        call(spans=[b.spans[0], (b.spans[1][0], 1 << 35)]),
        call(flags=SEARCH_TABLES), call(flags=16), call(flags=1 << 8), call(flags=1),
        call(count=(1 << 20) + 1), call(count=-1),
    ]
    assert refused == [-MLZ_ERR_ARG] * len(refused), refused
    torch.cuda.synchronize()
    assert list(out_count) == [123] * n and list(stats) == [77] * 8
    for k, v in (("sc", 1), ("pc", 2), ("pr", 3), ("hs", 4), ("hp", 5), ("hw", 6)):
        assert (outs[k].cpu().numpy() == v).all(), k + " was written by a refused call"
    assert np.array_equal(b.t.cpu().numpy(), b.image)
    assert call(count=0) == 0 and list(out_count) == [123] * n and list(stats) == [0] * 8
    assert (outs["pr"].cpu().numpy() == 3).all() and (outs["hp"].cpu().numpy() == 5).all()
    assert ctx.stream_search_batch_device(b.src, [], pats, prune=True) == (0, [], (0,) * 8)
    # and the same arguments, accepted; the guarded run of the same batch
    assert call() == PM.result(datas, pats)["total"] and list(stats)[2:4] == [0, 1] and list(stats)[6] == 1
    check(Pruned(ctx), b, datas, pats, "arguments, accepted", singles=[])


# ---- 7. the Python layers ----

def test_search_streams(ctx):
    codec = shard.HipTensorCodec(ctx)
    pat = needle(8)
    datas = [put(json_data(k), 2 * BS - 8, pat) for k in range(3)] + [b""]
    streams = [gather(ctx, [d], BS, search_match_len=6) for d in datas[:3]] + [O.stream_encode(b"", 1, BS)]
    buf, spans = BC.back_to_back(streams, 3)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    pats = [pat, b'"user"']
    want = PM.result(datas, pats)
    a = codec.search_streams(t, spans, pats, max_results=want["total"] + 5, prune=True)
    c = codec.search_streams(t, spans, pats, max_results=want["total"] + 5)
    assert a[6] == c[6] == want["total"] and a[0].tolist() == want["counts"]
    assert all(torch.equal(x, y) for x, y in zip(a[:6], c[:6]))
    assert list(zip(a[2].tolist(), a[3].tolist(), a[4].tolist())) == want["triples"]
    # the keyword reaches the pruned call: fewer chunks are decoded for the planted needle alone
    _, _, st = ctx.stream_search_batch_device(t.data_ptr(), spans, [pat], prune=True)
    assert len(st) == 8 and st[1] == PM.plan(streams, [pat])["decoded"] < st[0]
    # a failing stream: raise names the first one; keep returns the codes
    bad = bytearray(buf)
    ck = _data_chunks(streams[1])[1]                                                    # a chunk the plan takes
    bad[spans[1][0] + ck.off + 4 + ck.clen // 2] ^= 0x5A
    tb = torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda()
    with pytest.raises(mz.MinLZError) as e:
        codec.search_streams(tb, spans, [pat], prune=True)
    assert e.value.index == 1 and e.value.code in (MLZ_ERR_CORRUPT, MLZ_ERR_CRC)
    counts, present, hs, hp, hw, pc, total = codec.search_streams(tb, spans, [pat], max_results=10, on_error="keep", prune=True)
    keep = PM.result([datas[0], None, datas[2], datas[3]], [pat])
    assert counts.tolist()[1] in (-MLZ_ERR_CORRUPT, -MLZ_ERR_CRC) and [x for i, x in enumerate(counts.tolist()) if i != 1] == [1, 1, 0]
    assert total == keep["total"] == 2 and list(zip(hs.tolist(), hp.tolist(), hw.tolist())) == keep["triples"] and not present[1].any()
