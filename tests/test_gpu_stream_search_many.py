"""mlz_dev_reader_search_many (DeviceReader.search_many, DeviceStream.search_many) on the GPU: many patterns over a stream in HBM in one
call.  Counts, total and pairs must be those of a brute-force search of the decoded bytes, the counts those of mlz_dev_reader_search
pattern by pattern, and the chunks decoded the union of the models' plans.  Every call writes into guarded arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
from minlz_amd import _lib, shard, synth
from tests import search_cases as SC
from tests import search_long_prefix_cases as LC
from tests import search_model as SMod
from tests import search_prefix_cases as PC
from tests.search_gpu import SENT, Opened, Searcher, gather
from tests.test_gpu_stream_search import check_search

pytestmark = pytest.mark.gpu

MLZ_ERR_ARG = 8
SENT32 = 0x5A5A5A5A
GUARD = 8


class ManySearcher(Opened):
    def __call__(self, pats, cap, null=False, **kw):
        """-> (total, [(position, pattern)], counts, stats); nothing is written beyond min(total, cap) pairs and len(pats) counts."""
        n = len(pats)
        pos = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
        which = torch.full((cap + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        counts = torch.full((n + GUARD,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search_many(pats, counts.data_ptr(), None if null else pos.data_ptr(), None if null else which.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        p, w, c = pos.cpu().numpy(), which.cpu().numpy(), counts.cpu().numpy()
        k = min(total, cap)
        assert (p[k:] == SENT).all() and (w[k:] == SENT32).all() and (c[n:] == SENT).all(), "written beyond the results"
        assert self.ctx.search_plan() == stats[1:3]
        return total, list(zip(p[:k].tolist(), w[:k].tolist())), c[:n].tolist(), stats

    def single(self, p, **kw):
        return self.rd.search(p, None, 0, **kw)[0]


def brute_pairs(d, pats):
    per = [SMod.brute(d, p) for p in pats]
    return sorted((q, i) for i, qs in enumerate(per) for q in qs), [len(qs) for qs in per]


def check_many(sr, d, pats, what, cap=None, **kw):
    pairs, counts = brute_pairs(d, pats)
    cap = len(pairs) + 3 if cap is None else cap
    total, got, cnt, stats = sr(pats, cap, **kw)
    print(what, "pairs", len(pairs), "stats", stats)
    assert total == len(pairs) and cnt == counts, what
    assert got == pairs[:cap], what
    return stats


# ---- against brute force and against single calls ----

CONFIGS = {
    "type 1": dict(search_match_len=6),
    "type 2": dict(search_match_len=6, search_prefix=PC.SETS["json4"]),
    "type 3": dict(search_match_len=6, search_prefix=PC.SETS["nonalnum"]),
    "type 4": dict(search_match_len=6, search_long_prefix=LC.USER, search_extras=3),
    "no tables": {},
}


def mixed_patterns(d, M, bs):
    """Lengths 1, M - 1, M, M + 1, 16 and 256 inside a block and across a border, an absent needle, a duplicate, x and x + one more byte."""
    named = SC.patterns(d, M, bs)
    assert {len(p) for _, p in named} >= {1, M - 1, M, M + 1, 16, 256}
    pats = [p for _, p in named]
    o = 7 * bs // 3
    pats += [pats[8], d[o:o + 7], d[o:o + 8], b'","user":"user_']
    return pats


def served_needles(d, bs):
    """Needles the tables of every type can serve: 256 bytes inside a block and across a border, an absent one behind the long prefix, and
    records of the data that start with the long prefix (t_min = 1) or three bytes in front of it (t_min = 0)."""
    o = 5 * bs // 3
    at, at2 = d.find(LC.USER, o), d.find(LC.USER, 7 * bs + 99)
    return [d[o:o + 256], d[bs - 128:bs + 128], b"xy," + LC.USER + PC.letters(12, 3), d[at:at + 24], d[at - 3:at + 21], d[at2:at2 + 24], d[at2 - 3:at2 + 21]]


def model_plans(name, stream, pats):
    """-> (the models' plans, (windows or groups, t_min) per pattern) over the Writer's stream."""
    cfg, B, tables = SMod.read_tables(stream)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    assert cfg[0] == int(name[-1])
    starts = SMod.groups if cfg[0] == 4 else SMod.windows
    return [SMod.plan(tables, sizes, p, cfg, B) for p in pats], [(len(starts(p, cfg)[0]), starts(p, cfg)[1]) for p in pats]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_against_brute_force_and_single_calls(ctx, name):
    bs, M = 64 << 10, 6
    d = synth.json_like(bs * 9 + 500, 5).tobytes()
    stream = gather(ctx, [d], bs, True, **CONFIGS[name])
    assert O.stream_decode(stream, len(d)) == d
    pats = mixed_patterns(d, M, bs)
    sr = ManySearcher(ctx, stream)
    try:
        for kw in ({}, dict(no_tables=True), dict(ignore_crc=True)):
            what = "%s %s" % (name, kw)
            pairs, counts = brute_pairs(d, pats)
            stats = check_many(sr, d, pats, what, **kw)
            assert [sr.single(p, **kw) for p in pats] == counts, what       # mlz_dev_reader_search's totals, one by one
            assert stats[0] == 10 and stats[1] == 10                         # (the one-byte pattern is shorter than M: everything)
            assert stats[3] >= 1 and (stats[2] == 0) == (name == "no tables" or "no_tables" in kw)
        # served patterns only, so that search_many_plan_kernel runs: the decoded set is the union of the models' plans
        if name != "no tables":
            served = served_needles(d, bs)
            plans, groups = model_plans(name, stream, served if name in ("type 1", "type 4") else served[:3])
            served = served[:len(plans)]
            assert all(groups), (name, groups)                               # the model: the tables serve every one of them
            union = set().union(*[set(pl) for pl in plans])
            assert 0 < len(union) < 10, name                                 # a real selection
            if name == "type 4":                                             # groups of E + 1 windows; t_min 0 and 1; a pattern of two groups
                assert {g[1] for g in groups} == {0, 1} and max(g[0] for g in groups) == 2
            stats = check_many(sr, d, served, name + " served")
            assert stats[3] == 0 and stats[2] > 0 and stats[1] == len(union), (name, stats, sorted(union))
            for p, pl in zip(served, plans):                                 # and the single calls decode their own sets
                assert sr.rd.search(p, None, 0)[1][1] == len(pl), name
    finally:
        sr.close()


# ---- one pattern: the n = 1 case of the same plan ----

def single_call(sr, p, cap):
    """mlz_dev_reader_search with all four statistics -> (total, positions, stats); guarded like ManySearcher's arrays."""
    pos = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
    stats = (C.c_uint64 * 4)(*([SENT32] * 4))
    total = _lib.lib().mlz_dev_reader_search(sr.rd.handle, None, 0, p, len(p), pos.data_ptr(), cap, stats)
    torch.cuda.synchronize()
    assert total >= 0
    q = pos.cpu().numpy()
    k = min(total, cap)
    assert (q[k:] == SENT).all(), "written beyond the results"
    return total, q[:k].tolist(), tuple(int(v) for v in stats)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_single_is_many_with_one_pattern(ctx, name):
    """search(p, cap) and search_many([p], cap) share one layout, one decoded-set rule and one prefix scan: the same total, the same
    positions (`which` all 0), the same first three statistics, and the single call's fourth statistic is 0 whether the tables serve the
    pattern or not.  cap once above the total and once 1 below it.  (Both calls are held to brute force on this stream by
    test_against_brute_force_and_single_calls.)"""
    bs, M = 64 << 10, 6
    d = synth.json_like(bs * 9 + 500, 5).tobytes()
    stream = gather(ctx, [d], bs, True, **CONFIGS[name])
    sr = ManySearcher(ctx, stream)
    try:
        not_served = []                                                      # per pattern: search_many's fourth statistic
        for p in mixed_patterns(d, M, bs) + served_needles(d, bs):
            full = sr.single(p)
            for cap in (full + 3, max(full - 1, 0)):
                total, pos, st = single_call(sr, p, cap)
                mtotal, pairs, counts, mst = sr([p], cap)
                what = (name, p[:16], len(p), cap)
                assert total == mtotal == full and counts == [full], what
                assert pos == [q for q, _ in pairs] and all(w == 0 for _, w in pairs), what
                assert st[:3] == mst[:3] and st[3] == 0 and mst[3] in (0, 1), (what, st, mst)
            not_served.append(mst[3])                                        # (it does not depend on cap)
        # both branches of the plan: served_needles holds at least three patterns that every table type serves
        assert not_served.count(1) >= 1 and (not_served.count(0) >= 3 or name == "no tables")
    finally:
        sr.close()


# ---- the plan ----

@pytest.mark.parametrize("kind", SC.KINDS)
def test_plan_is_the_union_of_the_models_plans(ctx, kind):
    """128 x 64 KiB, M = 6, the planted needle of SC.planted and absent ones: the union of the models' plans is decoded, a handful of chunks."""
    bs, nblk, M = 64 << 10, 128, 6
    d, nd, at = SC.planted(kind, bs, nblk, 16, 1)
    stream = gather(ctx, [d], bs, True, search_match_len=M)
    cfg, B, tables = SMod.read_tables(stream, types=(1,))
    sizes = [n for n, _ in SMod.data_grid(stream)]
    assert cfg == (1, M, b"") and len(sizes) == nblk
    absent = [bytes(SC.needle(16, 200 + s)) for s in range(8)]
    planted_plan = SMod.plan(tables, sizes, nd, cfg, B)
    absent_plans = [SMod.plan(tables, sizes, p, cfg, B) for p in absent]
    union = set(planted_plan).union(*[set(a) for a in absent_plans])
    assert len(planted_plan) <= 12 and len(union) <= 12 + sum(len(a) for a in absent_plans)
    sr = ManySearcher(ctx, stream)
    try:
        stats = check_many(sr, d, [nd] + absent, kind)
        print(kind, "decoded", stats[1], "of", stats[0], "planted alone", len(planted_plan), "absent add", [len(a) for a in absent_plans])
        assert stats == (nblk, len(union), sum(t is not None for t in tables), 0)
        assert sorted(set(SMod.brute(d, nd)) & set(at)) == sorted(at)
        stats = check_many(sr, d, [nd] + absent + [nd[:M - 1]], kind + " + one unserved", cap=50)
        assert stats == (nblk, sum(1 for n in sizes if n), sum(t is not None for t in tables), 1)
        stats = check_many(sr, d, [nd[:3], nd[:5], nd], kind + " two unserved", cap=50)
        assert stats[3] == 2 and stats[1] == nblk
    finally:
        sr.close()


# ---- many patterns ----

@pytest.mark.parametrize("n", [300, 4096])
def test_many_patterns(ctx, n):
    """8-byte patterns from the data at random places plus absent ones (buckets hold several entries), then with a one-byte pattern (m = 1)."""
    bs = 64 << 10
    rng = np.random.default_rng(n)
    d = synth.text_like(bs * 9 + 321, 8).tobytes()
    stream = gather(ctx, [d], bs, True, search_match_len=6)
    pats = []
    for i in range(n - 1):
        if i % 3 == 2:
            pats.append(bytes(rng.integers(0, 256, 8, dtype=np.uint8)))
        else:
            o = int(rng.integers(0, len(d) - 8))
            pats.append(d[o:o + 8])
    sr = ManySearcher(ctx, stream)
    try:
        stats = check_many(sr, d, pats + [pats[0]], "n=%d" % n)
        assert stats[3] == 0
        stats = check_many(sr, d, pats + [b"q"], "n=%d with a one-byte pattern" % n)
        assert stats[3] == 1
        check_many(sr, d, pats + [b"q"], "n=%d, cap" % n, cap=1000, no_tables=True)
    finally:
        sr.close()


# ---- cap ----

def test_cap(ctx):
    bs = 64 << 10
    d = bytearray(synth.text_like(bs * 9 + 500, 5).tobytes())
    d[5 * bs - 20:5 * bs + 30] = b"a" * 50
    d[7 * bs - 8:7 * bs + 8] = bytes(SC.needle(16, 78))                         # across a border, behind the run of a
    d = bytes(d)
    stream = gather(ctx, [d], bs, True, search_match_len=6)
    pats = [b"aaaaaa", b"aaaaaaa", b"aaaaaa", bytes(SC.needle(16, 77)), bytes(SC.needle(16, 78))]
    pairs, counts = brute_pairs(d, pats)
    assert len(pairs) > 100 and pairs[0][0] == pairs[1][0] == pairs[2][0] and [i for _, i in pairs[:3]] == [0, 1, 2]
    sr = ManySearcher(ctx, stream)
    try:
        total, got, cnt, _ = sr(pats, 0, null=True)
        assert total == len(pairs) and got == [] and cnt == counts
        for cap in (1, 2, 4, len(pairs) - 1, len(pairs)):                    # 1, 2 and 4 cut between the pairs of one position
            check_many(sr, d, pats, "cap %d" % cap, cap=cap)
    finally:
        sr.close()


# ---- the border between decode groups ----

def test_group_border(ctx):
    """1 MiB blocks, a little over 64 MiB decoded, every chunk in the set.  There is one border between decode groups, at 64 MiB, so the
    needles of 2, 40 and 256 bytes are runs of one byte value inside a run of 512 such bytes around the border: each of them then ends
    exactly at the border, straddles it at every split and starts exactly at it.  A random 40-byte needle lies across the border of two
    blocks inside a group and at both ends of the data, and a frequent 3-byte pattern comes with a cap."""
    bs, border = 1 << 20, 64 << 20
    base = synth.json_like(8 << 20, 9).tobytes()
    d = bytearray((base * 9)[:border + (2 << 20) + 321])
    assert 0xF1 not in base
    d[border - 256:border + 256] = b"\xf1" * 512
    rnd = bytes(SC.needle(40, 12))
    for o in (0, 5 * bs - 20, len(d) - 40):
        d[o:o + 40] = rnd
    d = bytes(d)
    needles = [b"\xf1" * 2, b"\xf1" * 40, b"\xf1" * 256, rnd]
    stream = gather(ctx, [d], bs, True, search_match_len=6)
    sr = ManySearcher(ctx, stream)
    try:
        pairs, counts = brute_pairs(d, needles)
        assert counts == [511, 473, 257, 3]
        for i in range(3):
            L = len(needles[i])
            assert {(border - L, i), (border - L // 2, i), (border - 1, i), (border, i)} <= set(pairs)
        stats = check_many(sr, d, needles, "group border", no_tables=True)
        assert stats[1] == len([n for n, _ in SMod.data_grid(stream) if n]) == 67
        freq = b'":['                                                          # once per record
        assert len(SMod.brute(d[:1 << 20], freq)) > 1000
        check_many(sr, d, needles + [freq], "group border, frequent", cap=1000, no_tables=True)
    finally:
        sr.close()


def test_stored_chunks_on_both_sides_of_the_group_border(ctx):
    """9 blocks of 8 MiB, block 7 (the last of group 0) and block 8 (the first of group 1) random bytes, hence stored: the second group's
    stored chunk is copied into the scratch by pieces that lie behind the first group's.  Needles inside block 8, inside block 7 and
    across their border, which is the border of the groups; the search for one pattern takes the same way."""
    bs = 8 << 20
    base = synth.json_like(bs, 9).tobytes()
    d = bytearray(base * 7 + synth.random_bytes(2 * bs, seed=8).tobytes())
    needles = [bytes(SC.needle(24, 40 + i)) for i in range(3)]
    for nd, o in zip(needles, (8 * bs + 3 * (bs // 4) + 5, 7 * bs + 100_001, 8 * bs - 11)):
        d[o:o + 24] = nd
    d = bytes(d)
    stream = gather(ctx, [d], bs, True)
    grid = SMod.data_grid(stream)
    assert [n for n, _ in grid] == [bs] * 9 and grid[7][1] == grid[8][1] == 0x01 and all(t != 0x01 for _, t in grid[:7])
    sr = ManySearcher(ctx, stream)
    one = Searcher(ctx, stream)
    try:
        pairs, counts = brute_pairs(d, needles)
        assert counts == [1, 1, 1]
        stats = check_many(sr, d, needles + [d[8 * bs + 70_000:8 * bs + 70_003]], "stored chunks at the group border", no_tables=True)
        assert stats[1] == 9
        assert check_search(one, stream, d, needles[2], "stored chunks at the group border, one pattern")[1] == 9
    finally:
        sr.close()
        one.close()


# ---- arguments ----

def test_arguments(ctx):
    L = _lib.lib()
    stream = O.stream_encode(b"hello hello hello", 1, 4096)
    sr = ManySearcher(ctx, stream)
    try:
        h = sr.rd.handle
        pos = torch.full((4 + GUARD,), SENT, dtype=torch.int64, device="cuda")
        which = torch.full((4 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        counts = torch.full((3 + GUARD,), SENT, dtype=torch.int64, device="cuda")
        host = np.zeros(8, np.uint64)
        blob = b"hello" + b"llo h" + b"x" * 300
        stats = (C.c_uint64 * 4)()

        def call(n, lens, patterns=blob, c=counts.data_ptr(), p=pos.data_ptr(), w=which.data_ptr(), cap=4, handle=h):
            a = None if lens is None else np.asarray(lens, np.uint32)
            return L.mlz_dev_reader_search_many(handle, None, 0, patterns, None if a is None else a.ctypes.data, n, c, p, w, cap, stats)

        big = np.full(4097, 1, np.uint32)
        assert L.mlz_dev_reader_search_many(h, None, 0, b"x" * 4097, big.ctypes.data, 4097, None, pos.data_ptr(), which.data_ptr(), 4, None) == -MLZ_ERR_ARG
        assert call(2, [5, 0]) == -MLZ_ERR_ARG and call(3, [5, 5, 257]) == -MLZ_ERR_ARG
        assert call(2, [5, 5], patterns=None) == -MLZ_ERR_ARG and call(2, None) == -MLZ_ERR_ARG
        assert call(2, [5, 5], p=None) == -MLZ_ERR_ARG and call(2, [5, 5], w=None) == -MLZ_ERR_ARG
        assert call(2, [5, 5], p=host.ctypes.data) == -MLZ_ERR_ARG and call(2, [5, 5], w=host.ctypes.data) == -MLZ_ERR_ARG
        assert call(2, [5, 5], c=host.ctypes.data) == -MLZ_ERR_ARG
        assert call(2, [5, 5], handle=None) == -MLZ_ERR_ARG
        assert call(0, None, patterns=None) == 0 and call(0, [5]) == 0
        torch.cuda.synchronize()
        assert (pos.cpu().numpy() == SENT).all() and (which.cpu().numpy() == SENT32).all() and (counts.cpu().numpy() == SENT).all()
        assert call(3, [5, 5, 256]) == 5 and list(stats) == [1, 1, 0, 3]
        torch.cuda.synchronize()
        assert pos.cpu().tolist()[:4] == [0, 2, 6, 8] and which.cpu().tolist()[:4] == [0, 1, 0, 1] and counts.cpu().tolist()[:3] == [3, 2, 0]
        assert (pos.cpu().numpy()[4:] == SENT).all() and (which.cpu().numpy()[4:] == SENT32).all() and (counts.cpu().numpy()[3:] == SENT).all()
        assert call(2, [5, 5], c=None, p=None, w=None, cap=0) == 5
    finally:
        sr.close()
    for empty in (b"", O.stream_encode(b"", 1, 4096)):
        sr = ManySearcher(ctx, empty)
        try:
            assert sr([b"abc", b"d"], 4) == (0, [], [0, 0], (0, 0, 0, 0))
            assert sr([b"abc", b"d"], 0, null=True, no_tables=True) == (0, [], [0, 0], (0, 0, 0, 0))
        finally:
            sr.close()


# ---- the tensor front end ----

def test_tensor_front_end(ctx):
    bs = 64 << 10
    d, nd, at = SC.planted("text_like", bs, 9, 16, 2, tail=100)
    stream = gather(ctx, [d], bs, True, search_match_len=6)
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    pats = [nd, b"the ", nd[:8]]
    pairs, counts = brute_pairs(d, pats)
    with shard.HipTensorCodec(ctx).open_stream(t) as ds:
        pos, which, cnt, total = ds.search_many(pats, 5)
        assert total == len(pairs) and pos.dtype == torch.int64 and which.dtype == torch.int32 and cnt.dtype == torch.int64
        assert pos.device == which.device == cnt.device == t.device
        assert list(zip(pos.cpu().tolist(), which.cpu().tolist())) == pairs[:5] and cnt.cpu().tolist() == counts
        pos, which, cnt, total = ds.search_many(pats, 0)
        assert total == len(pairs) and pos.numel() == which.numel() == 0 and cnt.cpu().tolist() == counts
        pos, which, cnt, total = ds.search_many([], 3)
        assert total == 0 and pos.numel() == 0 and cnt.numel() == 0
