"""mlz_dev_reader_grep_regex_pruned (DeviceReader.grep_regex, DeviceStream.grep_regex and DeviceStreamSet.grep_streams_regex with prune=True) on the
GPU: the results are tests/regex_model.py's, Python's `re` over the decoded bytes, and the unpruned call's; what is decoded is what
tests/search_model.py plans for the expression's required literals (tests/regex_prune_model.py), widened to whole records.  The streams are
tests/test_gpu_stream_regex.py's, written by the device Writer with type 1 tables and match length 6.  Both output arrays are guarded by sentinels."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, api, shard, synth
from minlz_amd.api import search_config
from tests import corrupt as CM
from tests import fold_model as FM
from tests import grep_model as GM
from tests import regex_model as RM
from tests import regex_prune_model as PM
from tests import search_model as SMod
from tests import stream_batch_cases as BC
from tests.search_gpu import SENT, Opened, dev_u8, gather
from tests.test_gpu_stream_regex import BS, COMBOS, EXPRS, GUARD, KIND_SENT, NBLK, NL, Regexed, regex_case

pytestmark = pytest.mark.gpu

MLZ_ERR_CRC, MLZ_ERR_ARG = 5, 8
IGNORE_CRC, NO_TABLES, INVERT = 2, 8, 16
TABLES = dict(search_match_len=6)


class Pruned(Regexed):
    """tests/test_gpu_stream_regex.py's handle with the pruned call: check() compares a call whole with the model and returns (the model's answer, stats)."""

    def raw(self, handle, cap, flags=0, before=0, after=0, null=False, pruned=True):
        if not pruned:
            return super().raw(handle, cap, flags, before, after, null)
        no = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
        kd = torch.full((cap + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
        totals, stats = (C.c_uint64 * 4)(*([77] * 4)), (C.c_uint64 * 4)(*([77] * 4))
        r = _lib.lib().mlz_dev_reader_grep_regex_pruned(self.rd.handle, None, flags, handle, before, after, None if null else no.data_ptr(), None if null else kd.data_ptr(), cap, totals, stats)
        torch.cuda.synchronize()
        return r, no.cpu().numpy(), kd.cpu().numpy(), tuple(int(v) for v in totals), tuple(int(v) for v in stats)

    def check(self, exprs, what, cap=None, fold=False, invert=False, before=0, after=0, flags=0):
        m = self.model(exprs, fold, invert, before, after)
        cap = m["R"] + 3 if cap is None else cap
        want = RM.cut(m, cap)
        r, no, kd, totals, stats = self.raw(self.regex(exprs, fold).handle, cap, flags | (INVERT if invert else 0), before, after, null=cap == 0)
        k = min(want["R"], cap)
        what = "%s: invert %s, before %d, after %d, cap %d" % (what, invert, before, after, cap)
        assert r == want["R"] and totals == want["totals"], (what, r, totals, want["totals"])
        assert no[:k].tolist() == want["numbers"], what
        assert (no[k:] == SENT).all(), what + ": written beyond the numbers"
        assert kd[:k].tolist() == want["kinds"] and (kd[k:] == KIND_SENT).all(), what
        if self.nck is None:
            self.nck = sum(1 for n, _ in SMod.data_grid(self.stream) if n)
        assert stats[0] == len(SMod.data_grid(self.stream)) and stats[3] <= stats[1] <= self.nck and stats[2] <= self.nck, (what, stats)
        assert self.ctx.search_plan() == stats[1:3], what
        return want, stats

    def attach(self, cfgs):
        cap = self.rd.sidecar_bound(cfgs)
        room = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.side = room[:self.rd.build_sidecar(cfgs, room.data_ptr(), cap)].clone()
        self.rd.attach_sidecar(self.side.data_ptr(), self.side.numel())

    def planned(self, exprs, fold=False):
        """The chunks tests/search_model.py (tests/fold_model.py under the flag) plans for the expression's literals, united; None: no literals."""
        lits = PM.literals(exprs, fold)
        assert self.regex(exprs, fold).literals() == (lits, fold)
        if not lits:
            return None
        return set().union(*[set((FM if fold else SMod).plan_of_stream(self.stream, l)[0]) for l in lits])

    def usable(self, literal):
        """What stats[2] reports for a literal the tables serve: the chunks with a usable table, by the model."""
        return SMod.plan_of_stream(self.stream, literal)[2]


@pytest.fixture(scope="module")
def main(ctx):
    d = regex_case()
    stream = gather(ctx, [d], BS, True, **TABLES)
    assert len(SMod.data_grid(stream)) == NBLK + 1 and SMod.read_tables(stream)[0] is not None
    h = Pruned(ctx, stream, d)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(EXPRS))
def test_expressions_against_the_model(main, name):
    """Every expression of tests/test_gpu_stream_regex.py under (invert, before, after) in {(0,0,0), (1,0,0), (0,3,3), (0,N,N)} and rec_cap in
    {0, 1, R - 1, R, R + 5}: numbers, kinds and totals are the model's; the value and the arrays are the unpruned call's."""
    h, exprs = main, EXPRS[name]
    for invert, before, after in COMBOS:
        b, a = (h.N if before is None else before), (h.N if after is None else after)
        R = h.model(exprs, False, invert, b, a)["R"]
        for cap in sorted({0, 1, max(R - 1, 0), R, R + 5}):
            h.check(exprs, name, cap=cap, invert=invert, before=b, after=a)
        rx = h.regex(exprs).handle
        flags = INVERT if invert else 0
        got, plain = h.raw(rx, R + 5, flags, b, a), h.raw(rx, R + 5, flags, b, a, pruned=False)
        assert got[0] == plain[0] == R and (got[1] == plain[1]).all() and (got[2] == plain[2]).all() and got[3] == plain[3], name


@pytest.mark.parametrize("name", ["across a block border", "nothing"])
def test_pruning_happens(main, name):
    """The chunks the plan takes are those tests/search_model.py computes for the literals, fewer than the stream has; the unpruned call decodes all."""
    h, exprs = main, EXPRS[name]
    plan = h.planned(exprs)
    nck = NBLK + 1
    assert plan is not None and len(plan) < nck, (name, sorted(plan))                               # the model itself says that the tables prune
    want, stats = h.check(exprs, name)
    assert stats[3] == len(plan) and stats[2] == h.usable(PM.literals(exprs)[0]) > 0 and stats[1] < nck, (stats, sorted(plan))
    assert h.raw(h.regex(exprs).handle, 4, pruned=False)[4][1:] == (nck, 0, 0)
    if name == "nothing":
        assert want["R"] == 0
    else:
        assert want["R"] == 1 and {4, 5} <= plan                                                   # the needle lies across the border of blocks 4 and 5


def widen_case(last):
    """8 blocks of 64 KiB of lines; one record of about 150 KiB starts late in block 2 with an A and ends early in block 5 with `last`; its only
    `needle`, the stream's only one, lies in the middle of block 3."""
    d = bytearray(synth.json_like(BS * NBLK, 31).tobytes().replace(b"needle", b"noodle"))
    s, e = 2 * BS + 56000, 5 * BS + 9000
    d[s:e] = bytes(d[s:e]).replace(NL, b" ")
    d[s - 1:s], d[e:e + 1] = NL, NL
    d[s:s + 1], d[e - 1:e] = b"A", last
    d[3 * BS + 30000:3 * BS + 30006] = b"needle"
    d[-1:] = NL
    return bytes(d), bytes(d).count(NL, 0, s)


def test_widening_happens(ctx):
    """`^A.*needle.*Z$`, whose literal is `needle`: the plan takes the chunk that holds it and the one behind it (the bytes an occurrence may
    reach into); the record matches only through its first byte in block 2 and its last in block 5, so both are decoded too: stats[1] >=
    stats[3] + 2 and the record is selected.  The same record with its last byte changed is not."""
    expr = b"^A.*needle.*Z$"
    for last, selected in ((b"Z", True), (b"Y", False)):
        d, r = widen_case(last)
        assert d.count(b"needle") == 1 and len(GM.records(d, NL)[r]) > 140 << 10
        h = Pruned(ctx, gather(ctx, [d], BS, True, **TABLES), d)
        try:
            plan = h.planned(expr)
            assert 3 in plan and 2 not in plan and 5 not in plan                                     # (the model: neither end of the record is planned)
            want, stats = h.check(expr, "a record across four blocks", before=1, after=1)
            assert stats[3] == len(plan) and stats[1] >= stats[3] + 2 and stats[1] < NBLK, stats
            assert want["M"] == ([r] if selected else [])
        finally:
            h.close()


def test_degenerate_sets(ctx, main):
    """No literals, MLZ_SEARCH_NO_TABLES, a stream without tables and a set handle decode every chunk and give the model's answer; an attached
    sidecar prunes as the inline tables do.  Literals that hold the delimiter: M is empty and nothing is decoded, while the unpruned call decodes
    everything.  The case flag on a planted id with digits prunes and finds every case variant."""
    nck = NBLK + 1
    d, expr = main.data, EXPRS["across a block border"]
    inline = main.check(expr, "inline tables", before=2, after=1)
    assert inline[1][1] < nck
    assert main.check(b"^$", "no literals", before=1)[1][1:] == (nck, 0, nck)
    assert main.check(expr, "no tables asked for", before=2, after=1, flags=NO_TABLES)[1][1:] == (nck, 0, nck)
    assert main.check(expr, "no tables asked for, CRCs ignored", before=2, after=1, flags=NO_TABLES | IGNORE_CRC)[0] == inline[0]
    bare = Pruned(ctx, gather(ctx, [d], BS, True), d)
    try:
        want, stats = bare.check(expr, "a stream without tables", before=2, after=1)
        assert stats[1:] == (nck, 0, nck) and want == inline[0]
        bare.attach([search_config(1, 6)])
        want, stats = bare.check(expr, "a sidecar attached", before=2, after=1)
        assert want == inline[0] and stats[2] > 0 and stats[3] <= stats[1] < nck, stats
        bare.rd.detach_sidecar()
    finally:
        bare.close()
    datas = [d[:70000], b"", d[70000:70050], b"\n\n", d[70050:]]
    buf, spans = BC.back_to_back([gather(ctx, [x], BS, True, **TABLES) if x else O.stream_encode(x, 1, BS) for x in datas], 64)
    codec = shard.HipTensorCodec(ctx)
    with codec.open_streams(dev_u8(buf), spans) as st, api.Regex(expr) as rx:
        st.reader.index_records(NL)
        m = RM.result(b"".join(datas), NL, expr, before=2, after=1)                                  # the streams' concatenation
        no = torch.full((m["R"] + GUARD,), SENT, dtype=torch.int64, device="cuda")
        R, totals, stats = st.reader.grep_regex(rx, no.data_ptr(), None, m["R"], before=2, after=1, prune=True)
        torch.cuda.synchronize()
        assert R == m["R"] and totals == m["totals"] and no.cpu().numpy()[:R].tolist() == m["numbers"] and (no.cpu().numpy()[R:] == SENT).all()
        assert stats[1] == stats[3] >= nck and stats[2] == 0, stats                                 # a set handle: every chunk with bytes, no table
    # a literal that holds the delimiter cannot lie inside a record
    for e in (b'\\}\\n\\{"id"', b"a\\nb|c\\n"):
        lits = PM.literals(e)
        assert lits and all(NL in l for l in lits)
        want, stats = main.check(e, "literals across records", before=1, after=1)
        assert want["M"] == [] and stats[1:] == (0, 0, 0)
        assert main.check(e, "the same inverted", invert=True)[0]["R"] == main.N
        assert main.raw(main.regex(e).handle, 4, pruned=False)[4][1:] == (nck, 0, 0)
    # the case flag: an id with digits in three cases, in blocks 1 and 2 (the plan brings the block behind each along, the widening the blocks around)
    dd = bytearray(synth.json_like(BS * NBLK, 33).tobytes())
    for at, variant in ((BS + 777, b"Id#4711-q"), (BS + 30000, b"ID#4711-Z"), (2 * BS + 4000, b"id#4711-m")):
        dd[at:at + len(variant)] = variant
    dd = bytes(dd)
    h = Pruned(ctx, gather(ctx, [dd], BS, True, **TABLES), dd)
    try:
        e = b"iD#4711-[a-z]"
        plan = h.planned(e, True)
        assert {1, 2} <= plan and len(plan) + 2 < NBLK
        want, stats = h.check(e, "the case flag", fold=True)
        assert len(want["M"]) == 3 and stats[3] == len(plan) and stats[1] < NBLK, stats
        assert h.check(e, "the same without the flag")[0]["M"] == []
    finally:
        h.close()


def test_a_broken_chunk(ctx, main):
    """A flipped CRC byte in a chunk the tables prune goes unnoticed: the model's answer.  The same chunk admitted — by an expression whose literal it
    holds, or without tables — gives -MLZ_ERR_CRC with both arrays untouched, and the model's answer under MLZ_STREAM_IGNORE_CRC."""
    d, s = main.data, main.stream
    expr = EXPRS["across a block border"]
    plan = main.planned(expr)
    cs = [(c.off, c.clen) for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    j = next(j for j in range(2, NBLK) if not {j - 1, j, j + 1} & plan)                              # a compressed block far from the needle's
    b = bytearray(s)
    b[cs[j][0] + 5] ^= 0x10
    h = Pruned(ctx, bytes(b), d, ignore_crc=True)                                                    # (the index build decodes every chunk)
    try:
        want, stats = h.check(expr, "a broken chunk that is pruned", before=1, after=1)
        assert want["R"] == 3 and stats[1] < NBLK + 1
        at = d.find(NL, j * BS + 100) + 1
        while d.count(d[at:at + 24]) != 1 or NL in d[at:at + 24]:                                    # 24 bytes of block j that lie nowhere else
            at = d.find(NL, at) + 1
        assert at + 24 < (j + 1) * BS - 100
        admitted = b"".join(b"\\" + bytes([c]) if bytes([c]) in PM.META else bytes([c]) for c in d[at:at + 24])
        for e, flags in ((admitted, 0), (expr, NO_TABLES), (b"^$", 0)):
            r, no, kd, totals, _ = h.raw(h.regex(e).handle, 16, flags, 1, 1)
            assert r == -MLZ_ERR_CRC and (no == SENT).all() and (kd == KIND_SENT).all(), e
        with pytest.raises(mz.ErrCRC):
            h.rd.grep_regex(h.regex(admitted), None, None, 0, prune=True)
        assert h.check(admitted, "ignore crc", before=1, after=1, flags=IGNORE_CRC)[0]["R"] >= 1
    finally:
        h.close()


BEFORE = b"@before-the-groups-border-4711@"      # long, so that no block's table holds all of its windows by chance


def hole_case(blk):
    """Eleven blocks of blk bytes and a short twelfth.  BEFORE lies in every block but the third, the fourth and the fifth: the tables leave
    the fourth out (the third is the block behind an admitted one, the fifth may be admitted for what could begin at its end), and a delimiter
    ends each of the blocks around it, so no record reaches into it.  The record across the border of blocks 8 and 9 holds BEFORE in front of
    the border and `@after@` behind it; one more record holds both.  -> (the data, the border)."""
    unit = synth.json_like((1 << 20) + 37, 21).tobytes()
    n = 11 * blk + 4321
    d = bytearray((unit * (n // len(unit) + 1))[:n])
    border = 9 * blk
    d[border - 100:border + 60] = bytes(d[border - 100:border + 60]).replace(NL, b" ")
    assert border - d.rfind(NL, 0, border) > 80 and d.find(NL, border) - border > 40                 # a record straddles the border
    d[border - 60:border - 60 + len(BEFORE)] = BEFORE
    d[border + 10:border + 17] = b"@after@"
    for k in range(11):
        if k not in (2, 3, 4):
            at = d.find(NL, k * blk + 5000) + 1
            d[at + 3:at + 3 + len(BEFORE)] = BEFORE                                                  # (a record of its own, without @after@)
    at = d.find(NL, 5 * blk + 30000) + 1
    d[at + 3:at + 3 + len(BEFORE) + 12] = BEFORE + b" and @after@"
    d[3 * blk - 1:3 * blk], d[4 * blk - 1:4 * blk] = NL, NL
    d[-1:] = NL
    assert d.count(BEFORE, 2 * blk - 40, 5 * blk + 40) == 0
    return bytes(d), border


def test_two_decode_groups_with_a_hole(ctx):
    """About 88 MiB in 8 MiB blocks (hole_case): the plan and the widening leave the fourth block out, so the first decode group (64 MiB) holds the
    blocks 0 - 2 and 4 - 8, two pieces of runs, and the second the rest; the run of the blocks from 4 on goes on across the groups' border, and
    the record that straddles it matches through its carried state.  (A hole AT the groups' border would be closed by the widening of that very
    record, so the hole lies inside the first group.)  Against `re` on the records that hold the literal: no other record can match."""
    blk = 8 << 20
    d, border = hole_case(blk)
    expr = BEFORE + b".*@after@"
    assert PM.literals(expr) == [BEFORE]
    stream = gather(ctx, [d], blk, False, **TABLES)
    nck = len(SMod.data_grid(stream))
    plan = set(SMod.plan_of_stream(stream, BEFORE)[0])
    assert nck == 12 and 3 not in plan and plan >= set(range(12)) - {3, 4}                           # the model itself says so (the widening adds block 4 if the plan did not)
    h = Opened(ctx, stream)
    try:
        h.rd.index_records(NL)
        want = set()
        for m in re.finditer(re.escape(BEFORE), d):                                                        # the records that hold the literal; no other can match
            s0 = d.rfind(NL, 0, m.start()) + 1
            if RM.pattern(expr).search(d[s0:d.find(NL, s0)]):
                want.add(d.count(NL, 0, s0))
        want = sorted(want)
        assert len(want) == 2 and d.count(NL, 0, border) in want
        no = torch.full((8 + GUARD,), SENT, dtype=torch.int64, device="cuda")
        with api.Regex(expr) as rx:
            R, totals, stats = h.rd.grep_regex(rx, no.data_ptr(), None, 8, prune=True)
            torch.cuda.synchronize()
            assert R == 2 and no.cpu().numpy()[:2].tolist() == want and (no.cpu().numpy()[2:] == SENT).all()
            assert stats[:2] == (nck, nck - 1) and stats[2] > 0 and stats[3] == len(plan), stats
            assert h.rd.grep_regex(rx, None, None, 0, invert=True, prune=True)[0] == h.rd.record_count() - 2
            assert h.rd.grep_regex(rx, None, None, 0)[0] == 2
    finally:
        h.close()


def test_device_stream_and_set(ctx):
    """DeviceStream.grep_regex(prune=True) and DeviceStreamSet.grep_streams_regex(prune=True) return what they return with prune=False."""
    d = regex_case(BS, 6)
    t = dev_u8(gather(ctx, [d], BS, True, **TABLES))
    codec = shard.HipTensorCodec(ctx)

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y

    with codec.open_stream(t) as ds:
        for exprs, kw in ((b"tag1[0-9]{2}", dict(before=2, after=1)), ([b"^$", b"laws"], {}), (b"TAG00", dict(ignore_case=True, invert=True, max_records=50)), (b"nomatch[0-9]", {}),
                          (EXPRS["across a block border"], dict(after=2))):
            same(ds.grep_regex(exprs, prune=True, **kw), ds.grep_regex(exprs, **kw))
            assert ds.grep_regex(exprs, count_only=True, prune=True, **kw) == ds.grep_regex(exprs, count_only=True, **kw)
        assert ds.grep_regex(EXPRS["across a block border"], count_only=True, prune=True) == (1, 1)
        with api.Regex(b"nomatch[0-9]") as rx:
            assert ds.reader.grep_regex(rx, None, None, 0, prune=True)[2][1] < ds.reader.grep_regex(rx, None, None, 0)[2][1]
            with pytest.raises(ValueError):
                ds.reader.grep_regex(rx, None, None, 0, no_tables=True)
    datas = [d[:70000], b"", d[70000:70050], b"\n\n", d[70050:150000]]
    buf, spans = BC.back_to_back([gather(ctx, [x], BS, True, **TABLES) if x else b"" for x in datas], 64)
    with codec.open_streams(dev_u8(buf), spans) as st:
        for e in (b'"user_3[0-9]{2}7"|^$', b'"user_3[0-9]{2}7"'):
            same(st.grep_streams_regex(e, before=1, prune=True), st.grep_streams_regex(e, before=1))
            same(st.grep_regex(e, before=1, prune=True), st.grep_regex(e, before=1))
