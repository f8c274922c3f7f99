"""mlz_dev_reader_grep_regex (DeviceReader.grep_regex, DeviceStream.grep_regex, DeviceStreamSet.grep_streams_regex) on the GPU against
tests/regex_model.py, Python's `re` over the decoded bytes: the matching records, inverted match, context records, record numbers and kinds, the
four totals and the cut at rec_cap.  Both output arrays are guarded by sentinels and compared whole."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, api, shard, synth
from tests import corrupt as CM
from tests import grep_model as GM
from tests import regex_model as RM
from tests import search_model as SMod
from tests import stream_batch_cases as BC
from tests import stream_set_model as SetM
from tests.search_gpu import SENT, Opened, dev_u8, gather

pytestmark = pytest.mark.gpu

MLZ_ERR_UNSUPPORTED, MLZ_ERR_CRC, MLZ_ERR_ARG = 3, 5, 8
IGNORE_CRC, NO_TABLES, INVERT = 2, 8, 16
NL = b"\n"
GUARD = 8
KIND_SENT = 0x5A
SPAN = b"@zq-needle-77@"
BS, NBLK = 64 << 10, 8


def regex_case(bs=BS, nblk=NBLK):
    """JSON-like lines with a stored (random) block and delimiters planted at block borders (bs - 1, bs), doubled ones, at the stream's first and
    last byte: the shape of the grep's test streams.  One needle lies across a block border (5 * bs) and nowhere else; a pattern with thousands
    of occurrences fills two long records."""
    d = bytearray(synth.json_like(bs * nblk + 700, 11).tobytes())
    d[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
    for k in (1, 2, 3, 5):
        d[k * bs - 1:k * bs + 1] = b"\n\n"
    d[4 * bs - 1:4 * bs] = NL
    d[6 * bs:6 * bs + 1] = NL
    d[3 * bs + 50:3 * bs + 54] = b"\n\n\n\n"
    d[0:1] = NL
    d[-1:] = NL
    d[5 * bs - 27:5 * bs + 27] = b"x" * 20 + SPAN + b"y" * 20          # (no delimiter near it: the record crosses the border)
    half = len(d) // 2
    d[half + 3000:half + 9000] = b"hot!" * 1500
    return bytes(d)


# name -> expression(s): about a dozen of tests/test_stream_regex_host.py's constructs on lines that hold them
EXPRS = {
    "empty lines": b"^$",
    "class and counted repetition": b'"user_3[0-9]{2}7"',
    "three words": b"DON'T|flushed|laws-a-me",
    "opening brace": b"^\\{",
    "closing brace": b"\\}$",
    "across a block border": b"x{3}@zq-(needle|nail)-7+@y+",
    "nothing": b"nomatch[0-9]+zz",
    "anchored tail": b'"val":[0-9]+\\.[0-9]{6}\\}$',
    "anchored head": b'^\\{"id":\\d+,"ts":"2026-01-01T00:0[0-3]:',
    "one tag": b'"tags":\\["tag[0-9]{3}"\\],',
    "nested groups": b"(tag0(0[0-9]|1[0-5])\",?)+\\]",
    "two expressions": (b"user_1\\d+\"", b"^$"),
    "a long run": b"(hot!){200}.*\\}$",
    "any byte": b"^.[\\x80-\\xff].*\\x00",
}
COMBOS = [(False, 0, 0), (True, 0, 0), (False, 3, 3), (False, None, None)]     # (invert, before, after); None: N


class Regexed(Opened):
    """A stream on the device, its decoded bytes and an open handle with an index; check() compares a call whole with the model."""

    def __init__(self, ctx, stream, data, delim=NL, index=True, **kw):
        super().__init__(ctx, stream)
        self.data, self.stream, self.delim = bytes(data), bytes(stream), delim
        self.models, self.compiled, self.nck = {}, {}, None
        if index:
            self.N = self.rd.index_records(delim, **kw)[0]
            assert self.N == len(GM.records(self.data, delim))

    def regex(self, exprs, fold=False):
        key = (exprs, fold)
        if key not in self.compiled:
            self.compiled[key] = api.Regex(exprs, ignore_case=fold)
        return self.compiled[key]

    def raw(self, handle, cap, flags=0, before=0, after=0, null=False):
        """-> (the call's value, numbers, kinds, totals, stats): the guarded arrays whole."""
        no = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
        kd = torch.full((cap + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
        totals, stats = (C.c_uint64 * 4)(*([77] * 4)), (C.c_uint64 * 4)(*([77] * 4))
        r = _lib.lib().mlz_dev_reader_grep_regex(self.rd.handle, None, flags, handle, before, after, None if null else no.data_ptr(), None if null else kd.data_ptr(), cap, totals, stats)
        torch.cuda.synchronize()
        return r, no.cpu().numpy(), kd.cpu().numpy(), tuple(int(v) for v in totals), tuple(int(v) for v in stats)

    def model(self, exprs, fold, invert, before, after):
        key = (exprs, fold, invert, before, after)
        if key not in self.models:
            self.models[key] = RM.result(self.data, self.delim, exprs, fold, invert, before, after)
        return self.models[key]

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
        assert stats[1:] == (self.nck, 0, 0) and self.ctx.search_plan() == (self.nck, 0), what   # every chunk with bytes decoded once, no table
        return want

    def close(self):
        for rx in self.compiled.values():
            rx.close()
        super().close()


@pytest.fixture(scope="module")
def main(ctx):
    d = regex_case()
    stream = gather(ctx, [d], BS, True)
    grid = SMod.data_grid(stream)
    assert grid[1][1] == 0x01 and len(grid) == NBLK + 1                          # the random block: stored
    h = Regexed(ctx, stream, d)
    recs = GM.records(d, NL)
    assert sum(1 for r in recs if not r) >= 6 and d.count(SPAN) == 1 and d.find(SPAN) < 5 * BS < d.find(SPAN) + len(SPAN)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(EXPRS))
def test_expressions_against_the_model(main, name):
    """Numbers, kinds and the four totals for (invert, before, after) in {(0,0,0), (1,0,0), (0,3,3), (0,N,N)} and rec_cap in {0, 1, R - 1, R, R + 5}."""
    h, exprs = main, EXPRS[name]
    M = h.model(exprs, False, False, 0, 0)["M"]
    assert (len(M) == 0) == (name == "nothing") and len(M) < h.N
    if name == "across a block border":
        assert len(M) == 1
    if name == "empty lines":
        assert M == [r for r, rec in enumerate(GM.records(h.data, NL)) if not rec]
    for invert, before, after in COMBOS:
        b, a = (h.N if before is None else before), (h.N if after is None else after)
        R = h.model(exprs, False, invert, b, a)["R"]
        for cap in sorted({0, 1, max(R - 1, 0), R, R + 5}):
            h.check(exprs, name, cap=cap, invert=invert, before=b, after=a)


def test_a_literal_is_grep_records(main):
    """For an expression that is a literal the numbers, kinds and totals are mlz_dev_reader_grep_records' with that literal under MLZ_SEARCH_NO_TABLES."""
    h = main
    for lit in (b"user_3434", SPAN, b"hot!hot!", b'],"msg":"'):
        for invert, before, after in ((False, 0, 0), (True, 1, 2), (False, 2, 0)):
            cap = h.N + 3
            no = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
            kd = torch.full((cap + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
            R, totals, _ = h.rd.grep_records([lit], no.data_ptr(), kd.data_ptr(), cap, invert=invert, before=before, after=after, no_tables=True)
            torch.cuda.synchronize()
            r, rno, rkd, rtotals, _ = h.raw(h.regex(re.escape(lit)).handle, cap, INVERT if invert else 0, before, after)
            assert r == R and rtotals == totals and R > 0, lit
            assert (rno == no.cpu().numpy()).all() and (rkd == kd.cpu().numpy()).all(), lit


def test_ignore_case(main):
    """An expression in swapped case selects what the model selects under re.IGNORECASE; without the flag it selects nothing."""
    h = main
    swapped = b"LAWS-A-ME|\"USER_3[0-9]{2}7\"|don't [a-c]"
    want = h.check(swapped, "ignore case", fold=True)
    assert want["R"] > 5 and want["M"] == RM.result(h.data, NL, swapped.swapcase(), True)["M"]
    assert h.check(swapped, "the same without the flag")["R"] < want["R"]
    h.check(b"[^a-z]{30}", "a negated class under the fold", fold=True, before=1, after=1)


def test_argument_errors_write_nothing(ctx):
    d = regex_case(BS, 6)
    L = _lib.lib()
    h = Regexed(ctx, gather(ctx, [d], BS, True), d, index=False)
    try:
        rx = h.regex(b"tag1")
        r, no, kd, totals, stats = h.raw(rx.handle, 8)                                               # a handle without an index
        assert r == -MLZ_ERR_ARG and (no == SENT).all() and (kd == KIND_SENT).all()
        h.N = h.rd.index_records(NL)[0]
        host = np.zeros(16, np.uint64)
        no = torch.full((8 + GUARD,), SENT, dtype=torch.int64, device="cuda")
        kd = torch.full((8 + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")

        def call(flags=0, regex=rx.handle, p=no.data_ptr(), k=kd.data_ptr(), cap=8, handle=h.rd.handle):
            return L.mlz_dev_reader_grep_regex(handle, None, flags, regex, 1, 1, p, k, cap, None, None)

        bad = [call(regex=None), call(flags=NO_TABLES), call(flags=32), call(flags=1), call(flags=4), call(flags=INVERT | 64), call(p=None), call(p=host.ctypes.data),
               call(k=host.ctypes.data), call(handle=None)]
        torch.cuda.synchronize()
        assert bad == [-MLZ_ERR_ARG] * len(bad)
        assert (no == SENT).all() and (kd == KIND_SENT).all()
        R = RM.result(d, NL, b"tag1", before=1, after=1)["R"]
        assert R > 8 and call(p=None, k=None, cap=0) == R and call(k=None) == R                     # d_rec_kind may be NULL
        torch.cuda.synchronize()
        assert (no[8:] == SENT).all() and (no[:8] != SENT).all() and (kd == KIND_SENT).all()
        with pytest.raises(ValueError):
            rx.close()
            h.rd.grep_regex(rx, None, None, 0)                                                       # a closed Regex never reaches the library
        h.compiled.clear()
    finally:
        h.close()


def test_the_empty_stream_and_one_record(ctx):
    d = b"one record with a needle and no delimiter"
    h = Regexed(ctx, gather(ctx, [d], BS, True), d)
    try:
        assert h.N == 1
        for expr, R in ((b"ne+dle", 1), (b"^needle", 0), (b"delimiter$", 1), (b"^$", 0), (b"", 1)):
            assert h.check(expr, "one record", before=7, after=7)["R"] == R
            assert h.check(expr, "one record", invert=True)["R"] == 1 - R
    finally:
        h.close()
    for empty in (b"", O.stream_encode(b"", 1, 1 << 20)):
        h = Regexed(ctx, empty, b"")
        try:
            assert h.N == 0
            for flags in (0, INVERT):
                r, no, kd, totals, stats = h.raw(h.regex(b"").handle, 4, flags, 3, 3)
                assert r == 0 and totals == (0, 0, 0, 0) and (no == SENT).all() and (kd == KIND_SENT).all() and stats[1:] == (0, 0, 0)
        finally:
            h.close()


def test_broken_chunks(ctx):
    """A flipped CRC byte: -MLZ_ERR_CRC with nothing written, whichever chunk it is in (no table prunes); under MLZ_STREAM_IGNORE_CRC the model's answer."""
    d = regex_case()
    s = gather(ctx, [d], BS, True)
    cs = [(c.off, c.clen) for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    expr = EXPRS["three words"]
    for j in (0, 1, len(cs) - 1):                                                                    # the first, the stored one, the last
        b = bytearray(s)
        b[cs[j][0] + 5] ^= 0x10
        h = Regexed(ctx, bytes(b), d, ignore_crc=True)                                               # (the index build decodes every chunk)
        try:
            r, no, kd, totals, _ = h.raw(h.regex(expr).handle, 16, 0, 1, 1)
            assert r == -MLZ_ERR_CRC and (no == SENT).all() and (kd == KIND_SENT).all()
            with pytest.raises(mz.ErrCRC):
                h.rd.grep_regex(h.regex(expr), None, None, 0)
            h.check(expr, "ignore crc", before=1, after=1, flags=IGNORE_CRC)
        finally:
            h.close()


def long_record_case(length):
    """3 MiB of lines with one record of exactly `length` bytes from 1 MiB on: its newlines are blanks, an 'a' is its first and a 'z' its last byte."""
    d = bytearray(synth.json_like(3 << 20, 12).tobytes())
    a = 1 << 20
    d[a:a + length] = bytes(d[a:a + length]).replace(b"\n", b" ")
    d[a - 1:a] = NL
    d[a + length:a + length + 1] = NL
    d[a:a + 1] = b"a"
    d[a + length - 1:a + length] = b"z"
    d[-1:] = NL
    return bytes(d)


def test_record_length_bound(ctx):
    """An index whose longest record exceeds MLZ_REGEX_MAX_RECORD by one byte is refused before any chunk is decoded, nothing written; the length is
    kept beside the index and found anew when another delimiter replaces it; a record of exactly the bound is walked."""
    bound = api.REGEX_MAX_RECORD
    d = long_record_case(bound + 1)
    h = Regexed(ctx, gather(ctx, [d], 1 << 20, True), d)
    try:
        assert max(len(r) for r in GM.records(d, NL)) == bound + 1
        rx = h.regex(b"^a.*z$")
        for _ in range(2):                                                                           # the second call answers from the handle
            r, no, kd, totals, stats = h.raw(rx.handle, 8, 0, 1, 1)
            assert r == -MLZ_ERR_UNSUPPORTED and (no == SENT).all() and (kd == KIND_SENT).all() and stats[1:] == (0, 0, 0) and h.ctx.search_plan() == (0, 0)
        with pytest.raises(mz.ErrUnsupported):
            h.rd.grep_regex(rx, None, None, 0)
        h.N = h.rd.index_records(b",")[0]                                                            # by commas every record is short
        h.delim, h.models = b",", {}
        assert h.check(b'^"ts":"2026', "by commas", cap=50, after=1)["R"] > 1000
        h.N = h.rd.index_records(NL)[0]
        assert h.raw(rx.handle, 8)[0] == -MLZ_ERR_UNSUPPORTED
    finally:
        h.close()
    d = long_record_case(bound)
    h = Regexed(ctx, gather(ctx, [d], 1 << 20, True), d)
    try:
        want = h.check(b"^a.*z$", "a record of exactly the bound")
        assert want["R"] == 1 and len(want["recs"][want["numbers"][0]]) == bound
    finally:
        h.close()


def test_two_decode_groups(ctx):
    """About 72 MiB in 8 MiB blocks: a group of 8 chunks (64 MiB) and a second one.  The record that straddles the groups' border carries its state
    over: an expression whose only match begins in the first group and ends in the second, one that is decided in the first, one anchored at the end."""
    unit = synth.json_like((1 << 20) + 37, 21).tobytes()
    n = (72 << 20) + 4321
    d = bytearray((unit * (n // len(unit) + 1))[:n])
    border = 64 << 20
    d[border - 60:border + 60] = bytes(d[border - 60:border + 60]).replace(NL, b" ")
    lo, hi = d.rfind(NL, 0, border), d.find(NL, border)
    assert border - lo > 40 and hi - border > 40                                                     # a record straddles the border
    d[border - 30:border - 22] = b"@before@"
    d[border + 10:border + 17] = b"@after@"
    d[hi - 3:hi] = b"END"
    d = bytes(d)
    stream = gather(ctx, [d], 8 << 20)
    h = Opened(ctx, stream)
    try:
        N = h.rd.index_records(NL)[0]
        r = d.count(NL, 0, border)                                                                   # the straddling record's number
        no = torch.full((16,), SENT, dtype=torch.int64, device="cuda")
        for expr, want in ((b"@before@.*@after@", [r]), (b"@before@", [r]), (b"@after@.*END$", [r]), (b"^.*@after@", [r]), (b"@after@.*@before@", [])):
            with api.Regex(expr) as rx:
                R, totals, stats = h.rd.grep_regex(rx, no.data_ptr(), None, 8)
            torch.cuda.synchronize()
            assert R == len(want) and no.cpu().numpy()[:R].tolist() == want and stats[:2] == (10, 10), expr
        with api.Regex(b"^$") as rx:                                                                 # the complement counts every record once
            recs = GM.records(d, NL)
            assert len(recs) == N and h.rd.grep_regex(rx, None, None, 0, invert=True)[0] == sum(1 for rec in recs if rec)
    finally:
        h.close()


def test_device_stream_and_set(ctx):
    """DeviceStream.grep_regex returns what grep returns; DeviceStreamSet.grep_streams_regex is the same followed by locate_records."""
    d = regex_case(BS, 6)
    t = dev_u8(gather(ctx, [d], BS, True))
    codec = shard.HipTensorCodec(ctx)
    with codec.open_stream(t) as ds:
        for exprs, kw in ((b"tag1[0-9]{2}", dict(before=2, after=1)), ([b"^$", b"laws"], {}), (b"TAG00", dict(ignore_case=True, invert=True, max_records=50)), (b"nomatch", {})):
            m = RM.result(d, NL, exprs, kw.get("ignore_case", False), kw.get("invert", False), kw.get("before", 0), kw.get("after", 0))
            want = RM.cut(m, kw.get("max_records", 1 << 20))
            R, numbers, kinds, data, starts = ds.grep_regex(exprs, **kw)                              # (the first call builds the index)
            wdata, wstarts = GM.lines(d, NL, want["numbers"])
            assert R == want["R"] and numbers.tolist() == want["numbers"] and kinds.tolist() == want["kinds"]
            assert numbers.dtype == torch.int64 and kinds.dtype == torch.uint8 and numbers.device == t.device
            assert data.cpu().numpy().tobytes() == wdata and starts.tolist() == wstarts
            assert ds.grep_regex(exprs, count_only=True, **kw) == (want["R"], len(want["S"]))
        with api.Regex(b"tag1[0-9]{2}") as rx:                                                       # a compiled expression stays the caller's
            assert ds.grep_regex(rx, count_only=True)[0] == ds.grep_regex(b"tag1[0-9]{2}", count_only=True)[0] and rx.test(b"tag123")
        with pytest.raises(mz.MinLZError, match="in expression 0 at offset 2$"):
            ds.grep_regex(b"a**")
    datas = [d[:70000], b"", d[70000:70050], b"\n\n", d[70050:150000]]                               # records run on from stream to stream
    buf, spans = BC.back_to_back([O.stream_encode(x, 1, 4 << 10) for x in datas], 64)
    with codec.open_streams(dev_u8(buf), spans) as st:
        whole = b"".join(datas)
        which, line, kind = st.grep_streams_regex(b'"user_3[0-9]{2}7"|^$', before=1)
        R, numbers, kinds, _, _ = st.grep_regex(b'"user_3[0-9]{2}7"|^$', before=1)
        want = RM.result(whole, NL, b'"user_3[0-9]{2}7"|^$', before=1)
        assert R == want["R"] > 5 and numbers.tolist() == want["numbers"] and kind.tolist() == kinds.tolist() == want["kinds"]
        base = SetM.bases(st.sizes)
        assert list(zip(which.tolist(), line.tolist())) == [SetM.locate_record(base, whole, 10, r) for r in want["numbers"]]
