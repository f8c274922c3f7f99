"""MLZ_SEARCH_IGNORE_CASE on the GPU: mlz_dev_reader_search, _search_many, _search_records and _grep_records with the flag, each against two
yardsticks — tests/fold_model.py over the decoded bytes, and the UNFLAGGED call on a second stream that holds fold(data), asked for
fold(pattern) — and the chunks decoded against the model's folded plan.  Streams are the device Writer's: 9 blocks of 4 KiB and of 64 KiB and
a short one, with tables of type 1, 2, 3, 4 (a prefix without letters and one with), without tables, and with a sidecar of two
configurations.  Every output array lies between sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
from minlz_amd import _lib, shard, synth
from minlz_amd.api import search_config
from tests import fold_model as FM
from tests import grep_model as GM
from tests import search_long_prefix_cases as LC
from tests import search_model as SMod
from tests import sidecar_model as SCM
from tests.search_gpu import SENT, Opened, Searcher, gather
from tests.test_gpu_stream_grep import GUARD, KIND_SENT, Grep
from tests.test_gpu_stream_records import Records
from tests.test_gpu_stream_search_many import ManySearcher

pytestmark = pytest.mark.gpu

MLZ_ERR_ARG = 8
IGNORE_CASE, NO_TABLES, INVERT = 32, 8, 16
NL = b"\n"
M = 6
NEEDLE = b'"k":4711,"a'          # at most one letter per window of 6, prefix bytes of every table type in front of windows
ABSENT = b'"q":9911,"z'          # the same shape, nowhere in the data
WORD = b"ErrorLog"               # every window holds six letters: the tables cannot serve it under folding
PLAIN = b"#4711-;99"             # no letters
JSON4 = b'":, '
CONFIGS = {
    "type 1": dict(search_match_len=M),
    "type 2": dict(search_match_len=M, search_prefix=JSON4),
    "type 3": dict(search_match_len=M, search_prefix=SMod.NON_ALNUM),
    "type 4": dict(search_match_len=M, search_long_prefix=b'":', search_extras=1),
    "type 4, letters": dict(search_match_len=M, search_long_prefix=LC.USER, search_extras=3),
    "no tables": {},
    "sidecar": {},
}
SIDE_CFGS = [search_config(1, M), search_config(2, M, JSON4)]
NBLK, TAIL = 9, 777


def case(bs):
    """JSON-like lines (mixed case as they come) with the needle in upper, lower and mixed case at offset 0, as the stream's last bytes,
    across a block border by 1 and by L - 1 bytes and inside a block; the word in three cases, one of them across a border; the boundary
    bytes @ [ ` { in all four pairings; 0xC1 / 0xE1 next to a and A; the pattern without letters inside a block and across a border."""
    d = bytearray(synth.json_like(bs * NBLK + TAIL, 5).tobytes())
    L = len(NEEDLE)

    def plant(at, what):
        d[at:at + len(what)] = what
    plant(0, NEEDLE.upper())
    plant(len(d) - L, b'"K":4711,"a')
    plant(3 * bs - 1, b'"k":4711,"A')
    plant(5 * bs - (L - 1), NEEDLE.upper())
    plant(6 * bs + 100, NEEDLE)
    plant(bs + 7, b"eRRoRLoG")
    plant(2 * bs + 50, b"ERRORLOG")
    plant(7 * bs - 3, b"errorlog")
    plant(4 * bs + 200, b"@[ `{ @{ `[ `@ {[ @[ `{")
    plant(4 * bs + 300, b"\xc1a \xc1A \xe1a \xe1A \xc1a")
    plant(8 * bs + 10, PLAIN)
    plant(4 * bs - 4, PLAIN)
    return bytes(d)


class Fold(Opened):
    """A stream of the device Writer on the device, its decoded bytes and an open handle; `f`: the same for fold(data).  The calls are
    those of the existing tests' guarded wrappers."""

    def __init__(self, ctx, name, data, bs, second=True):
        self.name, self.data, self.bs = name, bytes(data), bs
        self.stream = gather(ctx, [self.data], bs, True, **CONFIGS[name])
        super().__init__(ctx, self.stream)
        self.sizes = [n for n, _ in SMod.data_grid(self.stream)]
        self.nck = len(self.sizes)
        self.side = None
        if name == "sidecar":
            cap = self.rd.sidecar_bound(SIDE_CFGS)
            room = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.side = room[:self.rd.build_sidecar(SIDE_CFGS, room.data_ptr(), cap)].clone()
            self.rd.attach_sidecar(self.side.data_ptr(), self.side.numel())
            self.cfgs, self.Bs, self.tables = SCM.parse(self.side.cpu().numpy().tobytes(), self.stream)
        else:
            cfg, B, tables = SMod.read_tables(self.stream)
            self.cfgs, self.Bs, self.tables = ([cfg], [B], [tables]) if cfg is not None else ([], [], [])
        self.f = Fold(ctx, name, FM.fold(self.data), bs, second=False) if second else None

    def close(self):
        if self.f is not None:
            self.f.close()
        super().close()

    def plan(self, pats, use_tables=True):
        """-> (the chunks the model decodes for the folded patterns, the patterns not served)"""
        if not use_tables or not self.cfgs:
            return [k for k in range(self.nck) if self.sizes[k]], len(pats)
        return FM.plan_many(self.tables, self.sizes, pats, self.cfgs, self.Bs, sidecar=self.side is not None)

    search = Searcher.__call__
    many = ManySearcher.__call__
    records = Records.raw


def check_search(h, pat, what, cap=None, **kw):
    """One flagged search against the model, against the unflagged search for fold(pat) in fold(data), and its plan against the model's."""
    want = FM.search(h.data, pat)
    cap = len(want) + 3 if cap is None else cap
    total, pos, st = h.search(pat, cap, ignore_case=True, **kw)
    what = "%s bs=%d %s %r %r" % (h.name, h.bs, what, pat[:16], kw)
    print(what, "found", total, "stats", st)
    assert total == len(want) and pos == want[:cap], what
    assert h.f.search(FM.fold(pat), cap, **kw)[:2] == (total, pos), what + ": the unflagged call on the folded stream"
    plan, unserved = h.plan([pat], not kw.get("no_tables"))
    assert st[0] == h.nck and st[1] == len(plan) and (st[2] > 0) == (unserved == 0), (what, st, plan)
    assert FM.chunks_with_a_start(h.sizes, want) <= set(plan), what
    return st


def check_many(h, pats, what, cap=None, **kw):
    want, counts = FM.search_many(h.data, pats)
    cap = len(want) + 3 if cap is None else cap
    total, pairs, cnt, st = h.many(pats, cap, ignore_case=True, **kw)
    what = "%s bs=%d %s n=%d %r" % (h.name, h.bs, what, len(pats), kw)
    print(what, "pairs", total, "stats", st)
    assert total == len(want) and cnt == counts and pairs == want[:cap], what
    assert h.f.many([FM.fold(p) for p in pats], cap, **kw)[:3] == (total, pairs, cnt), what + ": the unflagged call on the folded stream"
    plan, unserved = h.plan(pats, not kw.get("no_tables"))
    assert st[0] == h.nck and st[1] == len(plan) and st[3] == unserved, (what, st, plan, unserved)
    return st


# ---- the failing-first test, through the C ABI ----

def test_flag_is_honoured(ctx):
    """b"error" in data that holds only b"ERROR": nothing without the flag, every place with it (mlz_dev_reader_search called as a C
    client calls it, with the flag's value)."""
    bs = 4 << 10
    d = (b"2026-01-01 00:00:12 ERROR disk 7 is full\n2026-01-01 00:00:13 info all is well\n" * 400)[:8 * bs + 99]
    assert b"error" not in d
    want = SMod.brute(d, b"ERROR")
    for tables in (dict(search_match_len=M), {}):
        h = Opened(ctx, gather(ctx, [d], bs, True, **tables))
        try:
            out = torch.full((len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
            stats = (C.c_uint64 * 4)()
            L = _lib.lib()
            assert L.mlz_dev_reader_search(h.rd.handle, None, 0, b"error", 5, out.data_ptr(), len(want), stats) == 0
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == SENT).all()
            assert L.mlz_dev_reader_search(h.rd.handle, None, IGNORE_CASE, b"error", 5, out.data_ptr(), len(want), stats) == len(want) > 100
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert o[:len(want)].tolist() == want and (o[len(want):] == SENT).all()
            assert Searcher.__call__(h, b"eRRoR", 4, ignore_case=True)[:2] == (len(want), want[:4])
            assert Searcher.__call__(h, b"eRRoR", 4)[0] == 0
        finally:
            h.close()


# ---- one pattern ----

@pytest.fixture(scope="module", params=[(n, bs) for n in CONFIGS for bs in (4 << 10, 64 << 10)], ids=lambda p: "%s-%dK" % (p[0], p[1] >> 10))
def both(ctx, request):
    name, bs = request.param
    h = Fold(ctx, name, case(bs), bs)
    assert h.nck == NBLK + 1 and h.f.nck == h.nck
    yield h
    h.close()


def test_search(both):
    h = both
    d, bs, L = h.data, h.bs, len(NEEDLE)
    occ = FM.search(d, NEEDLE)
    assert occ == [0, 3 * bs - 1, 5 * bs - (L - 1), 6 * bs + 100, len(d) - L] and SMod.brute(d, NEEDLE) == [6 * bs + 100]
    st = check_search(h, NEEDLE, "the needle")
    assert check_search(h, NEEDLE.upper(), "the needle in upper case") == st
    check_search(h, NEEDLE, "cap", cap=2)
    check_search(h, ABSENT, "absent")
    assert FM.search(d, WORD) == [bs + 7, 2 * bs + 50, 7 * bs - 3]
    st = check_search(h, WORD, "the word")
    assert st[1] == h.nck and st[2] == 0                             # not served: everything
    assert len(FM.search(d, b"e")) > len(SMod.brute(d, b"e")) > 50
    check_search(h, b"E", "one letter", cap=40)
    o = 2 * bs - 100
    assert check_search(h, d[o:o + 256].swapcase(), "256 bytes across a border")[1] >= 2
    for p in (b"@[", b"`{"):                                          # 0x40 / 0x60 and 0x5B / 0x7B are no pair
        assert len(FM.search(d, p)) == len(SMod.brute(d, p)) == 2
        check_search(h, p, "boundary bytes")
    assert FM.search(d, b"\xc1a") == [4 * bs + 300, 4 * bs + 303, 4 * bs + 312]
    check_search(h, b"\xc1a", "bytes above 0x7f")
    check_search(h, b"\xE1A", "bytes above 0x7f")
    # without letters: the flag changes nothing, on the same handle
    for p in (PLAIN, b'"2026-01-01'):
        st = check_search(h, p, "no letters", cap=30)
        assert h.search(p, 30, ignore_case=True) == h.search(p, 30), p
    assert FM.search(d, PLAIN) == [4 * bs - 4, 8 * bs + 10]
    # no tables and the flag: the same results, everything decoded
    for p in (NEEDLE, WORD, b"\xc1A"):
        st = check_search(h, p, "no tables", no_tables=True)
        assert st[1] == h.nck and st[2] == 0


def test_search_plan_is_a_selection(ctx):
    """The cap keeps the folded plan useful: for the absent few-letter needle the served table types decode fewer chunks than there are."""
    for name in ("type 1", "type 2", "type 3", "type 4", "sidecar"):
        h = Fold(ctx, name, case(64 << 10), 64 << 10)
        try:
            assert check_search(h, ABSENT, "a selection")[1] < h.nck, name
            assert check_search(h, NEEDLE.swapcase(), "a selection")[2] > 0, name
        finally:
            h.close()


# ---- many patterns ----

def many_patterns(d, n, seed):
    """n patterns: the needle and its upper case (equal under folding), the absent one, the word (not served), 8-byte slices of the data in
    swapped case and random bytes."""
    rng = np.random.default_rng(seed)
    pats = [NEEDLE, NEEDLE.upper(), ABSENT, WORD, b"\xc1a", b"@["]
    while len(pats) < n:
        o = int(rng.integers(0, len(d) - 8))
        pats.append(d[o:o + 8].swapcase() if len(pats) % 3 else bytes(rng.integers(0, 256, 8, dtype=np.uint8)))
    return pats[:n]


@pytest.mark.parametrize("name,bs", [("type 1", 4 << 10), ("type 1", 64 << 10), ("type 3", 4 << 10), ("type 4", 64 << 10), ("sidecar", 4 << 10), ("no tables", 4 << 10)])
def test_search_many(ctx, name, bs):
    h = Fold(ctx, name, case(bs), bs)
    try:
        d = h.data
        st = check_many(h, [NEEDLE], "one")
        if h.cfgs:
            assert st[3] == 0
        st = check_many(h, [NEEDLE, NEEDLE.upper(), ABSENT, b'"K":4711'], "served ones")
        if h.cfgs:
            assert st[2] > 0
        want, counts = FM.search_many(d, [NEEDLE, NEEDLE.upper()])
        assert counts == [5, 5] and want[:2] == [(0, 0), (0, 1)]        # equal under folding: each counts for itself
        st = check_many(h, many_patterns(d, 17, 1), "17")
        assert st[3] >= 1 and st[1] == h.nck                             # the word is not served
        check_many(h, many_patterns(d, 17, 1), "17, cap", cap=9)
        st = check_many(h, many_patterns(d, 4096, 2), "4096", cap=3000)
        assert st[3] >= 1
        check_many(h, many_patterns(d, 17, 3), "17, no tables", no_tables=True)
        pats = [PLAIN, b'"2026-01-01', b"#4711-", b"-01-"]                # without letters: as without the flag, on the same handle
        assert h.many(pats, 50, ignore_case=True) == h.many(pats, 50)
    finally:
        h.close()


# ---- the border between decode groups ----

def test_group_border(ctx):
    """1 MiB blocks, a little over 64 MiB decoded, every chunk in the set: one border between decode groups, at 64 MiB.  A run of 512
    bytes xXxX.. lies around it, so needles of 2, 40 and 256 letters x in either case end exactly at the border, straddle it at every
    split and start exactly at it.  The needle lies at both ends of the data and across the border of two blocks inside a group."""
    bs, border = 1 << 20, 64 << 20
    base = synth.json_like(8 << 20, 9).tobytes()
    d = bytearray((base * 9)[:border + (2 << 20) + 321])
    assert b"xx" not in FM.fold(base)
    d[border - 256:border + 256] = b"xX" * 256
    L = len(NEEDLE)
    for o, nd in zip((0, 5 * bs - 5, len(d) - L), (NEEDLE.upper(), b'"K":4711,"a', b'"k":4711,"A')):
        d[o:o + L] = nd
    d = bytes(d)
    needles = [b"xx", b"X" * 40, b"Xx" * 128, NEEDLE]
    h = Fold(ctx, "type 1", d, bs)
    try:
        assert h.nck == 67
        pairs, counts = FM.search_many(d, needles)
        assert counts == [511, 473, 257, 3] and [len(SMod.brute(d, p)) for p in needles] == [0, 0, 128, 0]
        for i in range(3):
            n = len(needles[i])
            assert {(border - n, i), (border - n // 2, i), (border - 1, i), (border, i)} <= set(pairs)
        for p in needles:
            assert check_search(h, p, "group border", no_tables=True)[1] == 67
        check_search(h, NEEDLE.swapcase(), "group border, tables")
        check_many(h, needles, "group border", no_tables=True)
        check_many(h, needles + [b"\n{"], "group border, frequent", cap=1000, no_tables=True)
    finally:
        h.close()


# ---- records ----

def check_records(h, pat, what, W=0, rec_cap=4096, dst_cap=1 << 20, **kw):
    want = FM.records_result(h.data, pat, NL, W, rec_cap, dst_cap)
    got = h.records(pat, NL, W, rec_cap, dst_cap, ignore_case=True, **kw)
    R, totals, stats, dst, off, st, fl = got
    what = "%s bs=%d %s %r" % (h.name, h.bs, what, pat[:16])
    k, nb, ns = want["k"], len(want["dst"]), len(want["rec_start"])
    assert R == want["R"] and totals == want["totals"], (what, R, totals, want["totals"])
    assert off[:k].tolist() == want["rec_off"] and (off[k:] == SENT).all(), what
    assert st[:ns].tolist() == want["rec_start"] and (st[ns:] == SENT).all(), what
    assert fl[:k].tolist() == want["flags"] and (fl[k:] == 0x5A).all(), what
    assert dst[:nb].tobytes() == want["dst"] and (dst[nb:] == 0x5A).all(), what                 # the ORIGINAL bytes of the lines
    fR, ftotals, _, fdst, foff, fst, ffl = h.f.records(FM.fold(pat), NL, W, rec_cap, dst_cap, **kw)
    assert (fR, ftotals) == (R, totals) and (foff == off).all() and (fst == st).all() and (ffl == fl).all(), what + ": the unflagged call on the folded stream"
    assert fdst[:nb].tobytes() == FM.fold(want["dst"]), what
    plan, unserved = h.plan([pat], not kw.get("no_tables"))
    assert stats[1] == len(plan), what
    return want


@pytest.mark.parametrize("name,bs", [("type 1", 4 << 10), ("type 3", 64 << 10), ("no tables", 64 << 10)])
def test_search_records(ctx, name, bs):
    h = Fold(ctx, name, case(bs), bs)
    try:
        want = check_records(h, NEEDLE, "the needle")
        assert want["R"] == 5 and want["dst"] != FM.fold(want["dst"]) and NEEDLE.upper() in want["dst"]
        check_records(h, WORD.lower(), "the word")
        check_records(h, NEEDLE.upper(), "caps", rec_cap=3, dst_cap=400)
        check_records(h, b'"TS":"2026-01-01t00:0', "many lines", rec_cap=50, dst_cap=1 << 16, W=300)
        want = check_records(h, NEEDLE, "both caps 0", rec_cap=0, dst_cap=0)
        assert want["k"] == 0 and want["R"] == 5
        check_records(h, NEEDLE, "no tables", no_tables=True)
        # a delimiter that is a letter: refused with the flag, before anything is written; accepted without it
        lib = _lib.lib()
        dst = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
        off = torch.full((17,), SENT, dtype=torch.int64, device="cuda")
        st = torch.full((17,), SENT, dtype=torch.int64, device="cuda")
        fl = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda")
        totals = (C.c_uint64 * 4)(*([77] * 4))

        def call(flags, delim):
            return lib.mlz_dev_reader_search_records(h.rd.handle, None, flags, b"4711", 4, delim, 0, dst.data_ptr(), 4096, off.data_ptr(), st.data_ptr(), fl.data_ptr(), 16, totals, None)
        assert [call(IGNORE_CASE, ord(c)) for c in "azAZm"] == [-MLZ_ERR_ARG] * 5 and call(IGNORE_CASE | NO_TABLES, ord("q")) == -MLZ_ERR_ARG
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 0x5A).all() and (off.cpu().numpy() == SENT).all() and (st.cpu().numpy() == SENT).all() and (fl.cpu().numpy() == 0x5A).all()
        assert list(totals) == [77] * 4
        assert call(0, ord("q")) >= 0 and call(IGNORE_CASE, ord("@")) >= 0 and call(IGNORE_CASE, ord("{")) >= 0
    finally:
        h.close()


# ---- grep ----

class FoldGrep(Grep):
    def model(self, pats, invert, before, after, cap):
        key = (tuple(pats), invert, before, after)
        if key not in self.models:
            self.models[key] = FM.grep_result(self.data, self.delim, pats, invert, before, after)
        m = self.models[key]
        k = min(m["R"], cap)
        recs = GM.records(self.data, self.delim)
        return dict(m, numbers=m["C"][:k], kinds=m["kinds"][:k], totals=(m["R"], len(m["S"]), sum(len(recs[r]) for r in m["C"][:k]), m["totals"][3]))


@pytest.mark.parametrize("name,bs", [("type 1", 4 << 10), ("type 2", 64 << 10), ("no tables", 4 << 10)])
def test_grep_records(ctx, name, bs):
    d = case(bs)
    stream, fstream = gather(ctx, [d], bs, True, **CONFIGS[name]), gather(ctx, [FM.fold(d)], bs, True, **CONFIGS[name])
    g, f = FoldGrep(ctx, stream, d), Grep(ctx, fstream, FM.fold(d))
    try:
        sets = [[NEEDLE], [NEEDLE.upper(), WORD, b"\xc1a"], [b"tOm!", ABSENT, NEEDLE]]
        for pats in sets:
            for kw in (dict(), dict(invert=True), dict(before=2, after=2), dict(invert=True, before=2, after=2, cap=7), dict(cap=0, null=True), dict(flags=NO_TABLES)):
                kw = dict(kw)
                flags = kw.pop("flags", 0)
                want, stats = g.check(pats, name, flags=flags | IGNORE_CASE, **kw)
                fwant, _ = f.check([FM.fold(p) for p in pats], name + ", folded stream", flags=flags, **kw)
                assert (want["R"], want["numbers"], want["kinds"], want["totals"]) == (fwant["R"], fwant["numbers"], fwant["kinds"], fwant["totals"])
        want, _ = g.check([NEEDLE], name, flags=IGNORE_CASE)
        assert len(want["M"]) == 5 and len(GM.matching(GM.records(d, NL), [NEEDLE])) == 1
        # read_records over the result: the original lines
        r, no, kd, totals, _ = g.raw([NEEDLE], 16, IGNORE_CASE, 1, 1)
        k = min(r, 16)
        idx = torch.from_numpy(no[:k].copy()).cuda()
        out = torch.full((totals[2] + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert g.rd.read_records(idx.data_ptr(), k, out.data_ptr(), totals[2]) == totals[2]
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert o[:totals[2]].tobytes() == FM.grep_lines(d, NL, no[:k].tolist())[0] and (o[totals[2]:] == 0x5A).all()
    finally:
        g.close()
        f.close()
    # an index built on a letter: refused with the flag, nothing written; accepted without it
    g = Grep(ctx, stream, d, delim=b"e")
    try:
        r, no, kd, totals, stats = g.raw([b"4711"], 8, IGNORE_CASE)
        assert r == -MLZ_ERR_ARG and (no == SENT).all() and (kd == KIND_SENT).all() and totals == (77,) * 4 and stats == (77,) * 4
        assert g.raw([b"4711"], 8, IGNORE_CASE | INVERT)[0] == -MLZ_ERR_ARG
        assert g.raw([b"4711"], 8, 0)[0] >= 0
    finally:
        g.close()


# ---- the Python layers ----

def test_device_stream(ctx):
    bs = 64 << 10
    d = case(bs)
    t = torch.from_numpy(np.frombuffer(gather(ctx, [d], bs, True, search_match_len=M), np.uint8).copy()).cuda()
    with shard.HipTensorCodec(ctx).open_stream(t) as ds:
        want = FM.search(d, NEEDLE)
        pos, total = ds.search(NEEDLE, 3, ignore_case=True)
        assert total == len(want) == 5 and pos.tolist() == want[:3] and ds.search(NEEDLE, 3)[1] == 1
        pats = [NEEDLE.upper(), WORD, NEEDLE]
        pairs, counts = FM.search_many(d, pats)
        pos, which, cnt, total = ds.search_many(pats, 6, ignore_case=True)
        assert total == len(pairs) and list(zip(pos.tolist(), which.tolist())) == pairs[:6] and cnt.tolist() == counts
        assert ds.search_many(pats, 6)[3] == sum(len(SMod.brute(d, p)) for p in pats) == 3
        rw = FM.records_result(d, NEEDLE, NL, 0, 3, 1 << 20)
        total, data, rec_off, rec_start, flags, totals = ds.search_records(NEEDLE, max_records=3, ignore_case=True)
        assert total == rw["R"] == 5 and totals == rw["totals"] and data.cpu().numpy().tobytes() == rw["dst"]
        assert rec_off.tolist() == rw["rec_off"] and rec_start.tolist() == rw["rec_start"] and flags.tolist() == rw["flags"]
        with pytest.raises(mz.MinLZError):
            ds.search_records(NEEDLE, delimiter=b"Q", ignore_case=True)
        gw = FM.grep_result(d, NL, [NEEDLE, WORD], False, 1, 0, 1 << 20)
        R, numbers, kinds, data, starts = ds.grep([NEEDLE, WORD], before=1, ignore_case=True)
        wdata, wstarts = FM.grep_lines(d, NL, gw["numbers"])
        assert R == gw["R"] and numbers.tolist() == gw["numbers"] and kinds.tolist() == gw["kinds"]
        assert data.cpu().numpy().tobytes() == wdata and starts.tolist() == wstarts
        assert ds.grep([NEEDLE, WORD], before=1, ignore_case=True, count_only=True) == (gw["R"], len(gw["S"]))
        assert ds.grep([NEEDLE, WORD], count_only=True)[1] < len(gw["S"])
