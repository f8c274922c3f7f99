"""mlz_dev_reader_grep_records (DeviceReader.grep_records, DeviceStream.grep) on the GPU against tests/grep_model.py over the decoded bytes:
many patterns, inverted match, context records, record numbers and kinds, the four totals and the cut at rec_cap.  Both output arrays are
guarded by sentinels and compared whole.  On every stream and pattern set M must also be unique(record_numbers(search_many's positions)),
computed with the calls that existed before this one.  (N >= 2^32 is refused by the call; no test builds four billion records.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from minlz_amd.api import search_config
from tests import corrupt as CM
from tests import grep_model as GM
from tests import search_model as SMod
from tests.search_gpu import SENT, Opened, dev_u64, gather

pytestmark = pytest.mark.gpu

MLZ_ERR_CRC, MLZ_ERR_ARG = 5, 8
IGNORE_CRC, NO_TABLES, INVERT = 2, 8, 16
NL = b"\n"
GUARD = 8
KIND_SENT = 0x5A
RARE = b"@zq-needle-77@"
HOT = b"hot!"
SHORT = b'":'          # shorter than M = 6: the tables cannot serve it
CONTEXTS = [(0, 0), (1, 0), (0, 1), (3, 3), (None, None)]      # (before, after); None: N


def grep_case(bs, nblk):
    """JSON-like lines with a stored (random) block and delimiters planted at block borders (bs - 1, bs), doubled ones, at the stream's
    first and last byte: the shape of the record index's test streams.  Into it go a rare needle across a scan tile's border (3 * 16 KiB),
    across a block border (5 * bs) and near the end, and a pattern with thousands of occurrences in two long records."""
    d = bytearray(synth.json_like(bs * nblk + 700, 11).tobytes())
    d[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
    for k in (1, 2, 3, 5):
        d[k * bs - 1:k * bs + 1] = b"\n\n"
    d[4 * bs - 1:4 * bs] = NL
    d[6 * bs:6 * bs + 1] = NL
    d[3 * bs + 50:3 * bs + 54] = b"\n\n\n\n"
    d[0:1] = NL
    d[-1:] = NL
    for at in (3 * 16384 - 5, 5 * bs - 7, len(d) - 200):
        d[at:at + len(RARE)] = RARE
    half = len(d) // 2
    d[half + 3000:half + 9000] = HOT * 1500
    d[half + 20000:half + 24000] = HOT * 1000
    return bytes(d)


def lds_fits(pats):
    """search_many_lds' model: does the pattern index of these patterns fit the scan kernel's 64 KiB of LDS with offsets and bytes?"""
    n, blob = len(pats), sum(len(p) for p in pats)
    hb = max(8, min(12, (n - 1).bit_length()))
    tile = 16384 + 256 + 8
    tile_lds = (tile + ((tile >> 6) << 2) + 8) & ~3
    words = ((1 << hb) + 2) // 2 + (n + 1) // 2 + n + 256 + tile_lds // 4 + n + 1 + (blob + 3) // 4
    return words * 4 <= 64 << 10


class Grep(Opened):
    """A stream on the device, its decoded bytes and an open handle with an index; check() compares a call whole with the model."""

    def __init__(self, ctx, stream, data, delim=NL, index=True, **kw):
        super().__init__(ctx, stream)
        self.data, self.stream, self.delim = bytes(data), bytes(stream), delim
        self.side = None
        self.models = {}
        if index:
            self.N = self.rd.index_records(delim, **kw)[0]
            assert self.N == len(GM.records(self.data, delim))

    def attach(self, cfgs):
        cap = self.rd.sidecar_bound(cfgs)
        room = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.side = room[:self.rd.build_sidecar(cfgs, room.data_ptr(), cap)].clone()
        self.rd.attach_sidecar(self.side.data_ptr(), self.side.numel())

    def raw(self, pats, cap, flags=0, before=0, after=0, null=False, kinds=True):
        """-> (the call's value, numbers, kinds, totals, stats): the guarded arrays whole."""
        pats = [bytes(p) for p in pats]
        lens = np.asarray([len(p) for p in pats], dtype=np.uint32)
        no = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
        kd = torch.full((cap + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
        totals, stats = (C.c_uint64 * 4)(*([77] * 4)), (C.c_uint64 * 4)(*([77] * 4))
        r = _lib.lib().mlz_dev_reader_grep_records(self.rd.handle, None, flags, b"".join(pats) if pats else None, lens.ctypes.data if pats else None, len(pats), before, after,
                                                   None if null else no.data_ptr(), kd.data_ptr() if kinds and not null else None, cap, totals, stats)
        torch.cuda.synchronize()
        return r, no.cpu().numpy(), kd.cpu().numpy(), tuple(int(v) for v in totals), tuple(int(v) for v in stats)

    def model(self, pats, invert, before, after, cap):
        key = (tuple(pats), invert, before, after)
        if key not in self.models:
            self.models[key] = GM.result(self.data, self.delim, pats, invert, before, after)
        m = self.models[key]
        k = min(m["R"], cap)
        recs = GM.records(self.data, self.delim)
        return dict(m, numbers=m["C"][:k], kinds=m["kinds"][:k], totals=(m["R"], len(m["S"]), sum(len(recs[r]) for r in m["C"][:k]), m["totals"][3]))

    def check(self, pats, what, cap=None, invert=False, before=0, after=0, flags=0, **kw):
        want = self.model(pats, invert, before, after, self.N + 3 if cap is None else cap)
        cap = want["R"] + 3 if cap is None else cap
        r, no, kd, totals, stats = self.raw(pats, cap, flags | (INVERT if invert else 0), before, after, **kw)
        k = min(want["R"], cap)
        what = "%s: invert %s, before %d, after %d, cap %d" % (what, invert, before, after, cap)
        assert r == want["R"] and totals == want["totals"], (what, r, totals, want["totals"])
        if kw.get("null"):
            assert (no == SENT).all() and (kd == KIND_SENT).all(), what
        else:
            assert no[:k].tolist() == want["numbers"], what
            assert (no[k:] == SENT).all(), what + ": written beyond the numbers"
            if kw.get("kinds", True):
                assert kd[:k].tolist() == want["kinds"] and (kd[k:] == KIND_SENT).all(), what
            else:
                assert (kd == KIND_SENT).all(), what
        assert self.ctx.search_plan() == stats[1:3], what                 # counters 10 / 11 describe the search phase as stats do
        return want, stats

    def by_existing_calls(self, pats, **kw):
        """unique(record_numbers(search_many's positions)): the composition the call replaces."""
        if not pats:
            return []
        total, _ = self.rd.search_many(pats, None, None, None, 0, **kw)
        if total == 0:
            return []
        pos = torch.empty(total, dtype=torch.int64, device="cuda")
        which = torch.empty(total, dtype=torch.int32, device="cuda")
        assert self.rd.search_many(pats, None, pos.data_ptr(), which.data_ptr(), total, **kw)[0] == total
        no = torch.empty(total, dtype=torch.int64, device="cuda")
        assert self.rd.record_numbers(pos.data_ptr(), total, no.data_ptr()) == total
        torch.cuda.synchronize()
        return torch.unique(no).cpu().tolist()

    def check_equivalence(self, pats, what, **kw):
        flags = (IGNORE_CRC if kw.get("ignore_crc") else 0) | (NO_TABLES if kw.get("no_tables") else 0)
        r, no, kd, totals, _ = self.raw(pats, self.N, flags)
        assert r >= 0, what
        assert no[:r].tolist() == self.by_existing_calls(pats, **kw), what
        assert (no[r:] == SENT).all() and (kd[:r] == 1).all() and totals[:2] == (r, r), what
        return no[:r].tolist()


def pattern_sets(d):
    """name -> patterns: one; two that hit the same records; duplicates; the hot one; one the tables cannot serve; 300 whose index does
    not fit the LDS budget."""
    rng = np.random.default_rng(300)
    recs = [r for r in GM.records(d, NL) if 40 <= len(r) <= 4000 and HOT not in r]
    present = []
    for i in range(100):
        rec = recs[int(rng.integers(0, len(recs)))]
        o, n = int(rng.integers(0, len(rec) - 30)), int(rng.integers(6, 30))
        present.append(rec[o:o + n])
    absent = [bytes(np.where((a := rng.integers(0, 256, 220, dtype=np.uint8)) == 10, 11, a).astype(np.uint8)) for _ in range(198)]
    many = present + absent + [RARE, RARE[1:9]]
    assert len(many) == 300 and not lds_fits(many) and lds_fits([RARE, HOT]) and not any(NL in p for p in many) and min(len(p) for p in many) >= 6
    return {"one": [RARE], "two on the same records": [RARE, RARE[2:10]], "duplicates": [RARE, RARE, HOT], "hot": [HOT], "short": [SHORT], "rare and short": [RARE, SHORT],
            "300": many}


@pytest.fixture(scope="module", params=["type 1", "no tables", "sidecar", "4K blocks"])
def main(ctx, request):
    name = request.param
    bs, nblk = (4 << 10, 40) if name == "4K blocks" else (64 << 10, 6)
    d = grep_case(bs, nblk)
    stream = gather(ctx, [d], bs, True, **({} if name in ("no tables", "sidecar") else dict(search_match_len=6)))
    grid = SMod.data_grid(stream)
    assert grid[1][1] == 0x01 and len(grid) == nblk + 1                      # the random block: stored
    h = Grep(ctx, stream, d)
    if name == "sidecar":
        h.attach([search_config(1, 6)])
    recs = GM.records(d, NL)
    m = GM.matching(recs, [RARE])
    assert len(m) == 3 and len(GM.matching(recs, [HOT])) == 2 and d.count(HOT) == 2500 and sum(1 for r in recs if not r) >= 6
    yield h, name, pattern_sets(d)
    h.close()


def test_pattern_sets_against_the_model_and_the_existing_calls(main):
    h, name, sets = main
    for what, pats in sets.items():
        want, stats = h.check(pats, "%s, %s" % (name, what))
        assert h.check_equivalence(pats, "%s, %s" % (name, what)) == want["M"]
        h.check(pats, "%s, %s, no tables" % (name, what), flags=NO_TABLES)         # the same arrays as the run with tables
        served = name != "no tables" and all(len(p) >= 6 for p in pats)                # M = 6: a shorter pattern decodes every chunk
        assert (stats[3] == 0 and stats[2] > 0) == served, (name, what, stats)
        if what == "short":
            assert stats[1] == stats[0] and stats[3] == 1
    _, with_tables = h.check(sets["one"], name)
    _, without = h.check(sets["one"], name, flags=NO_TABLES)
    assert without[1] == without[0] and without[2] == 0
    assert (with_tables[1] < without[1]) == (name != "no tables"), (name, with_tables, without)   # the rare needle: the tables prune


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "invert"])
def test_context_and_invert(main, invert):
    h, name, sets = main
    for what in ("one", "hot", "rare and short"):
        for before, after in CONTEXTS:
            b, a = (h.N if before is None else before), (h.N if after is None else after)
            want, _ = h.check(sets[what], "%s, %s" % (name, what), invert=invert, before=b, after=a)
            if (before, after) == (None, None):
                assert want["R"] == (h.N if want["S"] else 0)
    want, _ = h.check(sets["one"], name, invert=invert, before=1 << 40, after=(1 << 64) - 1)      # values >= N behave like N
    assert want["R"] == h.N
    want, _ = h.check(sets["one"], name, invert=invert, before=3, after=3, kinds=False)           # d_rec_kind may be NULL
    assert 0 < want["R"] < h.N or invert
    if invert:
        empty = [r for r, rec in enumerate(GM.records(h.data, NL)) if not rec]
        want, _ = h.check(sets["short"], name, invert=True)
        assert set(empty) <= set(want["numbers"])                                                   # empty records never match


def test_no_patterns(main):
    h, name, _ = main
    want, stats = h.check([], name + ", no patterns")
    assert want["R"] == 0 and stats == (len(SMod.data_grid(h.stream)), 0, 0, 0)                    # no chunk is decoded
    want, stats = h.check([], name + ", no patterns", invert=True, before=2, after=2)
    assert want["R"] == h.N and want["totals"][1] == h.N and stats[1] == 0
    h.check([], name + ", no patterns", invert=True, cap=10)


def test_rec_cap(main):
    h, name, sets = main
    for pats, kw in ((sets["one"], dict(before=3, after=3)), (sets["rare and short"], dict(invert=True, after=1))):
        R = h.model(pats, kw.get("invert", False), kw.get("before", 0), kw.get("after", 0), 0)["R"]
        assert R > 4
        want, _ = h.check(pats, name, cap=0, null=True, **kw)                                       # grep -c: NULL arrays
        assert want["totals"][2] == 0 and want["totals"][3] > 0
        for cap in (1, R - 1, R, R + 5):
            want, _ = h.check(pats, name, cap=cap, **kw)
            assert (want["totals"][2] == want["totals"][3]) == (cap >= R)


def test_written_bytes_are_what_read_records_needs(main):
    h, name, sets = main
    cap = 5
    r, no, kd, totals, _ = h.raw(sets["one"], cap, before=2, after=2)
    assert r > cap
    want, starts = GM.lines(h.data, NL, no[:cap].tolist())
    assert totals[2] == len(want)
    d_no = dev_u64(no[:cap])
    dst = torch.full((totals[2] + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert h.rd.read_records(d_no.data_ptr(), cap, dst.data_ptr(), totals[2]) == totals[2]
    torch.cuda.synchronize()
    assert dst.cpu().numpy()[:totals[2]].tobytes() == want and (dst.cpu().numpy()[totals[2]:] == 0x5A).all()
    with pytest.raises(mz.MinLZError):
        h.rd.read_records(d_no.data_ptr(), cap, dst.data_ptr(), totals[2] - 1)


def test_every_record_empty(ctx):
    d = NL * 70000
    h = Grep(ctx, gather(ctx, [d], 64 << 10, True), d)
    try:
        assert h.N == 70000
        want, _ = h.check([b"x"], "70 000 empty records")
        assert want["R"] == 0
        want, _ = h.check([b"x"], "70 000 empty records", invert=True)
        assert want["totals"] == (70000, 70000, 0, 0)
        h.check([b"x"], "70 000 empty records", invert=True, cap=69999, before=5)
        assert h.check_equivalence([b"x"], "70 000 empty records") == []
    finally:
        h.close()


def test_one_record_and_the_empty_stream(ctx):
    d = b"one record with a needle and no delimiter"
    h = Grep(ctx, gather(ctx, [d], 64 << 10, True), d)
    try:
        assert h.N == 1
        for pats, inv, R in (([b"needle"], False, 1), ([b"needle"], True, 0), ([b"absent"], False, 0), ([b"absent"], True, 1), ([], True, 1)):
            want, _ = h.check(pats, "one record", invert=inv, before=7, after=7)
            assert want["R"] == R
        assert h.check_equivalence([b"needle", b"e"], "one record") == [0]
    finally:
        h.close()
    for empty in (b"", O.stream_encode(b"", 1, 1 << 20)):
        h = Grep(ctx, empty, b"")
        try:
            assert h.N == 0
            for flags in (0, INVERT):
                r, no, kd, totals, stats = h.raw([b"x"], 4, flags, 3, 3)
                assert r == 0 and totals == (0, 0, 0, 0) and (no == SENT).all() and (kd == KIND_SENT).all() and stats[1:] == (0, 0, 0)
        finally:
            h.close()


def test_argument_errors_write_nothing(ctx):
    bs = 64 << 10
    d = grep_case(bs, 6)
    L = _lib.lib()
    h = Grep(ctx, gather(ctx, [d], bs, True, search_match_len=6), d, index=False)
    try:
        r, no, kd, totals, stats = h.raw([RARE], 8)                                                 # a handle without an index
        assert r == -MLZ_ERR_ARG and (no == SENT).all() and (kd == KIND_SENT).all()
        h.N = h.rd.index_records(NL)[0]
        no = torch.full((8 + GUARD,), SENT, dtype=torch.int64, device="cuda")
        kd = torch.full((8 + GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
        host = np.zeros(16, np.uint64)
        blob = RARE + b"x" * 300

        def call(n, lens, patterns=blob, p=no.data_ptr(), k=kd.data_ptr(), cap=8, handle=h.rd.handle):
            a = None if lens is None else np.asarray(lens, np.uint32)
            return L.mlz_dev_reader_grep_records(handle, None, 0, patterns, None if a is None else a.ctypes.data, n, 1, 1, p, k, cap, None, None)

        big = np.full(4097, 1, np.uint32)
        bad = [L.mlz_dev_reader_grep_records(h.rd.handle, None, 0, b"x" * 4097, big.ctypes.data, 4097, 0, 0, no.data_ptr(), kd.data_ptr(), 8, None, None),
               call(2, [14, 0]), call(2, [14, 257]), call(1, [14], patterns=None), call(1, None),        # search_many's argument errors
               call(1, [5], patterns=b"ab\ncd"), call(2, [14, 3], patterns=RARE + b"a\n" + b"z"),       # a pattern that holds the delimiter
               call(1, [14], p=None), call(1, [14], p=host.ctypes.data), call(1, [14], k=host.ctypes.data),
               call(1, [14], handle=None)]
        torch.cuda.synchronize()
        assert bad == [-MLZ_ERR_ARG] * len(bad)
        assert (no == SENT).all() and (kd == KIND_SENT).all()
        R = GM.result(d, NL, [RARE], False, 1, 1)["R"]                                              # three records, a context of one around each
        assert 3 < R <= 9 and call(1, [14], p=None, k=None, cap=0) == R and call(1, [14], k=None) == R
        torch.cuda.synchronize()
        assert (no[R:] == SENT).all() and (kd == KIND_SENT).all()
        with pytest.raises(mz.MinLZError):
            h.rd.grep_records([b"a\nb"], None, None, 0)
    finally:
        h.close()


def test_another_delimiter_replaces_the_index(ctx):
    bs = 64 << 10
    d = grep_case(bs, 6)
    h = Grep(ctx, gather(ctx, [d], bs, True, search_match_len=6), d)
    try:
        h.check([RARE], "by lines", before=1, after=1)
        h.N = h.rd.index_records(b",")[0]
        h.delim, h.models = b",", {}
        assert h.N == len(GM.records(d, b","))
        want, _ = h.check([RARE, b'}\n{"'], "by commas", before=1, after=1)                         # a newline is a pattern byte like any other now
        assert want["R"] > 9
        h.check([RARE], "by commas", invert=True, cap=100)
        assert h.raw([b"a,b"], 4)[0] == -MLZ_ERR_ARG
    finally:
        h.close()


def test_broken_chunks(ctx):
    """A flipped CRC byte in a chunk that the plan decodes: -MLZ_ERR_CRC, the arrays untouched.  The same flip in a chunk that the tables
    prune goes unnoticed.  Under MLZ_STREAM_IGNORE_CRC the call follows search_many."""
    bs = 64 << 10
    d = grep_case(bs, 6)
    s = gather(ctx, [d], bs, True, search_match_len=6)
    cfg, B, tables = SMod.read_tables(s)
    sizes = [n for n, _ in SMod.data_grid(s)]
    plan = SMod.plan(tables, sizes, RARE, cfg, B)
    cs = [(c.off, c.clen) for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    comp = [j for j, (_, t) in enumerate(SMod.data_grid(s)) if t == 0x02]
    inside, outside = [j for j in comp if j in plan], [j for j in comp if j not in plan]
    assert inside and outside
    clean = Grep(ctx, s, d)
    try:
        want, stats = clean.check([RARE], "clean", before=1, after=1)
        assert stats[1] == len(plan)
    finally:
        clean.close()
    for j, refused in ((inside[0], True), (outside[0], False)):
        b = bytearray(s)
        b[cs[j][0] + 5] ^= 0x10
        h = Grep(ctx, bytes(b), d, ignore_crc=True)                                                 # (the index build decodes every chunk)
        try:
            r, no, kd, totals, _ = h.raw([RARE], 16, 0, 1, 1)
            if refused:
                assert r == -MLZ_ERR_CRC and (no == SENT).all() and (kd == KIND_SENT).all()
                with pytest.raises(mz.ErrCRC):
                    h.rd.grep_records([RARE], None, None, 0)
                with pytest.raises(mz.ErrCRC):
                    h.rd.search_many([RARE], None, None, None, 0)
            else:
                assert r == want["R"] and no[:r].tolist() == want["numbers"]
            h.check([RARE], "ignore crc", before=1, after=1, flags=IGNORE_CRC)
            assert h.check_equivalence([RARE, HOT], "ignore crc", ignore_crc=True) == sorted(set(want["M"]) | set(GM.matching(GM.records(d, NL), [HOT])))
        finally:
            h.close()


def test_device_stream_grep(ctx):
    bs = 64 << 10
    d = grep_case(bs, 6)
    t = torch.from_numpy(np.frombuffer(gather(ctx, [d], bs, True, search_match_len=6), np.uint8).copy()).cuda()
    with shard.HipTensorCodec(ctx).open_stream(t) as ds:
        for pats, kw in (([RARE], dict(before=2, after=1)), (RARE, {}), ([RARE, HOT], dict(invert=True, max_records=50)), ([HOT, SHORT], dict(after=1, max_records=7)), ([], {})):
            plist = [pats] if isinstance(pats, bytes) else pats
            want = GM.result(d, NL, plist, kw.get("invert", False), kw.get("before", 0), kw.get("after", 0), kw.get("max_records", 1 << 20))
            R, numbers, kinds, data, starts = ds.grep(pats, **kw)                                   # (the first call builds the index)
            wdata, wstarts = GM.lines(d, NL, want["numbers"])
            assert R == want["R"] and numbers.tolist() == want["numbers"] and kinds.tolist() == want["kinds"]
            assert numbers.dtype == torch.int64 and kinds.dtype == torch.uint8 and numbers.device == t.device
            assert data.cpu().numpy().tobytes() == wdata and starts.tolist() == wstarts
            assert ds.grep(pats, count_only=True, **kw) == (want["R"], len(want["S"]))
        assert ds.reader.record_count() == len(GM.records(d, NL))
