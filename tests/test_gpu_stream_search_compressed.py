"""Searches over streams whose block search tables are compressed (chunk 0x46): every stream is made by the device Writer with 0x45 tables
and passed through tests/search_compressed_model.py's recompress_stream, so that its data chunks are those of the 0x45 twin.  Every call
must return on the compressed stream what it returns on the twin and what brute force gives, plan the same chunks (counters 10 and 11),
and report the tables that came from 0x46 chunks in counter 14.  A broken compressed table is a table that is not there."""
import numpy as np
import pytest
import torch

from minlz_amd import synth
from minlz_amd.api import search_config
from tests import search_compressed_model as CM
from tests import search_model as SMod
from tests.search_gpu import SENT, Opened, Searcher, dev_u8, gather
from tests.test_stream_search_compressed_host import every_disposition, with_tiny_in_front

pytestmark = pytest.mark.gpu

TABLES = {1: dict(search_match_len=6), 2: dict(search_match_len=6, search_prefix=b'":, '), 4: dict(search_match_len=6, search_long_prefix=b'"user":"', search_extras=2)}


def planted(bs, nblk, seed=5, kind="json_like"):
    """Text with a needle inside block 1, across the border of blocks 3 and 4 and at the very end; -> (data, needle)."""
    d = bytearray(getattr(synth, kind)(bs * nblk, seed).tobytes())
    nd = b'"user":"' + bytes(np.random.default_rng(seed).choice(np.frombuffer(b"bcdfghjkmpqvwxz0123456789", np.uint8), 12)) + b'", x'
    for o in (bs + 1000, 4 * bs - 9, len(d) - len(nd)):
        if 0 <= o and o + len(nd) <= len(d):
            d[o:o + len(nd)] = nd
    return bytes(d), nd


def patterns_of(d, nd, n=16):
    rng = np.random.default_rng(3)
    out = [nd, nd[:9], nd[4:], b"no such bytes here"]
    while len(out) < n:
        o = int(rng.integers(0, len(d) - 24))
        s = d[o:o + int(rng.integers(7, 24))]
        if b"\n" not in s:                                    # (the record calls take no pattern that holds the delimiter)
            out.append(s)
    return out


class Reader(Searcher):
    """The four calls with guarded results -> plain Python values and (counter 10, counter 11, counter 14)."""

    def counters(self):
        return self.ctx.search_plan() + (self.ctx.search_compressed_tables(),)

    def one(self, pattern, **kw):
        total, pos, stats = self(pattern, 4096, **kw)
        return (total, pos, stats), self.counters()

    def many(self, pats, cap=1 << 14):
        pos = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        which = torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((len(pats) + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), cap)
        torch.cuda.synchronize()
        k = min(total, cap)
        assert (pos.cpu().numpy()[k:] == SENT).all() and (counts.cpu().numpy()[len(pats):] == SENT).all()
        return (total, pos.cpu().numpy()[:k].tolist(), which.cpu().numpy()[:k].tolist(), counts.cpu().numpy()[:len(pats)].tolist(), stats), self.counters()

    def records(self, pattern, cap=1 << 16, rec_cap=256):
        dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        off = torch.full((rec_cap + 8,), SENT, dtype=torch.int64, device="cuda")
        start = torch.full((rec_cap + 9,), SENT, dtype=torch.int64, device="cuda")
        k, totals, stats = self.rd.search_records(pattern, b"\n", dst.data_ptr(), cap, off.data_ptr(), start.data_ptr(), None, rec_cap)
        torch.cuda.synchronize()
        assert (dst.cpu().numpy()[cap:] == 0x5A).all() and (off.cpu().numpy()[max(k, 0):] == SENT).all()
        st = start.cpu().numpy()[:k + 1].tolist()
        return (k, totals, stats, off.cpu().numpy()[:k].tolist(), dst.cpu().numpy()[:st[-1] if k else 0].tobytes()), self.counters()

    def grep(self, pats, rec_cap=4096, **kw):
        self.rd.index_records(b"\n")
        no = torch.full((rec_cap + 8,), SENT, dtype=torch.int64, device="cuda")
        r, totals, stats = self.rd.grep_records(pats, no.data_ptr(), None, rec_cap, **kw)
        torch.cuda.synchronize()
        k = min(r, rec_cap)
        assert (no.cpu().numpy()[k:] == SENT).all()
        return (r, totals, stats, no.cpu().numpy()[:k].tolist()), self.counters()


def n_tables(stream, t=0x46):
    return sum(1 for _, ty, _ in SMod.chunks_of(stream) if ty == t)


def first_is_compressed(stream):
    """Per data chunk with a table in front of it: is the first one a 0x46 chunk."""
    out, first = [], None
    for _, t, _ in SMod.chunks_of(stream):
        if t in (0x45, 0x46) and first is None:
            first = t
        elif t in (1, 2, 3):
            if first is not None:
                out.append(first == 0x46)
            first = None
    return out


def check_pair(ctx, twin, comp, d, pats, want14=None, lines=True):
    """Every call on the compressed stream against the twin and brute force; -> the counters of the patterns' searches."""
    a, b = Reader(ctx, twin), Reader(ctx, comp)
    want14 = sum(first_is_compressed(comp)) if want14 is None else want14
    try:
        seen = []
        for p in pats[:6]:
            (ra, ca), (rb, cb) = a.one(p), b.one(p)
            brute = SMod.brute(d, p)
            assert ra == rb and ra[0] == len(brute) and ra[1] == brute[:4096], p
            assert ca[:2] == cb[:2] and ca[2] == 0 and cb[2] == (want14 if cb[1] else 0), (p, ca, cb)
            seen.append(cb)
        (ra, ca), (rb, cb) = a.many(pats), b.many(pats)
        assert ra == rb and ra[3] == [len(SMod.brute(d, p)) for p in pats]
        assert ca[:2] == cb[:2] and ca[2] == 0 and cb[2] == (want14 if cb[1] else 0)
        if lines:
            (ra, ca), (rb, cb) = a.records(pats[0]), b.records(pats[0])
            assert ra == rb and ra[0] >= 1 and ca[:2] == cb[:2]
            (ra, ca), (rb, cb) = a.grep(pats[:8]), b.grep(pats[:8])
            assert ra == rb and ra[0] >= 1 and ca[:2] == cb[:2]
        return seen
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("h0_bs", [13, 9])
def test_basic_shape(ctx, T, h0_bs):
    """6 blocks of 64 KiB (a bitmap of 8 KiB when unreduced): one sub-block, and sixteen forced.  Without the feature counter 11 is 0 on
    the compressed stream."""
    bs = 64 << 10
    d, nd = planted(bs, 6)
    twin = gather(ctx, [d], bs, **TABLES[T])
    sizes = [n - 8 - len(CM.table_config(twin[p + 4:p + 4 + n])[0][3]) for p, t, n in SMod.chunks_of(twin) if t == 0x45]
    comp = CM.recompress_stream(twin, h0_bs=lambda i: min(h0_bs, (sizes[i] - 1).bit_length()) if h0_bs == 13 else max(5, (sizes[i] - 1).bit_length() - 4))
    assert n_tables(comp) == n_tables(twin, 0x45) >= 4 and n_tables(comp, 0x45) == 0
    got = check_pair(ctx, twin, comp, d, patterns_of(d, nd))
    assert got[0][1:] == (n_tables(comp), n_tables(comp)) and min(c[0] for c in got) < 6


def test_small_blocks(ctx):
    """8 blocks of 4 KiB: a bitmap of 512 bytes in 16 sub-blocks of 32."""
    bs = 4 << 10
    d, nd = planted(bs, 8, kind="text_like")
    twin = gather(ctx, [d], bs, search_match_len=6)
    comp = CM.recompress_stream(twin, h0_bs=5, kinds=["huff", "raw", "sparse", "huff"] * 4)
    raw = [twin[p + 12:p + 4 + n] for p, t, n in SMod.chunks_of(twin) if t == 0x45]
    assert raw and all(len(r) == 512 for r in raw)
    check_pair(ctx, twin, comp, d, patterns_of(d, nd))


@pytest.mark.parametrize("h0_bs", [None, 17, 13])
def test_large_blocks(ctx, h0_bs):
    """2 blocks of 1 MiB (a bitmap of 128 KiB): the reference's partition (4 x 32 KiB), one sub-block of 128 KiB (32 Ki symbols a lane),
    16 x 8 KiB."""
    bs = 1 << 20
    d, nd = planted(bs, 2, kind="text_like")
    d = bytearray(d)
    for k in range(2):                                       # enough distinct windows that the table is not folded
        d[k * bs + (300 << 10):k * bs + (556 << 10)] = synth.random_bytes(256 << 10, seed=20 + k).tobytes()
    d = bytes(d)
    twin = gather(ctx, [d], bs, search_match_len=6)
    sizes = [n - 8 for p, t, n in SMod.chunks_of(twin) if t == 0x45]
    assert sizes == [128 << 10] * 2
    assert CM.default_bs(128 << 10) == 15
    h0_bs = 15 if h0_bs is None else h0_bs
    comp = CM.recompress_stream(twin, h0_bs=h0_bs, kinds=["huff"] * ((128 << 10) >> h0_bs))
    check_pair(ctx, twin, comp, d, patterns_of(d, nd, 8), lines=False)


def with_table(stream, k, payload):
    """The stream with the table chunk in front of data chunk k replaced by a 0x46 chunk of `payload`."""
    out, seen = [], 0
    cks = SMod.chunks_of(stream)
    for i, (p, t, n) in enumerate(cks):
        nxt = next((tt for _, tt, _ in cks[i + 1:] if tt in (1, 2, 3)), None)
        if t in (0x45, 0x46) and nxt is not None and sum(1 for _, tt, _ in cks[:i] if tt in (1, 2, 3)) == k:
            out.append(SMod.frame(0x46, payload))
            seen += 1
        else:
            out.append(stream[p:p + 4 + n])
    assert seen == 1
    return b"".join(out)


def test_every_disposition_in_one_chunk(ctx):
    """Block 2's table replaced by a made-up bitmap that holds every disposition (two tables, direct and FSE weights, one shared; raw;
    RLE 0x00 and 0xff; sparse with a gap above 255 and its last bit; an empty sparse one): the search plans as with the same bitmap in a
    0x45 chunk."""
    bs = 64 << 10
    d, nd = planted(bs, 6)
    base = gather(ctx, [d], bs, search_match_len=6)
    payload, bm = every_disposition(8192, 0, (1, 6, 16, b""))
    assert CM.parse_compressed_table(payload, (1, 6, 16, b"")) == (0, bm)
    twin = with_table(base, 2, b"")   # placeholder, replaced below
    twin = b"".join(SMod.table_chunk((1, 6, b""), 16, bm, 0) if (t == 0x46 and n == 0) else twin[p:p + 4 + n] for p, t, n in SMod.chunks_of(twin))
    comp = with_table(base, 2, payload)
    a, b = Reader(ctx, twin), Reader(ctx, comp)
    try:
        for p in patterns_of(d, nd):
            (ra, ca), (rb, cb) = a.one(p), b.one(p)
            assert ra[:2] == rb[:2] and ca[:2] == cb[:2] and cb[2] == (1 if cb[1] else 0)   # (the made-up table may prune wrongly: both streams alike)
    finally:
        a.close()
        b.close()


def test_reduced_table(ctx):
    """A block of few distinct windows: its table is folded twice (R = 2), 2 KiB of bitmap."""
    bs = 64 << 10
    d, nd = planted(bs, 5)
    d = bytearray(d)
    unit = synth.text_like(3000, seed=9).tobytes()
    d[2 * bs:3 * bs] = (unit * 22)[:bs]
    d = bytes(d)
    twin = gather(ctx, [d], bs, search_match_len=6)
    assert 2 in [twin[p + 7] for p, t, n in SMod.chunks_of(twin) if t == 0x45]
    check_pair(ctx, twin, CM.recompress_stream(twin), d, patterns_of(d, nd) + [unit[100:130]])


def test_mixed_chunks(ctx):
    """0x45 and 0x46 blocks in one stream, and blocks with one of each in front of them, in both orders: the first fitting table is taken."""
    bs = 64 << 10
    d, nd = planted(bs, 8)
    twin = gather(ctx, [d], bs, search_match_len=6)
    order = [("46",), ("45",), ("45", "46"), ("46", "45")]
    comp = CM.recompress_stream(twin, choose=lambda i: order[i % 4])
    first = first_is_compressed(comp)
    assert first[:4] == [True, False, False, True] and n_tables(comp) > sum(first)
    check_pair(ctx, twin, comp, d, patterns_of(d, nd), want14=sum(first))


def test_corrupt_set(ctx):
    """Each edit of the corrupt set in place of block 2's table: the search stays exact, block 2 counts as having no table (the model's plan
    without it), counter 11 drops by one.  Malformed inputs with defined verdicts; nothing here is built to fault."""
    bs = 64 << 10
    d, nd = planted(bs, 6)
    twin = gather(ctx, [d], bs, search_match_len=6)
    comp = CM.recompress_stream(twin)
    cfg, B, tables = SMod.read_tables(twin)
    sizes = [n for n, _ in SMod.data_grid(twin)]
    assert tables[2] is not None and len(tables[2][0]) >= 1024
    holed = list(tables)
    holed[2] = None
    usable = sum(t is not None for t in tables)
    pats = [nd, d[5 * bs + 77:5 * bs + 99]]
    brute = [SMod.brute(d, p) for p in pats]
    plans = [SMod.plan(holed, sizes, p, cfg, B) for p in pats]
    assert all(2 in pl for pl in plans) and any(2 not in SMod.plan(tables, sizes, p, cfg, B) for p in pats)
    cases = CM.corrupt_set((cfg[0], cfg[1], B, cfg[2]), tables[2][1], tables[2][0])
    assert len(cases) == 19
    for name, payload in cases:
        sr = Reader(ctx, with_table(comp, 2, payload))
        try:
            for p, want, plan in zip(pats, brute, plans):
                (total, pos, stats), cnt = sr.one(p)
                assert total == len(want) and pos == want, name
                assert stats == (len(sizes), len(plan), usable - 1) and cnt == (len(plan), usable - 1, usable - 1), (name, stats, cnt)
        finally:
            sr.close()


def test_flags(ctx):
    """MLZ_SEARCH_IGNORE_CASE and MLZ_SEARCH_NO_TABLES on the compressed stream, against the twin."""
    bs = 64 << 10
    d, nd = planted(bs, 6, kind="text_like")
    twin = gather(ctx, [d], bs, search_match_len=6)
    comp = CM.recompress_stream(twin)
    a, b = Reader(ctx, twin), Reader(ctx, comp)
    try:
        for p in (nd, nd.upper(), nd[2:14].swapcase(), d[3 * bs + 5:3 * bs + 25].upper()):
            for kw in (dict(ignore_case=True), dict(no_tables=True), dict(ignore_case=True, no_tables=True), dict(ignore_crc=True)):
                (ra, ca), (rb, cb) = a.one(p, **kw), b.one(p, **kw)
                assert ra == rb and ca[:2] == cb[:2], (p, kw)
                if kw.get("no_tables"):
                    assert cb == (6, 0, 0)
                fold = (lambda x: x.lower()) if kw.get("ignore_case") else (lambda x: x)
                assert ra[0] == len(SMod.brute(fold(d), fold(p)))
    finally:
        a.close()
        b.close()


def test_sidecar(ctx):
    """A sidecar of two configurations that the model recompressed attaches and plans as its 0x45 twin; a broken table of one
    configuration leaves the other in use."""
    bs = 64 << 10
    d, nd = planted(bs, 6)
    main = gather(ctx, [d], bs)
    cfgs = [search_config(1, 6), search_config(2, 6, b'":, ')]
    h = Opened(ctx, main)
    try:
        cap = h.rd.sidecar_bound(cfgs)
        dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        got = h.rd.build_sidecar(cfgs, dst.data_ptr(), cap)
        side = dst.cpu().numpy()[:got].tobytes()
    finally:
        h.close()
    ntab = n_tables(side, 0x45)
    assert ntab == 12                                        # 6 chunks x 2 configurations, configuration 0's table of chunk k is table 2 k
    side46 = CM.recompress_stream(side)
    broken = CM.recompress_stream(side, crc=lambda i: 0x12345678 if i == 2 * 3 else None)
    only_first = b"zq" + nd[8:20]                            # no window behind a prefix byte: configuration 1 cannot serve it
    results = {}
    for name, s in (("45", side), ("46", side46), ("broken", broken)):
        sr = Reader(ctx, main)
        t = dev_u8(s)
        try:
            sr.rd.attach_sidecar(t.data_ptr(), len(s))
            results[name] = [sr.one(p) for p in (nd, nd[:10], only_first, b"absent from the data")]
        finally:
            sr.close()
    for (ra, ca), (rb, cb), (rc, cc), p in zip(results["45"], results["46"], results["broken"], (nd, nd[:10], only_first, b"absent")):
        assert ra == rb and ra[:2] == rc[:2] and ra[0] == len(SMod.brute(d, p if p != b"absent" else b"absent from the data"))
        assert ca[:2] == cb[:2] and ca[2] == 0 and cb[2] == cb[1]
    # the pattern both configurations serve keeps chunk 3's table (configuration 1's); the one only configuration 0 serves loses it
    assert results["broken"][0][1][1] == results["46"][0][1][1] == 6
    assert results["46"][2][1][1] == 6 and results["broken"][2][1][1] == 5


def test_open_search_close_open_again(ctx):
    bs = 64 << 10
    d, nd = planted(bs, 6)
    comp = CM.recompress_stream(gather(ctx, [d], bs, search_match_len=6))
    seen = []
    for _ in range(3):
        sr = Reader(ctx, comp)
        try:
            seen.append([sr.one(nd), sr.one(nd, ignore_crc=True), sr.one(nd)])
        finally:
            sr.close()
    assert seen[0] == seen[1] == seen[2] and seen[0][0][0][0] == len(SMod.brute(d, nd)) and seen[0][0][1][2] == n_tables(comp)


def test_tiny_tables_in_front(ctx):
    """0x46 chunks whose bitmaps would have 2 and 16 bytes in front of block 0, valid tables behind them: they are no candidates (they take no
    room in the arena, whose bitmaps stay 16-byte aligned), and the search is that of the twin."""
    bs = 64 << 10
    d, nd = planted(bs, 6)
    twin = gather(ctx, [d], bs, search_match_len=6)
    comp = with_tiny_in_front(CM.recompress_stream(twin, h0_bs=9), (1, 6, 16, b""))
    assert n_tables(comp) == n_tables(twin, 0x45) + 2
    check_pair(ctx, twin, comp, d, patterns_of(d, nd), want14=n_tables(twin, 0x45))
