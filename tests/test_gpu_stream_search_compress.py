"""The write side of compressed block search tables (chunk 0x46) on the GPU.  The kernels of
minlz_amd/csrc/mlz_search_tables_compress.hip.inc behind mlz_search_bitmaps_compress_device must write, for every bitmap, the section the
host call writes (which tests/test_search_table_compress_host.py holds to the model byte for byte), into guarded room, with every item's
error its own.  The device Writer with MLZ_STREAM_SEARCH_COMPRESS must write its 0x45 twin with every table chunk replaced by the model's
0x46 chunk where that is strictly smaller, and the stream must search as the twin does."""
import numpy as np
import pytest
import torch

from minlz_amd import api
from tests import search_compress_cases as K
from tests.search_gpu import dev_u8, first_difference

pytestmark = pytest.mark.gpu

GUARD = 0x5A
GAP = 64


def run_batch(ctx, items):
    """items: [(bitmap bytes, src_len or None = its length, cap or None = the largest section, bytes of padding in front of the bitmap)]
    -> [(d_len, the item's room as the call left it)].  Every item's room is followed by a guard gap."""
    src, descs, rooms = bytearray(), [], []
    at = 0
    for bm, src_len, cap, pad in items:
        src += bytes(pad)
        n = len(bm) if src_len is None else src_len
        room = len(bm) + 18 if cap is None else cap
        descs.append((len(src), n, at, room))
        rooms.append((at, room))
        src += bm
        at += max(room, len(bm) + 18) + GAP + (at % 3)          # (sections start at every alignment)
    d_src = dev_u8(bytes(src))
    d_dst = torch.full((at + GAP,), GUARD, dtype=torch.uint8, device="cuda")
    d_len = torch.full((len(items) + 8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    ctx.search_bitmaps_compress_device(d_src.data_ptr(), d_dst.data_ptr(), descs, d_len.data_ptr())
    torch.cuda.synchronize()
    out, lens = d_dst.cpu().numpy(), d_len.cpu().numpy()
    assert (lens[len(items):] == 0x5A5A5A5A).all()
    got, covered = [], np.zeros(len(out), bool)
    for (off, room), ln in zip(rooms, lens[:len(items)].tolist()):
        if ln > 0:
            assert ln <= room
            covered[off:off + ln] = True
        got.append((ln, out[off:off + max(ln, 0)].tobytes()))
    assert (out[~covered] == GUARD).all(), "written outside the sections"
    return got


def test_batch_equals_host(ctx):
    """The designed set in one call, sizes mixed, some bitmaps at odd addresses."""
    cases = K.designed()
    items = [(bm, None, None, (i % 4) if i % 3 == 0 else 0) for i, (_, bm) in enumerate(cases)]
    assert len(items) >= 30 and len({len(bm) for bm, _, _, _ in items}) == len(K.SIZES)
    got = run_batch(ctx, items)
    for (name, bm), (ln, section) in zip(cases, got):
        want = api.compress_search_bitmap(bm)
        assert ln == len(want) and section == want, (name, ln, len(want), first_difference(section, want))


def test_real_tables(ctx):
    cases = K.real_tables()
    got = run_batch(ctx, [(bm, None, None, 0) for _, _, _, bm in cases])
    for (name, _, _, bm), (ln, section) in zip(cases, got):
        want = api.compress_search_bitmap(bm)
        assert ln == len(want) and section == want, (name, ln, len(want), first_difference(section, want))


def test_exact_room_and_errors_of_their_own(ctx):
    """A capacity of exactly the section's length is enough; one byte less, or a size that is no power of two, is that item's error, nothing
    is written for it, and its neighbours are exact."""
    d = dict(K.designed())
    names = ["density 0.05 8192", "kinds differ 65536", "escapes 8192", "alphabet 0..3 8192", "zeros 512", "uniform 512", "sixteen tables 524288"]
    want = {n: api.compress_search_bitmap(d[n]) for n in names}
    items, expect = [], []
    for n in names:
        items.append((d[n], None, len(want[n]), 0))
        expect.append((len(want[n]), want[n]))
        items.append((d[n], None, len(want[n]) - 1, 1))
        expect.append((-api.ERR_DST_TOO_SMALL, b""))
        items.append((d[n][:4096].ljust(4096, b"\1"), 48 if len(items) % 2 else 31, None, 0))
        expect.append((-api.ERR_ARG, b""))
    items.append((d["zeros 64"], 0, None, 0))
    expect.append((-api.ERR_ARG, b""))
    assert run_batch(ctx, items) == expect


def test_null_arguments(ctx):
    ctx.search_bitmaps_compress_device(None, None, [], None)                      # no items: nothing to do
    with pytest.raises(api.MinLZError, match="minlz error %d" % api.ERR_ARG):
        ctx.search_bitmaps_compress_device(None, None, [(0, 32, 0, 64)], None)


# ---- the device Writer with MLZ_STREAM_SEARCH_COMPRESS ----

import oracle as O  # noqa: E402
from minlz_amd import stream as S  # noqa: E402
from minlz_amd import synth  # noqa: E402
from tests import search_model as SMod  # noqa: E402
from tests.search_gpu import data_for, gather  # noqa: E402
from tests.test_gpu_stream_search_compressed import Reader, first_is_compressed, n_tables  # noqa: E402

TABLES = {"type 1": dict(search_match_len=6), "prefix": dict(search_match_len=6, search_prefix=b'":, '),
          "long prefix": dict(search_match_len=6, search_long_prefix=b'"user":"', search_extras=3)}


def json_with_needle(bs, nblk, tail):
    d = bytearray(synth.json_like(bs * nblk + tail, 5).tobytes())
    nd = b'"user":"' + b"qzjxkvwq0192" + b'", x'
    for o in (bs // 2, bs - 9, len(d) - len(nd)):
        d[o:o + len(nd)] = nd
    return bytes(d), nd


def shapes():
    """name -> (ranges, block size, table keywords, the needle or None)"""
    out = {}
    d = data_for("text_like", 64 << 10, 3, 100)                  # block 1 random: stored, no table
    out["text 64 KiB x 3 + 100, block 1 stored"] = ([d], 64 << 10, TABLES["type 1"], None)
    dj, nd = json_with_needle(1 << 20, 2, 100)
    for name, kw in TABLES.items():
        out["json 1 MiB x 2 + 100, " + name] = ([dj], 1 << 20, kw, nd)
    out["json 1 MiB x 2 + 100, two ranges"] = ([dj[:1 << 20], dj[1 << 20:]], 1 << 20, TABLES["type 1"], nd)
    out["text 4 KiB x 3"] = ([synth.text_like(3 * 4096, 8).tobytes()], 4 << 10, TABLES["type 1"], None)
    out["zeros 64 KiB x 2"] = ([bytes(128 << 10)], 64 << 10, TABLES["type 1"], None)
    return out


SHAPES = shapes()
_made = {}


def made(ctx, name):
    """(twin, the stream with search_compress, the expected stream, 0x46 chunks expected, counter 15 after the call), made once a shape."""
    if name not in _made:
        parts, bs, kw, _ = SHAPES[name]
        twin = gather(ctx, parts, bs, **kw)
        comp = gather(ctx, parts, bs, search_compress=True, **kw)
        counter = ctx.tables_written_compressed
        want, wrote = K.rewrite(twin)
        _made[name] = (twin, comp, want, wrote, counter)
    return _made[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_writer_stream_is_the_rewritten_twin(ctx, name):
    twin, comp, want, wrote, counter = made(ctx, name)
    assert len(comp) == len(want) and comp == want, (name, len(comp), len(want), first_difference(comp, want))
    assert counter == wrote == n_tables(comp, 0x46)
    if name.startswith("json") or name.startswith("zeros"):
        assert wrote >= 2 and len(comp) < len(twin)
    if name.startswith("text 4 KiB"):
        assert wrote == 0 and comp == twin and n_tables(comp, 0x45) == 3
    if "stored" in name:
        assert wrote >= 2 and [t for _, t in SMod.data_grid(comp)][1] == 0x01      # the stored block: no table, nothing compressed for it


@pytest.mark.parametrize("name", list(SHAPES))
def test_writer_with_index(ctx, name):
    """With a seek index the offsets move.  The stream is the one without an index and, behind it, the index the model's Index makes for
    it (a block's entry: where its chunks start, its table chunk when it has one), byte for byte, as the Writer's index tests hold the
    0x45 streams to search_model.splice; the oracle's Reader decodes the stream, and reads through the index find their bytes."""
    parts, bs, kw, _ = SHAPES[name]
    d = b"".join(parts)
    comp = gather(ctx, parts, bs, add_index=True, search_compress=True, **kw)
    assert n_tables(comp, 0x46) == made(ctx, name)[3] == ctx.tables_written_compressed
    want = K.with_index(made(ctx, name)[2], len(d))
    assert comp == want, (name, len(comp), len(want), first_difference(comp, want))
    assert O.stream_decode(comp, len(d)) == d and api.stream_decode(comp, ctx=ctx) == d
    rs = S.ReadSeeker(comp, backend=S.HipBackend(ctx))
    for o in (0, bs - 5, 2 * bs + 17, len(d) - 60):
        if o + 60 <= len(d):
            assert rs.ReadAt(60, o) == d[o:o + 60], o


def needle_of(name):
    """The shape's planted needle, or 20 bytes cut from its data (from the third block where there is one)."""
    parts, bs, _, nd = SHAPES[name]
    d = b"".join(parts)
    o = 2 * bs + 50 if len(d) >= 2 * bs + 70 else bs + 50
    return nd or d[o:o + 20]


@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip_searches_as_the_twin(ctx, name):
    """Every shape's stream opened and searched: a needle that is there, an absent one, a short one, four at once.  Totals, positions and
    stats are the twin's, and counter 14 is the number of 0x46 chunks in front of compressed blocks wherever the tables served the
    pattern (the zeros shape: its tables are RLE sections; the 4 KiB shape: no 0x46 chunk, so 0)."""
    twin, comp, _, wrote, _ = made(ctx, name)
    parts, bs, kw, _ = SHAPES[name]
    d = b"".join(parts)
    nd = needle_of(name)
    served = 0
    a, b = Reader(ctx, twin), Reader(ctx, comp)
    try:
        for p in (nd, b"absent from the data", nd[:9] if len(nd) > 12 else nd[:5]):
            (ra, ca), (rb, cb) = a.one(p), b.one(p)
            brute = SMod.brute(d, p)
            assert ra == rb and ra[0] == len(brute) and ra[1] == brute[:4096], p
            assert ca[:2] == cb[:2] and ca[2] == 0 and cb[2] == (sum(first_is_compressed(comp)) if cb[1] else 0), (p, ca, cb)
            served += 1 if cb[1] else 0
        pats = [nd, nd[4:], b"no such bytes here", d[bs + 100:bs + 120]]
        (ra, ca), (rb, cb) = a.many(pats), b.many(pats)
        assert ra == rb and ra[3] == [len(SMod.brute(d, p)) for p in pats] and ca[:2] == cb[:2]
        assert ca[2] == 0 and cb[2] == (sum(first_is_compressed(comp)) if cb[1] else 0)
    finally:
        a.close()
        b.close()
    assert sum(first_is_compressed(comp)) == wrote and served >= 1


def test_refusals(ctx):
    """The flag without tables in the three Writer calls is -MLZ_ERR_ARG; mlz_stream_encode and the batch encode behave as without it."""
    import ctypes as C
    from minlz_amd import _lib
    d = synth.text_like(3 * 4096, 8).tobytes()
    with pytest.raises(api.MinLZError, match="minlz error %d" % api.ERR_ARG):
        gather(ctx, [d], 4096, search_compress=True)
    t = dev_u8(d)
    dst = torch.full((api.stream_bound(len(d), 4096) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    srcs, lens = (C.c_void_p * 1)(t.data_ptr()), (C.c_size_t * 1)(len(d))
    L = _lib.lib()
    assert L.mlz_stream_encode_gather_device_tables(ctx.handle, 1, 4096, api.COMPRESS_TABLES, None, srcs, lens, 1, dst.data_ptr(), dst.numel() - 64) == -api.ERR_ARG
    assert L.mlz_stream_encode_gather_device_long_prefix(ctx.handle, 1, 4096, api.COMPRESS_TABLES, None, srcs, lens, 1, dst.data_ptr(), dst.numel() - 64) == -api.ERR_ARG
    assert (dst.cpu().numpy() == GUARD).all()
    assert api.stream_bound(len(d), 4096, search_match_len=6, search_compress=True) == api.stream_bound(len(d), 4096, search_match_len=6)
    assert api.stream_bound(len(d), 4096, search_compress=True) == api.stream_bound(len(d), 4096)
    a = np.frombuffer(d, np.uint8)
    out = [np.zeros(api.stream_bound(len(d), 4096), np.uint8) for _ in range(2)]
    got = [ctx._call("mlz_stream_encode", 1, 4096, f, a.ctypes.data, a.size, o.ctypes.data, o.size) for f, o in zip((0, api.COMPRESS_TABLES), out)]
    assert got[0] == got[1] and out[0].tobytes() == out[1].tobytes()
    outs = []
    for f in (0, api.COMPRESS_TABLES):
        bd = torch.full((api.stream_bound(len(d), 4096) + 64,), GUARD, dtype=torch.uint8, device="cuda")
        r = ctx.stream_encode_batch_device(1, 4096, False, t.data_ptr(), bd.data_ptr(), [(0, len(d), 0, bd.numel() - 64)], flags=f)
        torch.cuda.synchronize()
        outs.append((r, bd.cpu().numpy().tobytes()))
    assert outs[0] == outs[1] and outs[0][0][0] > 0


# ---- mlz_dev_reader_build_sidecar with the flag ----

def test_sidecar(ctx):
    """Two configurations over a stream with a stored block: the compressed sidecar is the uncompressed one rewritten by the same helper;
    a capacity of exactly its size is enough, one byte less is -MLZ_ERR_DST_TOO_SMALL with nothing written; attached, it searches as the
    uncompressed one."""
    from minlz_amd.api import search_config
    from tests.search_gpu import Opened
    bs = 64 << 10
    d = bytearray(data_for("json_like", bs, 6, 100))
    nd = b'"user":"qzjxkvwq0192", x'
    d[4 * bs - 9:4 * bs - 9 + len(nd)] = nd
    d = bytes(d)
    main = gather(ctx, [d], bs)
    assert [t for _, t in SMod.data_grid(main)][1] == 0x01
    cfgs = [search_config(1, 6), search_config(2, 6, b'":, ')]
    h = Opened(ctx, main)
    try:
        cap = h.rd.sidecar_bound(cfgs)
        dst = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
        n45 = h.rd.build_sidecar(cfgs, dst.data_ptr(), cap)
        side45 = dst.cpu().numpy()[:n45].tobytes()
        dst.fill_(GUARD)
        n46 = h.rd.build_sidecar(cfgs, dst.data_ptr(), cap, compress=True)
        counter = ctx.tables_written_compressed
        o = dst.cpu().numpy()
        side46 = o[:n46].tobytes()
        assert (o[n46:] == GUARD).all()
        want, wrote = K.rewrite(side45)
        assert side46 == want, (n46, len(want), first_difference(side46, want))
        assert counter == wrote == n_tables(side46, 0x46) >= 6 and n46 < n45
        dst.fill_(GUARD)
        assert h.rd.build_sidecar(cfgs, dst.data_ptr(), n46, compress=True) == n46 and dst.cpu().numpy()[:n46].tobytes() == want
        assert (dst.cpu().numpy()[n46:] == GUARD).all()
        dst.fill_(GUARD)
        with pytest.raises(api.MinLZError, match="minlz error %d" % api.ERR_DST_TOO_SMALL):
            h.rd.build_sidecar(cfgs, dst.data_ptr(), n46 - 1, compress=True)
        assert (dst.cpu().numpy() == GUARD).all()
    finally:
        h.close()
    results = {}
    for name, s in (("45", side45), ("46", side46)):
        sr = Reader(ctx, main)
        t = dev_u8(s)
        try:
            sr.rd.attach_sidecar(t.data_ptr(), len(s))
            results[name] = [sr.one(p) for p in (nd, nd[:10], b"zq" + nd[8:20], b"absent from the data")] + [sr.many([nd, nd[4:], b"no such bytes", d[bs + 5:bs + 25]])]
        finally:
            sr.close()
    for (ra, ca), (rb, cb) in zip(results["45"], results["46"]):
        assert ra == rb and ca[:2] == cb[:2] and ca[2] == 0
    assert results["46"][0][0][0] == len(SMod.brute(d, nd)) and results["46"][0][1][2] > 0
