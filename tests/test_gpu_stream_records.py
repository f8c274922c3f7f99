"""mlz_dev_reader_search_records (DeviceReader.search_records, DeviceStream.search_records): the records of a stream in HBM that hold a
pattern, against tests/records_model.py over the decoded bytes.  Every output array is guarded by sentinels and compared whole."""
import numpy as np
import pytest
import torch

import minlz_amd as mz
from minlz_amd import _lib, api, shard, synth
from tests import records_model as RM
from tests import search_model as SMod
from tests.search_gpu import SENT, Opened, gather

pytestmark = pytest.mark.gpu

MLZ_ERR_ARG = 8
NL = b"\n"


def lines(n, seed, kind="json_like"):
    return bytearray(getattr(synth, kind)(n, seed).tobytes())


def plant(d, at, what):
    d[at:at + len(what)] = what


class Records(Opened):
    """A stream on the device and its decoded bytes; a call compares everything the call returns and writes with the model."""

    def __init__(self, ctx, stream, data):
        super().__init__(ctx, stream)
        self.data = bytes(data)
        self.nck = len(SMod.data_grid(stream))

    def raw(self, pat, delim, W, rec_cap, dst_cap, starts=True, flags=True, **kw):
        """-> (R, totals, stats, dst, rec_off, rec_start, rec_flags): the guarded arrays whole, as numpy."""
        dst = torch.full((dst_cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        off = torch.full((rec_cap + 8,), SENT, dtype=torch.int64, device="cuda")
        st = torch.full((rec_cap + 9,), SENT, dtype=torch.int64, device="cuda")
        fl = torch.full((rec_cap + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        R, totals, stats = self.rd.search_records(pat, delim, dst.data_ptr() if dst_cap else None, dst_cap, off.data_ptr() if rec_cap else None,
                                                  st.data_ptr() if starts else None, fl.data_ptr() if flags and rec_cap else None, rec_cap, max_reach=W, **kw)
        torch.cuda.synchronize()
        assert self.ctx.search_plan() == stats[1:]
        return R, totals, stats, dst.cpu().numpy(), off.cpu().numpy(), st.cpu().numpy(), fl.cpu().numpy()

    def __call__(self, pat, delim=NL, W=0, rec_cap=4096, dst_cap=1 << 20, **kw):
        """-> (the model's result, stats)."""
        want = RM.result(self.data, pat, delim, W, rec_cap, dst_cap)
        R, totals, stats, dst, off, st, fl = self.raw(pat, delim, W, rec_cap, dst_cap, **kw)
        what = "%r W=%d caps %d / %d %r" % (pat[:16], W, rec_cap, dst_cap, kw)
        k = want["k"]
        assert R == want["R"] and totals == want["totals"], what
        assert off[:k].tolist() == want["rec_off"] and (off[k:] == SENT).all(), what
        if kw.get("starts", True):
            ns = len(want["rec_start"])
            assert st[:ns].tolist() == want["rec_start"] and (st[ns:] == SENT).all(), what
        else:
            assert (st == SENT).all(), what
        if kw.get("flags", True):
            assert fl[:k].tolist() == want["flags"] and (fl[k:] == 0x5A).all(), what
        else:
            assert (fl == 0x5A).all(), what
        nb = len(want["dst"])
        assert dst[:nb].tobytes() == want["dst"], what + ": first difference at %d" % next((i for i in range(nb) if dst[i] != want["dst"][i]), -1)
        assert (dst[nb:] == 0x5A).all(), what
        return want, stats


NEEDLE = b"@zq-needle-77@"


def plain_case(bs, nblk):
    """Lines with the needle planted: at the stream's start, twice in one line, across a block border, in a line inside a stored (random)
    block, and as the stream's last bytes (a stream that ends without a delimiter)."""
    d = lines(bs * nblk + 700, 11)
    d[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
    plant(d, 0, NEEDLE)
    plant(d, bs + bs // 2, NL + b"a planted line with " + NEEDLE + b" inside a stored block" + NL)
    plant(d, 3 * bs + 100, NL + NEEDLE + b" and " + NEEDLE + b" again" + NL)
    plant(d, 5 * bs - 5, NEEDLE)
    plant(d, len(d) - len(NEEDLE) - 30, b"the last line " + NEEDLE.replace(b"\n", b"") + b"x" * 16)
    plant(d, len(d) - len(NEEDLE), NEEDLE)
    return bytes(d)


@pytest.fixture(scope="module", params=[(4 << 10, 40), (64 << 10, 7)], ids=["4K", "64K"])
def plain(ctx, request):
    bs, nblk = request.param
    d = plain_case(bs, nblk)
    stream = gather(ctx, [d], bs)
    assert SMod.data_grid(stream)[1][1] == 0x01   # the random block: stored
    h = Records(ctx, stream, d)
    yield h, bs
    h.close()


def test_no_table_stream(plain):
    h, bs = plain
    want, stats = h(NEEDLE)
    assert want["R"] == 5 and want["totals"][2] == 7 and want["totals"][3] == 0 and stats[1] == h.nck and stats[2] == 0
    assert want["rec_off"][0] == 0 and want["dst"].endswith(NEEDLE)
    assert b"inside a stored block" in want["dst"]
    h(NEEDLE, starts=False, flags=False)
    # a common piece of the lines: many records
    want, _ = h(b'"user"', rec_cap=8192)
    assert want["R"] > 100 and want["k"] == want["R"]


def test_counting_form_and_caps(plain):
    h, bs = plain
    want, _ = h(NEEDLE, rec_cap=0, dst_cap=0)
    assert want["k"] == 0 and want["rec_start"] == [0] and want["totals"][0] == 5
    h(NEEDLE, rec_cap=0, dst_cap=0, starts=False)
    full = RM.result(h.data, NEEDLE, NL, 0, 1 << 20, 1 << 30)
    ends = full["rec_start"][1:]
    for rc in (1, 2, 5, 6):
        assert h(NEEDLE, rec_cap=rc)[0]["k"] == min(rc, 5)
    for e in ends[:3]:
        for dlt in (-1, 0, 1):
            want, _ = h(NEEDLE, dst_cap=e + dlt)
            assert want["k"] == ends.index(e) + (1 if dlt >= 0 else 0)   # nothing in part
    assert h(NEEDLE, rec_cap=2, dst_cap=ends[0])[0]["k"] == 1
    assert h(NEEDLE, rec_cap=1, dst_cap=ends[2])[0]["k"] == 1


def test_no_occurrence_and_arguments(plain):
    h, bs = plain
    R, totals, stats, dst, off, st, fl = h.raw(b"@never-there-0123@", NL, 0, 16, 4096)
    assert R == 0 and totals == (0, 0, 0, 0) and stats[0] == h.nck
    assert (dst == 0x5A).all() and (off == SENT).all() and (st == SENT).all() and (fl == 0x5A).all()
    L = _lib.lib()
    dst = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    off = torch.full((17,), SENT, dtype=torch.int64, device="cuda")
    st = torch.full((17,), SENT, dtype=torch.int64, device="cuda")
    fl = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda")
    host = np.zeros(64, np.uint64)
    hd = h.rd.handle

    def call(pat, n, delim=10, W=0, d=dst.data_ptr(), dc=4096, o=off.data_ptr(), s=st.data_ptr(), f=fl.data_ptr(), rc=16, rd=hd):
        return L.mlz_dev_reader_search_records(rd, None, 0, pat, n, delim, W, d, dc, o, s, f, rc, None, None)
    bad = [call(b"two\nlines", 9), call(NEEDLE, len(NEEDLE), delim=ord("@")), call(NEEDLE, 0), call(b"x" * 300, 257), call(None, 3),
           call(NEEDLE, len(NEEDLE), W=(1 << 20) + 1), call(NEEDLE, len(NEEDLE), d=None), call(NEEDLE, len(NEEDLE), o=None),
           call(NEEDLE, len(NEEDLE), d=host.ctypes.data), call(NEEDLE, len(NEEDLE), o=host.ctypes.data), call(NEEDLE, len(NEEDLE), s=host.ctypes.data),
           call(NEEDLE, len(NEEDLE), f=host.ctypes.data), call(NEEDLE, len(NEEDLE), rd=None)]
    assert bad == [-MLZ_ERR_ARG] * len(bad)
    torch.cuda.synchronize()
    assert (dst == 0x5A).all() and (off == SENT).all() and (st == SENT).all() and (fl == 0x5A).all()
    with pytest.raises(mz.MinLZError) as e:
        h.rd.search_records(b"a\nb", NL, dst.data_ptr(), 4096, off.data_ptr(), st.data_ptr(), fl.data_ptr(), 16)
    assert int(str(e.value).split()[2]) == MLZ_ERR_ARG
    assert call(NEEDLE, len(NEEDLE), W=1 << 20) == 5 and call(NEEDLE, len(NEEDLE), d=None, dc=0, o=None, s=None, f=None, rc=0) == 5


def test_default_reach(plain):
    h, bs = plain
    a = h.raw(NEEDLE, NL, 0, 64, 1 << 16)
    b = h.raw(NEEDLE, NL, 65536, 64, 1 << 16)
    assert a[0] == b[0] and a[1] == b[1] and all((x == y).all() for x, y in zip(a[3:], b[3:]))


def test_sidecar_gives_the_same(ctx, plain):
    h, bs = plain
    before = h.raw(NEEDLE, NL, 0, 64, 1 << 16)
    cfgs = [api.search_config(1, 6)]
    cap = h.rd.sidecar_bound(cfgs)
    side = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = h.rd.build_sidecar(cfgs, side.data_ptr(), cap)
    h.rd.attach_sidecar(side.data_ptr(), n)
    try:
        want, stats = h(NEEDLE, rec_cap=64, dst_cap=1 << 16)
        after = h.raw(NEEDLE, NL, 0, 64, 1 << 16)
        assert stats[2] > 0 and (stats[1] < h.nck or bs > 4096)   # the sidecar's tables serve the search; among 41 chunks they prune
        assert after[0] == before[0] and after[1] == before[1] and all((x == y).all() for x, y in zip(after[3:], before[3:]))
    finally:
        h.rd.detach_sidecar()


# ---- type 1 tables: a record that reaches into a chunk the tables prune ----

def typed_case(bs, nblk):
    """Lines; needle i lies 5 bytes into block 2 + 2 i and its line begins 40 bytes in front of that block -> (data, [(needle, block)])."""
    d = lines(bs * nblk + 300, 5)
    out = []
    for i, k in enumerate(range(2, nblk, 2)):
        nd = b"@qz%02d-Needle-%02d@" % (i, 7 * i + 3)
        line = NL + b"x" * 39 + b"y" * 5 + nd + b" the rest of the line" + NL
        plant(d, k * bs - 40, line)
        assert d[k * bs + 5:k * bs + 5 + len(nd)] == nd
        out.append((nd, k))
    return bytes(d), out


@pytest.fixture(scope="module", params=[(4 << 10, 24), (64 << 10, 7)], ids=["4K", "64K"])
def typed(ctx, request):
    bs, nblk = request.param
    d, needles = typed_case(bs, nblk)
    stream = gather(ctx, [d], bs, search_match_len=6)
    cfg, B, tables = SMod.read_tables(stream, types=(1,))
    sizes = [n for n, _ in SMod.data_grid(stream)]
    assert cfg is not None and sum(t is not None for t in tables) >= len(tables) // 2
    # a needle whose line begins in a chunk that its plan leaves out
    pick = next(((nd, k, SMod.plan(tables, sizes, nd, cfg, B)) for nd, k in needles if k - 1 not in SMod.plan(tables, sizes, nd, cfg, B)), None)
    assert pick is not None, "every needle's tables admit the chunk in front of it"
    h = Records(ctx, stream, d)
    yield h, bs, stream, pick
    h.close()


def test_record_reaches_into_a_pruned_chunk(typed):
    h, bs, stream, (nd, k, plan) = typed
    want, stats = h(nd)
    assert stats == (h.nck, len(plan), stats[2]) and stats[2] > 0 and stats[1] < h.nck
    assert want["R"] == 1 and want["rec_off"] == [k * bs - 39] and want["flags"] == [0]
    assert want["dst"] == b"x" * 39 + b"y" * 5 + nd + b" the rest of the line"
    assert h.ctx.range_plan()[0] >= 2   # the read phase decoded the pruned chunk and the needle's
    # without the tables: the same result, every chunk decoded
    want2, stats2 = h(nd, no_tables=True)
    assert want2 == want and stats2[1] == h.nck and stats2[2] == 0
    # many records over the tables
    want, _ = h(b'"user"', rec_cap=8192)
    assert want["R"] > 100


def test_broken_chunk_that_only_the_read_phase_touches(ctx, typed):
    h, bs, stream, (nd, k, plan) = typed
    datas = [c for c in SMod.chunks_of(stream) if c[1] in (1, 2, 3)]
    assert len(datas) == h.nck
    b = bytearray(stream)
    b[datas[k - 1][0] + 5] ^= 0x40          # the pruned chunk's CRC
    bad = Records(ctx, bytes(b), h.data)
    try:
        out = torch.zeros(8, dtype=torch.int64, device="cuda")
        assert bad.rd.search(nd, out.data_ptr(), 8)[0] == 1      # the search alone never sees the chunk
        with pytest.raises(mz.ErrCRC):
            bad.raw(nd, NL, 0, 16, 4096)
        want, _ = bad(nd, ignore_crc=True)
        assert want["R"] == 1
    finally:
        bad.close()


# ---- long records ----

@pytest.mark.parametrize("bs,nblk", [(4 << 10, 12), (64 << 10, 7)], ids=["4K", "64K"])
def test_record_over_four_chunks(ctx, bs, nblk):
    n = 3 * bs + 17
    d = lines(bs * nblk + 99, 8)
    at = 2 * bs - 50
    long_line = bytes(lines(n, 9)).replace(NL, b" ")
    mid = n // 2
    long_line = long_line[:mid] + NEEDLE + long_line[mid + len(NEEDLE):]
    plant(d, at, NL + long_line + NL)
    d = bytes(d)
    for M in (None, 6):
        h = Records(ctx, gather(ctx, [d], bs, search_match_len=M), d)
        try:
            want, _ = h(NEEDLE, W=n + 5, rec_cap=4, dst_cap=n + 100)
            assert want["R"] == 1 and want["dst"] == long_line and want["rec_off"] == [at + 1] and want["flags"] == [0]
            assert h.ctx.range_plan()[0] >= 4
            want, _ = h(NEEDLE, W=bs, rec_cap=4, dst_cap=n + 100)
            assert want["R"] == 1 and want["flags"] == [3] and len(want["dst"]) == 2 * bs + len(NEEDLE)
            want, _ = h(NEEDLE, W=n + 5, rec_cap=4, dst_cap=n - 1)   # the one record does not fit: nothing of it is written
            assert want["R"] == 1 and want["k"] == 0
        finally:
            h.close()


def test_stream_without_a_delimiter(ctx):
    bs = 64 << 10
    d = lines(3 * bs + 1234, 4, "text_like").replace(NL, b" ")
    for at in (0, 70000, 70100, len(d) - len(NEEDLE)):
        plant(d, at, NEEDLE)
    d = bytes(d)
    assert NL not in d
    h = Records(ctx, gather(ctx, [d], bs, search_match_len=6), d)
    try:
        want, _ = h(NEEDLE, dst_cap=1 << 20)                  # the default reach cuts: two overlapping pieces
        assert want["R"] == 4 and want["flags"] == [2, 3, 3, 1]
        want, _ = h(NEEDLE, W=1 << 20, dst_cap=1 << 20)       # a reach beyond the stream: one record, all of it
        assert want["R"] == 1 and want["dst"] == d and want["flags"] == [0]
        want, _ = h(NEEDLE, W=1, dst_cap=1 << 20)
        assert want["R"] == 4 and want["totals"][1] == 4 * len(NEEDLE) + 6
    finally:
        h.close()


def test_empty_stream(ctx):
    h = Records(ctx, b"", b"")
    try:
        R, totals, stats, dst, off, st, fl = h.raw(NEEDLE, NL, 0, 4, 64)
        assert R == 0 and totals == (0, 0, 0, 0) and stats == (0, 0, 0) and (st == SENT).all() and (dst == 0x5A).all()
    finally:
        h.close()


# ---- many short records, many occurrences per window ----

def test_words(ctx):
    bs = 64 << 10
    d = synth.text_like(5 * bs + 4321, 3).tobytes()
    pat = b"the"
    occ = RM.occurrences(d, pat)
    assert len(occ) >= 2000 and b" " not in pat
    for M in (None, 6):
        h = Records(ctx, gather(ctx, [d], bs, search_match_len=M), d)
        try:
            want, _ = h(pat, delim=b" ", W=64, rec_cap=len(occ) + 8, dst_cap=1 << 20)
            assert want["R"] > 1024 and want["k"] == want["R"] and want["totals"][2] == len(occ)
            want, _ = h(pat, delim=b" ", W=64, rec_cap=1500, dst_cap=1 << 20)
            assert want["k"] == 1500
            want, _ = h(pat, delim=b" ", W=2, rec_cap=len(occ) + 8, dst_cap=1 << 20)   # a reach below the words: cut records
            assert want["totals"][3] > 0
        finally:
            h.close()


def test_device_stream(ctx):
    bs = 64 << 10
    d = plain_case(bs, 6)
    codec = shard.HipTensorCodec(ctx)
    t = torch.from_numpy(np.frombuffer(gather(ctx, [d], bs, search_match_len=6), np.uint8).copy()).cuda()
    ds = codec.open_stream(t)
    want = RM.result(d, NEEDLE, NL, 0, 3, 1 << 20)
    total, data, rec_off, rec_start, flags, totals = ds.search_records(NEEDLE, max_records=3)
    assert total == want["R"] == 5 and totals == want["totals"]
    assert data.cpu().numpy().tobytes() == want["dst"] and rec_off.tolist() == want["rec_off"] and rec_start.tolist() == want["rec_start"]
    assert flags.tolist() == want["flags"]
    total, data, rec_off, rec_start, flags, totals = ds.search_records(NEEDLE, max_records=0, max_bytes=0)
    assert total == 5 and data.numel() == 0 and rec_off.numel() == 0 and rec_start.tolist() == [0] and totals[2] == 7
