"""The record index of a stream in HBM (DeviceReader.index_records, record_spans, read_records, record_numbers, record_range and
DeviceStream's forms of them) against tests/record_index_model.py over the decoded bytes.  Every output array is guarded by sentinels and
compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from tests import corrupt as CM
from tests import record_index_model as IM
from tests import records_model as RM
from tests import search_model as SMod
from tests import stream_device_cases as SC
from tests.search_gpu import SENT, Opened, dev_u64, gather

pytestmark = pytest.mark.gpu

MLZ_ERR_CORRUPT, MLZ_ERR_CRC, MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 1, 5, 6, 8
NL = b"\n"
NONE = -1   # UINT64_MAX as the int64 the tensors hold


def lines(n, seed, kind="json_like"):
    return bytearray(getattr(synth, kind)(n, seed).tobytes())


def guarded(n, extra=8):
    return torch.full((n + extra,), SENT, dtype=torch.int64, device="cuda")


class Indexed(Opened):
    """A stream on the device, its decoded bytes and an open handle; the calls compare everything they return and write with the model."""

    def __init__(self, ctx, stream, data):
        super().__init__(ctx, stream)
        self.data, self.stream = bytes(data), bytes(stream)
        self.grid = SMod.data_grid(stream) if len(stream) else []
        self.nck = sum(1 for n, _ in self.grid if n)
        self.ck_start = np.concatenate([[0], np.cumsum([n for n, _ in self.grid])]).astype(np.int64)

    def index(self, delim=NL, fresh=True, **kw):
        N, info = self.rd.index_records(delim, **kw)
        wN, wk = IM.count(self.data, delim)
        assert (N, info[0], info[1]) == (wN, wN, wk), "delimiter %r" % delim
        assert info[3] == (self.nck if fresh else 0)
        assert self.rd.record_count() == wN
        self.delim = delim
        return N, info

    def spans_raw(self, idx):
        """-> (the call's value, off, len): the guarded arrays whole."""
        n = len(idx)
        d_idx, off, ln = dev_u64(idx), guarded(n), guarded(n)
        r = _lib.lib().mlz_dev_reader_record_spans(self.rd.handle, None, d_idx.data_ptr() if n else None, n, off.data_ptr(), ln.data_ptr())
        torch.cuda.synchronize()
        return r, off.cpu().numpy(), ln.cpu().numpy()

    def check_all_spans(self):
        """record_spans(arange(N)) against the model: the whole table."""
        start, length = IM.spans(self.data, self.delim)
        N = len(start)
        r, off, ln = self.spans_raw(np.arange(N))
        assert r == int(length.sum())
        bad = np.flatnonzero((off[:N] != start) | (ln[:N] != length))
        assert bad.size == 0, "record %d of %d: got (%d, %d), want (%d, %d)" % (bad[0], N, off[bad[0]], ln[bad[0]], start[bad[0]], length[bad[0]])
        assert (off[N:] == SENT).all() and (ln[N:] == SENT).all()
        return start, length

    def read_raw(self, idx, dst_cap, starts=True, **kw):
        """-> (the call's value, dst, starts): the guarded arrays whole."""
        n = len(idx)
        d_idx = dev_u64(idx)
        dst = torch.full((dst_cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        st = guarded(n + 1)
        flags = 1 if kw.get("ignore_crc") else 0
        r = _lib.lib().mlz_dev_reader_read_records(self.rd.handle, None, flags, d_idx.data_ptr() if n else None, n, dst.data_ptr() if dst_cap else None, dst_cap,
                                                   st.data_ptr() if starts else None)
        torch.cuda.synchronize()
        return r, dst.cpu().numpy(), st.cpu().numpy()

    def touched(self, idx):
        """The data chunks that the records' bytes lie in."""
        start, length = IM.spans(self.data, self.delim)
        seen = set()
        for r in set(int(i) for i in idx):
            if length[r]:
                j0 = int(np.searchsorted(self.ck_start, start[r], side="right")) - 1
                j1 = int(np.searchsorted(self.ck_start, start[r] + length[r] - 1, side="right")) - 1
                seen.update(range(j0, j1 + 1))
        return seen


def plain_case(bs, nblk):
    """Lines with a stored (random) block; delimiters planted at block borders (bs - 1, bs), doubled ones, at the stream's first byte and at
    its last byte."""
    d = lines(bs * nblk + 700, 11)
    d[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
    for k in (1, 2, 3, 5):
        d[k * bs - 1:k * bs + 1] = b"\n\n"
    d[4 * bs - 1:4 * bs] = NL
    d[6 * bs:6 * bs + 1] = NL
    d[3 * bs + 50:3 * bs + 54] = b"\n\n\n\n"
    d[0:1] = NL
    d[-1:] = NL
    return bytes(d)


@pytest.fixture(scope="module", params=[(4 << 10, 40), (64 << 10, 7)], ids=["4K", "64K"])
def plain(ctx, request):
    bs, nblk = request.param
    d = plain_case(bs, nblk)
    stream = gather(ctx, [d], bs)
    assert SMod.data_grid(stream)[1][1] == 0x01   # the random block: stored
    h = Indexed(ctx, stream, d)
    N, info = h.index()
    assert info[2] == 8 * info[1]                  # one group: the table is sized exactly
    yield h, bs
    h.close()


def test_small_streams_with_a_stored_block(plain):
    h, bs = plain
    start, length = h.check_all_spans()
    N = len(start)
    assert h.data[0:1] == NL and start[0] == 0 and length[0] == 0 and start[1] == 1          # the first byte is a delimiter
    assert N == IM.count(h.data, NL)[1] and start[-1] + length[-1] == len(h.data) - 1       # ... and the last one
    for k in (1, 2, 3, 5):
        assert bs * k in start.tolist() and length[start.tolist().index(bs * k)] == 0       # the empty record between bs - 1 and bs
    assert (length == 0).sum() >= 8
    h.index(fresh=False)                                                                      # the same delimiter again decodes nothing


EDGES = [b"\n", b"x", b"\nabc\ndef", b"abc\ndef\n", b"abc\ndef", b"a\n\nb\n\n\nc\n\n", b"no delimiter at all, in more than sixteen bytes", b"\n" * 100, b"\n" * 16]


def border_data(at):
    d = bytearray(b"abcdefghijklmnopqrstuvwxyz" * 5042)[:131072]
    for a in at:
        d[a] = 10
    return bytes(d)


def test_edge_streams(ctx):
    cases = [(gather(ctx, [d], 64 << 10), d) for d in EDGES]
    cases += [(gather(ctx, [border_data(at)], 64 << 10), border_data(at)) for at in ((15, 16, 17), (65535, 65536, 65537), (16,), (65536,), (0, 131071))]
    cases += [(b"", b""), (O.stream_encode(b"", 1, 1 << 20), b"")]
    for stream, d in cases:
        h = Indexed(ctx, stream, d)
        try:
            N, info = h.index()
            h.check_all_spans()
            assert info[2] == 8 * info[1]
            if not d:
                assert N == 0 and info == (0, 0, 0, 0)
                assert h.spans_raw([0])[0] == -MLZ_ERR_ARG and h.rd.record_range(0, 0) == (0, 0)
        finally:
            h.close()


def test_every_byte_a_delimiter(ctx):
    n = 1 << 20
    d = b"," * n
    h = Indexed(ctx, gather(ctx, [d], 64 << 10), d)
    try:
        before = ctx.workspace_bytes()[1]
        N, info = h.index(b",")
        assert N == n and info[:3] == (n, n, 8 * n)
        assert ctx.workspace_bytes()[1] - before < 4 * n     # the 8 n bytes of table are the handle's, not context workspace
        r, off, ln = h.spans_raw(np.arange(n))
        assert r == 0 and (off[:n] == np.arange(n)).all() and (ln[:n] == 0).all() and (off[n:] == SENT).all() and (ln[n:] == SENT).all()
    finally:
        h.close()


@pytest.mark.parametrize("delim", [0x00, 0x0A, 0x80, 0xFF])
def test_exact_mask(ctx, delim):
    """delimiter ^ 1 directly behind and in front of a hit, and delimiter ^ 0x80 present."""
    d, n1, n80 = bytes([delim]), bytes([delim ^ 1]), bytes([delim ^ 0x80])
    unit = d + n1 + n1 + d + n80 + n1 + d + d + n1 + n80 + n80 + d + n1
    rng = np.random.default_rng(delim)
    noise = bytes(np.frombuffer(d + n1 + n80 + bytes([delim ^ 0x7f]), np.uint8)[rng.integers(0, 4, 70001)])
    data = (unit * 40 + n1 * 7 + d + n1 + n80 * 3) * 3 + noise + (n1 + d) * 150 + n80 * 300
    h = Indexed(ctx, gather(ctx, [data], 64 << 10), data)
    try:
        h.index(d)
        h.check_all_spans()
    finally:
        h.close()


@pytest.fixture(scope="module")
def two_groups(ctx):
    """About 72 MiB of compressible lines in 8 MiB blocks: a group of 8 chunks (64 MiB) and a second one."""
    unit = bytes(lines((1 << 20) + 37, 21))
    n = (72 << 20) + 4321
    d = (unit * (n // len(unit) + 1))[:n]
    stream = gather(ctx, [d], 8 << 20)
    assert len(stream) < len(d) // 2
    h = Indexed(ctx, stream, d)
    yield h
    h.close()


def test_two_groups(two_groups):
    h = two_groups
    assert h.nck == 10
    N, info = h.index()
    assert 8 * info[1] <= info[2] <= 16 * info[1]       # geometric growth: at most twice the delimiters
    start, length = h.check_all_spans()
    border = 64 << 20
    r = int(IM.numbers(h.data, NL, [border])[0][0])     # the record that holds the first byte of the second group
    assert start[r] < border < start[r] + length[r], "no record straddles the group border"
    for q in (r - 1, r, r + 1):
        got, off, ln = h.spans_raw([q])
        assert (off[0], ln[0]) == (start[q], length[q]) and got == length[q]
    want, wst = IM.read(h.data, NL, [r + 1, r, r - 1])
    got, dst, st = h.read_raw([r + 1, r, r - 1], len(want))
    assert got == len(want) and dst[:got].tobytes() == want and st[:4].tolist() == wst and (dst[got:] == 0x5A).all()
    assert h.ctx.range_plan()[0] == 2                   # the chunks on either side of the border, each once


def test_stored_chunks_on_both_sides_of_the_group_border(ctx):
    """9 blocks of 8 MiB, block 7 (the last of group 0) and block 8 (the first of group 1) random bytes, hence stored: the second group's
    stored chunk is copied into the scratch by pieces that lie behind the first group's, and its delimiters enter the table."""
    bs = 8 << 20
    unit = bytes(lines((1 << 20) + 37, 21))
    d = (unit * (7 * bs // len(unit) + 1))[:7 * bs] + synth.random_bytes(2 * bs, seed=8).tobytes()
    stream = gather(ctx, [d], bs)
    grid = SMod.data_grid(stream)
    assert [n for n, _ in grid] == [bs] * 9 and grid[7][1] == grid[8][1] == 0x01 and all(t != 0x01 for _, t in grid[:7])
    h = Indexed(ctx, stream, d)
    try:
        h.index()
        start, length = h.check_all_spans()
        assert (start >= 8 * bs).sum() > 1000               # records that lie in the second group's stored chunk
    finally:
        h.close()


def test_read_records(plain):
    h, bs = plain
    start, length = IM.spans(h.data, NL)
    N = len(start)
    rng = np.random.default_rng(7)
    idx = rng.integers(0, N, 5000)
    idx[:40] = np.flatnonzero(length == 0)[rng.integers(0, int((length == 0).sum()), 40)]   # empty records among them
    idx[40:80] = idx[100:140]                                                                 # repeats
    idx[80], idx[81] = 0, N - 1
    rng.shuffle(idx)
    want, wst = IM.read(h.data, NL, idx.tolist())
    for starts in (True, False):
        got, dst, st = h.read_raw(idx, len(want) + 100, starts=starts)
        assert got == len(want)
        assert dst[:got].tobytes() == want and (dst[got:] == 0x5A).all()
        if starts:
            assert st[:len(idx) + 1].tolist() == wst and (st[len(idx) + 1:] == SENT).all()
        else:
            assert (st == SENT).all()
        assert h.ctx.range_plan()[0] == len(h.touched(idx))          # each touched chunk once
    got, dst, st = h.read_raw(idx, len(want))                        # a destination that fits exactly
    assert got == len(want) and dst[:got].tobytes() == want and (dst[got:] == 0x5A).all()
    # a few records of one chunk: that chunk alone is decoded
    few = np.flatnonzero((start > 4 * bs + 10) & (start + length < 5 * bs - 10) & (length > 0))[:5]
    want2, wst2 = IM.read(h.data, NL, few.tolist())
    got, dst, st = h.read_raw(few, len(want2))
    assert got == len(want2) and dst[:got].tobytes() == want2 and st[:len(few) + 1].tolist() == wst2 and h.ctx.range_plan()[0] == 1
    # nothing asked
    got, dst, st = h.read_raw([], 64)
    assert got == 0 and (dst == 0x5A).all() and (st == SENT).all()
    # refusals: nothing is written
    bad = idx.copy()
    bad[2500] = N
    got, dst, st = h.read_raw(bad, len(want) + 100)
    assert got == -MLZ_ERR_ARG and (dst == 0x5A).all() and (st == SENT).all()
    got, dst, st = h.read_raw(idx, len(want) - 1)
    assert got == -MLZ_ERR_DST_TOO_SMALL and (dst == 0x5A).all() and (st == SENT).all()
    d_bad = dev_u64(bad)
    with pytest.raises(mz.MinLZError):
        h.rd.read_records(d_bad.data_ptr(), len(bad), None, 0)


def test_record_spans_arguments(plain):
    h, bs = plain
    start, length = IM.spans(h.data, NL)
    N = len(start)
    idx = [N - 1, 0, 5, 5, N - 1]
    r, off, ln = h.spans_raw(idx)
    assert r == int(length[idx].sum()) and off[:5].tolist() == start[idx].tolist() and ln[:5].tolist() == length[idx].tolist()
    assert (off[5:] == SENT).all() and (ln[5:] == SENT).all()
    r, off, ln = h.spans_raw([3, N, 4])
    assert r == -MLZ_ERR_ARG and (off[3:] == SENT).all() and (ln[3:] == SENT).all()
    r, off, ln = h.spans_raw([])
    assert r == 0 and (off == SENT).all() and (ln == SENT).all()
    L = _lib.lib()
    host = np.zeros(8, np.uint64)
    d_idx, o, l_ = dev_u64([1, 2]), guarded(2), guarded(2)
    bad = [L.mlz_dev_reader_record_spans(h.rd.handle, None, host.ctypes.data, 2, o.data_ptr(), l_.data_ptr()),
           L.mlz_dev_reader_record_spans(h.rd.handle, None, d_idx.data_ptr(), 2, host.ctypes.data, l_.data_ptr()),
           L.mlz_dev_reader_record_spans(h.rd.handle, None, d_idx.data_ptr(), 2, o.data_ptr(), host.ctypes.data),
           L.mlz_dev_reader_record_spans(h.rd.handle, None, d_idx.data_ptr(), (1 << 31) + 1, o.data_ptr(), l_.data_ptr()),
           L.mlz_dev_reader_record_spans(h.rd.handle, None, None, 2, o.data_ptr(), l_.data_ptr()),
           L.mlz_dev_reader_record_spans(None, None, d_idx.data_ptr(), 2, o.data_ptr(), l_.data_ptr())]
    torch.cuda.synchronize()
    assert bad == [-MLZ_ERR_ARG] * len(bad) and (o == SENT).all() and (l_ == SENT).all()


def numbers_raw(h, pos):
    n = len(pos)
    d_pos, no = dev_u64(pos), guarded(n)
    r = _lib.lib().mlz_dev_reader_record_numbers(h.rd.handle, None, d_pos.data_ptr() if n else None, n, no.data_ptr())
    torch.cuda.synchronize()
    return r, no.cpu().numpy()


def test_record_numbers(plain):
    h, bs = plain
    start, length = IM.spans(h.data, NL)
    D = IM.delimiters(h.data, NL)
    size = len(h.data)
    pos = start[::7].tolist() + (start + np.maximum(length, 1) - 1)[::5].tolist() + D[::3].tolist() + [0, size - 1, size, size + 1, (1 << 63) + 5, (1 << 64) - 1]
    pos = np.asarray(pos, dtype=np.uint64)
    np.random.default_rng(3).shuffle(pos)
    want, inside = IM.numbers(h.data, NL, [int(p) for p in pos])
    r, no = numbers_raw(h, pos)
    assert r == inside == len(pos) - 4
    assert no[:len(pos)].view(np.uint64).tolist() == want and (no[len(pos):] == SENT).all()
    assert IM.NO_RECORD in want
    r, no = numbers_raw(h, [])
    assert r == 0 and (no == SENT).all()


NEEDLE = b"@zq-needle-77@"


def test_line_numbers_of_a_search(ctx):
    """search_records' d_rec_off through record_numbers: the line numbers of the matching lines, as grep -n counts them (0-based)."""
    bs = 64 << 10
    d = lines(bs * 6 + 300, 5)
    for at in (0, 2 * bs - 5, 3 * bs + 1000, 3 * bs + 1100, len(d) - len(NEEDLE)):
        d[at:at + len(NEEDLE)] = NEEDLE
    d = bytes(d)
    h = Indexed(ctx, gather(ctx, [d], bs, search_match_len=6), d)
    try:
        h.index()
        want = RM.result(d, NEEDLE, NL, 0, 64, 1 << 20)
        dst = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        off, st = guarded(64), guarded(65)
        R, totals, stats = h.rd.search_records(NEEDLE, NL, dst.data_ptr(), 1 << 20, off.data_ptr(), st.data_ptr(), None, 64)
        assert R == want["R"] >= 4 and stats[2] > 0
        no = guarded(R)
        assert h.rd.record_numbers(off.data_ptr(), R, no.data_ptr()) == R
        torch.cuda.synchronize()
        by_split = [i for i, ln in enumerate(d.split(NL)) if NEEDLE in ln]
        assert no.cpu().numpy()[:R].tolist() == IM.numbers(d, NL, want["rec_off"])[0] == by_split
    finally:
        h.close()


def test_lifecycle(ctx):
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    h = Indexed(ctx, s, d)
    L = _lib.lib()
    try:
        a, b, c = guarded(4), guarded(4), guarded(4)
        dst = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
        o, n = C.c_uint64(77), C.c_uint64(77)
        hd = h.rd.handle
        before = [L.mlz_dev_reader_record_count(hd), L.mlz_dev_reader_record_spans(hd, None, a.data_ptr(), 4, b.data_ptr(), c.data_ptr()),
                  L.mlz_dev_reader_read_records(hd, None, 0, a.data_ptr(), 4, dst.data_ptr(), 256, b.data_ptr()),
                  L.mlz_dev_reader_record_numbers(hd, None, a.data_ptr(), 4, b.data_ptr()), L.mlz_dev_reader_record_range(hd, 0, 0, C.byref(o), C.byref(n)),
                  L.mlz_dev_reader_record_spans(hd, None, None, 0, None, None), L.mlz_dev_reader_read_records(hd, None, 0, None, 0, None, 0, None)]
        torch.cuda.synchronize()
        assert before == [-MLZ_ERR_ARG] * len(before)
        assert (a == SENT).all() and (b == SENT).all() and (c == SENT).all() and (dst == 0x5A).all() and (o.value, n.value) == (77, 77)
        with pytest.raises(mz.MinLZError):
            h.rd.record_count()
        N, info = h.index()
        h.check_all_spans()
        N2, info2 = h.index(fresh=False)
        assert N2 == N and info2[:3] == info[:3]
        Nc, _ = h.index(b",")                  # another delimiter replaces the index
        assert Nc != N
        h.check_all_spans()
        h.index(b" ")
        h.check_all_spans()
        with pytest.raises(ValueError):
            h.rd.index_records(b"ab")
    finally:
        h.close()


def _data_chunks(stream):
    return [(c.off, c.clen) for c in CM.chunks(stream) if c.type in (0x01, 0x02, 0x03)]


def test_broken_chunks(ctx):
    """Verdicts on streams that the decoder refuses cleanly: a chunk's CRC, a chunk's body, the earlier one wins; the handle keeps its index."""
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    cs = _data_chunks(s)
    comp = [j for j, (_, t) in enumerate(SMod.data_grid(s)) if t == 0x02]
    a, z = comp[2], comp[-3]

    def crc_fault(b, j):
        b[cs[j][0] + 5] ^= 0x10

    def body_fault(b, j):
        for p in range(cs[j][0] + 12, cs[j][0] + 4 + cs[j][1]):
            t = bytearray(s)
            t[p] ^= 0xFF
            if CM.stream_verdict(bytes(t), len(d) + 16)[0] == 1:
                b[p] ^= 0xFF
                return
        raise AssertionError("no corrupting byte found")

    b = bytearray(s)
    crc_fault(b, a)
    h = Indexed(ctx, bytes(b), d)
    try:
        with pytest.raises(mz.ErrCRC):
            h.rd.index_records(NL)
        with pytest.raises(mz.MinLZError):
            h.rd.record_count()                      # nothing was kept of the failed build
        N, _ = h.index(ignore_crc=True)              # the same stream indexes under MLZ_STREAM_IGNORE_CRC
        with pytest.raises(mz.ErrCRC):
            h.rd.index_records(b",")
        assert h.rd.record_count() == N              # the earlier index is still answering
        h.check_all_spans()
        h.index(fresh=False)
    finally:
        h.close()
    for first, second, want in ((crc_fault, body_fault, mz.ErrCRC), (body_fault, crc_fault, mz.ErrCorrupt)):
        b = bytearray(s)
        first(b, a)
        second(b, z)
        h = Indexed(ctx, bytes(b), d)
        try:
            with pytest.raises(want):
                h.rd.index_records(NL)
        finally:
            h.close()


def test_record_range(plain):
    h, bs = plain
    start, length = IM.spans(h.data, NL)
    N = len(start)
    dst = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    for first, cnt in ((3, 9), (0, 1), (0, 0), (7, 0), (N - 4, 4), (N, 0), (N - 1, 1)):
        want = IM.record_range(h.data, NL, first, cnt)
        got = h.rd.record_range(first, cnt)
        assert got == want, (first, cnt)
        if got[1]:
            assert h.rd.read([(got[0], got[1], 0)], dst.data_ptr(), 1 << 16) == got[1]
            torch.cuda.synchronize()
            piece = dst[:got[1]].cpu().numpy().tobytes()
            assert piece == h.data[got[0]:got[0] + got[1]] and piece.count(NL) >= cnt - 1
    assert h.rd.record_range(3, 9)[1] > int(length[3:12].sum())      # the inner delimiters are included
    o, n = C.c_uint64(77), C.c_uint64(77)
    L = _lib.lib()
    bad = [L.mlz_dev_reader_record_range(h.rd.handle, N - 3, 4, C.byref(o), C.byref(n)), L.mlz_dev_reader_record_range(h.rd.handle, N + 1, 0, C.byref(o), C.byref(n)),
           L.mlz_dev_reader_record_range(h.rd.handle, 1, (1 << 64) - 1, C.byref(o), C.byref(n)), L.mlz_dev_reader_record_range(h.rd.handle, 0, 1, None, C.byref(n))]
    assert bad == [-MLZ_ERR_ARG] * 4 and (o.value, n.value) == (77, 77)


def test_device_stream(ctx):
    bs = 64 << 10
    d = plain_case(bs, 6)
    codec = shard.HipTensorCodec(ctx)
    t = torch.from_numpy(np.frombuffer(gather(ctx, [d], bs, search_match_len=6), np.uint8).copy()).cuda()
    with codec.open_stream(t) as ds:
        with pytest.raises(mz.MinLZError):
            ds.read_records(torch.tensor([0], dtype=torch.int64, device="cuda"))
        N = ds.index_records()
        assert N == IM.count(d, NL)[0]
        idx = [5, N - 1, 0, 5, 17]
        want, wst = IM.read(d, NL, idx)
        data, starts = ds.read_records(torch.tensor(idx, dtype=torch.int64, device="cuda"))
        assert data.cpu().numpy().tobytes() == want and starts.tolist() == wst
        data, starts = ds.read_records(torch.empty(0, dtype=torch.int64, device="cuda"))
        assert data.numel() == 0 and starts.tolist() == [0]
        pos = [0, 1, bs, len(d) - 1, len(d)]
        assert ds.line_numbers(torch.tensor(pos, dtype=torch.int64, device="cuda")).tolist() == [v if v != IM.NO_RECORD else NONE for v in IM.numbers(d, NL, pos)[0]]
        off, ln = IM.record_range(d, NL, 10, 6)
        assert ds.read_record_range(10, 6).cpu().numpy().tobytes() == d[off:off + ln]
        assert ds.read_record_range(4, 0).numel() == 0
        with pytest.raises(ValueError):
            ds.read_records([1, 2])
