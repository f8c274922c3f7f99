"""mlz_dev_reader_read_device (DeviceReader.read_device, DeviceStream.read_ranges with CUDA tensors): range reads whose offsets and lengths lie
in device memory and are planned by kernels.  The sentinel-band harness of tests/test_gpu_stream_device.py (an odd band in front of the stream,
a stale valid chunk and a band behind it, bands round the output) with bands round the two range arrays and round d_starts as well: after every
call the stream and the range arrays are unchanged and nothing outside d_dst[0, total) and d_starts[0, n] was written.  Expected bytes are
slices of the data the streams were made from, expected plans the brute-force model's (tests/stream_ranges_cases.py), and every read is
repeated through mlz_dev_reader_read with packed destinations: same bytes, same plan.

Left out, with the reason: a pointer on another device of a several-device context (-MLZ_ERR_ARG) needs two GPUs, these tests run on one (the
refusal of pointers that are on no device at all is tested)."""
import numpy as np
import pytest
import torch

import minlz_amd as mz
from minlz_amd import _lib, shard, synth
from tests import stream_device_cases as SC
from tests import stream_ranges_cases as RC
from tests.test_gpu_stream_device import BACK, FRONT, SENT, Dev, _host_len, _valid_cases
from tests.test_gpu_stream_ranges import _data_chunks, _selected_mutants
from tests.test_gpu_tile_levels import LEGS
from tests.test_stream_ranges_device_host import border_sets, extra_sets, packed

pytestmark = pytest.mark.gpu

MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 6, 8
AFRONT = 40   # the band in front of an array of 64-bit values (a multiple of 8: the values stay aligned)
MiB = 1 << 20


class Arr:
    """uint64 values in device memory between two bands."""

    def __init__(self, values=None, count=None):
        body = np.full(8 * count, SENT, np.uint8) if values is None else np.ascontiguousarray(values, dtype=np.uint64).view(np.uint8)
        self.image = np.concatenate([np.full(AFRONT, SENT, np.uint8), body, np.full(BACK, SENT, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()
        self.n = body.size // 8

    @property
    def ptr(self):
        return self.t.data_ptr() + AFRONT

    def get(self, what):
        """The values now; the bands must be intact."""
        a = self.t.cpu().numpy()
        assert (a[:AFRONT] == SENT).all() and (a[AFRONT + 8 * self.n:] == SENT).all(), what + ": bytes written outside the array"
        return a[AFRONT:AFRONT + 8 * self.n].view(np.uint64)

    def unchanged(self, what):
        assert np.array_equal(self.t.cpu().numpy(), self.image), what + ": a range array was modified"


def _read_dev(dv, rd, pairs, cap, what, ignore_crc=False):
    """One read into dv.out (filled with the band's byte first) -> (code, result, the cap bytes of the destination, d_starts as it is left)."""
    assert cap <= dv.cap
    p = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    off, ln, st = Arr(p[:, 0]), Arr(p[:, 1]), Arr(count=len(p) + 1)
    dv.out.fill_(SENT)
    torch.cuda.synchronize()
    try:
        code, got = 0, rd.read_device(off.ptr, ln.ptr, len(p), dv.dst, cap, d_starts=st.ptr, ignore_crc=ignore_crc)
    except mz.MinLZError as e:
        code, got = e.code or int(str(e).split()[2]), None
    o = dv.check(what)
    assert (o[cap:] == SENT).all(), what + ": bytes written behind dst_cap"
    off.unchanged(what); ln.unchanged(what)
    return code, got, o[:cap], st.get(what)


def _read_host(dv, rd, r, cap, what, ignore_crc=False):
    dv.out.fill_(SENT)
    got = rd.read(r, dv.dst, cap, ignore_crc=ignore_crc)
    return got, dv.check(what)[:cap]


SENT64 = np.frombuffer(bytes([SENT]) * 8, np.uint64)[0]


def _check_pairs(ctx, dv, rd, grid, d, name, pairs, ignore_crc=(False, True), model=True):
    r, total = packed(pairs)
    cap = total + 3
    want = RC.expected_image(d, r, cap)
    for ic in ignore_crc:
        what = "%s (ignore_crc=%s)" % (name, ic)
        code, got, o, starts = _read_dev(dv, rd, r[:, :2], cap, what, ic)
        assert code == 0 and got == total, what
        assert np.array_equal(o, want), what + ": bytes differ, or bytes behind the total were written"
        assert np.array_equal(starts, np.concatenate([r[:, 2], [total]]).astype(np.uint64)), what + ": d_starts"
        plan = ctx.range_plan()
        if model:
            touched, scratch = RC.model(grid, r)
            assert plan == (len(touched), scratch), what
        hgot, ho = _read_host(dv, rd, r, cap, what, ic)
        assert hgot == total and np.array_equal(ho, o) and ctx.range_plan() == plan, what + ": the host-planned read differs"


def _check_stream(ctx, name, s, d, extras=False, ignore_crc=(False, True)):
    grid = RC.chunk_grid(s)
    sets = [(rname, r[:, :2]) for rname, r, _ in RC.range_sets(grid)]
    if extras and len(d):
        sets += extra_sets(grid) + [("every_border", border_sets(grid))]
    dv = Dev(s, max(packed(p)[1] for _, p in sets) + 3)
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        assert rd.size == len(d) == _host_len(s)[0], name
        for rname, pairs in sets:
            _check_pairs(ctx, dv, rd, grid, d, "%s/%s" % (name, rname), pairs, ignore_crc)


def test_valid_streams_every_range_set(ctx):
    for name, s, d in _valid_cases(ctx):
        _check_stream(ctx, name, s, d, extras=name in ("oracle_L1_bs4096_idx0", "oracle_L1_bs8388608_idx0", "oracle_L2_bs1048576_idx0", "skippables", "two_streams",
                                                       "gpu_L2_bs65536_idx1", "gpu_L1_bs4096_idx0"))


def test_many_tiny_chunks_and_stored_chunks(ctx):
    s, d = SC.tiny_chunks()
    _check_stream(ctx, "tiny", s, d, extras=True)
    r = np.random.default_rng(11).integers(0, 256, 3 << 20, dtype=np.uint8).tobytes()
    st = mz.stream_encode(r, mz.LevelFastest, 64 << 10, False, ctx)
    assert all(t == 0x01 for _, t in RC.chunk_grid(st))
    _check_stream(ctx, "stored", st, r, extras=True, ignore_crc=(False,))


@pytest.mark.parametrize("leg,opts,counts", LEGS, ids=[l[0] for l in LEGS])
def test_option_legs(leg, opts, counts):
    c = mz.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        d = SC.data_mix()
        for name, s in (("L1", SC.oracle_stream(1 << 20, 1)), ("L2", SC.oracle_stream(1 << 20, 2)), ("gpu_L2", mz.stream_encode(d, mz.LevelBalanced, 1 << 20, False, c))):
            _check_stream(c, "%s_%s" % (leg, name), s, d, ignore_crc=(False,))
    finally:
        c.close()


def test_refusals_leave_everything_untouched(ctx):
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    size = len(d)
    ok = [(1000 * i % (size - 100), 7) for i in range(3000)]
    dv = Dev(s, 21010)
    L = _lib.lib()
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        for tag, pairs, cap, want in (("beyond_at_the_first_index", [(size - 5, 6)] + ok, 21006, MLZ_ERR_ARG),
                                      ("beyond_in_the_middle", ok[:1500] + [(size, 1)] + ok[1500:], 21001, MLZ_ERR_ARG),
                                      ("beyond_at_the_last_index", ok + [(0, size + 1)], 21000, MLZ_ERR_ARG),
                                      ("offset_minus_one", ok[:7] + [((1 << 64) - 1, 1)], 21000, MLZ_ERR_ARG),
                                      ("length_minus_one", [(5, (1 << 64) - 1)], 21000, MLZ_ERR_ARG),
                                      ("empty_range_beyond_the_end", [(size + 1, 0)], 21000, MLZ_ERR_ARG),
                                      ("total_is_cap_plus_one", ok, 20999, MLZ_ERR_DST_TOO_SMALL),
                                      ("cap_zero", [(0, 1)], 0, MLZ_ERR_DST_TOO_SMALL)):
            code, _, o, starts = _read_dev(dv, rd, pairs, cap, tag)
            assert code == want, tag
            assert (o == SENT).all() and (starts == SENT64).all(), tag + ": a refused call wrote"
            assert ctx.range_plan_host_bytes() == 32, tag
        code, got, o, starts = _read_dev(dv, rd, ok, 21000, "total_is_cap")
        r, total = packed(ok)
        assert code == 0 and got == total == 21000 and np.array_equal(o, RC.expected_image(d, r, 21000)) and starts[-1] == 21000
        # pointers that are not device memory, one at a time
        off, ln, st = Arr([3, 9]), Arr([10, 20]), Arr(count=3)
        host = np.full(64, SENT, np.uint8)
        hp = host.ctypes.data
        dv.out.fill_(SENT)
        for tag, args in (("d_off", (hp, ln.ptr, 2, dv.dst, 100, st.ptr)), ("d_len", (off.ptr, hp, 2, dv.dst, 100, st.ptr)), ("d_dst", (off.ptr, ln.ptr, 2, hp, 64, st.ptr)),
                          ("d_starts", (off.ptr, ln.ptr, 2, dv.dst, 100, hp))):
            assert L.mlz_dev_reader_read_device(rd.handle, None, 0, *args) == -MLZ_ERR_ARG, tag
            assert (host == SENT).all() and (dv.check(tag) == SENT).all() and (st.get(tag) == SENT64).all(), tag
        assert L.mlz_dev_reader_read_device(rd.handle, None, 0, None, ln.ptr, 2, dv.dst, 100, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_read_device(rd.handle, None, 0, off.ptr, ln.ptr, (1 << 31) + 1, dv.dst, 100, None) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_read_device(None, None, 0, off.ptr, ln.ptr, 2, dv.dst, 100, None) == -MLZ_ERR_ARG
        # nothing asked for
        assert rd.read_device(None, None, 0, None, 0) == 0 and ctx.range_plan_host_bytes() == 0
        assert rd.read_device(off.ptr, ln.ptr, 2, dv.dst, 30, d_starts=None) == 30 and dv.check("no_starts")[:30].tobytes() == d[3:13] + d[9:29]
        code, got, o, starts = _read_dev(dv, rd, [(5, 0), (size, 0)], 0, "empty_ranges_only")
        assert code == 0 and got == 0 and (starts == 0).all() and ctx.range_plan() == (0, 0)
    with pytest.raises(ValueError):
        rd.read_device(off.ptr, ln.ptr, 2, dv.dst, 30)   # a closed handle
    with ctx.stream_open_device(None, 0) as rd0:   # an empty stream
        z = Arr([0, 0])
        assert rd0.read_device(z.ptr, z.ptr, 2, None, 0) == 0
        one = Arr([0, 1])
        with pytest.raises(mz.MinLZError):
            rd0.read_device(z.ptr, one.ptr, 2, dv.dst, 10)


@pytest.mark.parametrize("bs", [1 << 20, 64 << 10])
def test_broken_chunks(ctx, bs):
    d = SC.data_mix()
    muts = _selected_mutants(bs)
    assert sum(1 for m in muts if m[2] == 5) >= 3 and sum(1 for m in muts if m[2] == 1) >= 1 and sum(1 for m in muts if m[2] == 0) >= 1
    for name, b, want, broken in muts:
        grid = RC.chunk_grid(b)
        starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
        dv = Dev(b, len(d) + 16)
        with ctx.stream_open_device(dv.src, dv.n) as rd:
            if broken is None:
                code, got, o, _ = _read_dev(dv, rd, [(0, len(d))], len(d), name)
                assert code == 0 and o.tobytes() == d, name
                continue
            b0, b1 = int(starts[broken]), int(starts[broken + 1])
            pairs = [(0, b0), (b1, len(d) - b1), (b1, 0)]   # everything but the broken chunk, up to its very borders
            r, total = packed(pairs)
            code, got, o, _ = _read_dev(dv, rd, pairs, total, name + "/avoid")
            assert code == 0 and got == total and np.array_equal(o, RC.expected_image(d, r, total)), name
            for tag, pairs in (("one_byte", [((b0 + b1) // 2, 1)]), ("first_byte_and_more", [(0, 10), (b0, 1), (len(d) - 10, 10)]), ("whole", [(0, len(d))])):
                code = _read_dev(dv, rd, pairs, len(d) + 16, "%s/%s" % (name, tag))[0]
                try:
                    hcode = 0
                    rd.read(packed(pairs)[0], dv.dst, len(d) + 16)
                except mz.MinLZError as e:
                    hcode = e.code or int(str(e).split()[2])
                assert code == hcode == want, "%s/%s: device-planned %d, host-planned %d, the oracle's Reader %d" % (name, tag, code, hcode, want)


def test_two_broken_chunks_the_earlier_one_wins(ctx):
    from tests import corrupt as CM
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    cs = _data_chunks(s)
    grid = RC.chunk_grid(s)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
    comp = [j for j, (_, t) in enumerate(grid) if t == 0x02]
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

    for first, second, want in ((crc_fault, body_fault, 5), (body_fault, crc_fault, 1)):
        b = bytearray(s)
        first(b, a)
        second(b, z)
        b = bytes(b)
        dv = Dev(b, 4096)
        ra, rz = (int(starts[a]) + 100, 50), (int(starts[z]) + 100, 50)
        with ctx.stream_open_device(dv.src, dv.n) as rd:
            for pairs in ([ra, rz], [rz, ra]):
                assert _read_dev(dv, rd, pairs, 100, "two_faults")[0] == want
            assert _read_dev(dv, rd, [ra], 100, "first_alone")[0] == want
            assert _read_dev(dv, rd, [rz], 100, "second_alone")[0] == (1 if want == 5 else 5)
            mid = (int(starts[a + 1]) + 1, 4000)
            code, got, o, _ = _read_dev(dv, rd, [mid], 4000, "between")
            assert code == 0 and o.tobytes() == d[mid[0]:mid[0] + 4000]


def test_plan_bytes_do_not_depend_on_the_number_of_ranges(ctx):
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    grid = RC.chunk_grid(s)
    assert len(grid) >= 16 and grid[5][1] != 0x01
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
    rng = np.random.default_rng(2)
    dv = Dev(s, max(len(d), 50 * 100_000) + 8)
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        assert _read_dev(dv, rd, [(0, 10)], 10, "warm_up")[0] == 0   # (the handle's chunk table goes up here)
        seen = []
        for k in (1000, 100_000):
            offs = starts[5] + rng.integers(0, grid[5][0] - 60, k)
            pairs = np.stack([offs, np.full(k, 50)], axis=1)
            r, total = packed(pairs)
            code, got, o, st = _read_dev(dv, rd, pairs, total, "%d_in_one_chunk" % k)
            assert code == 0 and got == 50 * k and np.array_equal(o, RC.expected_image(d, r, total))
            assert ctx.range_plan() == (1, grid[5][0])
            seen.append(ctx.range_plan_host_bytes())
        assert seen[0] == seen[1] and 0 < seen[0] < 24 * 1000, seen
        code, got, o, _ = _read_dev(dv, rd, [(1, len(d) - 2)], len(d) - 2, "all_chunks")
        assert code == 0 and o.tobytes() == d[1:-1] and ctx.range_plan() == (len(grid), grid[0][0] + grid[-1][0])
        assert ctx.range_plan_host_bytes() > seen[0]
        assert ctx.workspace_bytes()[1] >= 16 * 100_000   # the plan's workspace is counted


def test_codec_read_ranges_with_cuda_tensors(ctx):
    d = SC.data_mix()
    codec = shard.HipTensorCodec(ctx)
    s = SC.oracle_stream(64 << 10, 1, True)
    t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    rng = np.random.default_rng(4)
    offs = [3_000_000, 5, 70_000, 5, 0] + rng.integers(0, len(d) - 600, 500).tolist()
    lens = [100, 70_000, 1, 10, 0] + rng.integers(0, 600, 500).tolist()
    want = b"".join(d[a:a + n] for a, n in zip(offs, lens))
    with codec.open_stream(t) as ds:
        ref = ds.read_ranges(offs, lens)
        assert ref.cpu().numpy().tobytes() == want
        for dt in (torch.int64, torch.uint64):
            to = torch.tensor(offs, dtype=torch.int64).to(dt).cuda()
            tl = torch.tensor(lens, dtype=torch.int64).to(dt).cuda()
            o = ds.read_ranges(to, tl)
            assert o.device == t.device and o.dtype == torch.uint8 and torch.equal(o, ref), dt
            o, st = ds.read_ranges(to, tl, return_starts=True)
            assert torch.equal(o, ref) and st.dtype == torch.int64 and st.device == t.device
            assert st.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
            assert ctx.range_plan_host_bytes() > 0
        o, st = ds.read_ranges(offs, lens, return_starts=True)     # the host path hands the same starts back
        assert torch.equal(o, ref) and st.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        # tensors on the CPU keep the host path
        assert ds.read_ranges(torch.tensor([], dtype=torch.int64).cuda(), torch.tensor([], dtype=torch.int64).cuda()).numel() == 0
        assert ctx.range_plan_host_bytes() == 0
        o = ds.read_ranges(torch.tensor(offs), torch.tensor(lens))
        assert torch.equal(o, ref) and ctx.range_plan_host_bytes() == 0
        with pytest.raises(mz.MinLZError) as e:
            ds.read_ranges(torch.tensor([5, -1, 7]).cuda(), torch.tensor([1, 1, 1]).cuda())
        assert "error %d" % MLZ_ERR_ARG in str(e.value)
        with pytest.raises(mz.MinLZError) as e:
            ds.read_ranges(torch.tensor([5, 6]).cuda(), torch.tensor([1, -1]).cuda())
        assert "error %d" % MLZ_ERR_ARG in str(e.value)
        with pytest.raises(ValueError):
            ds.read_ranges(torch.tensor([5, 6], dtype=torch.int32).cuda(), torch.tensor([1, 1], dtype=torch.int32).cuda())


def test_several_groups():
    """136 MiB in 8 MiB blocks: 17 chunks, three groups under the 64 MiB rule."""
    n = 136 * MiB
    a = synth.enwik_like(n, seed=6)
    d = a.tobytes()
    c, cb = mz.Context(0), mz.Context(0)
    try:
        s = mz.stream_encode(d, mz.LevelFastest, 8 << 20, False, c)
        grid = RC.chunk_grid(s)
        assert len(grid) == 17 and all(t != 0x01 for _, t in grid)
        rng = np.random.default_rng(8)
        short = lambda k: list(zip(rng.integers(0, n - 600, k).tolist(), rng.integers(1, 600, k).tolist()))
        b1, b2 = 64 * MiB, 128 * MiB
        straddle = [(b1 - 3, 7), (b2 - 1, 2), (b1 - 70_000, 140_001), (b2 - 2000, 2100), (b1, 1), (b1 - 1, 1)]
        lists = (("everything_and_2000_short", short(1000) + [(0, n)] + short(1000), (17, n)),
                 ("20000_short", short(20_000), None),
                 ("straddling_the_group_borders", straddle, (4, 32 * MiB)),
                 ("straddling_with_every_chunk_touched", straddle[:3] + [(0, n)] + straddle[3:], (17, 32 * MiB)))   # (here the borders ARE group borders)
        dv = Dev(s, n + 2 * MiB)
        with c.stream_open_device(dv.src, dv.n) as rd:
            for name, pairs, plan in lists:
                r, total = packed(pairs)
                code, got, o, st = _read_dev(dv, rd, pairs, total, name)
                assert code == 0 and got == total, name
                want = np.concatenate([a[o_:o_ + l_] for o_, l_ in pairs])
                assert np.array_equal(o, want), name
                assert np.array_equal(st, np.concatenate([r[:, 2], [total]]).astype(np.uint64)), name
                got_plan = c.range_plan()
                assert plan is None or got_plan == plan, name
                o = o.copy()
                hgot, ho = _read_host(dv, rd, r, total, name)
                assert hgot == total and np.array_equal(ho, o) and c.range_plan() == got_plan, name + ": the host-planned read differs"
        # the scratch is reused from group to group: a context that put all 136 MiB through it holds no more workspace than one that put a single
        # group (the first 8 chunks = 64 MiB, touched by two ranges each) through it, but for the plan's 16 bytes per range
        dvb = Dev(s, 2 * b1)
        with cb.stream_open_device(dvb.src, dvb.n) as rd:
            code, got, o, _ = _read_dev(dvb, rd, [(0, b1), (1, b1 - 1)], 2 * b1 - 1, "one_group")
            assert code == 0 and cb.range_plan() == (8, b1)
        assert c.workspace_bytes()[1] <= cb.workspace_bytes()[1] + MiB, (c.workspace_bytes(), cb.workspace_bytes())
    finally:
        c.close(); cb.close()
