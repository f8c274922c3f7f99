"""The device-resident ReadSeeker (mlz_stream_open_device, mlz_dev_reader_read, HipTensorCodec.open_stream): range reads of streams that lie
in HBM, with the sentinel-band harness of tests/test_gpu_stream_device.py: an odd band in front of the stream, a stale valid chunk and a band
behind it, bands round the output; after every call the input is unchanged and nothing outside the ranges' destinations was written (the
output is filled with the band's byte before a call, so gaps between destinations are checked with the bands).  Expected bytes are slices of
the data the oracle's streams were made from; expected plans are the brute-force model's (tests/stream_ranges_cases.py).

Left out, with the reason: a d_dst on another device of a several-device context (-MLZ_ERR_ARG) needs two GPUs, these tests run on one
(the refusal of a pointer that is on no device at all is tested); body mutants under ignore_crc (the destination of a failed read is
unspecified and a body fault fails either way)."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard
from tests import corrupt as CM
from tests import stream_device_cases as SC
from tests import stream_ranges_cases as RC
from tests.test_gpu_stream_device import BACK, FRONT, SENT, Dev, _host_len, _valid_cases
from tests.test_gpu_tile_levels import LEGS

pytestmark = pytest.mark.gpu

MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 6, 8
assert RC.FILL == SENT


def _read(dv, rd, ranges, cap, what, ignore_crc=False):
    """One read into dv.out (filled with the band's byte first) -> (code, result, the cap bytes of the destination)."""
    assert cap <= dv.cap
    dv.out.fill_(SENT)
    try:
        code, got = 0, rd.read(ranges, dv.dst, cap, ignore_crc=ignore_crc)
    except mz.MinLZError as e:
        code, got = e.code or int(str(e).split()[2]), None
    o = dv.check(what)
    assert (o[cap:] == SENT).all(), what + ": bytes written behind dst_cap"
    return code, got, o[:cap]


def _check_sets(ctx, name, s, d, sets=None, ignore_crc=(False, True), plans=True):
    grid = RC.chunk_grid(s)
    sets = RC.range_sets(grid) if sets is None else sets
    dv = Dev(s, max(cap for _, _, cap in sets) + 3)
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        assert rd.size == len(d) == _host_len(s)[0], name
        for rname, ranges, cap in sets:
            want = RC.expected_image(d, ranges, cap)
            for ic in ignore_crc:
                what = "%s/%s (ignore_crc=%s)" % (name, rname, ic)
                code, got, o = _read(dv, rd, ranges, cap, what, ic)
                assert code == 0 and got == int(ranges[:, 1].sum()), what
                assert np.array_equal(o, want), what + ": bytes differ, or a gap between destinations was written"
            if plans:
                touched, scratch = RC.model(grid, ranges)
                assert ctx.range_plan() == (len(touched), scratch), "%s/%s" % (name, rname)


def test_valid_streams_every_range_set(ctx):
    for name, s, d in _valid_cases(ctx):
        _check_sets(ctx, name, s, d)


def test_many_tiny_chunks_and_stored_chunks(ctx):
    s, d = SC.tiny_chunks()
    _check_sets(ctx, "tiny", s, d, ignore_crc=(False,))
    r = np.random.default_rng(11).integers(0, 256, 3 << 20, dtype=np.uint8).tobytes()
    st = mz.stream_encode(r, mz.LevelFastest, 64 << 10, False, ctx)
    assert all(t == 0x01 for _, t in RC.chunk_grid(st))
    _check_sets(ctx, "stored", st, r, ignore_crc=(False,))


def _R(*rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 3)


def test_counters(ctx):
    d = SC.data_mix()
    s = SC.oracle_stream(64 << 10)
    grid = RC.chunk_grid(s)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
    dv = Dev(s, len(d) + 8)
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        # 1 000 ranges inside one chunk: it is decoded once
        rng = np.random.default_rng(2)
        offs = starts[5] + rng.integers(0, grid[5][0] - 60, 1000)
        r = np.stack([offs, np.full(1000, 50), np.arange(1000) * 50], axis=1).astype(np.uint64)
        code, got, o = _read(dv, rd, r, 50_000, "one_chunk")
        assert code == 0 and got == 50_000 and np.array_equal(o, RC.expected_image(d, r, 50_000))
        assert grid[5][1] != 0x01 and ctx.range_plan() == (1, grid[5][0])
        # the whole stream as one range: every chunk straight into its place
        code, got, o = _read(dv, rd, _R((0, len(d), 0)), len(d), "whole")
        assert code == 0 and o.tobytes() == d
        assert ctx.range_plan() == (sum(1 for n, _ in grid if n), 0)
        # all but the first and the last byte: the two edge chunks go through the scratch
        code, got, o = _read(dv, rd, _R((1, len(d) - 2, 0)), len(d) - 2, "all_but_the_ends")
        assert code == 0 and o.tobytes() == d[1:-1]
        assert grid[0][1] != 0x01 and grid[-1][1] != 0x01
        assert ctx.range_plan() == (len(grid), grid[0][0] + grid[-1][0])
        # ranges inside stored chunks only (the random bytes of the mix): nothing is decoded, nothing visits the scratch
        stored = [j for j, (n, t) in enumerate(grid) if t == 0x01]
        assert len(stored) >= 10 and all((2 << 20) <= starts[j] < (3 << 20) + 300_000 for j in stored)
        rows, pos = [], 0
        for j in stored[:8]:
            rows += [(int(starts[j]) + 7, 1000, pos), (int(starts[j]), grid[j][0], pos + 1000)]
            pos += 1000 + grid[j][0]
        r = _R(*rows)
        code, got, o = _read(dv, rd, r, pos, "stored_only")
        assert code == 0 and np.array_equal(o, RC.expected_image(d, r, pos))
        assert ctx.range_plan() == (8, 0)
    # a stream of one chunk (the mix at 8 MiB blocks): counted once
    s8 = SC.oracle_stream(8 << 20)
    assert len(RC.chunk_grid(s8)) == 1
    dv = Dev(s8, len(d))
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        code, got, o = _read(dv, rd, _R((1, len(d) - 2, 0)), len(d) - 2, "single_chunk")
        assert code == 0 and o.tobytes() == d[1:-1] and ctx.range_plan() == (1, len(d))


@pytest.mark.parametrize("leg,opts,counts", LEGS, ids=[l[0] for l in LEGS])
def test_option_legs(leg, opts, counts):
    c = mz.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        d = SC.data_mix()
        for name, s in (("L1", SC.oracle_stream(1 << 20, 1)), ("L2", SC.oracle_stream(1 << 20, 2)), ("gpu_L2", mz.stream_encode(d, mz.LevelBalanced, 1 << 20, False, c))):
            sets = {n: (n, r, cap) for n, r, cap in RC.range_sets(RC.chunk_grid(s))}
            _check_sets(c, "%s_%s" % (leg, name), s, d, sets=[sets["whole"], sets["nested_and_overlapping"], sets["borders"]], ignore_crc=(False,))
    finally:
        c.close()


def _data_chunks(s):
    """(header offset, chunk length) of the data chunks, in order."""
    return [(c.off, c.clen) for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]


def _selected_mutants(bs):
    """stream_mutants whose framing the host Reader's walk accepts: (name, bytes, the oracle's code, index of the broken data chunk or None)."""
    s, d = SC.oracle_stream(bs), SC.data_mix()
    cs = _data_chunks(s)
    out = []
    for name, b in CM.stream_mutants(s):
        if _host_len(b)[0] < 0:
            continue
        want = CM.stream_verdict(b, len(d) + 16)[0]
        broken = None
        if want:
            p = next(i for i in range(min(len(s), len(b))) if s[i] != b[i])
            broken = max(j for j, (off, _) in enumerate(cs) if off <= p)
            assert p < cs[broken][0] + 4 + cs[broken][1], name
        out.append((name, b, want, broken))
    return out


@pytest.mark.parametrize("bs", [1 << 20, 64 << 10])
def test_broken_chunks(ctx, bs):
    d = SC.data_mix()
    muts = _selected_mutants(bs)
    assert sum(1 for m in muts if m[2] == 5) >= 3 and sum(1 for m in muts if m[2] == 1) >= 1 and sum(1 for m in muts if m[2] == 0) >= 1
    for name, b, want, broken in muts:
        assert _host_len(b)[0] == len(d), name
        grid = RC.chunk_grid(b)
        starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
        dv = Dev(b, len(d) + 16)
        with ctx.stream_open_device(dv.src, dv.n) as rd:
            assert rd.size == len(d)
            if broken is None:
                code, got, o = _read(dv, rd, _R((0, len(d), 5)), len(d) + 5, name)
                assert code == 0 and o[5:].tobytes() == d, name
                continue
            b0, b1 = int(starts[broken]), int(starts[broken + 1])
            # everything but the broken chunk, up to its very borders
            r = _R((0, b0, 3), (b1, len(d) - b1, b0 + 3 + 2))
            code, got, o = _read(dv, rd, r, len(d) + 16, name + "/avoid")
            assert code == 0 and np.array_equal(o, RC.expected_image(d, r, len(d) + 16)), name
            for tag, r in (("one_byte", _R(((b0 + b1) // 2, 1, 0))), ("first_byte_and_more", _R((0, 10, 0), (b0, 1, 50), (len(d) - 10, 10, 20))), ("whole", _R((0, len(d), 0)))):
                code, _, _ = _read(dv, rd, r, len(d) + 16, "%s/%s" % (name, tag))
                assert code == want, "%s/%s: read %d, the oracle's Reader %d" % (name, tag, code, want)
            if want == 5 and name.startswith(("crc_", "type_03")):   # a wrong CRC (or a 0x02 chunk retyped 0x03): the bytes are fine
                r = _R((b0 + 1, b1 - b0 - 1, 0), (0, 7, b1 - b0))
                code, got, o = _read(dv, rd, r, len(d), name + "/ignore_crc", ignore_crc=True)
                assert code == 0 and np.array_equal(o, RC.expected_image(d, r, len(d))), name


def test_two_broken_chunks_the_earlier_one_wins(ctx):
    s, d = SC.oracle_stream(64 << 10), SC.data_mix()
    cs = _data_chunks(s)
    grid = RC.chunk_grid(s)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])])
    comp = [j for j, (_, t) in enumerate(grid) if t == 0x02]
    a, z = comp[2], comp[-3]

    def crc_fault(b, j):
        b[cs[j][0] + 5] ^= 0x10

    def body_fault(b, j):
        # a token byte whose change the oracle calls corrupt (not merely other bytes with a wrong CRC)
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
        assert CM.stream_verdict(b, len(d) + 16)[0] == want and _host_len(b)[0] == len(d)
        dv = Dev(b, 4096)
        ra, rz = (int(starts[a]) + 100, 50, 0), (int(starts[z]) + 100, 50, 50)
        with ctx.stream_open_device(dv.src, dv.n) as rd:
            for r in (_R(ra, rz), _R((rz[0], 50, 0), (ra[0], 50, 50))):
                assert _read(dv, rd, r, 100, "two_faults")[0] == want
            # each alone gives its own code; between them all is well
            assert _read(dv, rd, _R(ra), 100, "first_alone")[0] == want
            assert _read(dv, rd, _R(rz), 100, "second_alone")[0] == (1 if want == 5 else 5)
            mid = _R((int(starts[a + 1]), int(starts[z] - starts[a + 1]), 0))
            dv2 = Dev(b, int(mid[0, 1]))
            with ctx.stream_open_device(dv2.src, dv2.n) as rd2:
                code, got, o = _read(dv2, rd2, mid, int(mid[0, 1]), "between")
                assert code == 0 and o.tobytes() == d[int(mid[0, 0]):int(mid[0, 0] + mid[0, 1])]


def test_framing_errors_get_no_handle(ctx):
    s = SC.oracle_stream(1 << 20)
    L = _lib.lib()
    seen = set()
    for name, b in CM.stream_mutants(s):
        want = _host_len(b)[0]
        if want >= 0:
            continue
        dv = Dev(b, 16)
        h = C.c_void_p(0xDEAD)
        r = L.mlz_stream_open_device(ctx.handle, None, dv.src, dv.n, C.byref(h))
        assert r == want and not h.value, "%s: open %d, the host Reader's walk %d" % (name, r, want)
        dv.check(name)
        with pytest.raises(mz.MinLZError):
            ctx.stream_open_device(dv.src, dv.n)
        seen.add(want)
    assert seen >= {-1, -2, -3}
    h = C.c_void_p(0xDEAD)
    hb = np.frombuffer(s, np.uint8).copy()
    c2 = mz.Context(devices=[0, 0])
    try:   # a pointer that no device of the context holds
        assert L.mlz_stream_open_device(c2.handle, None, hb.ctypes.data, hb.size, C.byref(h)) == -MLZ_ERR_ARG and not h.value
        dv = Dev(s, 100)
        with c2.stream_open_device(dv.src, dv.n) as rd:   # and one it does
            assert _read(dv, rd, _R((5, 100, 0)), 100, "two_contexts")[2].tobytes() == SC.data_mix()[5:105]
    finally:
        c2.close()


def test_argument_errors_leave_the_output_untouched(ctx):
    s, d = SC.oracle_stream(1 << 20), SC.data_mix()
    dv = Dev(s, 5000)
    with ctx.stream_open_device(dv.src, dv.n) as rd:
        for tag, r, cap, want in (("beyond_the_end", _R((0, 10, 0), (len(d) - 5, 6, 10)), 5000, MLZ_ERR_ARG),
                                  ("offset_beyond_the_end", _R((len(d) + 1, 0, 0)), 5000, MLZ_ERR_ARG),
                                  ("destinations_overlap", _R((0, 100, 0), (5000, 100, 99)), 5000, MLZ_ERR_ARG),
                                  ("dst_too_small", _R((0, 100, 0), (5000, 100, 4901)), 5000, MLZ_ERR_DST_TOO_SMALL),
                                  ("dst_cap_zero", _R((0, 1, 0)), 0, MLZ_ERR_DST_TOO_SMALL)):
            code, _, o = _read(dv, rd, r, cap, tag)
            assert code == want and (o == SENT).all(), tag
        host = np.full(5000, SENT, np.uint8)
        with pytest.raises(mz.MinLZError) as e:
            rd.read(_R((0, 100, 0)), host.ctypes.data, 5000)
        assert "error %d" % MLZ_ERR_ARG in str(e.value) and (host == SENT).all()
        # nothing asked for: any destination will do
        assert rd.read(_R((3, 0, 0)), None, 0) == 0 and rd.read(_R(), None, 0) == 0
        code, got, o = _read(dv, rd, _R((0, 100, 4900)), 5000, "fits")
        assert code == 0 and o[4900:].tobytes() == d[:100] and (o[:4900] == SENT).all()
    L = _lib.lib()
    assert L.mlz_dev_reader_size(None) == -MLZ_ERR_ARG and L.mlz_dev_reader_read(None, None, 0, None, 0, None, 0) == -MLZ_ERR_ARG
    L.mlz_dev_reader_close(None)
    with ctx.stream_open_device(None, 0) as rd:   # no bytes at all: an empty stream
        assert rd.size == 0 and rd.read(_R((0, 0, 0)), None, 0) == 0


def test_codec_open_stream(ctx):
    d = SC.data_mix()
    codec = shard.HipTensorCodec(ctx)
    for s in (SC.oracle_stream(64 << 10, 1, True), mz.stream_encode(d, mz.LevelBalanced, 1 << 20, False, ctx)):
        t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
        with codec.open_stream(t) as ds:
            assert ds.size == len(d)
            o = ds.ReadAt(1000, 123_457)
            assert o.device == t.device and o.dtype == torch.uint8 and o.cpu().numpy().tobytes() == d[123_457:124_457]
            assert ds.ReadAt(1000, len(d) - 10).cpu().numpy().tobytes() == d[-10:]      # clamped at the end
            assert ds.ReadAt(5, len(d)).numel() == 0 and ds.ReadAt(0, 7).numel() == 0
            with pytest.raises(ValueError):
                ds.ReadAt(1, len(d) + 1)
            offs, lens = [3_000_000, 5, 70_000, 5], [100, 70_000, 1, 10]
            o = ds.read_ranges(offs, lens)
            assert o.cpu().numpy().tobytes() == b"".join(d[a:a + n] for a, n in zip(offs, lens))     # packed in the order given
            assert ds.read_ranges([], []).numel() == 0
    bad = bytearray(SC.oracle_stream(1 << 20))
    bad[-3] ^= 0x04     # the EOF chunk's size
    with pytest.raises(mz.MinLZError):
        codec.open_stream(torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda())
    with codec.open_stream(torch.from_numpy(np.frombuffer(O.stream_encode(b"", 1, 1 << 20), np.uint8).copy()).cuda()) as ds:
        assert ds.size == 0 and ds.ReadAt(10, 0).numel() == 0


def test_handle_survives_other_calls_on_its_context(ctx):
    d = SC.data_mix()
    s1, s2 = SC.oracle_stream(64 << 10), SC.oracle_stream(1 << 20, 2)
    sets = {n: (n, r, cap) for n, r, cap in RC.range_sets(RC.chunk_grid(s1))}
    pick = [sets["nested_and_overlapping"], sets["borders"], sets["ten_thousand_short_shuffled"]]
    dv1, dv2 = Dev(s1, max(cap for _, _, cap in pick)), Dev(s2, len(d))
    with ctx.stream_open_device(dv1.src, dv1.n) as r1, ctx.stream_open_device(dv2.src, dv2.n) as r2:
        for rname, ranges, cap in pick:
            assert np.array_equal(_read(dv1, r1, ranges, cap, rname)[2], RC.expected_image(d, ranges, cap))
        assert ctx.stream_decode_device(dv2.src, dv2.n, dv2.dst, dv2.cap) == len(d)          # the whole-stream call: walk tables and workspace change hands
        assert dv2.check("whole")[:len(d)].tobytes() == d
        blocks = [O.encode(d[i:i + (300 << 10)], 1) for i in range(0, 3 << 20, 300 << 10)]
        assert b"".join(bytes(x) for x in mz.decode_batch(blocks, ctx)) == d[:len(blocks) * (300 << 10)]   # a batch call
        for rname, ranges, cap in pick:
            assert np.array_equal(_read(dv1, r1, ranges, cap, rname + "_again")[2], RC.expected_image(d, ranges, cap))
        code, got, o = _read(dv2, r2, _R((1, len(d) - 2, 0)), len(d) - 2, "other_handle")
        assert code == 0 and o.tobytes() == d[1:-1]
