"""mlz_dev_reader_extract_sidecar on the device (include/minlz_hip_sidecar_extract.h; DeviceReader.extract_sidecar, DeviceStream.extract_sidecar)
against tests/sidecar_extract_model.py, the reference's ExtractSidecar in plain Python: both modes byte for byte and count for count between
sentinels, the searches through the extracted sidecar against the same searches through the inline tables, and the refusals, which write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, api, shard, synth
from tests import search_model as SMod
from tests import sidecar_extract_cases as XC
from tests import sidecar_extract_model as XM
from tests import sidecar_model as SM
from tests.search_gpu import SENT, Opened, dev_u8, gather

pytestmark = pytest.mark.gpu

MLZ_ERR_CORRUPT, MLZ_ERR_UNSUPPORTED, MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 1, 3, 6, 8
BS = 64 << 10
GUARD = 64
NON_ALNUM = bytes(v for v in range(256) if not chr(v).isalnum())


def writer_stream(ctx, d, bs, **kw):
    return gather(ctx, [d], bs, **kw)


def build_case(ctx, name):
    """-> (stream, decoded bytes)"""
    if name == "300 blocks of 4 KiB":
        d = synth.json_like(300 * (4 << 10) - 100, 8).tobytes()
        return writer_stream(ctx, d, 4 << 10, search_match_len=6), d
    if name == "compressed and plain tables":
        d = XC.mixed_compress_data(BS)
        return writer_stream(ctx, d, BS, search_match_len=6, search_compress=True), d
    if name in ("type 2", "type 3", "type 4"):
        d = synth.json_like(5 * BS + 300, 9).tobytes()
        kw = {"type 2": dict(search_prefix=b'":, '), "type 3": dict(search_prefix=NON_ALNUM), "type 4": dict(search_long_prefix=b'"user":"', search_extras=3)}[name]
        return writer_stream(ctx, d, BS, add_index=(name == "type 3"), search_match_len=6, **kw), d
    if name == "no tables":
        d = synth.text_like(6 * BS + 17, 10).tobytes()
        return writer_stream(ctx, d, BS), d
    if name == "hand framed":
        return XC.hand_framed()
    assert name == "header and EOF"
    return XC.HEADER_AND_EOF, b""


CASES = ["300 blocks of 4 KiB", "compressed and plain tables", "type 2", "type 3", "type 4", "no tables", "hand framed", "header and EOF"]
_built = {}


def case(ctx, name):
    if name not in _built:
        _built[name] = build_case(ctx, name)
    return _built[name]


class Extracting(Opened):
    """An opened stream; extract into sentinel-filled room with a guard band behind it."""

    def raw(self, side_cap, main_cap, strip, flags=0, side_ptr=None):
        side = torch.full((side_cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        main = torch.full((main_cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        out = _lib.SidecarExtractResult()
        r = _lib.lib().mlz_dev_reader_extract_sidecar(self.rd.handle, None, flags, side.data_ptr() if side_ptr is None else side_ptr, side_cap,
                                                      main.data_ptr() if strip else None, main_cap if strip else 0, C.byref(out))
        torch.cuda.synchronize()
        s, m = side.cpu().numpy(), main.cpu().numpy()
        res = api.SidecarExtract(*(int(getattr(out, f)) for f in api.SidecarExtract._fields))
        if r < 0:
            assert (s == 0x5A).all() and (m == 0x5A).all(), "a refused call wrote"
            return r, None, None, res
        assert r == res.side_len <= side_cap and res.main_len <= main_cap
        assert (s[res.side_len:] == 0x5A).all() and (m[res.main_len if strip else 0:] == 0x5A).all(), "written behind the result"
        return r, s[:res.side_len].tobytes(), m[:res.main_len].tobytes() if strip else None, res

    def bound(self):
        return self.rd.extract_sidecar_bound()


def searches(h, pats, cap=1 << 14):
    """search of every pattern and one search_many over all -> what they return (positions, counts), and the chunks each search decoded."""
    out, decoded = [], []
    for p in pats:
        o = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = h.rd.search(p, o.data_ptr(), cap)
        torch.cuda.synchronize()
        o = o.cpu().numpy()
        assert (o[min(total, cap):] == SENT).all()
        out.append((total, o[:min(total, cap)].tolist()))
        decoded.append(h.ctx.counter(api.COUNTER_SEARCH_CHUNKS))
    pos = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
    which = torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((len(pats) + 8,), SENT, dtype=torch.int64, device="cuda")
    total, stats = h.rd.search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), cap)
    torch.cuda.synchronize()
    k = min(total, cap)
    out.append((total, pos.cpu().numpy()[:k].tolist(), which.cpu().numpy()[:k].tolist(), counts.cpu().numpy()[:len(pats)].tolist()))
    decoded.append(h.ctx.counter(api.COUNTER_SEARCH_CHUNKS))
    return out, decoded


# ---- both modes are the model's, byte for byte and count for count ----

@pytest.mark.parametrize("name", CASES)
def test_extract_equals_the_model(ctx, name):
    """Every case in both modes with the bound's room and with exactly the result's: the sidecar, the stripped main and *out are the model's;
    nothing is written behind them; IGNORE_CRC changes nothing; and a capacity one byte short, each side alone, is refused with the sizes
    needed in *out and not a byte written."""
    stream, d = case(ctx, name)
    kinds = [t for _, t, _ in SMod.chunks_of(stream)]
    if name == "300 blocks of 4 KiB":
        offs = [p for p, _ in SM.main_chunks(stream)]
        # (the references' offsets cross 2^14 in both modes; 2^21 lies beyond a stream of this size: tools/sidecar_extract_check.cpp crosses it)
        assert len(offs) == 300 and offs[1] < 1 << 14 < offs[-1] and kinds.count(0x45) > 290
    if name == "compressed and plain tables":
        assert 0 < kinds.count(0x46) and 0 < kinds.count(0x45)
    if name == "hand framed":
        assert {0x01, 0x02, 0x40, 0x47, 0x80, 0xFE} <= set(kinds) and kinds.count(0xFE) > 300
    h = Extracting(ctx, stream)
    try:
        side_bound, main_bound = h.bound()
        for strip in (False, True):
            want_side, want_main, want = XM.extract(stream, strip)
            assert want.side_len <= side_bound and want.main_len <= main_bound, "the bound does not suffice"
            for side_cap, main_cap, flags in ((side_bound, main_bound, 0), (want.side_len, max(want.main_len, 1), api.STREAM_IGNORE_CRC)):
                r, side, main, got = h.raw(side_cap, main_cap, strip, flags)
                assert r == want.side_len and got == want, (name, strip)
                assert side == want_side, (name, strip, XC.first_difference(side, want_side))
                assert main == want_main, (name, strip, XC.first_difference(main or b"", want_main or b""))
            r, _, _, got = h.raw(want.side_len - 1, main_bound, strip)
            assert r == -MLZ_ERR_DST_TOO_SMALL and (got.side_len, got.main_len) == (want.side_len, want.main_len)
            if strip:
                r, _, _, got = h.raw(side_bound, want.main_len - 1, strip)
                assert r == -MLZ_ERR_DST_TOO_SMALL and (got.side_len, got.main_len) == (want.side_len, want.main_len)
        if name == "compressed and plain tables":
            assert 0 < want.tables_compressed < want.tables
    finally:
        h.close()


# ---- the extracted sidecar serves the searches as the inline tables do ----

@pytest.mark.parametrize("name", ["300 blocks of 4 KiB", "compressed and plain tables", "type 4"])
def test_search_through_the_extracted_sidecar(ctx, name):
    """search and search_many on the stripped main with the extracted sidecar attached, and on the original with the mode-a sidecar attached,
    return the positions and counts of the same calls on the original with its inline tables and decode the same number of chunks, fewer
    than the stream has;
    the stripped main decodes to the data and the sidecar to nothing."""
    stream, d = case(ctx, name)
    nck = len(SM.main_chunks(stream))
    rng = np.random.default_rng(3)
    pats = [d[o:o + 24] for o in rng.integers(0, len(d) - 24, 6).tolist()] + [b"\x00absent needle\x00"]
    if name == "type 4":
        at = d.index(b'"user":"', len(d) // 2)
        pats = [d[at:at + 20], b'"user":"\x00nobody\x00'] + pats[:2]
    orig = Extracting(ctx, stream)
    try:
        want, decoded = searches(orig, pats)
        # the inline tables prune: the absent needle's search and most of the others decode fewer chunks than the stream has (a pattern of
        # this text's common phrases is admitted by every table, and search_many decodes the union of its patterns' chunks); the long-prefix
        # tables serve the pattern that begins with the prefix, the others decode every chunk
        pruned = [n < nck for n in decoded[:-1]]
        assert pruned[0] if name == "type 4" else (pruned[-1] and sum(pruned) * 2 >= len(pruned)), decoded
        assert want[0][0] >= 1 and want[0][1] == SMod.brute(d, pats[0])
        side_bound, main_bound = orig.bound()
        _, side_a, _, _ = orig.raw(side_bound, main_bound, False)
        _, side_b, main_b, res = orig.raw(side_bound, main_bound, True)
        t_a = dev_u8(side_a)
        orig.rd.attach_sidecar(t_a.data_ptr(), len(side_a))
        got, decoded_a = searches(orig, pats)
        assert got == want and decoded_a == decoded, "the same tables prune the same chunks"
        orig.rd.detach_sidecar()
    finally:
        orig.close()
    stripped = Extracting(ctx, main_b)
    try:
        t_b = dev_u8(side_b)
        stripped.rd.attach_sidecar(t_b.data_ptr(), len(side_b))
        got, decoded_b = searches(stripped, pats)
        assert got == want and decoded_b == decoded, "the same tables prune the same chunks"
        # the stripped main and the sidecar as streams
        dst = torch.full((len(d) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        assert ctx.stream_decode_device(stripped.t.data_ptr(), len(main_b), dst.data_ptr(), len(d)) == len(d)
        assert dst.cpu().numpy()[:len(d)].tobytes() == d and (dst.cpu().numpy()[len(d):] == 0x5A).all()
        assert ctx.stream_decode_device(t_b.data_ptr(), len(side_b), dst.data_ptr(), len(d)) == 0
        assert O.stream_decode(main_b, len(d)) == d
    finally:
        stripped.close()


def test_device_stream_front_end(ctx):
    stream, d = case(ctx, "300 blocks of 4 KiB")
    want_side, want_main, _ = XM.extract(stream, True)
    ds = shard.DeviceStream(ctx, dev_u8(stream))
    try:
        side = ds.extract_sidecar()
        assert side.is_cuda and side.dtype == torch.uint8 and side.cpu().numpy().tobytes() == XM.extract(stream, False)[0]
        side, main = ds.extract_sidecar(strip=True)
        assert side.cpu().numpy().tobytes() == want_side and main.cpu().numpy().tobytes() == want_main
    finally:
        ds.close()
    ds = shard.DeviceStream(ctx, main)
    try:
        ds.attach_sidecar(side)
        pat = d[3 * BS + 100:3 * BS + 124]
        pos, total = ds.search(pat, 100)
        assert pos.cpu().tolist() == SMod.brute(d, pat) and ctx.search_plan()[0] < 300
    finally:
        ds.close()


# ---- refusals ----

def test_refusals(ctx):
    """A set handle and a two-stream concatenation give -MLZ_ERR_UNSUPPORTED, from the bound as well; bad flags, NULLs, a main buffer of no
    room and a destination in host memory give -MLZ_ERR_ARG; nothing is written."""
    stream, d = case(ctx, "type 2")
    L = _lib.lib()
    h = Extracting(ctx, stream)
    try:
        sb, mb = h.bound()
        for flags in (1, 4, 64, 1 << 31, api.STREAM_IGNORE_CRC | 8):
            assert h.raw(sb, mb, True, flags)[0] == -MLZ_ERR_ARG, flags
        out = _lib.SidecarExtractResult()
        room = torch.full((sb + mb,), 0x5A, dtype=torch.uint8, device="cuda")
        call = L.mlz_dev_reader_extract_sidecar
        assert call(None, None, 0, room.data_ptr(), sb, None, 0, C.byref(out)) == -MLZ_ERR_ARG
        assert call(h.rd.handle, None, 0, None, sb, None, 0, C.byref(out)) == -MLZ_ERR_ARG
        assert call(h.rd.handle, None, 0, room.data_ptr(), sb, None, 0, None) == -MLZ_ERR_ARG
        assert call(h.rd.handle, None, 0, room.data_ptr(), sb, room.data_ptr() + sb, 0, C.byref(out)) == -MLZ_ERR_ARG
        host = np.full(sb, 0x5A, np.uint8)
        assert h.raw(sb, mb, False, side_ptr=host.ctypes.data)[0] == -MLZ_ERR_ARG and (host == 0x5A).all()
        assert (room.cpu().numpy() == 0x5A).all()
        assert L.mlz_dev_reader_extract_sidecar_bound(None, None) == -MLZ_ERR_ARG
        with pytest.raises(mz.MinLZError) as e:
            h.rd.extract_sidecar(room.data_ptr(), 20)
        assert e.value.needed == (XM.extract(stream, False)[2].side_len, 0) and (room.cpu().numpy() == 0x5A).all()
    finally:
        h.close()
    two = Extracting(ctx, stream + stream)
    try:
        assert two.raw(2 * len(stream), 4 * len(stream), True)[0] == -MLZ_ERR_UNSUPPORTED
        assert L.mlz_dev_reader_extract_sidecar_bound(two.rd.handle, None) == -MLZ_ERR_UNSUPPORTED
    finally:
        two.close()
    t = dev_u8(stream + stream)
    rd, results = ctx.stream_open_batch_device(t.data_ptr(), [(0, len(stream)), (len(stream), len(stream))])
    try:
        assert results == [len(d), len(d)]
        out = _lib.SidecarExtractResult()
        room = torch.full((4 * len(stream),), 0x5A, dtype=torch.uint8, device="cuda")
        assert L.mlz_dev_reader_extract_sidecar(rd.handle, None, 0, room.data_ptr(), room.numel(), None, 0, C.byref(out)) == -MLZ_ERR_UNSUPPORTED
        assert (room.cpu().numpy() == 0x5A).all()
        with pytest.raises(mz.ErrUnsupported):
            rd.extract_sidecar_bound()
    finally:
        rd.close()
    ss = shard.HipTensorCodec(ctx).open_streams(t, [(0, len(stream)), (len(stream), len(stream))])
    try:
        with pytest.raises(mz.ErrUnsupported):
            ss.extract_sidecar()
    finally:
        ss.close()
    empty = Extracting(ctx, b"")
    try:
        assert empty.raw(64, 64, True)[0] == -MLZ_ERR_CORRUPT
    finally:
        empty.close()
