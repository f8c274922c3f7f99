"""Batches of streams in HBM (mlz_stream_decoded_len_batch_device, mlz_stream_decode_batch_device, mlz_stream_encode_batch_device and
HipTensorCodec.decode_streams / encode_streams).  The contract of every stream of a batch is the single-stream call's: results are compared
with that call on the same bytes, with the host walk and with the oracle.  The sources lie in one buffer between sentinel bands, the
destinations in another with a 64-byte sentinel gap between two; after every call the bands are intact and the input is unchanged."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from tests import corrupt as CM
from tests import stream_batch_cases as BC
from tests import stream_device_cases as SC

pytestmark = pytest.mark.gpu

SENT = 0xA5
FRONT, GAP, BACK = 37, 64, 64          # (odd: the buffers start at no aligned address)
MLZ_ERR_CRC, MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 5, 6, 8
STREAM_SEARCH_TABLES = 4


class Batch:
    """Sources back to back (src_gap bytes of sentinel between two) in one device buffer between its bands, and one destination buffer:
    caps[i] bytes per stream, zeroed, with sentinel gaps between them and bands around them."""

    def __init__(self, sources, caps, src_gap=0):
        buf, self.spans = BC.back_to_back(sources, src_gap)
        self.image = np.concatenate([np.full(FRONT, SENT, np.uint8), np.frombuffer(buf, np.uint8), np.full(BACK, SENT, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()
        self.caps = list(caps)
        self.dst_off, o = [], 0
        for c in self.caps:
            self.dst_off.append(o)
            o += c + GAP
        self.clean = np.full(FRONT + o + BACK, SENT, np.uint8)
        for off, c in zip(self.dst_off, self.caps):
            self.clean[FRONT + off:FRONT + off + c] = 0
        self.reset()

    def reset(self):
        self.out = torch.from_numpy(self.clean.copy()).cuda()
        torch.cuda.synchronize()

    @property
    def src(self):
        return self.t.data_ptr() + FRONT

    @property
    def dst(self):
        return self.out.data_ptr() + FRONT

    def descs(self):
        return [(o, n, d, c) for (o, n), d, c in zip(self.spans, self.dst_off, self.caps)]

    def check(self, what):
        """-> the destinations' bytes, one array per stream."""
        torch.cuda.synchronize()
        assert np.array_equal(self.t.cpu().numpy(), self.image), what + ": the input was modified"
        o = self.out.cpu().numpy()
        keep = np.ones(o.size, bool)
        for off, c in zip(self.dst_off, self.caps):
            keep[FRONT + off:FRONT + off + c] = False
        assert (o[keep] == SENT).all(), what + ": bytes written outside the streams' destinations"
        return [o[FRONT + off:FRONT + off + c] for off, c in zip(self.dst_off, self.caps)]

    def untouched(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.out.cpu().numpy(), self.clean), what + ": bytes were written"
        assert np.array_equal(self.t.cpu().numpy(), self.image), what + ": the input was modified"


def _host_len(s):
    a = np.frombuffer(s, np.uint8)
    p = a.ctypes.data if a.size else None
    return _lib.lib().mlz_stream_decoded_len(p, a.size), _lib.lib().mlz_stream_decoded_prefix_len(p, a.size)


def _single(ctx, b, i, cap, ignore_crc=False):
    """mlz_stream_decode_device on stream i of the batch's source buffer alone -> (raw result, bytes)."""
    off, n = b.spans[i]
    out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    r = _lib.lib().mlz_stream_decode_device(ctx.handle, None, 2 if ignore_crc else 0, b.src + off, n, out.data_ptr(), cap)
    torch.cuda.synchronize()
    return int(r), out.cpu().numpy()


_VALID = {}


def _valid_cases(ctx):
    """(name, stream, data): oracle-made and library-made at every level and three block sizes, with and without index, hand-framed ones."""
    if "v" in _VALID:
        return _VALID["v"]
    d = BC.small_data()
    d300 = d[:300_000 + 77]
    cases = []
    for level, bs, idx, data in ((1, 4 << 10, False, d300), (1, 64 << 10, True, d), (1, 1 << 20, False, d300), (2, 64 << 10, False, d300), (2, 4 << 10, True, d300),
                                 (3, 64 << 10, True, d300), (2, 1 << 20, True, d)):
        cases.append(("oracle_L%d_bs%d_idx%d" % (level, bs, idx), O.stream_encode(data, level, bs, idx), data))
    for level, bs, idx, data in ((mz.LevelSuperFast, 64 << 10, False, d300), (0, 4 << 10, True, d300), (mz.LevelFastest, 1 << 20, True, d300),
                                 (mz.LevelBalanced, 64 << 10, False, d), (mz.LevelFastest, 4 << 10, False, d300), (mz.LevelBalanced, 1 << 20, True, d300),
                                 (0, 64 << 10, False, d300), (mz.LevelSuperFast, 4 << 10, True, d300), (mz.LevelFastest, 64 << 10, True, d)):
        cases.append(("gpu_L%d_bs%d_idx%d" % (level, bs, idx), mz.stream_encode(data, level, bs, idx, ctx), data))
    s, sd = SC.with_skippables()
    cases.append(("skippables", s, sd))
    cases.append(("compcrc", SC.to_compcrc(O.stream_encode(d300, 1, 64 << 10)), d300))
    cases.append(("empty", O.stream_encode(b"", 1, 1 << 20), b""))
    cases.append(("no_bytes", b"", b""))
    cases.append(("one_byte", O.stream_encode(b"x", 1, 1 << 20), b"x"))
    cases.append(("two_streams", O.stream_encode(d300[:150_001], 1, 64 << 10) + O.stream_encode(d300[150_001:], 2, 4 << 10, True), d300))
    cases.append(("stored", O.stream_encode(synth.random_bytes(200_003, seed=31).tobytes(), 1, 64 << 10), synth.random_bytes(200_003, seed=31).tobytes()))
    cases.append(("no_bytes_last", b"", b""))
    _VALID["v"] = cases
    return cases


def _check_valid_batch(ctx, cases, what):
    b = Batch([s for _, s, _ in cases], [len(d) + 5 for _, _, d in cases])
    lens = ctx.stream_decoded_len_batch_device(b.src, b.spans)
    b.untouched(what + " walk")
    for (name, s, d), got in zip(cases, lens):
        assert got == _host_len(s) == (len(d), len(d)), name
    for ic in (False, True):
        b.reset()
        res = ctx.stream_decode_batch_device(b.src, b.dst, b.descs(), ignore_crc=ic)
        outs = b.check(what)
        for i, ((name, s, d), r, o) in enumerate(zip(cases, res, outs)):
            one, one_bytes = _single(ctx, b, i, len(d) + 5, ic)
            assert r == one == len(d), "%s (ignore_crc=%s): batch %d, single call %d, data %d" % (name, ic, r, one, len(d))
            assert o[:r].tobytes() == d == one_bytes[:r].tobytes(), "%s (ignore_crc=%s): bytes differ" % (name, ic)
            assert (o[r:] == 0).all(), name + ": bytes written behind the result"
    return b


def test_valid_batch(ctx):
    cases = _valid_cases(ctx)
    assert len(cases) >= 24
    _check_valid_batch(ctx, cases, "valid")
    assert ctx.batch_long_streams() == 0


def test_every_mutant_in_one_batch(ctx):
    d = BC.small_data()
    muts = BC.small_mutants()
    assert len(muts) == BC.MUTANT_COUNT            # none left out
    cap = len(d) + 16
    b = Batch([m for _, m in muts], [cap] * len(muts))
    lens = ctx.stream_decoded_len_batch_device(b.src, b.spans)
    res = ctx.stream_decode_batch_device(b.src, b.dst, b.descs())
    outs = b.check("mutants")
    assert len(res) == len(muts)
    codes, bad = Counter(), []
    for i, ((name, m), r, o) in enumerate(zip(muts, res, outs)):
        want, data = CM.stream_verdict(m, cap)
        one, _ = _single(ctx, b, i, cap)
        code = 0 if r >= 0 else -r
        codes[want] += 1
        if not (r == one and code == want):
            bad.append("%s: batch %d, single call %d, oracle code %d" % (name, r, one, want))
        elif want == 0 and (r != len(data) or o[:r].tobytes() != data):
            bad.append("%s: bytes differ" % name)
        if lens[i] != _host_len(m):
            bad.append("%s: batch walk %s, host walk %s" % (name, lens[i], _host_len(m)))
    assert not bad, "\n".join(bad[:20])
    assert dict(codes) == BC.MUTANT_CODES and all(codes[c] > 0 for c in (0, 1, 2, 3, 5)), codes


def test_long_stream_between_ordinary_ones(ctx):
    tiny, td = SC.tiny_chunks()
    v = _valid_cases(ctx)
    cases = [v[1], ("tiny", tiny, td), v[0], v[10]]
    _check_valid_batch(ctx, cases, "tiny")
    assert ctx.batch_long_streams() == 1
    broken, _ = SC.tiny_chunks(break_crc=True)
    cases[1] = ("tiny_crc", broken, td)
    b = Batch([s for _, s, _ in cases], [len(d) + 5 for _, _, d in cases])
    res = ctx.stream_decode_batch_device(b.src, b.dst, b.descs())
    outs = b.check("tiny_crc")
    assert res == [len(cases[0][2]), -MLZ_ERR_CRC, len(cases[2][2]), len(cases[3][2])]
    assert _single(ctx, b, 1, len(td) + 5)[0] == -MLZ_ERR_CRC
    for i in (0, 2, 3):
        assert outs[i][:res[i]].tobytes() == cases[i][2]
    assert ctx.batch_long_streams() == 1
    assert ctx.stream_decode_batch_device(b.src, b.dst, b.descs(), ignore_crc=True)[1] == len(td)
    assert b.check("tiny_crc_ignored")[1][:len(td)].tobytes() == td


def test_caps_and_arguments(ctx):
    v = _valid_cases(ctx)
    cases = [v[0], v[3], v[8], v[11]]
    caps = [len(d) for _, _, d in cases]
    caps[2] -= 1                                        # a byte short
    b = Batch([s for _, s, _ in cases], caps)
    res = ctx.stream_decode_batch_device(b.src, b.dst, b.descs())
    outs = b.check("short")
    assert res == [len(cases[0][2]), len(cases[1][2]), -MLZ_ERR_DST_TOO_SMALL, len(cases[3][2])]
    assert _single(ctx, b, 2, caps[2])[0] == -MLZ_ERR_DST_TOO_SMALL
    assert (outs[2] == 0).all(), "the short stream's destination was written"
    for i in (0, 1, 3):
        assert outs[i].tobytes() == cases[i][2]
    # refused calls: nothing is written
    b.reset()
    L = _lib.lib()
    n = len(cases)
    out_len = (C.c_int64 * n)(*([123] * n))

    def call(d_src, descs, count):
        arr = (_lib.BlockDesc * max(len(descs), 1))(*[_lib.BlockDesc(*d) for d in descs])
        return L.mlz_stream_decode_batch_device(ctx.handle, None, 0, d_src, b.dst, arr, count, out_len)
    descs = b.descs()
    over = list(descs)
    over[3] = (descs[3][0], descs[3][1], descs[1][2] + 10, descs[3][3])      # into stream 1's destination
    assert call(b.src, over, n) == -MLZ_ERR_ARG
    host = b.image.copy()
    assert call(host.ctypes.data + FRONT, descs, n) == -MLZ_ERR_ARG
    assert call(b.src, descs, (1 << 20) + 1) == -MLZ_ERR_ARG
    assert call(b.src, descs, -1) == -MLZ_ERR_ARG
    assert L.mlz_stream_decode_batch_device(ctx.handle, None, 0, b.src, b.dst, None, n, out_len) == -MLZ_ERR_ARG
    big = list(descs)
    big[0] = (descs[0][0], (1 << 36) + 1, descs[0][2], descs[0][3])
    assert call(b.src, big, n) == -MLZ_ERR_ARG
    assert L.mlz_stream_decoded_len_batch_device(ctx.handle, None, host.ctypes.data + FRONT, (_lib.BlockDesc * n)(*[_lib.BlockDesc(*d) for d in descs]), n, out_len, None) == -MLZ_ERR_ARG
    assert list(out_len) == [123] * n
    b.untouched("refused")
    assert call(b.src, descs, 0) == 0
    assert ctx.stream_decode_batch_device(b.src, b.dst, []) == [] and ctx.stream_decoded_len_batch_device(b.src, []) == []
    b.untouched("empty batch")


_ENC_INPUTS = {}


def _encode_inputs():
    if not _ENC_INPUTS:
        text = synth.text_like((1 << 20) + 7, 41).tobytes()
        _ENC_INPUTS["v"] = [b"", text[:1], text[100:115], text[200:216], text[:4095], text[4096:4096 + 65536], text[1000:1000 + 65537],
                            synth.random_bytes(300_000, seed=42).tobytes(), text]
    return _ENC_INPUTS["v"]


@pytest.mark.parametrize("add_index", [False, True], ids=["plain", "index"])
@pytest.mark.parametrize("level", [-1, 0, 1, 2])
def test_encode_batch(ctx, level, add_index):
    bs = 64 << 10
    inputs = _encode_inputs()
    bounds = [int(_lib.lib().mlz_stream_bound(len(x), bs, 1 if add_index else 0)) for x in inputs]
    b = Batch(inputs, bounds)
    res = ctx.stream_encode_batch_device(level, bs, add_index, b.src, b.dst, b.descs())
    outs = b.check("encode")
    streams = []
    for x, r, o in zip(inputs, res, outs):
        want = mz.stream_encode(x, level, bs, add_index, ctx)
        assert r == len(want) and o[:r].tobytes() == want, "input of %d bytes: %d bytes, stream_encode gives %d" % (len(x), r, len(want))
        assert (o[r:] == 0).all(), "bytes written behind the stream"
        assert O.stream_decode(want, len(x) + 16) == x
        streams.append(want)
    # the encode batch's output, where it lies, through the decode batch
    back = Batch([b""], [len(x) + 3 for x in inputs])
    descs = [(b.dst_off[i], res[i], back.dst_off[i], back.caps[i]) for i in range(len(inputs))]
    got = ctx.stream_decode_batch_device(b.dst, back.dst, descs)
    o2 = back.check("round trip")
    assert got == [len(x) for x in inputs]
    for x, o in zip(inputs, o2):
        assert o[:len(x)].tobytes() == x
    if level == 1:
        # one dst_cap below the bound: that stream alone
        caps = list(bounds)
        caps[6] -= 1
        b2 = Batch(inputs, caps)
        res2 = ctx.stream_encode_batch_device(level, bs, add_index, b2.src, b2.dst, b2.descs())
        outs2 = b2.check("encode short")
        assert res2 == res[:6] + [-MLZ_ERR_DST_TOO_SMALL] + res[7:]
        assert (outs2[6] == 0).all()
        for i in (0, 5, 7, 8):
            assert outs2[i][:res2[i]].tobytes() == streams[i]
        # the tables flag: the whole call
        b2.reset()
        arr = (_lib.BlockDesc * len(inputs))(*[_lib.BlockDesc(*d) for d in b2.descs()])
        out_len = (C.c_int64 * len(inputs))()
        L = _lib.lib()
        assert L.mlz_stream_encode_batch_device(ctx.handle, None, level, bs, STREAM_SEARCH_TABLES, b2.src, b2.dst, arr, len(inputs), out_len) == -MLZ_ERR_ARG
        assert L.mlz_stream_encode_batch_device(ctx.handle, None, level, bs, 6 << 8, b2.src, b2.dst, arr, len(inputs), out_len) == -MLZ_ERR_ARG
        assert L.mlz_stream_encode_batch_device(ctx.handle, None, 3, bs, 0, b2.src, b2.dst, arr, len(inputs), out_len) == -4
        assert L.mlz_stream_encode_batch_device(ctx.handle, None, level, 1000, 0, b2.src, b2.dst, arr, len(inputs), out_len) == -MLZ_ERR_ARG
        b2.untouched("refused encode")


def test_two_contexts_on_one_device(ctx):
    c2 = mz.Context(devices=[0, 0])
    try:
        _check_valid_batch(c2, _valid_cases(ctx), "multi")
    finally:
        c2.close()


def test_codec_streams(ctx):
    codec = shard.HipTensorCodec(ctx)
    v = _valid_cases(ctx)
    cases = [v[i] for i in (0, 2, 4, 7, 8, 9, 12, 16, 17, 18, 19, 20)]
    buf, spans = BC.back_to_back([s for _, s, _ in cases], 3)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    out, starts = codec.decode_streams(t, spans)
    assert out.device == t.device and out.dtype == torch.uint8 and len(starts) == len(cases) + 1
    o = out.cpu().numpy()
    assert starts[-1] == o.size == sum(len(d) for _, _, d in cases)
    for i, (name, s, d) in enumerate(cases):
        assert o[starts[i]:starts[i + 1]].tobytes() == d, name
    # the error names the failing stream
    bad = bytearray(buf)
    off, n = spans[5]
    bad[off + n // 2] ^= 0x04
    with pytest.raises(mz.MinLZError) as e:
        codec.decode_streams(torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda(), spans)
    assert e.value.index == 5 and "stream 5" in str(e.value) and e.value.code in (1, 5)
    # encode_streams: stream_encode's bytes; decode_streams gives the inputs back
    inputs = _encode_inputs()[:8] + [v[0][2][:70_000], b"", v[1][2][:200_000], b"y" * 5000]
    ibuf, ispans = BC.back_to_back(inputs)
    it = torch.from_numpy(np.frombuffer(ibuf, np.uint8).copy()).cuda()
    enc, espans = codec.encode_streams(it, ispans, mz.LevelFastest, 64 << 10, True)
    e_host = enc.cpu().numpy()
    for x, (eo, en) in zip(inputs, espans):
        assert e_host[eo:eo + en].tobytes() == mz.stream_encode(x, mz.LevelFastest, 64 << 10, True, ctx)
    dec, dstarts = codec.decode_streams(enc, espans)
    assert dec.cpu().numpy().tobytes() == b"".join(inputs) and dstarts[-1] == len(ibuf)
    with pytest.raises(mz.MinLZError) as e:
        codec.encode_streams(it, ispans, 3, 64 << 10)
    assert e.value.code == 4
