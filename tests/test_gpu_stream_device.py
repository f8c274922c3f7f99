"""The device-resident Reader (mlz_stream_decoded_len_device, mlz_stream_decode_device, HipTensorCodec.decode_stream): streams that lie in
HBM, walked and decoded there.  Every stream is uploaded into a tensor larger than itself: sentinel bytes in front, and behind the stream
first stale bytes that form a valid further data chunk, then sentinel; the output has sentinel bands on both sides.  After every call the
bands are intact and the input is unchanged.  Verdicts must be the host Reader's and the oracle's, bytes exact."""
from collections import Counter

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from tests import corrupt as CM
from tests import stream_device_cases as SC
from tests.test_gpu_tile_levels import LEGS

pytestmark = pytest.mark.gpu

SENT = 0xA5
FRONT, BACK = 37, 64          # (odd: the stream and the output start at no aligned address)
MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 6, 8
_STALE = None


def _stale():
    global _STALE
    if _STALE is None:
        _STALE = SC.data_chunk(synth.text_like(3000, 9).tobytes())
    return _STALE


class Dev:
    """A stream in device memory between its bands, and an output buffer between its own."""

    def __init__(self, s, cap):
        self.n, self.cap = len(s), cap
        self.image = np.concatenate([np.full(FRONT, SENT, np.uint8), np.frombuffer(s, np.uint8), np.frombuffer(_stale(), np.uint8), np.full(BACK, SENT, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()
        self.out = torch.full((FRONT + cap + BACK,), SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    @property
    def src(self):
        return self.t.data_ptr() + FRONT

    @property
    def dst(self):
        return self.out.data_ptr() + FRONT

    def check(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.t.cpu().numpy(), self.image), what + ": the input was modified"
        o = self.out.cpu().numpy()
        assert (o[:FRONT] == SENT).all() and (o[FRONT + self.cap:] == SENT).all(), what + ": bytes written outside d_dst[0, dst_cap)"
        return o[FRONT:FRONT + self.cap]


def _code(f):
    try:
        return 0, f()
    except mz.MinLZError as e:
        return e.code, None


def _host_len(s):
    a = np.frombuffer(s, np.uint8)
    p = a.ctypes.data if a.size else None
    return _lib.lib().mlz_stream_decoded_len(p, a.size), _lib.lib().mlz_stream_decoded_prefix_len(p, a.size)


def _check_valid(ctx, name, s, d, ignore_crc=(False, True)):
    dv = Dev(s, len(d) + 5)
    r, prefix = ctx.stream_decoded_len_device(dv.src, dv.n)
    assert (r, prefix) == _host_len(s) == (len(d), len(d)), name
    for ic in ignore_crc:
        dv.out[FRONT:FRONT + dv.cap] = 0
        got = ctx.stream_decode_device(dv.src, dv.n, dv.dst, dv.cap, ignore_crc=ic)
        o = dv.check(name)
        assert got == len(d) and o[:got].tobytes() == d, "%s (ignore_crc=%s)" % (name, ic)
        assert (o[got:] == 0).all(), name + ": bytes written behind the result"


def _valid_cases(ctx):
    d = SC.data_mix()
    cases = SC.valid_streams_cpu()
    for level in (mz.LevelSuperFast, 0, mz.LevelFastest, mz.LevelBalanced):
        for bs in (4 << 10, 64 << 10, 1 << 20, 8 << 20):
            for idx in (False, True):
                if level != mz.LevelFastest and (bs, idx) not in (((64 << 10), True), ((1 << 20), False), ((8 << 20), False)):
                    continue   # (every level; every size and the index at LevelFastest: the framing does not depend on the level)
                cases.append(("gpu_L%d_bs%d_idx%d" % (level, bs, idx), mz.stream_encode(d, level, bs, idx, ctx), d))
    return cases


def test_valid_streams_bit_exact(ctx):
    for name, s, d in _valid_cases(ctx):
        _check_valid(ctx, name, s, d)


def _check_mutants(ctx, bs, host_ctx):
    s, d = SC.oracle_stream(bs), SC.data_mix()
    muts = CM.stream_mutants(s)
    codes, bad = Counter(), []
    for name, b in muts:
        want, data = CM.stream_verdict(b, len(d) + 16)
        host = _code(lambda: mz.stream_decode(b, ctx=host_ctx))[0]
        dv = Dev(b, len(d) + 16)
        r, prefix = ctx.stream_decoded_len_device(dv.src, dv.n)
        got, n = _code(lambda: ctx.stream_decode_device(dv.src, dv.n, dv.dst, dv.cap))
        o = dv.check(name)
        codes[want] += 1
        if not (got == want == host):
            bad.append("%s: device Reader %d, oracle %d, host Reader %d" % (name, got, want, host))
        elif want == 0 and o[:n].tobytes() != data:
            bad.append("%s: bytes differ" % name)
        if (r, prefix) != _host_len(b):
            bad.append("%s: walk %s, host walk %s" % (name, (r, prefix), _host_len(b)))
    assert not bad, "\n".join(bad[:20])
    return len(muts), codes


@pytest.mark.parametrize("bs,count", [(1 << 20, 65), (64 << 10, 125)])
def test_every_mutant_exact_code(ctx, bs, count):
    n, codes = _check_mutants(ctx, bs, ctx)
    assert n >= count                                    # none left out
    assert all(codes[c] > 0 for c in (0, 1, 2, 3, 5)), codes


def test_many_tiny_chunks(ctx):
    s, d = SC.tiny_chunks()
    _check_valid(ctx, "tiny", s, d)
    sb, _ = SC.tiny_chunks(break_crc=True)
    dv = Dev(sb, len(d) + 5)
    with pytest.raises(mz.ErrCRC):
        ctx.stream_decode_device(dv.src, dv.n, dv.dst, dv.cap)
    dv.check("tiny_crc")
    assert ctx.stream_decode_device(dv.src, dv.n, dv.dst, dv.cap, ignore_crc=True) == len(d)
    assert dv.check("tiny_crc_ignored")[:len(d)].tobytes() == d


def test_stored_chunks(ctx):
    d = synth.random_bytes(64 << 20, seed=11).tobytes()
    s = mz.stream_encode(d, mz.LevelFastest, 64 << 10, False, ctx)
    assert all(c.type == 0x01 for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03))
    _check_valid(ctx, "stored", s, d, ignore_crc=(False,))


def test_dst_one_byte_short(ctx):
    s, d = SC.oracle_stream(1 << 20), SC.data_mix()
    host = np.empty(len(d), np.uint8)
    a = np.frombuffer(s, np.uint8)
    want = _lib.lib().mlz_stream_decode(ctx.handle, 0, a.ctypes.data, a.size, host.ctypes.data, len(d) - 1)
    assert want == -MLZ_ERR_DST_TOO_SMALL
    dv = Dev(s, len(d) - 1)
    with pytest.raises(mz.MinLZError) as e:
        ctx.stream_decode_device(dv.src, dv.n, dv.dst, dv.cap)
    assert type(e.value) is mz.MinLZError and "error %d" % MLZ_ERR_DST_TOO_SMALL in str(e.value)
    dv.check("short")


@pytest.mark.parametrize("leg,opts,counts", LEGS, ids=[l[0] for l in LEGS])
def test_option_legs(leg, opts, counts):
    c = mz.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        d = SC.data_mix()
        for level in (1, 2):
            _check_valid(c, "%s_L%d" % (leg, level), SC.oracle_stream(1 << 20, level), d, ignore_crc=(False,))
        _check_valid(c, leg + "_gpu_L2", mz.stream_encode(d, mz.LevelBalanced, 1 << 20, False, c), d, ignore_crc=(False,))
        _check_mutants(c, 1 << 20, c)
    finally:
        c.close()


def test_two_contexts_on_one_device():
    c2 = mz.Context(devices=[0, 0])
    try:
        d = SC.data_mix()
        _check_valid(c2, "multi", SC.oracle_stream(1 << 20), d)
        # a pointer that no device of the context holds: a host buffer's address
        hb = np.frombuffer(SC.oracle_stream(1 << 20), np.uint8).copy()
        out = torch.empty(len(d), dtype=torch.uint8, device="cuda")
        r, _ = c2.stream_decoded_len_device(hb.ctypes.data, hb.size)
        assert r == -MLZ_ERR_ARG
        assert _lib.lib().mlz_stream_decode_device(c2.handle, None, 0, hb.ctypes.data, hb.size, out.data_ptr(), len(d)) == -MLZ_ERR_ARG
    finally:
        c2.close()


def test_codec_decode_stream(ctx):
    d = SC.data_mix()
    codec = shard.HipTensorCodec(ctx)
    for s in (SC.oracle_stream(1 << 20), SC.oracle_stream(4 << 10, 1, True), mz.stream_encode(d, mz.LevelBalanced, 64 << 10, True, ctx)):
        t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
        o = codec.decode_stream(t)
        assert o.device == t.device and o.dtype == torch.uint8 and o.cpu().numpy().tobytes() == d
    assert codec.decode_stream(torch.from_numpy(np.frombuffer(O.stream_encode(b"", 1, 1 << 20), np.uint8).copy()).cuda()).numel() == 0
    bad = bytearray(SC.oracle_stream(1 << 20))
    bad[len(bad) // 2] ^= 0x04
    with pytest.raises(mz.MinLZError):
        codec.decode_stream(torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda())


def test_workspace_is_counted(ctx):
    s = SC.oracle_stream(1 << 20)
    dv = Dev(s, 16)
    ctx.stream_decoded_len_device(dv.src, dv.n)
    assert ctx.workspace_bytes()[1] >= 8 * len(s)
