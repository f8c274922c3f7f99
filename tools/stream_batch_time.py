"""Batches of streams in HBM (mlz_stream_decode_batch_device, mlz_stream_encode_batch_device) against the loop of single calls and against
the block batch calls, on an MI355X: one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and
interquartile ranges, a device synchronise inside every timed window.  All inputs text-like, LevelFastest.

  shapes   1024 streams of one 64 KiB block; 256 streams of 1 MiB in 64 KiB blocks; 16 streams of 8 MiB in 1 MiB blocks
  A        the batch call
  B        the loop of single calls (mlz_stream_decode_device / mlz_stream_encode_gather_device over one range): what there was before
  C        the floor without any walk, framing or read-back: mlz_decode_batch_device over the same blocks with descriptors prepared
           beforehand; for encode mlz_encode_batch_device + mlz_crc_batch_device
  cap      mlz_stream_decoded_len_batch_device on ONE stream of exactly 4096 chunk headers (a lane at the step cap), beside the same
           call on a stream of two

The bar: A below B by more than both interquartile ranges, for every shape; A / C is stated beside it, and where A exceeds twice C at 1024
streams the share of the block kernels' own time (the context's timers) in A is printed: the rest is the walk, the read-backs and the host.

usage: python tools/stream_batch_time.py [out.txt]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import minlz_amd as mz
from minlz_amd import _lib, synth
from minlz_amd._lib import BlockDesc

REPS = 25
LEVEL = mz.LevelFastest
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (16, 8 << 20, 1 << 20)]   # (streams, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def timed(fs):
    for _ in range(3):
        for _, f in fs:
            f()
            torch.cuda.synchronize()
    ts = {k: [] for k, _ in fs}
    for _ in range(REPS):
        for k, f in fs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def kernel_ms(f):
    """The block kernels' own time in one call of f, from the context's timers."""
    ctx.set_option(mz.OPT_TIMING, 1)
    f()
    torch.cuda.synchronize()
    t = ctx.timers()
    ctx.set_option(mz.OPT_TIMING, 0)
    return sum(t.values()), t


def report(what, n, ts):
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in ts:
        v = sorted(ts[k])
        say("    %s %-2s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (what, k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
    held = med["B"] - med["A"] > max(iqr(ts["A"]), iqr(ts["B"]))
    say("    %s: B / A = %.2f, A / C = %.2f; the bar (A below B by more than both IQRs): %s" % (what, med["B"] / med["A"], med["A"] / med["C"], "held" if held else "MISSED"))
    return med, held


base = torch.from_numpy(synth.text_like(40 << 20, seed=7).copy()).cuda()
results = {}
for n, size, bs in SHAPES:
    flags = 0
    bound = int(L.mlz_stream_bound(size, bs, flags))
    slot = (bound + 255) & ~255
    src_off = [(i * 1_000_003 * 64) % (base.numel() - size) for i in range(n)]
    enc = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    enc1 = torch.empty(slot, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    e_descs = (BlockDesc * n)(*[BlockDesc(src_off[i], size, i * slot, slot) for i in range(n)])
    res = ctx.stream_encode_batch_device(LEVEL, bs, False, base.data_ptr(), enc.data_ptr(), e_descs)
    assert min(res) > 0
    d_descs = (BlockDesc * n)(*[BlockDesc(i * slot, res[i], i * size, size) for i in range(n)])
    # the same blocks for the block batch calls
    per = size // bs
    nb = n * per
    stride = (bs + 2 + 255) & ~255
    benc = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    blen = torch.zeros(nb, dtype=torch.int64, device="cuda")
    bcrc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    b_descs = (BlockDesc * nb)(*[BlockDesc(src_off[i // per] + (i % per) * bs, bs, i * stride, stride) for i in range(nb)])
    ctx.encode_batch_device(None, LEVEL, base.data_ptr(), benc.data_ptr(), b_descs, blen.data_ptr())
    torch.cuda.synchronize()
    bl = blen.cpu().numpy()
    bd_descs = (BlockDesc * nb)(*[BlockDesc(i * stride, int(bl[i]), i * bs, bs) for i in range(nb)])
    dlen = torch.zeros(nb, dtype=torch.int64, device="cuda")
    p1, l1 = (C.c_void_p * 1)(), (C.c_size_t * 1)(size)

    def dec_a():
        assert ctx.stream_decode_batch_device(enc.data_ptr(), out.data_ptr(), d_descs) == [size] * n

    def dec_b():
        for i in range(n):
            assert L.mlz_stream_decode_device(ctx.handle, None, 0, enc.data_ptr() + i * slot, res[i], out.data_ptr() + i * size, size) == size

    def dec_c():
        ctx.decode_batch_device(None, benc.data_ptr(), out.data_ptr(), bd_descs, dlen.data_ptr())

    def enc_a():
        assert ctx.stream_encode_batch_device(LEVEL, bs, False, base.data_ptr(), enc.data_ptr(), e_descs) == res

    def enc_b():
        for i in range(n):
            p1[0] = base.data_ptr() + src_off[i]
            assert L.mlz_stream_encode_gather_device(ctx.handle, LEVEL, bs, 0, p1, l1, 1, enc1.data_ptr(), slot) == res[i]

    def enc_c():
        ctx.encode_batch_device(None, LEVEL, base.data_ptr(), benc.data_ptr(), b_descs, blen.data_ptr())
        ctx.crc_batch_device(None, base.data_ptr(), b_descs, bcrc.data_ptr())

    # the checks first: the batch's bytes are the single call's, and the inputs come back
    dec_a()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    bh = base.cpu().numpy()
    assert all(np.array_equal(o[i * size:(i + 1) * size], bh[src_off[i]:src_off[i] + size]) for i in range(0, n, max(1, n // 16)))
    enc_b()
    torch.cuda.synchronize()
    assert torch.equal(enc1[:res[n - 1]], enc[(n - 1) * slot:(n - 1) * slot + res[n - 1]])
    say("%d streams of %d bytes in blocks of %d (%d blocks, %.1f MB raw, %.1f MB of streams); %d repetitions, the calls alternated" %
        (n, size, bs, nb, n * size / 1e6, sum(res) / 1e6, REPS))
    dm, dheld = report("decode", n, timed([("A", dec_a), ("B", dec_b), ("C", dec_c)]))
    em, eheld = report("encode", n, timed([("A", enc_a), ("B", enc_b), ("C", enc_c)]))
    for what, med, f in (("decode", dm, dec_a), ("encode", em, enc_a)):
        if n == 1024 and med["A"] > 2 * med["C"]:
            k, t = kernel_ms(f)
            say("    %s: A exceeds twice C: the block kernels take %.3f ms of A's %.3f (%s); the walk or layout, the read-backs and the host take the rest" %
                (what, k, med["A"], ", ".join("%s %.3f" % kv for kv in sorted(t.items()))))
    results["%dx%d" % (n, size)] = {"decode": {k: round(v, 4) for k, v in dm.items()}, "decode_bar_held": dheld, "encode": {k: round(v, 4) for k, v in em.items()}, "encode_bar_held": eheld}
    del enc, out, benc


def frame(t, body=b""):
    return bytes([t, len(body) & 0xFF, len(body) >> 8 & 0xFF, len(body) >> 16]) + body


# one lane at the step cap: identifier, 4094 empty skippable chunks, EOF = 4096 headers
ident = b"\xff\x06\x00\x00MinLz\x02"
for name, s in (("cap", ident + frame(0x80) * 4094 + frame(0x20, b"\x00")), ("two", ident + frame(0x20, b"\x00"))):
    t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    one = (BlockDesc * 1)(BlockDesc(0, len(s), 0, 0))
    f = lambda: ctx.stream_decoded_len_batch_device(t.data_ptr(), one)
    assert f() == [(0, 0)] and ctx.batch_long_streams() == 0
    ts = timed([(name, f)])[name]
    results["walk_" + name] = round(statistics.median(ts), 4)
    say("decoded-length batch call on one stream of %d chunk headers: median %.3f ms, IQR %.3f" % (4096 if name == "cap" else 2, statistics.median(ts), iqr(ts)))
say("a lane at the step cap takes about %.3f ms more than one of two headers" % (results["walk_cap"] - results["walk_two"]))
say(json.dumps(results))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
