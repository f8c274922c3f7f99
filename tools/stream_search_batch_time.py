"""The search over a batch of streams in HBM (mlz_stream_search_batch_device) against the loop of single-stream searches, the batch decode
and one search over a single stream of the same bytes, on an MI355X: one process, every call warmed up, REPS timed repetitions with the
calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.  All inputs text-like, LevelFastest.

  shapes   1024 streams of one 64 KiB block; 256 streams of 1 MiB in 64 KiB blocks; 16 streams of 8 MiB in 1 MiB blocks; 4096 streams of
           one 4 KiB block.  1 needle and 16 needles (12 bytes each, cut from the data).
  A        mlz_stream_search_batch_device with the presence matrix and cap = 1000
  B        the loop mlz_stream_open_device / mlz_dev_reader_search_many(MLZ_SEARCH_NO_TABLES, cap 1000) / mlz_dev_reader_close per stream: what
           there was before.  With --parent-lib it runs in the library given there (a build of the parent commit, loaded beside this one), so
           that the yardstick is not the code under test; without it, in this library, and the output says so.
  C        mlz_stream_decode_batch_device over the same batch
  D        one mlz_dev_reader_search_many(MLZ_SEARCH_NO_TABLES, cap 1000) over a single stream that holds the same total bytes (opened beforehand)

The bar: A's median below B's by more than both interquartile ranges, at every shape with at least 16 streams.  A / C and A / D are
recorded without a bar.

usage: python tools/stream_search_batch_time.py [--parent-lib libminlz_hip.so] [--trace] [out.txt]
  --trace: only leg A at the 4096 x 4 KiB shape with 16 needles, 20 calls, nothing timed — the program of a
           `rocprofv3 --kernel-trace --stats -- python tools/stream_search_batch_time.py --trace` run, whose statistics give the scan kernels' share."""
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

args = sys.argv[1:]
TRACE = "--trace" in args
args = [a for a in args if a != "--trace"]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else None

REPS, CAP, NO_TABLES = 25, 1000, 8
LEVEL = mz.LevelFastest
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (16, 8 << 20, 1 << 20), (4096, 4 << 10, 4 << 10)]   # (streams, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# leg B's library: the parent commit's, loaded beside this one, with a context of its own
B, bh = L, ctx.handle
if PARENT:
    B = C.CDLL(PARENT)
    for name in ("mlz_init", "mlz_stream_open_device", "mlz_dev_reader_search_many", "mlz_dev_reader_close"):
        getattr(B, name).restype, getattr(B, name).argtypes = _lib.ABI[name]
    bh = C.c_void_p()
    assert B.mlz_init(0, C.byref(bh)) == 0


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


base = torch.from_numpy(synth.text_like(40 << 20, seed=7).copy()).cuda()
base_h = base.cpu().numpy()
rng = np.random.default_rng(5)
results = {"B_library": "parent" if PARENT else "this library"}
say("leg B runs in %s" % (("the parent commit's library, " + os.path.basename(PARENT)) if PARENT else "THIS library (no --parent-lib given): the yardstick is the code under test"))
for n, size, bs in SHAPES[3:] if TRACE else SHAPES:
    bound = int(L.mlz_stream_bound(size, bs, 0))
    slot = (bound + 255) & ~255
    src_off = [(i * 1_000_003 * 64) % (base.numel() - size) for i in range(n)]
    enc = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    e_descs = (BlockDesc * n)(*[BlockDesc(src_off[i], size, i * slot, slot) for i in range(n)])
    res = ctx.stream_encode_batch_device(LEVEL, bs, False, base.data_ptr(), enc.data_ptr(), e_descs)
    assert min(res) > 0
    d_descs = (BlockDesc * n)(*[BlockDesc(i * slot, res[i], i * size, size) for i in range(n)])
    s_descs = (BlockDesc * n)(*[BlockDesc(i * slot, res[i], 0, 0) for i in range(n)])
    # the same bytes as ONE stream, opened once
    ctx.stream_decode_batch_device(enc.data_ptr(), out.data_ptr(), d_descs)
    total_bytes = n * size
    one_bound = int(L.mlz_stream_bound(total_bytes, bs, 0))
    one = torch.empty(one_bound, dtype=torch.uint8, device="cuda")
    one_len = ctx.stream_encode_batch_device(LEVEL, bs, False, out.data_ptr(), one.data_ptr(), [(0, total_bytes, 0, one_bound)])[0]
    assert one_len > 0
    rd = ctx.stream_open_device(one.data_ptr(), one_len)
    present = torch.zeros(n, dtype=torch.int32, device="cuda")
    hs, hw = torch.zeros(CAP, dtype=torch.int32, device="cuda"), torch.zeros(CAP, dtype=torch.int32, device="cuda")
    hp = torch.zeros(CAP, dtype=torch.int64, device="cuda")
    say("%d streams of %d bytes in blocks of %d (%.1f MB raw, %.1f MB of streams); %d repetitions, the calls alternated" % (n, size, bs, total_bytes / 1e6, sum(res) / 1e6, REPS))
    for npat in (16,) if TRACE else (1, 16):
        pats = []
        for k in range(npat):   # cut from the data of the batch's streams
            o = src_off[int(rng.integers(0, n))] + int(rng.integers(0, size - 12))
            pats.append(base_h[o:o + 12].tobytes())
        blob, lens = b"".join(pats), (C.c_uint32 * npat)(*([12] * npat))
        counts_a = {}

        def leg_a():
            counts_a["total"], counts_a["res"], _ = ctx.stream_search_batch_device(enc.data_ptr(), s_descs, pats, None, None, present.data_ptr(), hs.data_ptr(), hp.data_ptr(),
                                                                                   hw.data_ptr(), CAP)

        counts_b = [0] * n

        def leg_b():
            h = C.c_void_p()
            for i in range(n):
                assert B.mlz_stream_open_device(bh, None, enc.data_ptr() + i * slot, res[i], C.byref(h)) == size
                counts_b[i] = B.mlz_dev_reader_search_many(h, None, NO_TABLES, blob, lens, npat, None, hp.data_ptr(), hw.data_ptr(), CAP, None)
                B.mlz_dev_reader_close(h)

        def leg_c():
            ctx.stream_decode_batch_device(enc.data_ptr(), out.data_ptr(), d_descs)

        found_d = {}

        def leg_d():
            found_d["total"] = rd.search_many(pats, None, hp.data_ptr(), hw.data_ptr(), CAP, no_tables=True)[0]

        if TRACE:
            for _ in range(20):
                leg_a()
            torch.cuda.synchronize()
            say("leg A, %d needles: 20 calls, total %d" % (npat, counts_a["total"]))
            continue
        # the checks first: the batch's counts are the loop's, stream by stream
        leg_a(); leg_b(); leg_d()
        torch.cuda.synchronize()
        assert counts_a["res"] == counts_b and counts_a["total"] == sum(counts_b) > 0
        assert found_d["total"] >= counts_a["total"]   # (the single stream also finds what lies across two of the batch's streams)
        ts = timed([("A", leg_a), ("B", leg_b), ("C", leg_c), ("D", leg_d)])
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            v = sorted(ts[k])
            say("    %2d needles %-2s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (npat, k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
        held = med["B"] - med["A"] > max(iqr(ts["A"]), iqr(ts["B"]))
        say("    %2d needles, %d occurrences: B / A = %.2f, A / C = %.2f, A / D = %.2f; the bar (A below B by more than both IQRs): %s" %
            (npat, counts_a["total"], med["B"] / med["A"], med["A"] / med["C"], med["A"] / med["D"], "held" if held else "MISSED"))
        results["%dx%d_%d" % (n, size, npat)] = dict({k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}, bar_held=held)
    rd.close()
    del enc, out, one
say(json.dumps(results))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
