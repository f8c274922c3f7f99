"""A batch of streams in HBM opened as ONE handle (mlz_stream_open_batch_device, include/minlz_hip_stream_set.h) against what a caller
did before, on an MI355X: one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and interquartile
ranges, a device synchronise inside every timed window.  All inputs text-like (lines of about 140 bytes), LevelFastest.

  shapes   1024 streams of one 64 KiB block; 256 streams of 1 MiB in 64 KiB blocks; 4096 streams of one 4 KiB block
  open     A  mlz_stream_open_batch_device + close
           B  the loop of mlz_stream_open_device + close per stream.  With --parent-lib it runs in the library given there (a build of the
              parent commit, loaded beside this one, with a context of its own); without, in this library.
           bar 1: A below B by more than both interquartile ranges, at every shape
  sample   100 000 ranges of 100 bytes through mlz_dev_reader_read_streams_device on the set,
           A  drawn from a tenth of the streams      A_all  drawn from all streams (losing to C is expected there)
           C  mlz_stream_decode_batch_device of the whole batch (the parent's library with --parent-lib) followed by a torch gather of the
              same bytes: what a caller does today
           bar 2: A below C by more than both interquartile ranges, at every shape
  index    I  mlz_dev_reader_index_records on the set (the index of a handle is kept, so every repetition opens a fresh handle in front of
              the timed window and closes it behind)      D  mlz_stream_decode_batch_device of the same batch
           the record index's bar: the build within 1.25 x a whole decode
  grep     G  DeviceStreamSet.grep_streams with 16 needles (the index built beforehand)      S  HipTensorCodec.search_streams with the same
           needles, the presence matrix and 1000 triples.  Reported without a bar: G answers per line, S per stream.

usage: python tools/stream_open_batch_time.py [--parent-lib libminlz_hip.so] [out.txt]"""
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
from minlz_amd.device import HipTensorCodec

args = sys.argv[1:]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else None

REPS, SAMPLE, PIECE = 25, 100_000, 100
LEVEL = mz.LevelFastest
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (4096, 4 << 10, 4 << 10)]   # (streams, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
codec = HipTensorCodec(ctx)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# the yardstick's library: the parent commit's, loaded beside this one, with a context of its own
B, bh = L, ctx.handle
if PARENT:
    B = C.CDLL(PARENT)
    for name in ("mlz_init", "mlz_stream_open_device", "mlz_dev_reader_close", "mlz_stream_decode_batch_device"):
        getattr(B, name).restype, getattr(B, name).argtypes = _lib.ABI[name]
    bh = C.c_void_p()
    assert B.mlz_init(0, C.byref(bh)) == 0
    assert not hasattr(B, "mlz_stream_open_batch_device"), "--parent-lib names a library that has the call under test"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def timed(fs):
    """fs: (name, f) or (name, f, before, after): f(before()) is timed, after(that value) runs outside the window."""
    fs = [(x + (lambda: None, lambda v: None))[:4] if len(x) == 2 else x for x in fs]
    call = lambda f, v: f() if v is None else f(v)
    for _ in range(3):
        for _, f, before, after in fs:
            v = before()
            call(f, v)
            torch.cuda.synchronize()
            after(v)
    ts = {k: [] for k, *_ in fs}
    for _ in range(REPS):
        for k, f, before, after in fs:
            v = before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(f, v)
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
            after(v)
    return ts


def report(what, ts):
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in ts:
        v = sorted(ts[k])
        say("    %s %-5s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (what, k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
    return med


def below(ts, a, b):
    """a's median below b's by more than both interquartile ranges"""
    return statistics.median(ts[b]) - statistics.median(ts[a]) > max(iqr(ts[a]), iqr(ts[b]))


base = torch.from_numpy(synth.text_like(40 << 20, seed=7).copy()).cuda()
base_h = base.cpu().numpy()
rng = np.random.default_rng(5)
results = {"yardstick_library": "parent" if PARENT else "this library"}
say("legs B and C run in %s" % (("the parent commit's library, " + os.path.basename(PARENT)) if PARENT else "THIS library (no --parent-lib given)"))
for n, size, bs in SHAPES:
    bound = int(L.mlz_stream_bound(size, bs, 0))
    slot = (bound + 255) & ~255
    src_off = [(i * 1_000_003 * 64) % (base.numel() - size) for i in range(n)]
    enc = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    e_descs = (BlockDesc * n)(*[BlockDesc(src_off[i], size, i * slot, slot) for i in range(n)])
    res = ctx.stream_encode_batch_device(LEVEL, bs, False, base.data_ptr(), enc.data_ptr(), e_descs)
    assert min(res) > 0
    spans = [(i * slot, res[i]) for i in range(n)]
    o_descs = (BlockDesc * n)(*[BlockDesc(o, m, 0, 0) for o, m in spans])
    d_descs = (BlockDesc * n)(*[BlockDesc(i * slot, res[i], i * size, size) for i in range(n)])
    lens = (C.c_int64 * n)()
    say("%d streams of %d bytes in blocks of %d (%.1f MB raw, %.1f MB of streams); %d repetitions, the calls alternated" % (n, size, bs, n * size / 1e6, sum(res) / 1e6, REPS))

    # ---- open ----
    def open_a():
        rd, r = ctx.stream_open_batch_device(enc.data_ptr(), o_descs)
        rd.close()
        return r

    def open_b():
        h = C.c_void_p()
        for i in range(n):
            assert B.mlz_stream_open_device(bh, None, enc.data_ptr() + i * slot, res[i], C.byref(h)) == size
            B.mlz_dev_reader_close(h)

    assert open_a() == [size] * n
    ts = timed([("A", open_a), ("B", open_b)])
    med = report("open  ", ts)
    held1 = below(ts, "A", "B")
    say("    open: B / A = %.1f, %.4f ms per stream in B; bar 1 (A below B by more than both IQRs): %s" % (med["B"] / med["A"], med["B"] / n, "held" if held1 else "MISSED"))
    entry = {"open": {k: round(v, 4) for k, v in med.items()}, "bar1_held": held1}

    # ---- the sampled read ----
    rd, _ = ctx.stream_open_batch_device(enc.data_ptr(), o_descs)
    dst = torch.empty(SAMPLE * PIECE, dtype=torch.uint8, device="cuda")
    ar = torch.arange(PIECE, device="cuda")

    def sample(streams):
        w = rng.choice(streams, SAMPLE)
        o = rng.integers(0, size - PIECE + 1, SAMPLE)
        return (torch.from_numpy(w.astype(np.int32)).cuda(), torch.from_numpy(o.astype(np.int64)).cuda(), torch.full((SAMPLE,), PIECE, dtype=torch.int64, device="cuda"),
                torch.from_numpy((w.astype(np.int64) * size + o)).cuda(), w, o)

    tenth, every = sample(rng.choice(n, max(1, n // 10), replace=False)), sample(np.arange(n))

    def read_a(s):
        return lambda: rd.read_streams_device(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), SAMPLE, dst.data_ptr(), dst.numel())

    def read_c(s):
        def f():
            assert B.mlz_stream_decode_batch_device(bh, None, 0, enc.data_ptr(), out.data_ptr(), d_descs, n, lens) == 0
            return out[(s[3][:, None] + ar[None, :]).reshape(-1)]
        return f

    for s in (tenth, every):   # the checks first: both ways give the bytes of the source
        assert read_a(s)() == SAMPLE * PIECE
        got_c = read_c(s)()
        torch.cuda.synchronize()
        assert torch.equal(dst, got_c)
        k = 4242
        assert np.array_equal(dst[k * PIECE:(k + 1) * PIECE].cpu().numpy(), base_h[src_off[s[4][k]] + s[5][k]:src_off[s[4][k]] + s[5][k] + PIECE])
    ts = timed([("A", read_a(tenth)), ("C", read_c(tenth)), ("A_all", read_a(every)), ("C_all", read_c(every))])
    med = report("sample", ts)
    held2 = below(ts, "A", "C")
    say("    sample of %d x %d bytes from a tenth of the streams: C / A = %.2f; bar 2 (A below C by more than both IQRs): %s.  From all streams: C_all / A_all = %.2f" %
        (SAMPLE, PIECE, med["C"] / med["A"], "held" if held2 else "MISSED", med["C_all"] / med["A_all"]))
    entry.update(sample={k: round(v, 4) for k, v in med.items()}, bar2_held=held2)
    rd.close()

    # ---- the record index ----
    fresh = lambda: ctx.stream_open_batch_device(enc.data_ptr(), o_descs)[0]
    count = []

    def decode_d():
        assert ctx.stream_decode_batch_device(enc.data_ptr(), out.data_ptr(), d_descs) == [size] * n

    ts = timed([("I", lambda r: count.append(r.index_records()[0]), fresh, lambda r: r.close()), ("D", decode_d)])
    med = report("index ", ts)
    say("    %d records; the build = %.2f x the whole decode (the record index's bar: within 1.25 x): %s" %
        (count[0], med["I"] / med["D"], "held" if med["I"] <= 1.25 * med["D"] else "MISSED"))
    entry.update(index={k: round(v, 4) for k, v in med.items()}, index_over_decode=round(med["I"] / med["D"], 3))

    # ---- grep per line against search per stream ----
    needles = [bytes(base_h[src_off[(37 * k) % n] + 1000 + k:src_off[(37 * k) % n] + 1012 + k]).replace(b"\n", b" ") for k in range(16)]
    st = codec.open_streams(enc, spans)
    st.index_records()
    which, line, kind = st.grep_streams(needles)
    counts, present, *_ = codec.search_streams(enc, spans, needles, max_results=1000)
    assert which.numel() > 0 and int(counts.sum()) > 0
    ts = timed([("G", lambda: st.grep_streams(needles)), ("S", lambda: codec.search_streams(enc, spans, needles, max_results=1000))])
    med = report("grep  ", ts)
    say("    16 needles: %d matching lines in %d streams; G / S = %.2f (no bar)" % (which.numel(), int(present.any(dim=1).sum()), med["G"] / med["S"]))
    entry.update(grep={k: round(v, 4) for k, v in med.items()})
    st.close()
    results["%dx%d" % (n, size)] = entry
    del enc, out, dst

say(json.dumps(results))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
