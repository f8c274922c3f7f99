"""The device-resident ReadSeeker against what a caller had to do without it, on an MI355X (the protocol of tools/stream_device_time.py: one
process, every shape warmed up, REPS timed repetitions with the variants alternated, medians, host clock round a call that ends in a device
synchronise):

  t_open   mlz_stream_open_device (the chunk walk + keeping the table), once per stream: the median of REPS opens
  t_read   mlz_dev_reader_read of the shape's ranges (a host array, planned on the host)
  t_read_dev  mlz_dev_reader_read_device of the same offsets and lengths as two CUDA tensors (uploaded outside the timed window, as t_alt's
           index tensor is built outside it): planned by kernels; mlz_get_counter 9 (plan bytes between host and device) is printed with it
  t_alt    the same bytes without it: mlz_stream_decode_device of the whole stream into a buffer, plus for (c) a torch gather of the same
           ranges from that buffer (its index tensor is built outside the timed window)

Streams: (a) the bench stream (100 MB enwik-like, LevelFastest, 8 MiB blocks), (b) its first 64 MiB in 4 KiB blocks, (d) the 100 MB in 2 MiB
blocks (the reference Writer's default).  Shapes: (r1) one range of 4 KiB at a seeded offset, (r2) 1 MiB straddling a chunk border, (r3) the
middle half, (c) 100 000 seeded ranges of 64 - 512 bytes, packed output, (w) everything.
(s) is the copy alone: shape (c) on a stream of stored chunks (64 MiB of random bytes in 64 KiB blocks) with the CRC check off: nothing is
decoded, the call is the plan and the copy kernel.  Run once more with MINLZ_HIP_LIB pointing at a build with -DMLZ_RANGE_SHORT_MAX=0
(tools/exp_build.sh) it gives the same figures with one workgroup per segment in the place of the packed short form.
usage: python tools/stream_ranges_time.py [out.txt [streams, e.g. a,b,d,s [shapes, e.g. c]]]"""
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
from minlz_amd import synth

REPS = 25
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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


def shapes(n, bs, seed):
    rng = np.random.default_rng(seed)
    out = {}
    off = int(rng.integers(0, n - 4096))
    out["r1"] = np.array([[off, 4096, 0]], dtype=np.uint64)
    border = (n // bs // 2) * bs
    out["r2"] = np.array([[border - (512 << 10), 1 << 20, 0]], dtype=np.uint64)
    out["r3"] = np.array([[n // 4, n // 2, 0]], dtype=np.uint64)
    lens = rng.integers(64, 513, 100_000)
    offs = rng.integers(0, n - 512, 100_000)
    out["c"] = np.stack([offs, lens, np.cumsum(lens) - lens], axis=1).astype(np.uint64)
    out["w"] = np.array([[0, n, 0]], dtype=np.uint64)
    return out


SHAPES = sys.argv[3].split(",") if len(sys.argv) > 3 else None


def measure(name, s, d, bs, only=None, ignore_crc=False):
    only = only or SHAPES
    n = len(s)
    t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    whole = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
    out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
    dn = np.frombuffer(d, np.uint8)
    opens = []
    for _ in range(REPS + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = ctx.stream_open_device(t.data_ptr(), n)
        torch.cuda.synchronize()
        opens.append((time.perf_counter() - t0) * 1e3)
        rd.close()
    rd = ctx.stream_open_device(t.data_ptr(), n)
    assert rd.size == len(d)
    say("%s: stream %d B, decoded %d B, %d repetitions; t_open median %.3f ms (min %.3f)" % (name, n, len(d), REPS, statistics.median(opens[3:]), min(opens[3:])))
    for shape, r in shapes(len(d), bs, 7).items():
        if only and shape not in only:
            continue
        total = int(r[:, 1].sum())
        idx = None
        if shape == "c":   # the gather's index: every wanted byte's offset, in output order
            starts = np.repeat(r[:, 0].astype(np.int64) - r[:, 2].astype(np.int64), r[:, 1].astype(np.int64))
            idx = torch.from_numpy(starts + np.arange(total, dtype=np.int64)).cuda()

        def read():
            assert rd.read(r, out.data_ptr(), total, ignore_crc=ignore_crc) == total

        d_off = torch.from_numpy(r[:, 0].astype(np.int64)).cuda()
        d_len = torch.from_numpy(r[:, 1].astype(np.int64)).cuda()
        out_dev = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")

        def read_dev():
            assert rd.read_device(d_off.data_ptr(), d_len.data_ptr(), len(r), out_dev.data_ptr(), total, ignore_crc=ignore_crc) == total

        def alt():
            assert ctx.stream_decode_device(t.data_ptr(), n, whole.data_ptr(), len(d), ignore_crc=ignore_crc) == len(d)
            if idx is not None:
                alt.res = torch.index_select(whole, 0, idx)

        read()
        torch.cuda.synchronize()
        got = out[:total].cpu().numpy()
        for off, ln, dst in r[:: max(1, len(r) // 50)].tolist():
            assert np.array_equal(got[dst:dst + ln], dn[off:off + ln]), (name, shape)
        chunks, scratch = ctx.range_plan()
        read_dev()
        torch.cuda.synchronize()
        got = out_dev[:total].cpu().numpy()
        for off, ln, dst in r[:: max(1, len(r) // 50)].tolist():
            assert np.array_equal(got[dst:dst + ln], dn[off:off + ln]), (name, shape, "device ranges")
        assert ctx.range_plan() == (chunks, scratch)
        plan_bytes = ctx.range_plan_host_bytes()
        ts = timed([("t_read", read), ("t_read_dev", read_dev), ("t_alt", alt)])
        med = {k: statistics.median(v) for k, v in ts.items()}
        say("  (%s) %6d ranges, %9d bytes, %5d chunks touched, %9d bytes through the scratch" % (shape, len(r), total, chunks, scratch))
        for k in ("t_read", "t_read_dev", "t_alt"):
            v = sorted(ts[k])
            say("       %-10s median %8.3f ms   min %8.3f   p90 %8.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))]))
        say("       t_read %s t_alt, t_read_dev %s t_alt   %s" % ("<=" if med["t_read"] <= med["t_alt"] else "> ", "<=" if med["t_read_dev"] <= med["t_alt"] else "> ", json.dumps(
            {"input": name[:3], "shape": shape, "t_read": round(med["t_read"], 4), "t_read_dev": round(med["t_read_dev"], 4), "t_alt": round(med["t_alt"], 4), "plan_bytes": plan_bytes})))
    rd.close()


say("library: %s" % os.environ.get("MINLZ_HIP_LIB", "minlz_amd/libminlz_hip.so"))
a = synth.enwik_like(100_000_000, seed=1).tobytes()
which = sys.argv[2].split(",") if len(sys.argv) > 2 else ["a", "b", "d", "s"]
if "a" in which:
    measure("(a) bench stream, 8 MiB blocks", mz.stream_encode(a, mz.LevelFastest, 8 << 20, False, ctx), a, 8 << 20)
if "b" in which:
    b = a[:64 << 20]
    measure("(b) 64 MiB in 4 KiB blocks", mz.stream_encode(b, mz.LevelFastest, 4 << 10, False, ctx), b, 4 << 10)
if "d" in which:
    measure("(d) 100 MB in 2 MiB blocks", mz.stream_encode(a, mz.LevelFastest, 2 << 20, False, ctx), a, 2 << 20)
if "s" in which:
    r = np.random.default_rng(3).integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
    measure("(s) 64 MiB of stored chunks, CRC check off: the copy alone", mz.stream_encode(r, mz.LevelFastest, 64 << 10, False, ctx), r, 64 << 10, only=("c",), ignore_crc=True)
say("decode-side workspace held: %d bytes" % ctx.workspace_bytes()[1])
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
