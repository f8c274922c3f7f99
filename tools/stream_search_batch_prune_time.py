"""The pruned search over a batch of streams in HBM (mlz_stream_search_batch_device_pruned) against the unpruned call of the parent commit, on
an MI355X: one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and interquartile ranges, a device
synchronise inside every timed window.  JSON-like data; every stream written by the device Writer (LevelFastest) with table type 1, M = 6.

  shapes   1024 streams of one 64 KiB block; 256 streams of 1 MiB in 64 KiB blocks; 16 streams of 8 MiB in 1 MiB blocks; 4096 streams of
           one 4 KiB block (tools/stream_batch_time.py's).  1 needle planted in 3 streams, and 16 needles planted in 3 streams each
           (16 random bytes above 0x7f).
  A        mlz_stream_search_batch_device_pruned with the presence matrix and cap = 1000
  B        mlz_stream_search_batch_device on the same batch.  With --parent-lib it runs in the library given there (a build of the parent
           commit, loaded beside this one), so that the yardstick is not the code under test; without it, in this library, and the output says so.
  C        A on the same data written without tables
  D        B on that table-less batch
Every row is first checked against the model on the host (tests/search_batch_prune_model.py): the counts by brute force, stats 1, 4, 5 by the plan;
and the bytes the plan brings to the host (mlz_get_counter 16) against the bound of 32 per stream and one per data chunk.

The bar: A's median below B's by more than both interquartile ranges at every shape but 4096 x 4 KiB (a 4 KiB block's table may cost as much as
the block), which is reported without one.  C / D (what the info, class and locate passes cost a batch without tables), chunks decoded of
chunks present and streams skipped are recorded without a bar.

usage: python tools/stream_search_batch_prune_time.py [--parent-lib libminlz_hip.so] [--trace] [out.txt]
  --trace: only leg A at the 256 x 1 MiB shape with 16 needles, 20 calls, nothing timed — the program of a
           `rocprofv3 --kernel-trace --stats -- python tools/stream_search_batch_prune_time.py --trace` run, whose statistics give the kernels' times."""
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
from minlz_amd import _lib, api, synth
from minlz_amd._lib import BlockDesc
from tests import search_batch_prune_model as PM

args = sys.argv[1:]
TRACE = "--trace" in args
args = [a for a in args if a != "--trace"]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else None

REPS, CAP = 25, 1000
LEVEL = mz.LevelFastest
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (16, 8 << 20, 1 << 20), (4096, 4 << 10, 4 << 10)]   # (streams, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# leg B's and D's library: the parent commit's, loaded beside this one, with a context of its own
B, bh = L, ctx.handle
NAME = "mlz_stream_search_batch_device"
if PARENT:
    B = C.CDLL(PARENT)
    B.mlz_init.restype, B.mlz_init.argtypes = _lib.ABI["mlz_init"]
    getattr(B, NAME).restype, getattr(B, NAME).argtypes = _lib.ABI_EXT["minlz_hip_search_batch.h"][NAME]
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


def write_batch(datas, size, bs, tables):
    """Every stream by the device Writer into a slot of one buffer -> (the buffer, the descriptors, the streams' sizes)."""
    kw = dict(search_match_len=6) if tables else {}
    slot = (api.stream_bound(size, bs, False, **kw) + 255) & ~255
    enc = torch.empty(len(datas) * slot, dtype=torch.uint8, device="cuda")
    res = []
    for i, d in enumerate(datas):
        t = torch.from_numpy(d).cuda()
        res.append(ctx.stream_encode_gather_device(LEVEL, bs, False, [t.data_ptr()], [t.numel()], enc.data_ptr() + i * slot, slot, **kw))
    torch.cuda.synchronize()
    return enc, (BlockDesc * len(datas))(*[BlockDesc(i * slot, res[i], 0, 0) for i in range(len(datas))]), res, slot


rng = np.random.default_rng(5)
base = synth.json_like(48 << 20, seed=7)
results = {"B_library": "parent" if PARENT else "this library"}
say("legs B and D run in %s" % (("the parent commit's library, " + os.path.basename(PARENT)) if PARENT else "THIS library (no --parent-lib given): the yardstick is the code under test"))
for n, size, bs in SHAPES[1:2] if TRACE else SHAPES:
    src_off = [(i * 1_000_003 * 64) % (len(base) - size) for i in range(n)]
    for npat in (16,) if TRACE else (1, 16):
        pats = [bytes(rng.integers(128, 256, 16, dtype=np.uint8)) for _ in range(npat)]
        datas = [base[o:o + size].copy() for o in src_off]
        used = set()
        for p in pats:   # each needle in 3 streams, in a slot of 32 bytes that no other plant has
            for s in rng.choice(n, 3, replace=False):
                o = int(rng.integers(0, size // 32 - 1)) * 32 + 8
                while (int(s), o) in used:
                    o = int(rng.integers(0, size // 32 - 1)) * 32 + 8
                used.add((int(s), o))
                datas[s][o:o + 16] = np.frombuffer(p, np.uint8)
        enc, descs, res, slot = write_batch(datas, size, bs, True)
        bare, bare_descs, bare_res, bare_slot = write_batch(datas, size, bs, False)
        present = torch.zeros(n * ((npat + 31) // 32), dtype=torch.int32, device="cuda")
        hs, hw = torch.zeros(CAP, dtype=torch.int32, device="cuda"), torch.zeros(CAP, dtype=torch.int32, device="cuda")
        hp = torch.zeros(CAP, dtype=torch.int64, device="cuda")
        blob, lens = b"".join(pats), (C.c_uint32 * npat)(*([16] * npat))
        got = {}

        def pruned(key, buf, d):
            def f():
                got[key] = ctx.stream_search_batch_device(buf.data_ptr(), d, pats, None, None, present.data_ptr(), hs.data_ptr(), hp.data_ptr(), hw.data_ptr(), CAP, prune=True)
                got[key + " home"] = ctx.counter(16)   # the bytes the plan brought to the host
            return f

        def unpruned(key, buf, d):
            out, st = (C.c_int64 * n)(), (C.c_uint64 * 4)()

            def f():
                r = getattr(B, NAME)(bh, None, 0, buf.data_ptr(), d, n, blob, lens, npat, out, None, None, present.data_ptr(), hs.data_ptr(), hp.data_ptr(), hw.data_ptr(), CAP, st)
                got[key] = (r, list(out), tuple(st))
            return f
        legs = [("A", pruned("A", enc, descs)), ("B", unpruned("B", enc, descs)), ("C", pruned("C", bare, bare_descs)), ("D", unpruned("D", bare, bare_descs))]
        if TRACE:
            for _ in range(20):
                legs[0][1]()
            torch.cuda.synchronize()
            say("leg A, %d streams of %d bytes in blocks of %d, %d needles: 20 calls, total %d, stats %s, %d bytes of plan home per call" % (n, size, bs, npat, got["A"][0], got["A"][2], got["A home"]))
            continue
        # the checks first, on the host: counts by brute force, the plan by the model
        for _, f in legs:
            f()
        torch.cuda.synchronize()
        want = PM.result([d.tobytes() for d in datas], pats)
        for k in "ABCD":
            assert got[k][0] == want["total"] == 3 * npat and got[k][1] == want["counts"], k
        enc_h = enc.cpu().numpy()
        m = PM.plan([enc_h[i * slot:i * slot + res[i]].tobytes() for i in range(n)], pats)
        sa, sc = got["A"][2], got["C"][2]
        assert (sa[1], sa[4], sa[5]) == (m["decoded"], m["tabbed"], m["skipped"]) and got["B"][2][1] == got["D"][2][1] == sc[1] == sc[0], (sa, sc, m["decoded"])
        say("%d streams of %d bytes in blocks of %d (%.1f MB raw, %.1f MB of streams with tables, %.1f MB without), %d needles; %d repetitions, the calls alternated" %
            (n, size, bs, n * size / 1e6, sum(res) / 1e6, sum(bare_res) / 1e6, npat, REPS))
        assert got["A home"] == 17 * n + 8 + sa[0] <= 32 * n + sa[0] and got["C home"] == 16 * n, (got["A home"], got["C home"])
        say("    A decodes %d of %d chunks (%d with a usable table) and skips %d of %d streams; the model agrees.  Its plan brings %d bytes to the host (the bound: %d), C's %d" %
            (sa[1], sa[0], sa[4], sa[5], n, got["A home"], 32 * n + sa[0], got["C home"]))
        ts = timed(legs)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            v = sorted(ts[k])
            say("    %2d needles %-2s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (npat, k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
        held = med["B"] - med["A"] > max(iqr(ts["A"]), iqr(ts["B"]))
        barred = size > 4 << 10
        say("    %2d needles: B / A = %.2f, C / D = %.2f; the bar (A below B by more than both IQRs): %s" %
            (npat, med["B"] / med["A"], med["C"] / med["D"], ("held" if held else "MISSED") if barred else "none at this shape (A %s B)" % ("below" if held else "NOT below")))
        results["%dx%d_%d" % (n, size, npat)] = dict({k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()},
                                                     decoded=sa[1], chunks=sa[0], skipped=sa[5], bar_held=held if barred else None)
        del enc, bare
say(json.dumps(results))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
