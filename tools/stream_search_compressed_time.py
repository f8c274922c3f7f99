"""Searches through compressed block search tables (chunk 0x46) against the same searches through uncompressed ones (0x45), on an MI355X:
one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and interquartile ranges, a device
synchronise inside every timed window.
Input: 100 MB json-like (FRACTION of it with FRACTION=4: a quarter), LevelFastest, 1 MiB blocks, type 1 tables with M = 6, written by the
device Writer with 0x45 tables (the twin) and rewritten by tests/search_compressed_model.py with the reference's partition (the 0x46
stream: the same data chunks).  The needle is planted in three places.

  steady      a search on a handle whose tables are located and expanded, 0x46 stream against 0x45 twin (the plan kernel reads the same
              bitmaps: the expectation is equality; the bar: the medians lie apart by no more than the larger interquartile range)
  first       per repetition a fresh handle on the 0x46 stream: its first search (locate, expansion, CRC included) and its second;
              the same on the twin; and MLZ_SEARCH_NO_TABLES on the 0x46 stream, which is what a library from before the feature does
              with this stream (PARENT_RESULT = the out.txt of a run of this tool on the parent commit's library gives that library's own
              median).  The bar: first + second < 2 x the parent's median, beyond the interquartile ranges.
  sizes       the two streams, the table chunks alone, and the arena (the expanded bitmaps of the 0x46 tables)

With ONE_CALL=1 the tool opens four handles on the 0x46 stream, searches once on each and does nothing else (the profiler's run: a
quarter of the totals of cst_parse_kernel, cst_expand_kernel and the CRC kernels is one handle's expansion).
A library from before the feature is noticed (counter 11 is 0 on the 0x46 stream): only its searches of that stream are timed.

usage: python tools/stream_search_compressed_time.py [out.txt]"""
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
from tests import search_compressed_model as CM
from tests import search_model as SM

REPS = 25
BS, M = 1 << 20, 6
FRACTION = int(os.environ.get("FRACTION", "1"))
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


NEEDLE = b"#4711-a/Zqxjkv"
n_bytes = 100_000_000 // FRACTION
d = bytearray(synth.json_like(n_bytes, seed=1).tobytes())
nblk = n_bytes // BS
for o in (3 * BS + BS // 3, (nblk // 2) * BS + 17, (nblk - 5) * BS - 3):
    d[o:o + len(NEEDLE)] = NEEDLE
d = bytes(d)
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4 | M << 8)
buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
size45 = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], buf.data_ptr(), cap, search_match_len=M)
twin = buf[:size45].cpu().numpy().tobytes()
t0 = time.perf_counter()
comp = CM.recompress_stream(twin)
t_model = time.perf_counter() - t0
tab45 = sum(4 + n for _, t, n in SM.chunks_of(twin) if t == 0x45)
tab46 = sum(4 + n for _, t, n in SM.chunks_of(comp) if t == 0x46)
arena = sum(n - 8 for _, t, n in SM.chunks_of(twin) if t == 0x45)
n46 = sum(1 for _, t, _ in SM.chunks_of(comp) if t == 0x46)
s45 = torch.from_numpy(np.frombuffer(twin, np.uint8).copy()).cuda()
s46 = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).cuda()
CAP = 1 << 12
pos = torch.empty(CAP, dtype=torch.int64, device="cuda")


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def search(rd, **kw):
    return rd.search(NEEDLE, pos.data_ptr(), CAP, **kw)


if os.environ.get("ONE_CALL"):
    for _ in range(4):
        rd = ctx.stream_open_device(s46.data_ptr(), len(comp))
        search(rd)
        torch.cuda.synchronize()
        rd.close()
    sys.exit(0)

rd45, rd46 = ctx.stream_open_device(s45.data_ptr(), len(twin)), ctx.stream_open_device(s46.data_ptr(), len(comp))
for _ in range(3):
    for rd in (rd45, rd46):
        total, st = search(rd)
        assert total == 3
        search(rd, no_tables=True)
        torch.cuda.synchronize()
st45, st46 = search(rd45)[1], search(rd46)[1]
feature = st46[2] > 0
ts = {k: [] for k in ("steady_45", "steady_46", "all_46", "first_46", "second_46", "first_45", "second_45")}
for _ in range(REPS):
    ts["steady_45"].append(timed(lambda: search(rd45))[0])
    if feature:
        ts["steady_46"].append(timed(lambda: search(rd46))[0])
    ts["all_46"].append(timed(lambda: search(rd46, no_tables=True))[0])
    for name, t, n in (("46", s46, len(comp)), ("45", s45, len(twin))):
        if name == "46" and not feature:
            continue
        fresh = ctx.stream_open_device(t.data_ptr(), n)
        ts["first_" + name].append(timed(lambda: search(fresh))[0])
        ts["second_" + name].append(timed(lambda: search(fresh))[0])
        fresh.close()
ts = {k: v for k, v in ts.items() if v}
med = {k: statistics.median(v) for k, v in ts.items()}
say("%d MB json-like, LevelFastest, 1 MiB blocks, type 1 tables (M = 6); %d repetitions, the calls alternated; library %s: %s" %
    (n_bytes // 1_000_000, REPS, os.path.basename(os.path.dirname(os.environ.get("MINLZ_HIP_LIB", "")) or "this tree's"),
     "0x46 tables are read" if feature else "0x46 TABLES ARE STEPPED OVER (a library from before the feature)"))
say("  streams: 0x45 twin %d B, 0x46 stream %d B (%.2f %% smaller); table chunks %d B -> %d B (%.1f %%); %d tables, arena %d B; the model wrote them in %.1f s" %
    (len(twin), len(comp), 100 * (len(twin) - len(comp)) / len(twin), tab45, tab46, 100 * tab46 / tab45, n46, arena, t_model))
say("  plan: twin decodes %d of %d chunks with %d usable tables; 0x46 stream %d of %d with %d" % (st45[1], st45[0], st45[2], st46[1], st46[0], st46[2]))
for k, v in ts.items():
    s = sorted(v)
    say("  %-10s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], s[0], s[int(0.9 * (len(s) - 1))], iqr(v)))
result = {"feature": feature, "stream45": len(twin), "stream46": len(comp), "tables45": tab45, "tables46": tab46, "arena": arena,
          **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}
verdicts = {}
if feature:
    gap, width = abs(med["steady_46"] - med["steady_45"]), max(iqr(ts["steady_46"]), iqr(ts["steady_45"]))
    verdicts["steady"] = "held" if gap <= width else "MISSED"
    say("  steady: the medians lie %.3f ms apart, the larger interquartile range is %.3f ms: %s" % (gap, width, verdicts["steady"]))
    yard, yard_iqr, whose = med["all_46"], iqr(ts["all_46"]), "this library's MLZ_SEARCH_NO_TABLES"
    parent = os.environ.get("PARENT_RESULT")
    if parent:
        pr = json.loads([ln for ln in open(parent).read().splitlines() if ln.strip().startswith("{")][-1])
        yard, yard_iqr, whose = pr["all_46"], pr["all_46_iqr"], "the parent library's MLZ_SEARCH_NO_TABLES search of the 0x46 stream"
        say("  the parent library on the 0x46 stream: default search %.3f ms, MLZ_SEARCH_NO_TABLES %.3f ms (IQR %.3f)" % (pr.get("default_46", pr["all_46"]), pr["all_46"], pr["all_46_iqr"]))
    both = med["first_46"] + med["second_46"]
    slack = iqr(ts["first_46"]) + iqr(ts["second_46"]) + 2 * yard_iqr
    verdicts["pays_by_second"] = "held" if both + slack < 2 * yard else "MISSED"
    verdicts["pays_at_first"] = "yes" if med["first_46"] + iqr(ts["first_46"]) + yard_iqr < yard else "no"
    say("  first search %.3f ms + second %.3f ms = %.3f ms against 2 x %.3f ms = %.3f ms (%s), interquartile ranges together %.3f ms: %s; pays at the first search: %s" %
        (med["first_46"], med["second_46"], both, yard, 2 * yard, whose, slack, verdicts["pays_by_second"], verdicts["pays_at_first"]))
    say("  the expansion's share: first search on the 0x46 stream %.3f ms against %.3f ms on the twin (both locate, check CRCs and allocate)" % (med["first_46"], med["first_45"]))
else:
    ts_def = [timed(lambda: search(rd46))[0] for _ in range(REPS)]
    result["default_46"] = round(statistics.median(ts_def), 4)
    say("  default_46 median %8.3f ms   IQR %7.3f   (the default search of the 0x46 stream: no table is found, every chunk is decoded)" % (result["default_46"], iqr(ts_def)))
result["verdicts"] = verdicts
say("  " + json.dumps(result))
rd45.close()
rd46.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
