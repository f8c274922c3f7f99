"""The search that returns records (mlz_dev_reader_search_records) against what a caller pays today to get at the lines without leaving the
device — mlz_dev_reader_search plus mlz_stream_decode_device of the whole stream — on an MI355X: one process, every call warmed up, REPS
timed repetitions with the calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables with M = 6, newline delimiter; a selective needle (16 bytes planted in
three places) and a dense one (a piece of the records chosen on the host for about 10^5 occurrences).

  t_records_<n>   mlz_dev_reader_search_records with needle n (every record written: the caps hold them all)
  t_count_<n>     the counting form (rec_cap = dst_cap = 0)
  t_search_<n>    mlz_dev_reader_search alone with the same pattern (64 positions)
  t_all           mlz_stream_decode_device of the whole stream

The bar, for the selective needle: t_records < t_search + t_all.  The ratio t_records / t_search is reported.

usage: python tools/stream_records_time.py [out.txt]"""
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

REPS = 25
BS, M = 1 << 20, 6
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
selective = b'"id":"' + np.random.default_rng(1).integers(97, 123, 10, dtype=np.uint8).tobytes()
for o in (3 * BS + BS // 3, 50 * BS + 17, 90 * BS - 8):
    d[o:o + 16] = selective
d = bytes(d)
# the dense needle: the piece of the first records (between quotes and commas, at least M bytes) whose count is nearest to 10^5
cands = sorted({p for rec in d[:4000].split(b"\n")[:8] for q in rec.split(b'"') for p in q.split(b",") if len(p) >= M and b"\n" not in p})
counts = {p: d.count(p) for p in cands}
dense = min(cands, key=lambda p: abs(np.log(max(counts[p], 1) / 1e5)))
needles = {"selective": selective, "dense": dense}

src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4 | M << 8)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap, search_match_len=M)
rd = ctx.stream_open_device(stream.data_ptr(), size)
out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
pos = torch.zeros(64, dtype=torch.int64, device="cuda")
REC_CAP, DST_CAP = 1 << 19, 128 << 20
dst = torch.empty(DST_CAP, dtype=torch.uint8, device="cuda")
rec_off = torch.empty(REC_CAP, dtype=torch.int64, device="cuda")
rec_start = torch.empty(REC_CAP + 1, dtype=torch.int64, device="cuda")
rec_flags = torch.empty(REC_CAP, dtype=torch.uint8, device="cuda")
seen = {}


def records(n, count=False):
    if count:
        R, totals, st = rd.search_records(needles[n], b"\n", None, 0, None, None, None, 0)
    else:
        R, totals, st = rd.search_records(needles[n], b"\n", dst.data_ptr(), DST_CAP, rec_off.data_ptr(), rec_start.data_ptr(), rec_flags.data_ptr(), REC_CAP)
        assert R <= REC_CAP and totals[1] <= DST_CAP
    seen[n] = (R, totals, st, ctx.range_plan()[0])


def search(n):
    total, st = rd.search(needles[n], pos.data_ptr(), 64)
    assert total == seen[n][1][2]


def decode_all():
    assert ctx.stream_decode_device(stream.data_ptr(), size, out.data_ptr(), len(d)) == len(d)


fs = []
for n in needles:
    fs += [("t_records_" + n, (lambda n=n: records(n))), ("t_count_" + n, (lambda n=n: records(n, True))), ("t_search_" + n, (lambda n=n: search(n)))]
fs.append(("t_all", decode_all))
for _ in range(3):
    for _, f in fs:
        f()
        torch.cuda.synchronize()
assert out[:len(d)].cpu().numpy().tobytes() == d
# the records are the lines that hold the needle (the host's split is the reference here; no line of this input is longer than the reach)
for n in needles:
    records(n)
    torch.cuda.synchronize()
    R, totals = seen[n][0], seen[n][1]
    want = [ln for ln in d.split(b"\n") if needles[n] in ln]
    st = rec_start[:R + 1].cpu().numpy()
    got = dst[:int(st[R])].cpu().numpy().tobytes()
    assert R == len(want) and totals[3] == 0 and got == b"".join(want), n
ts = {k: [] for k, _ in fs}
for _ in range(REPS):
    for k, f in fs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts[k].append((time.perf_counter() - t0) * 1e3)
med = {k: statistics.median(v) for k, v in ts.items()}


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


say("100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables, M = %d, stream %d B; %d repetitions, the calls alternated" % (M, size, REPS))
for n in needles:
    R, totals, st, read_chunks = seen[n]
    say("  %-9s %r: %d occurrences in %d records of %d bytes; search phase %d of %d chunks (%d usable tables), read phase %d chunks" %
        (n, needles[n], totals[2], R, totals[1], st[1], st[0], st[2], read_chunks))
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-20s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
for n in needles:
    r, s = med["t_records_" + n], med["t_search_" + n]
    say("  %-9s t_records %.3f ms %s t_search + t_all %.3f ms;  t_records / t_search = %.2f" % (n, r, "<" if r < s + med["t_all"] else ">=", s + med["t_all"], r / s))
held = med["t_records_selective"] < med["t_search_selective"] + med["t_all"]
say("  the bar (selective needle: t_records < t_search + t_all): %s" % ("held" if held else "FAILED"))
say("  " + json.dumps({"stream": size, "occurrences": {n: seen[n][1][2] for n in needles}, "records": {n: seen[n][0] for n in needles},
                       "bar_held": held, **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
