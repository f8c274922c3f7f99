"""MLZ_SEARCH_IGNORE_CASE against the unflagged searches, on an MI355X: one process, every call warmed up, REPS timed repetitions with the
calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables with M = 6.  Three needle sets:

  few       an id with few letters, '#4711-a', planted in three places in other cases (windows of at most one letter: the tables prune)
  word      a word of six letters, planted likewise (its one window is above the letter cap: not served, every chunk decoded)
  sixteen   the few-letter needle and 15 pieces of 16 bytes from random places of the data, in swapped case (search_many)

Per set, with the tables and under MLZ_SEARCH_NO_TABLES: the unflagged call and the flagged call — time, chunks decoded of data chunks,
usable tables, occurrences.  The library is the one MINLZ_HIP_LIB names (default: this tree's); a library from before the flag ignores the
bit, which the tool notices (the flagged call finds what the unflagged one finds) and says.

The bars (environment: PARENT_RESULT = the out.txt of a run of this tool on the parent commit's library, SCAN_KERNEL_MS = the parent's
search_scan_kernel time for one unflagged MLZ_SEARCH_NO_TABLES search of `few`, from a `rocprofv3 --kernel-trace --stats` run of its own):
  1  flagged NO_TABLES search of `few` <= the parent's unflagged NO_TABLES search + SCAN_KERNEL_MS (folding may at most double the scan)
  2  every unflagged row of this library within the parent's interquartile range of that row (the templates cost nothing)
  3  `few`, flagged, with tables: fewer chunks decoded than there are data chunks

With ONE_CALL=1 the tool makes four unflagged MLZ_SEARCH_NO_TABLES searches of `few` and nothing else (the profiler's run: a quarter of
search_scan_kernel's total duration is one search's scan).

usage: python tools/stream_search_fold_time.py [out.txt]"""
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


FEW, WORD = b"#4711-a", b"Zqxjkv"
d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
for o, f in ((3 * BS + BS // 3, bytes.upper), (50 * BS + 17, bytes.lower), (90 * BS - 3, bytes.swapcase)):
    d[o:o + len(FEW)] = f(FEW)
    d[o + 64:o + 64 + len(WORD)] = f(WORD)
d = bytes(d)
rng = np.random.default_rng(16)
sixteen = [FEW]
while len(sixteen) < 16:
    o = int(rng.integers(0, len(d) - 16))
    if b"\n" not in d[o:o + 16] and d.count(d[o:o + 16]) <= 10:
        sixteen.append(d[o:o + 16].swapcase())
sets = {"few": [FEW], "word": [WORD], "sixteen": sixteen}

src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4 | M << 8)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap, search_match_len=M)
rd = ctx.stream_open_device(stream.data_ptr(), size)
CAP = 1 << 16
pos = torch.empty(CAP, dtype=torch.int64, device="cuda")
which = torch.empty(CAP, dtype=torch.int32, device="cuda")
counts = torch.empty(16, dtype=torch.int64, device="cuda")
seen = {}


def run(name, flagged, no_tables):
    pats = sets[name]
    kw = dict(no_tables=no_tables, ignore_case=flagged)
    if len(pats) == 1:
        total, st = rd.search(pats[0], pos.data_ptr(), CAP, **kw)
    else:
        total, st = rd.search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), CAP, **kw)
    seen[(name, flagged, no_tables)] = (total, st)


def key(name, flagged, no_tables):
    return "%s_%s_%s" % (name, "fold" if flagged else "plain", "all" if no_tables else "tables")


if os.environ.get("ONE_CALL"):   # the profiler's run: four calls of one kind, so the kernel's total over four is one call's time
    for _ in range(4):
        run("few", False, True)
        torch.cuda.synchronize()
    rd.close()
    sys.exit(0)

fs = [(key(n, f, a), lambda n=n, f=f, a=a: run(n, f, a)) for n in sets for a in (False, True) for f in (False, True)]
for _ in range(3):
    for _, f in fs:
        f()
        torch.cuda.synchronize()
honoured = seen[("few", True, True)][0] != seen[("few", False, True)][0]
fd = d.lower()
if honoured:   # the flagged calls find what a folded search of the host's copy finds
    assert seen[("few", True, False)][0] == seen[("few", True, True)][0] == fd.count(FEW.lower()) == 3
    assert seen[("word", True, False)][0] == seen[("word", True, True)][0] == fd.count(WORD.lower()) == 3
    assert seen[("sixteen", True, False)][0] == seen[("sixteen", True, True)][0] == sum(fd.count(p.lower()) for p in sixteen)
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


say("100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables (M = 6), stream %d B; %d repetitions, the calls alternated; library %s: %s" %
    (size, REPS, os.path.basename(os.environ.get("MINLZ_HIP_LIB", "libminlz_hip.so")), "the flag is honoured" if honoured else "THE FLAG IS IGNORED (a library from before it)"))
for n in sets:
    for a in (False, True):
        for f in (False, True):
            k = key(n, f, a)
            total, st = seen[(n, f, a)]
            v = sorted(ts[k])
            say("  %-22s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f   decoded %3d of %3d chunks, %3d usable tables%s, %d found" %
                (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k]), st[1], st[0], st[2], ", %d not served" % st[3] if len(st) > 3 else "", total))
result = {"stream": size, "honoured": honoured, **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()},
          **{key(*k) + "_decoded": v[1][1] for k, v in seen.items()}}
verdicts = {}
if honoured:
    total, st = seen[("few", True, False)]
    verdicts["bar3"] = "held" if st[1] < st[0] else "MISSED"
    say("  bar 3: few, flagged, with tables: %d of %d chunks decoded: %s" % (st[1], st[0], verdicts["bar3"]))
parent = os.environ.get("PARENT_RESULT")
if parent and honoured:
    pr = json.loads([ln for ln in open(parent).read().splitlines() if ln.strip().startswith("{")][-1])
    worst = None
    for k in med:
        if "_plain_" in k:
            off = abs(med[k] - pr[k])
            inside = off <= pr[k + "_iqr"]
            say("  bar 2: %-22s %8.3f ms against the parent's %8.3f ms (IQR %.3f): %s" % (k, med[k], pr[k], pr[k + "_iqr"], "within" if inside else "OUTSIDE"))
            worst = worst or not inside
    verdicts["bar2"] = "MISSED" if worst else "held"
    scan = os.environ.get("SCAN_KERNEL_MS")
    if scan:
        limit = pr["few_plain_all"] + float(scan)
        verdicts["bar1"] = "held" if med["few_fold_all"] <= limit else "MISSED"
        say("  bar 1: few, flagged, NO_TABLES %8.3f ms against the parent's unflagged %8.3f ms + its scan kernel %8.3f ms = %8.3f ms: %s" %
            (med["few_fold_all"], pr["few_plain_all"], float(scan), limit, verdicts["bar1"]))
result["verdicts"] = verdicts
say("  " + json.dumps(result))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
