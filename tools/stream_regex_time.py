"""mlz_dev_reader_grep_regex on an MI355X beside the calls it shares its phases with: one process, every call warmed up, REPS timed repetitions
with the calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, no tables, the newline index built beforehand (tools/grep_records_time.py's stream).

  index            mlz_dev_reader_index_records for another delimiter and back: two decodes of every chunk with the count / scan / emit kernels and
                   a total home per group
  fixed_<literal>  mlz_dev_reader_grep_records with one literal under MLZ_SEARCH_NO_TABLES: the fixed-string scan of every chunk
  regex_<name>     mlz_dev_reader_grep_regex, every record number written:
                     literal      the same literal as an expression (a match ends a lane's walk early)
                     class        "status"-like: a class with a counted repetition
                     words        an alternation of three words
                     head         ^\\{ : decided by a record's first byte
                     tail         \\}$ : no early exit, every byte of every record is stepped
                     empty        ^$
                     nothing      an expression that never matches and never dies: the full walk of every record
                     wide         (hot!){200}: a table of about 800 states
  The figure of merit is decoded bytes per second of a call, 100 MB over its median; "walk" is the call's median less regex_empty's, whose lanes
  stop in front of every record's first byte: an estimate of what stepping through the bytes costs, not a kernel time.
Every regex row is checked first against Python's `re` on the host (the count of matching lines).

usage: python tools/stream_regex_time.py [out.txt]"""
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import minlz_amd as mz
from minlz_amd import api, synth

REPS = 15
BS = 1 << 20
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
half = len(d) // 2
d[half:half + 4000] = bytes(d[half:half + 4000]).replace(b"\n", b" ")
d[half + 100:half + 100 + 1200] = b"hot!" * 300
d = bytes(d)
LITERAL = b"user_3434"
EXPRS = {"literal": LITERAL, "class": b'"user_3[0-9]{2}7"', "words": b"DON'T|flushed|laws-a-me", "head": b"^\\{", "tail": b"\\}$", "empty": b"^$",
         "nothing": b"nomatch[0-9]+zz$", "wide": b"(hot!){200}"}

src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = api.stream_bound(len(d), BS, False)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap)
rd = ctx.stream_open_device(stream.data_ptr(), size)
N = rd.index_records(b"\n")[0]
rec_no = torch.empty(N + 1, dtype=torch.int64, device="cuda")
rec_kind = torch.empty(N + 1, dtype=torch.uint8, device="cuda")
compiled = {k: api.Regex(e) for k, e in EXPRS.items()}
recs = d.split(b"\n")
if not recs[-1]:
    recs.pop()
assert len(recs) == N


def run_regex(name):
    return rd.grep_regex(compiled[name], rec_no.data_ptr(), rec_kind.data_ptr(), N)[0]


def run_fixed():
    return rd.grep_records([LITERAL], rec_no.data_ptr(), rec_kind.data_ptr(), N, no_tables=True)[0]


def run_index():
    rd.index_records(b",")
    rd.index_records(b"\n")


# the checks first: the host's `re` is the reference
found = {}
for name, e in EXPRS.items():
    p = re.compile(e.replace(b"^", b"\\A").replace(b"$", b"\\Z"), re.DOTALL)
    want = sum(1 for r in recs if p.search(r))
    got = run_regex(name)
    torch.cuda.synchronize()
    assert got == want, (name, got, want)
    found[name] = got
assert run_fixed() == found["literal"]

fs = [("index", run_index), ("fixed_literal", run_fixed)] + [("regex_" + k, lambda n=k: run_regex(n)) for k in EXPRS]
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
med = {k: statistics.median(v) for k, v in ts.items()}


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


say("100 MB json-like, LevelFastest, 1 MiB blocks, no tables, stream %d B, %d records, the longest %d B; %d repetitions, the calls alternated" %
    (size, N, max(map(len, recs)), REPS))
for k, _ in fs:
    v = sorted(ts[k])
    extra = ""
    if k.startswith("regex_"):
        S, C, image, _ = compiled[k[6:]].info()
        extra = "   %6.1f GB/s   walk ~%6.3f ms   %d lines, %d states x %d classes, %d B in LDS" % (len(d) / med[k] / 1e6, med[k] - med["regex_empty"], found[k[6:]], S, C, image)
    elif k == "fixed_literal":
        extra = "   %6.1f GB/s" % (len(d) / med[k] / 1e6)
    say("  %-16s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f%s" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k]), extra))
say("  " + json.dumps({"stream": size, "records": N, **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
