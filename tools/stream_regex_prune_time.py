"""mlz_dev_reader_grep_regex_pruned on an MI355X against the unpruned call of the parent commit's library: one process, every call warmed up, REPS
timed repetitions with the calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, table type 1 with match length 6, the newline index built beforehand; an id planted three times
(in the middle of a block, across a block border, in the stream's last block).

  PARENT_LIB      the parent commit's libminlz_hip.so, loaded into this process beside this tree's with a context and a handle of its own (this tree's
                  own library where the variable is not set: the rows then compare this tree with itself)
  selective       #4711-[a-z]: three matching lines.  pruned / unpruned (this tree) / parent unpruned, and mlz_dev_reader_grep_records of the bare
                  literal with the tables, the floor of this design.  Bar 1: pruned below the parent's unpruned, beyond both interquartile ranges.
  no literals     ^$: pruned / unpruned / parent unpruned.  Bar 2: pruned within the parent's unpruned by no more than the two interquartile ranges.
  everywhere      "user_3[0-9]{2}7": its literal lies in every chunk; the price of the plan when nothing is pruned.  No bar.
Every row is checked first against Python's `re` on the host (the count of matching lines).  With KERNELS_ONLY=1 only one call of each pruned row is run,
for a kernel trace of its own.

usage: python tools/stream_regex_prune_time.py [out.txt]"""
import ctypes as C
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
from minlz_amd import _lib, api, synth

REPS = 25
BS = 1 << 20
M = 6
ID = b"#4711-"
EXPRS = {"selective": b"#4711-[a-z]", "no literals": b"^$", "everywhere": b'"user_3[0-9]{2}7"'}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


class Lib:
    """A library loaded by path, with a context of its own: open, index, compile and the unpruned grep, through plain ctypes."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.h = C.c_void_p()
        assert self.L.mlz_init(0, C.byref(self.h)) == 0
        for name in ("mlz_stream_open_device", "mlz_dev_reader_index_records", "mlz_regex_compile", "mlz_dev_reader_grep_regex"):
            f = getattr(self.L, name)
            f.restype, f.argtypes = (_lib.ABI.get(name) or _lib.ABI_EXT["minlz_hip_regex.h"][name])

    def open(self, t, n):
        rd = C.c_void_p()
        assert self.L.mlz_stream_open_device(self.h, None, t.data_ptr(), n, C.byref(rd)) >= 0
        info = (C.c_uint64 * 4)()
        assert self.L.mlz_dev_reader_index_records(rd, None, 0, 10, info) > 0
        return rd

    def compile(self, expr):
        rx = C.c_void_p()
        assert self.L.mlz_regex_compile(expr, (C.c_uint32 * 1)(len(expr)), 1, 0, C.byref(rx), None) == 0
        return rx

    def grep(self, rd, rx, no, kd, cap):
        stats = (C.c_uint64 * 4)()
        r = self.L.mlz_dev_reader_grep_regex(rd, None, 0, rx, 0, 0, no.data_ptr(), kd.data_ptr(), cap, None, stats)
        assert r >= 0, r
        return r, tuple(int(v) for v in stats)


d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
nblk = len(d) // BS
for o, variant in ((3 * BS + BS // 3, b"#4711-a"), ((nblk // 2) * BS - 3, b"#4711-m"), (nblk * BS + 1000, b"#4711-z")):
    d[o:o + len(variant)] = variant
d = bytes(d)
assert d.count(ID) == 3
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
ctx = mz.Context(0)
parent = Lib(os.environ.get("PARENT_LIB") or _lib.SO)
whose = "the parent commit's library" if os.environ.get("PARENT_LIB") else "this tree's own library (no PARENT_LIB)"
cap = api.stream_bound(len(d), BS, search_match_len=M)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap, search_match_len=M)
rd = ctx.stream_open_device(stream.data_ptr(), size)
N = rd.index_records(b"\n")[0]
prd = parent.open(stream, size)
rec_no = torch.empty(N + 1, dtype=torch.int64, device="cuda")
rec_kind = torch.empty(N + 1, dtype=torch.uint8, device="cuda")
compiled = {k: api.Regex(e) for k, e in EXPRS.items()}
pcompiled = {k: parent.compile(e) for k, e in EXPRS.items()}
recs = d.split(b"\n")
if not recs[-1]:
    recs.pop()
assert len(recs) == N
stats_of = {}


def pruned(name):
    r, _, st = rd.grep_regex(compiled[name], rec_no.data_ptr(), rec_kind.data_ptr(), N, prune=True)
    stats_of[name] = st
    return r


def unpruned(name):
    return rd.grep_regex(compiled[name], rec_no.data_ptr(), rec_kind.data_ptr(), N)[0]


def parent_unpruned(name):
    return parent.grep(prd, pcompiled[name], rec_no, rec_kind, N)[0]


def fixed():
    r, _, st = rd.grep_records([ID], rec_no.data_ptr(), rec_kind.data_ptr(), N)
    stats_of["fixed"] = st
    return r


if os.environ.get("KERNELS_ONLY"):
    for name in EXPRS:
        pruned(name)
        torch.cuda.synchronize()
    sys.exit(0)

# the checks first: the host's `re` is the reference
found = {}
for name, e in EXPRS.items():
    p = re.compile(e.replace(b"^", b"\\A").replace(b"$", b"\\Z"), re.DOTALL)
    found[name] = sum(1 for r in recs if p.search(r))
    for f in (pruned, unpruned, parent_unpruned):
        got = f(name)
        torch.cuda.synchronize()
        assert got == found[name], (name, f.__name__, got, found[name])
assert found["selective"] == 3 and fixed() == 3

fs = [("fixed " + ID.decode(), fixed)]
for name in EXPRS:
    fs += [(name + ": pruned", lambda n=name: pruned(n)), (name + ": unpruned", lambda n=name: unpruned(n)), (name + ": parent unpruned", lambda n=name: parent_unpruned(n))]
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

say("100 MB json-like, LevelFastest, 1 MiB blocks, table type 1, M = %d, stream %d B, %d records; %d repetitions, the calls alternated; the yardstick is %s" %
    (M, size, N, REPS, whose))
for k, _ in fs:
    v = sorted(ts[k])
    name = k.partition(":")[0]
    extra = ""
    if k.endswith(": pruned"):
        st = stats_of[name]
        extra = "   %d lines; literals %r; %d chunks, %d decoded, %d with a usable table, %d planned" % ((found[name], compiled[name].literals()[0]) + st)
    elif k.startswith("fixed"):
        extra = "   %d chunks, %d decoded" % stats_of["fixed"][:2]
    say("  %-30s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f%s" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k]), extra))
a, b = "selective: pruned", "selective: parent unpruned"
margin = med[b] - med[a] - max(iqr(ts[a]), iqr(ts[b]))
say("  bar 1, selective: pruned %.3f ms against the parent's unpruned %.3f ms: %s; grep_records of the bare literal %.3f ms" %
    (med[a], med[b], "met, %.2f x faster" % (med[b] / med[a]) if margin > 0 else "MISSED (the medians are %.3f ms apart, the larger interquartile range is %.3f ms)" %
     (med[b] - med[a], max(iqr(ts[a]), iqr(ts[b]))), med["fixed " + ID.decode()]))
a, b = "no literals: pruned", "no literals: parent unpruned"
slack = iqr(ts[a]) + iqr(ts[b])
say("  bar 2, no literals: pruned %.3f ms against the parent's unpruned %.3f ms, the two interquartile ranges are %.3f ms: %s" %
    (med[a], med[b], slack, "met" if med[a] - med[b] <= slack else "MISSED by %.3f ms" % (med[a] - med[b] - slack)))
say("  unpruned, this tree against the parent: " + ", ".join("%s %.3f / %.3f ms" % (n, med[n + ": unpruned"], med[n + ": parent unpruned"]) for n in EXPRS))
say("  " + json.dumps({"stream": size, "records": N, **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
