"""mlz_dev_reader_grep_records against the composition it replaces, on an MI355X: one process, every call warmed up, REPS timed repetitions
with the calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables with M = 6, the newline index built beforehand.  Three needle sets: the
selective needle of tools/stream_records_time.py (16 bytes planted in three places), 16 needles (that one and 15 pieces of 16 bytes from
random places of the data that occur at most ten times), and that tool's dense needle (a piece of the records with about 10^5 / 2 occurrences).

  A_<set>          grep_records (every record number written), then read_records of its result
  B_<set>          the composition through the interface without the call: search_many with cap = 0 for the total, search_many with
                   cap = total, record_numbers over the positions, torch.unique, read_records
  grep_<set>       grep_records alone; grep_inv_<set> with MLZ_GREP_INVERT; grep_ctx_<set> with before = after = 2
  select_count     the select and compact kernels alone: no patterns, MLZ_GREP_INVERT, rec_cap = 0 (every record selected, none written)
  select_write     ... with rec_cap = N (every record number and kind written)

In a tree without the call (the parent commit) only the B rows are timed: that figure is the yardstick, and B in the new tree shows that it
did not move.  The bar: A's median below B's for each set; medians closer than their interquartile ranges count as equal.

usage: python tools/grep_records_time.py [out.txt]"""
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
from minlz_amd.api import DeviceReader

REPS = 25
BS, M = 1 << 20, 6
HAVE = hasattr(DeviceReader, "grep_records")
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
cands = sorted({p for rec in d[:4000].split(b"\n")[:8] for q in rec.split(b'"') for p in q.split(b",") if len(p) >= M and b"\n" not in p})
counts = {p: d.count(p) for p in cands}
dense = min(cands, key=lambda p: abs(np.log(max(counts[p], 1) / 1e5)))
rng = np.random.default_rng(16)
sixteen = [selective]
while len(sixteen) < 16:   # rare ones: a piece that occurs more than ten times is passed over
    o = int(rng.integers(0, len(d) - 16))
    if b"\n" not in d[o:o + 16] and d.count(d[o:o + 16]) <= 10:
        sixteen.append(d[o:o + 16])
sets = {"selective": [selective], "sixteen": sixteen, "dense": [dense]}

src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4 | M << 8)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap, search_match_len=M)
rd = ctx.stream_open_device(stream.data_ptr(), size)
N = rd.index_records(b"\n")[0]
DST_CAP = 128 << 20
dst = torch.empty(DST_CAP, dtype=torch.uint8, device="cuda")
rec_no = torch.empty(N + 1, dtype=torch.int64, device="cuda")
rec_kind = torch.empty(N + 1, dtype=torch.uint8, device="cuda")
starts = torch.empty(N + 2, dtype=torch.int64, device="cuda")
seen = {}


def run_a(name):
    R, totals, st = rd.grep_records(sets[name], rec_no.data_ptr(), rec_kind.data_ptr(), N)
    got = rd.read_records(rec_no.data_ptr(), R, dst.data_ptr(), totals[2], d_starts=starts.data_ptr()) if R else 0
    seen["A_" + name] = (R, got, st)
    return rec_no[:R]


def run_b(name):
    pats = sets[name]
    total, st = rd.search_many(pats, None, None, None, 0)
    pos = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
    which = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    rd.search_many(pats, None, pos.data_ptr(), which.data_ptr(), total)
    no = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
    rd.record_numbers(pos.data_ptr(), total, no.data_ptr())
    u = torch.unique(no[:total])
    got = rd.read_records(u.data_ptr(), u.numel(), dst.data_ptr(), DST_CAP, d_starts=starts.data_ptr()) if u.numel() else 0
    seen["B_" + name] = (u.numel(), got, st, total)
    return u


def grep_only(name, **kw):
    return rd.grep_records(sets[name], rec_no.data_ptr(), rec_kind.data_ptr(), N, **kw)[0]


def select_only(write):
    R = rd.grep_records([], rec_no.data_ptr() if write else None, rec_kind.data_ptr() if write else None, N if write else 0, invert=True)[0]
    assert R == N


# the checks first: both ways give the lines that hold a needle (the host's split is the reference)
for name, pats in sets.items():
    u = run_b(name)
    torch.cuda.synchronize()
    want = [i for i, ln in enumerate(d.split(b"\n")) if any(p in ln for p in pats)] if name != "dense" else None
    if want is not None:
        assert u.cpu().tolist() == want, name
    if HAVE:
        a = run_a(name)
        torch.cuda.synchronize()
        assert torch.equal(a, u) and seen["A_" + name][:2] == seen["B_" + name][:2], name

fs = []
for name in sets:
    if HAVE:
        fs.append(("A_" + name, lambda n=name: run_a(n)))
    fs.append(("B_" + name, lambda n=name: run_b(n)))
if HAVE:
    for name in sets:
        fs += [("grep_" + name, lambda n=name: grep_only(n)), ("grep_inv_" + name, lambda n=name: grep_only(n, invert=True)),
               ("grep_ctx_" + name, lambda n=name: grep_only(n, before=2, after=2))]
    fs += [("select_count", lambda: select_only(False)), ("select_write", lambda: select_only(True))]
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


say("100 MB json-like, LevelFastest, 1 MiB blocks, type 1 tables (M = 6), stream %d B, %d records; %d repetitions, the calls alternated; %s" %
    (size, N, REPS, "with grep_records" if HAVE else "a tree without grep_records: the composition alone"))
for name in sets:
    u, got, st, total = seen["B_" + name]
    say("  %-9s %d pattern(s): %d occurrences in %d records of %d bytes; search phase %d of %d chunks (%d usable tables)" % (name, len(sets[name]), total, u, got, st[1], st[0], st[2]))
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-18s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
verdicts = {}
if HAVE:
    for name in sets:
        a, b = "A_" + name, "B_" + name
        close = abs(med[a] - med[b]) < max(iqr(ts[a]), iqr(ts[b]))
        verdicts[name] = "equal" if close else "held" if med[a] < med[b] else "MISSED"
        say("  %-9s A / B = %.3f (%+.3f ms): %s" % (name, med[a] / med[b], med[a] - med[b], verdicts[name]))
    for k in ("select_count", "select_write"):
        say("  %-18s %.3f ms per million records" % (k, med[k] / N * 1e6))
say("  " + json.dumps({"stream": size, "records": N, "verdicts": verdicts, **{k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
