"""The record index (mlz_dev_reader_index_records, mlz_dev_reader_read_records, mlz_dev_reader_record_numbers) against what it is built
from, on an MI355X: one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and interquartile ranges, a
device synchronise inside every timed window.
Input: 100 MB json-like, LevelFastest, 1 MiB blocks, newline delimiter; 100 000 random record numbers (repeats allowed, unordered).

  t_build          mlz_dev_reader_index_records; the index is dropped between repetitions by alternating two delimiters (newline and comma)
  t_build_comma    ... the other one (more delimiters: a larger table)
  t_decode         mlz_stream_decode_device of the whole stream
  t_read_records   mlz_dev_reader_read_records of the record numbers
  t_read_device    mlz_dev_reader_read_device over the same records' spans, computed beforehand
  t_spans          mlz_dev_reader_record_spans alone
  t_gather         decode everything, then gather the same records from the decoded bytes with torch (index arithmetic on the device)
  t_numbers        mlz_dev_reader_record_numbers of 100 000 random positions

The bars: t_build <= 1.25 x t_decode; t_read_records within 10 % or one interquartile range of t_read_device, whichever is larger.

usage: python tools/record_index_time.py [out.txt]"""
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
BS, NREC = 1 << 20, 100_000
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


d = synth.json_like(100_000_000, seed=1).tobytes()
a = np.frombuffer(d, np.uint8)
D = np.flatnonzero(a == 10).astype(np.int64)
N = len(D) + (1 if D[-1] != len(d) - 1 else 0)
start = np.concatenate([[0], D + 1])[:N]
length = np.concatenate([D, [len(d)]])[:N] - start

src = torch.from_numpy(a.copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 0)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], stream.data_ptr(), cap)
rd = ctx.stream_open_device(stream.data_ptr(), size)
out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")

rng = np.random.default_rng(1)
idx_h = rng.integers(0, N, NREC)
idx = torch.from_numpy(idx_h).cuda()
off = torch.from_numpy(start[idx_h].copy()).cuda()
ln = torch.from_numpy(length[idx_h].copy()).cuda()
total = int(length[idx_h].sum())
dst = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
dst2 = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
starts = torch.empty(NREC + 1, dtype=torch.int64, device="cuda")
sp_off, sp_len = torch.empty(NREC, dtype=torch.int64, device="cuda"), torch.empty(NREC, dtype=torch.int64, device="cuda")
pos_h = rng.integers(0, len(d), NREC)
pos = torch.from_numpy(pos_h).cuda()
no = torch.empty(NREC, dtype=torch.int64, device="cuda")
info = {}


def build(delim):
    info[delim] = rd.index_records(delim)[1]
    assert info[delim][3] > 0


def decode_all():
    assert ctx.stream_decode_device(stream.data_ptr(), size, out.data_ptr(), len(d)) == len(d)


def read_records():
    assert rd.read_records(idx.data_ptr(), NREC, dst.data_ptr(), total, d_starts=starts.data_ptr()) == total


def read_device():
    assert rd.read_device(off.data_ptr(), ln.data_ptr(), NREC, dst2.data_ptr(), total, d_starts=starts.data_ptr()) == total


def spans():
    assert rd.record_spans(idx.data_ptr(), NREC, sp_off.data_ptr(), sp_len.data_ptr()) == total


def gather():
    decode_all()
    st = torch.cumsum(ln, 0) - ln
    which = torch.repeat_interleave(torch.arange(NREC, device="cuda"), ln, output_size=total)
    return out[off[which] + (torch.arange(total, device="cuda") - st[which])]


def numbers():
    assert rd.record_numbers(pos.data_ptr(), NREC, no.data_ptr()) == NREC


# the checks first, against the host's split
build(b"\n")
assert info[b"\n"][:2] == (N, len(D))
read_records()
read_device()
torch.cuda.synchronize()
want = b"".join(d[s:s + n] for s, n in zip(start[idx_h].tolist(), length[idx_h].tolist()))
assert dst[:total].cpu().numpy().tobytes() == want and dst2[:total].cpu().numpy().tobytes() == want and gather().cpu().numpy().tobytes() == want
numbers()
assert (no.cpu().numpy() == np.searchsorted(D, pos_h, side="left")).all()

# the reads and the numbers need the newline index, so the two builds run back to back and the newline one is the later
fs = [("t_build_comma", lambda: build(b",")), ("t_build", lambda: build(b"\n")), ("t_decode", decode_all), ("t_read_records", read_records), ("t_read_device", read_device),
      ("t_spans", spans), ("t_gather", gather), ("t_numbers", numbers)]
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


say("100 MB json-like, LevelFastest, 1 MiB blocks, stream %d B; %d repetitions, the calls alternated" % (size, REPS))
for dl in (b"\n", b","):
    say("  delimiter %r: %d records, %d delimiters, %d bytes of index, %d chunks decoded per build" % ((dl,) + info[dl]))
say("  %d record numbers: %d bytes, %d chunks touched" % (NREC, total, ctx.range_plan()[0]))
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-16s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
build_held = med["t_build"] <= 1.25 * med["t_decode"]
margin = max(0.10 * med["t_read_device"], iqr(ts["t_read_device"]))
read_held = med["t_read_records"] - med["t_read_device"] <= margin
say("  build: t_build / t_decode = %.3f (comma: %.3f); the bar (<= 1.25): %s" % (med["t_build"] / med["t_decode"], med["t_build_comma"] / med["t_decode"], "held" if build_held else "MISSED"))
say("  read: t_read_records - t_read_device = %+.3f ms, margin %.3f ms; the bar: %s;  t_gather / t_read_records = %.2f" %
    (med["t_read_records"] - med["t_read_device"], margin, "held" if read_held else "MISSED", med["t_gather"] / med["t_read_records"]))
say("  " + json.dumps({"stream": size, "records": N, "build_bar_held": build_held, "read_bar_held": read_held, **{k: round(v, 4) for k, v in med.items()},
                       **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
