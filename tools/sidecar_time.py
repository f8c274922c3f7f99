"""Sidecar search indexes on an MI355X: what a sidecar costs to build and what a search through it costs, against the calls that do the
same work piecewise (one process, every shape warmed up, REPS timed repetitions with the variants alternated, medians with interquartile
range, a device synchronise inside every timed window).  Input: 100 MB json-like, LevelFastest, 1 MiB blocks, table type 1 at M = 6, a
16-byte needle planted in three places.  Every block of this input compresses, so the inline stream and the sidecar hold the same tables.

  t_build        mlz_dev_reader_build_sidecar of the plain stream (one configuration) into room of mlz_dev_reader_sidecar_bound
  t_decode       mlz_stream_decode_device of the same stream
  t_write_on/off the device Writer with and without the same tables; their difference is what the tables cost the Writer
  bar            (t_decode + t_write_on - t_write_off) * 1.25: decode and tables are the work a sidecar build cannot avoid, the quarter
                 covers the placement kernel and the second look at the sizes.  The tool says by how much t_build misses or meets the bar.
  t_search_side  mlz_dev_reader_search on the plain stream with the sidecar attached
  t_search_inl   the same search on the Writer's stream with inline tables; the two run the same plan, decode and scan, so they are expected
                 to agree within the interquartile range.

usage: python tools/sidecar_time.py [out.txt]"""
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

REPS = 15
BS, M = 1 << 20, 6
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
needle = b'"id":"' + np.random.default_rng(1).integers(0, 256, 10, dtype=np.uint8).tobytes()
for o in (3 * BS + BS // 3, 50 * BS + 17, 90 * BS - 8):
    d[o:o + 16] = needle
d = bytes(d)
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4 | M << 8)
dst = {v: torch.empty(cap, dtype=torch.uint8, device="cuda") for v in ("off", "on")}
size = {}
out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
pos = torch.zeros(64, dtype=torch.int64, device="cuda")


def write(v):
    size[v] = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], dst[v].data_ptr(), cap, search_match_len=M if v == "on" else None)


write("off")
write("on")
torch.cuda.synchronize()
plain = ctx.stream_open_device(dst["off"].data_ptr(), size["off"])
inline = ctx.stream_open_device(dst["on"].data_ptr(), size["on"])
cfgs = [mz.api.search_config(1, M)]
side_cap = plain.sidecar_bound(cfgs)
side = torch.empty(side_cap, dtype=torch.uint8, device="cuda")
side_n = plain.build_sidecar(cfgs, side.data_ptr(), side_cap)
plain.attach_sidecar(side.data_ptr(), side_n)
stats = {}


def build():
    assert plain.build_sidecar(cfgs, side.data_ptr(), side_cap) == side_n


def decode():
    assert ctx.stream_decode_device(dst["off"].data_ptr(), size["off"], out.data_ptr(), len(d)) == len(d)


def search(which):
    total, st = (plain if which == "side" else inline).search(needle, pos.data_ptr(), 64)
    assert total == 3
    stats[which] = st


fs = [("t_build", build), ("t_decode", decode), ("t_write_off", lambda: write("off")), ("t_write_on", lambda: write("on")),
      ("t_search_side", lambda: search("side")), ("t_search_inl", lambda: search("inl"))]
for _ in range(3):
    for _, f in fs:
        f()
        torch.cuda.synchronize()
assert stats["side"] == stats["inl"], stats   # the same plan: every block compressed, so both streams hold a table per block
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


say("100 MB json-like, LevelFastest, 1 MiB blocks, table type 1, M = %d; %d repetitions, the variants alternated" % (M, REPS))
say("  stream %d B, with inline tables %d B, sidecar %d B (room %d B)" % (size["off"], size["on"], side_n, side_cap))
say("  search: %d data chunks, %d decoded, %d usable tables (sidecar and inline alike)" % stats["side"])
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-14s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
bar = (med["t_decode"] + med["t_write_on"] - med["t_write_off"]) * 1.25
say("  build: %.3f ms against the bar (t_decode + t_write_on - t_write_off) * 1.25 = %.3f ms: %s" %
    (med["t_build"], bar, "met" if med["t_build"] <= bar else "MISSED by %.3f ms (%.0f %%)" % (med["t_build"] - bar, 100 * (med["t_build"] / bar - 1))))
gap, spread = med["t_search_side"] - med["t_search_inl"], max(iqr(ts["t_search_side"]), iqr(ts["t_search_inl"]))
say("  search: through the sidecar %.3f ms, through inline tables %.3f ms: %s" %
    (med["t_search_side"], med["t_search_inl"], "equal within the interquartile range" if abs(gap) <= spread else "apart by %.3f ms (IQR %.3f)" % (gap, spread)))
say("  " + json.dumps({"sizes": size, "sidecar": side_n, "bar_ms": round(bar, 4), **{k: round(v, 4) for k, v in med.items()}}))
plain.close()
inline.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
