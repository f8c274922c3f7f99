"""mlz_dev_reader_extract_sidecar on an MI355X against the only route the parent commit has for moving a stream's search tables into a sidecar:
mlz_dev_reader_build_sidecar, which decodes every block and builds the tables again (one process, every shape warmed up, REPS timed repetitions
with the variants alternated, medians with interquartile range, a device synchronise inside every timed window).  Input: 100 MB json-like,
LevelFastest, 1 MiB blocks, table type 1 at M = 6, written by the device Writer with inline tables, once plain (0x45) and once under
search_compress (0x46 where smaller); a 14-byte needle planted in three places.

  extract a      the call without d_main: the tables copied into a sidecar whose references name the source
  extract b      the call with d_main: and the stream written again without them, with a fresh index
  parent build   PARENT_LIB's (the parent commit's libminlz_hip.so, loaded into this process beside this tree's; this tree's own where the
                 variable is not set) mlz_dev_reader_build_sidecar of the same stream, with MLZ_STREAM_SEARCH_COMPRESS for the 0x46 stream
  bar            median(extract a) and median(extract b) each below median(parent build), beyond both interquartile ranges
recorded without a bar:
  d2d copy       a plain device-to-device copy of the stream's bytes in the same loop, and extract b / d2d copy
  copy rate      (bytes read + bytes written by the copy kernel) / the whole time of extract b: a lower bound of the kernel's own rate, since
                 the call also holds the gap pass, the layout on the host and two round trips
  search         mlz_dev_reader_search on the stripped main through the extracted sidecar against the same search on the original through
                 its inline tables

usage: [PARENT_LIB=libminlz_hip.so] [FRACTION=n] python tools/sidecar_extract_time.py [out.txt]"""
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

REPS = 25
BS, M = 1 << 20, 6
FRACTION = int(os.environ.get("FRACTION", "1"))
NEEDLE = b"#4711-a/Zqxjkv"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


class Lib:
    """A library loaded by path, with a context of its own: open and build_sidecar, through plain ctypes."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.h = C.c_void_p()
        assert self.L.mlz_init(0, C.byref(self.h)) == 0
        self.L.mlz_stream_open_device.restype = C.c_int64
        self.L.mlz_stream_open_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.mlz_dev_reader_sidecar_bound.restype = C.c_int64
        self.L.mlz_dev_reader_sidecar_bound.argtypes = [C.c_void_p, C.POINTER(_lib.SearchConfig), C.c_int]
        self.L.mlz_dev_reader_build_sidecar.restype = C.c_int64
        self.L.mlz_dev_reader_build_sidecar.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_lib.SearchConfig), C.c_int, C.c_void_p, C.c_size_t]

    def open(self, t, n):
        rd = C.c_void_p()
        assert self.L.mlz_stream_open_device(self.h, None, t.data_ptr(), n, C.byref(rd)) >= 0
        return rd

    def bound(self, rd, cfg):
        return self.L.mlz_dev_reader_sidecar_bound(rd, C.byref(cfg), 1)

    def build(self, rd, flags, cfg, dst, cap):
        r = self.L.mlz_dev_reader_build_sidecar(rd, None, flags, C.byref(cfg), 1, dst.data_ptr(), cap)
        assert r > 0, r
        return r


n_bytes = 100_000_000 // FRACTION
d = bytearray(synth.json_like(n_bytes, seed=1).tobytes())
nblk = n_bytes // BS
for o in (3 * BS + BS // 3, (nblk // 2) * BS + 17, (nblk - 5) * BS - 3):
    d[o:o + len(NEEDLE)] = NEEDLE
src = torch.from_numpy(np.frombuffer(bytes(d), np.uint8).copy()).cuda()
ctx = mz.Context(0)
parent = Lib(os.environ.get("PARENT_LIB") or _lib.SO)
whose = "the parent library's" if os.environ.get("PARENT_LIB") else "this tree's own (no PARENT_LIB)"
cfg = api.search_config(1, M)
pos = torch.zeros(64, dtype=torch.int64, device="cuda")
say("%d MB json-like, LevelFastest, 1 MiB blocks, table type 1, M = %d; %d repetitions, the variants alternated; the yardstick is %s build_sidecar" %
    (n_bytes // 1_000_000, M, REPS, whose))
result = {}
for compress in (False, True):
    cap = api.stream_bound(n_bytes, BS, search_match_len=M)
    stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [n_bytes], stream.data_ptr(), cap, search_match_len=M, search_compress=compress)
    rd = ctx.stream_open_device(stream.data_ptr(), n)
    side_cap, main_cap = rd.extract_sidecar_bound()
    side = torch.empty(side_cap, dtype=torch.uint8, device="cuda")
    main = torch.empty(main_cap, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    prd = parent.open(stream, n)
    pcap = parent.bound(prd, cfg)
    pside = torch.empty(pcap, dtype=torch.uint8, device="cuda")
    got = {}

    def extract_a():
        got["a"] = rd.extract_sidecar(side.data_ptr(), side_cap)

    def extract_b():
        got["b"] = rd.extract_sidecar(side.data_ptr(), side_cap, main.data_ptr(), main_cap)

    def parent_build():
        got["p"] = parent.build(prd, api.COMPRESS_TABLES if compress else 0, cfg, pside, pcap)

    def d2d():
        copy_dst.copy_(stream[:n])

    extract_b()
    torch.cuda.synchronize()
    stripped = ctx.stream_open_device(main.data_ptr(), got["b"].main_len)
    side_keep = side[:got["b"].side_len].clone()
    stripped.attach_sidecar(side_keep.data_ptr(), side_keep.numel())
    stats = {}

    def search(which):
        total, st = (stripped if which == "side" else rd).search(NEEDLE, pos.data_ptr(), 64)
        assert total == 3, total
        stats[which] = st

    # (extract b runs behind the searches' warm-up only: the stripped handle reads `main`, which every extract b rewrites with the same bytes)
    fs = [("extract a", extract_a), ("extract b", extract_b), ("parent build", parent_build), ("d2d copy", d2d),
          ("search, sidecar", lambda: search("side")), ("search, inline", lambda: search("inl"))]
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
    b = got["b"]
    say("%s tables: stream %d B; sidecar %d B (a: %d B), stripped main %d B; %d blocks, %d tables of which %d compressed; the parent's sidecar %d B" %
        ("0x46 (search_compress)" if compress else "0x45", n, b.side_len, got["a"].side_len, b.main_len, b.blocks, b.tables, b.tables_compressed, got["p"]))
    for k, _ in fs:
        v = sorted(ts[k])
        say("  %-16s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
    for mode in ("extract a", "extract b"):
        margin = med["parent build"] - med[mode] - max(iqr(ts[mode]), iqr(ts["parent build"]))
        say("  bar, %s: %.3f ms against the parent's build %.3f ms: %s" % (mode, med[mode], med["parent build"], "met, %.1f x faster" % (med["parent build"] / med[mode]) if margin > 0 else
            "MISSED (the medians are %.3f ms apart, the larger interquartile range is %.3f ms)" % (med["parent build"] - med[mode], max(iqr(ts[mode]), iqr(ts["parent build"])))))
    moved = 2 * (b.side_len + b.main_len)
    say("  extract b / d2d copy = %.2f; the copy moves %d B read + written, %.1f GB/s over the whole call (a lower bound of the kernel's rate)" %
        (med["extract b"] / med["d2d copy"], moved, moved / med["extract b"] / 1e6))
    gap, spread = med["search, sidecar"] - med["search, inline"], max(iqr(ts["search, sidecar"]), iqr(ts["search, inline"]))
    say("  search: stripped main through the extracted sidecar %.3f ms, original through inline tables %.3f ms: %s; plans %s and %s" %
        (med["search, sidecar"], med["search, inline"], "equal within the interquartile range" if abs(gap) <= spread else "apart by %.3f ms (IQR %.3f)" % (gap, spread),
         stats["side"], stats["inl"]))
    result["0x46" if compress else "0x45"] = {**{k: round(v, 4) for k, v in med.items()}, **{k + " iqr": round(iqr(v), 4) for k, v in ts.items()},
                                              "stream": n, "side": b.side_len, "main": b.main_len}
    stripped.close()
    rd.close()
say("  " + json.dumps(result))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
