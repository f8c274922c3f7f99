"""The device Writer with compressed block search tables (MLZ_STREAM_SEARCH_COMPRESS, chunk 0x46) against the same Writer with
uncompressed ones (0x45), on an MI355X: one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and
interquartile ranges; every call is synchronous and a device synchronise stands inside every timed window.
Input: 100 MB json-like (FRACTION of it with FRACTION=4: a quarter), LevelFastest, 1 MiB blocks, type 1 tables with M = 6.

  writer      mlz_stream_encode_gather_device with 0x45 tables, with the flag, and (PARENT_LIB = the parent commit's libminlz_hip.so, loaded
              into the same process beside this tree's) the parent's Writer with 0x45 tables.  Bar 1: the Writer with the flag within
              1.25 x the parent's Writer (this tree's own 0x45 Writer where there is no PARENT_LIB).  "tables stage" is the difference of
              the medians with and without tables.
  sidecar     mlz_dev_reader_build_sidecar of the plain stream (no inline tables; one configuration, type 1, M = 6) into room of
              mlz_dev_reader_sidecar_bound: without the flag, with it, and the parent's build; and with the flag into room of exactly the
              sidecar's size, which is below the bound, so that the sizing pass runs in front of the placing one.  Bar 1, second half: the
              build with the flag within 1.25 x the parent's build.
  sizes       the two streams and the two sidecars, and their table chunks alone
  search      per repetition a fresh handle on each stream: its first search (locate, expansion and CRC included) and its second

With ONE_CALL=1 the tool writes the stream with the flag four times and does nothing else (the profiler's run: a quarter of the totals of
cstw_plan_kernel, cstw_layout_kernel and cstw_encode_kernel is one call's stage).

usage: python tools/stream_tables_compress_time.py [out.txt]"""
import ctypes as C
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
from tests import search_model as SM

REPS = 25
BS, M = 1 << 20, 6
FRACTION = int(os.environ.get("FRACTION", "1"))
TABLES = api.STREAM_SEARCH_TABLES | M << 8
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    q = statistics.quantiles(v, n=4)
    return "%.3f ms (IQR %.3f)" % (statistics.median(v), q[2] - q[0])


class Lib:
    """A library loaded by path, with a context of its own: the Writer call alone, through plain ctypes."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.mlz_stream_encode_gather_device.restype = C.c_int64
        self.L.mlz_stream_encode_gather_device.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p, C.c_size_t]
        self.h = C.c_void_p()
        assert self.L.mlz_init(0, C.byref(self.h)) == 0

        self.L.mlz_stream_open_device.restype = C.c_int64
        self.L.mlz_stream_open_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.mlz_dev_reader_sidecar_bound.restype = C.c_int64
        self.L.mlz_dev_reader_sidecar_bound.argtypes = [C.c_void_p, C.POINTER(_lib.SearchConfig), C.c_int]
        self.L.mlz_dev_reader_build_sidecar.restype = C.c_int64
        self.L.mlz_dev_reader_build_sidecar.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_lib.SearchConfig), C.c_int, C.c_void_p, C.c_size_t]
        self.L.mlz_dev_reader_close.restype = None
        self.L.mlz_dev_reader_close.argtypes = [C.c_void_p]

    def open(self, t):
        rd = C.c_void_p()
        assert self.L.mlz_stream_open_device(self.h, None, t.data_ptr(), t.numel(), C.byref(rd)) >= 0
        return rd

    def sidecar(self, rd, flags, cfg, dst, cap):
        r = self.L.mlz_dev_reader_build_sidecar(rd, None, flags, C.byref(cfg), 1, dst.data_ptr(), cap)
        torch.cuda.synchronize()
        assert r > 0, r
        return r

    def write(self, flags, src, dst):
        srcs, lens = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(src.numel())
        r = self.L.mlz_stream_encode_gather_device(self.h, 1, BS, flags, srcs, lens, 1, dst.data_ptr(), dst.numel())
        torch.cuda.synchronize()
        assert r > 0, r
        return r


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


n_bytes = 100_000_000 // FRACTION
NEEDLE = b"#4711-a/Zqxjkv"
d = bytearray(synth.json_like(n_bytes, seed=1).tobytes())
nblk = n_bytes // BS
for o in (3 * BS + BS // 3, (nblk // 2) * BS + 17, (nblk - 5) * BS - 3):
    d[o:o + len(NEEDLE)] = NEEDLE
src = torch.from_numpy(np.frombuffer(bytes(d), np.uint8).copy()).cuda()
dst = torch.empty(api.stream_bound(n_bytes, BS, search_match_len=M) + 64, dtype=torch.uint8, device="cuda")
new = Lib(_lib.SO)

if os.environ.get("ONE_CALL"):
    for _ in range(4):
        new.write(TABLES | api.COMPRESS_TABLES, src, dst)
    sys.exit(0)

parent = Lib(os.environ["PARENT_LIB"]) if os.environ.get("PARENT_LIB") else None
calls = [("this tree, no tables", new, 0), ("this tree, 0x45 tables", new, TABLES), ("this tree, 0x46 tables (the flag)", new, TABLES | api.COMPRESS_TABLES)]
if parent:
    calls += [("parent, no tables", parent, 0), ("parent, 0x45 tables", parent, TABLES)]
for _, lib, flags in calls * 3:
    lib.write(flags, src, dst)
times = {name: [] for name, _, _ in calls}
for _ in range(REPS):
    for name, lib, flags in calls:
        times[name].append(timed(lambda: lib.write(flags, src, dst))[0])
say("writer, %d bytes json-like, %d blocks of 1 MiB, type 1, M = %d, %d alternated repetitions" % (n_bytes, (n_bytes + BS - 1) // BS, M, REPS))
for name, _, _ in calls:
    say("  %-36s %s" % (name, med(times[name])))
m = {name: statistics.median(v) for name, v in times.items()}
say("  tables stage, this tree: 0x45 %.3f ms, 0x46 %.3f ms" % (m["this tree, 0x45 tables"] - m["this tree, no tables"], m["this tree, 0x46 tables (the flag)"] - m["this tree, no tables"]))
yard = "parent, 0x45 tables" if parent else "this tree, 0x45 tables"
ratio = m["this tree, 0x46 tables (the flag)"] / m[yard]
say("  bar 1: the flag's Writer / %s = %.3f (allowed 1.25): %s" % (yard, ratio, "held" if ratio <= 1.25 else "MISSED"))
if parent:
    say("  this tree's 0x45 Writer / the parent's = %.3f" % (m["this tree, 0x45 tables"] / m["parent, 0x45 tables"]))

# the sidecar of the plain stream
n_plain = new.write(0, src, dst)
plain = dst[:n_plain].clone()
cfg = api.search_config(1, M)
handles = {"new": new.open(plain)}
if parent:
    handles["parent"] = parent.open(plain)
side_cap = new.L.mlz_dev_reader_sidecar_bound(handles["new"], C.byref(cfg), 1)
side = torch.empty(side_cap + 64, dtype=torch.uint8, device="cuda")
n45 = new.sidecar(handles["new"], 0, cfg, side, side_cap)
side45 = side[:n45].cpu().numpy().tobytes()
n46 = new.sidecar(handles["new"], api.COMPRESS_TABLES, cfg, side, side_cap)
side46 = side[:n46].cpu().numpy().tobytes()
scalls = [("this tree, 0x45 sidecar", new, "new", 0, side_cap), ("this tree, 0x46 sidecar (the flag)", new, "new", api.COMPRESS_TABLES, side_cap),
          ("this tree, 0x46 sidecar, room of exactly its size", new, "new", api.COMPRESS_TABLES, n46)]
if parent:
    scalls.append(("parent, 0x45 sidecar", parent, "parent", 0, side_cap))
for _, lib, h, flags, cap in scalls * 3:
    lib.sidecar(handles[h], flags, cfg, side, cap)
stimes = {name: [] for name, _, _, _, _ in scalls}
for _ in range(REPS):
    for name, lib, h, flags, cap in scalls:
        stimes[name].append(timed(lambda: lib.sidecar(handles[h], flags, cfg, side, cap))[0])
say("build_sidecar of the plain stream (%d B), one configuration (type 1, M = %d), %d alternated repetitions" % (n_plain, M, REPS))
for name, _, _, _, _ in scalls:
    say("  %-52s %s" % (name, med(stimes[name])))
sm = {name: statistics.median(v) for name, v in stimes.items()}
syard = "parent, 0x45 sidecar" if parent else "this tree, 0x45 sidecar"
sratio = sm["this tree, 0x46 sidecar (the flag)"] / sm[syard]
say("  bar 1, build_sidecar: the flag's build / %s = %.3f (allowed 1.25): %s" % (syard, sratio, "held" if sratio <= 1.25 else "MISSED"))
say("  with room of exactly its size (sizing pass + placing pass) / %s = %.3f" % (syard, sm["this tree, 0x46 sidecar, room of exactly its size"] / sm[syard]))
for lib, h in ((new, "new"), (parent, "parent")):
    if lib:
        lib.L.mlz_dev_reader_close(handles[h])

streams = {}
for name, flags in (("0x45", TABLES), ("0x46", TABLES | api.COMPRESS_TABLES)):
    n = new.write(flags, src, dst)
    streams[name] = dst[:n].cpu().numpy().tobytes()
say("sizes")
sized = {k + " stream": v for k, v in streams.items()}
sized.update({"0x45 sidecar": side45, "0x46 sidecar": side46})
for name, s in sized.items():
    cks = SM.chunks_of(s)
    say("  %s %d B; table chunks: %d x 0x45 (%d B), %d x 0x46 (%d B)" % (name, len(s), sum(t == 0x45 for _, t, _ in cks), sum(4 + n for _, t, n in cks if t == 0x45),
                                                                              sum(t == 0x46 for _, t, _ in cks), sum(4 + n for _, t, n in cks if t == 0x46)))

ctx = mz.Context(0)
out = torch.empty(4096, dtype=torch.int64, device="cuda")
say("search for a planted needle, a fresh handle per repetition")
res = {}
for name, s in streams.items():
    t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    first, second = [], []
    for rep in range(REPS + 3):
        rd = ctx.stream_open_device(t.data_ptr(), t.numel())
        a, r1 = timed(lambda: rd.search(NEEDLE, out.data_ptr(), 4096))
        b, r2 = timed(lambda: rd.search(NEEDLE, out.data_ptr(), 4096))
        rd.close()
        assert r1 == r2
        res[name] = r1
        if rep >= 3:
            first.append(a)
            second.append(b)
    say("  %s stream: first %s, second %s; (total, stats) = %s" % (name, med(first), med(second), res[name]))
assert res["0x45"] == res["0x46"]
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
