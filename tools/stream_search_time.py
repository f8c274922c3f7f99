"""The pattern search over a stream in HBM against decoding everything, and the Writer with and without search tables, on an MI355X (one
process, every shape warmed up, REPS timed repetitions with the variants alternated, medians, a device synchronise inside every timed
window).  Input: 100 MB json-like, LevelFastest, 1 MiB blocks, M = 6.

  t_search       mlz_dev_reader_search for a 16-byte needle planted in three places (its decoded set must be at most a tenth of the chunks)
  t_search_all   the same with MLZ_SEARCH_NO_TABLES: every chunk decoded and scanned
  t_all          mlz_stream_decode_device of the same stream, by the library given as PARENT_LIB (a build of the parent commit, loaded
                 beside this one) or, without it, by this library
  t_write        mlz_stream_encode_gather_device without / with MLZ_STREAM_SEARCH_TABLES, and the two stream sizes

usage: python tools/stream_search_time.py [out.txt]        (environment: PARENT_LIB=path of the parent commit's libminlz_hip.so)"""
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
from minlz_amd import _lib, synth

REPS = 25
BS, M = 1 << 20, 6
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


parent = None
if os.environ.get("PARENT_LIB"):
    P = C.CDLL(os.environ["PARENT_LIB"])
    vp, sz, i64 = C.c_void_p, C.c_size_t, C.c_int64
    P.mlz_init.argtypes = [C.c_int, C.POINTER(vp)]; P.mlz_init.restype = C.c_int
    P.mlz_stream_decode_device.argtypes = [vp, vp, C.c_uint32, vp, sz, vp, sz]; P.mlz_stream_decode_device.restype = i64
    ph = vp()
    assert P.mlz_init(0, C.byref(ph)) == 0
    parent = (P, ph)

d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
needle = np.random.default_rng(1).integers(0, 256, 16, dtype=np.uint8).tobytes()
for o in (3 * BS + BS // 3, 50 * BS + 17, 90 * BS - 8):
    d[o:o + 16] = needle
d = bytes(d)
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound(len(d), BS, 4)
dst = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
size = [0, 0]
out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
pos = torch.zeros(64, dtype=torch.int64, device="cuda")


def write(tables):
    size[tables] = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], dst[tables].data_ptr(), cap, search_match_len=M if tables else None)


write(0)
write(1)
torch.cuda.synchronize()
rd = ctx.stream_open_device(dst[1].data_ptr(), size[1])
stats = {}


def search():
    total, st = rd.search(needle, pos.data_ptr(), 64)
    assert total == 3
    stats["tables"] = st


def search_all():
    total, st = rd.search(needle, pos.data_ptr(), 64, no_tables=True)
    assert total == 3
    stats["all"] = st


def decode_all():
    if parent:
        assert parent[0].mlz_stream_decode_device(parent[1], None, 0, dst[1].data_ptr(), size[1], out.data_ptr(), len(d)) == len(d)
    else:
        assert ctx.stream_decode_device(dst[1].data_ptr(), size[1], out.data_ptr(), len(d)) == len(d)


fs = [("t_search", search), ("t_search_all", search_all), ("t_all", decode_all), ("t_write_plain", lambda: write(0)), ("t_write_tables", lambda: write(1))]
for _ in range(3):
    for _, f in fs:
        f()
        torch.cuda.synchronize()
assert out[:len(d)].cpu().numpy().tobytes() == d
assert stats["tables"][1] * 10 <= stats["tables"][0], stats
ts = {k: [] for k, _ in fs}
for _ in range(REPS):
    for k, f in fs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts[k].append((time.perf_counter() - t0) * 1e3)
med = {k: statistics.median(v) for k, v in ts.items()}
say("100 MB json-like, LevelFastest, 1 MiB blocks, M = %d: stream %d B plain, %d B with tables (+%.2f %%); %d repetitions; t_all by %s" %
    (M, size[0], size[1], 100.0 * (size[1] - size[0]) / size[0], REPS, "the parent commit's library" if parent else "this library"))
say("search with tables: %d data chunks, %d decoded, %d usable tables; without: %d decoded" % (stats["tables"] + (stats["all"][1],)))
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-14s median %8.3f ms   min %8.3f   p90 %8.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))]))
say("  t_search %s t_all" % ("<" if med["t_search"] < med["t_all"] else ">="))
say("  " + json.dumps({"stream_plain": size[0], "stream_tables": size[1], "decoded_chunks": stats["tables"][1], "chunks": stats["tables"][0], **{k: round(v, 4) for k, v in med.items()}}))
rd.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
