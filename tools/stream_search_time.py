"""The pattern search over a stream in HBM against decoding everything, and the Writer with and without search tables, on an MI355X (one
process, every shape warmed up, REPS timed repetitions with the variants alternated, medians, a device synchronise inside every timed
window).  Input: 100 MB json-like, LevelFastest, 1 MiB blocks, M = 6, a 16-byte needle that holds '"' and ':' planted in three places.
The table variants: type 1 (every position), the prefix tables (type 2) with the sets '":' and '":, ', and the long-prefix tables (type 4)
with the prefix '"user":"', M = 6, E = 3, searched with a 22-byte record pattern behind that prefix, planted in the same three blocks.

  t_search_<v>   mlz_dev_reader_search over the stream of variant v (its decoded set must be at most a tenth of the chunks)
  t_search_all   the same with MLZ_SEARCH_NO_TABLES: every chunk decoded and scanned
  t_all          mlz_stream_decode_device of the type 1 stream by this library; t_all_parent: by the library given as PARENT_LIB (a build of
                 the parent commit, loaded beside this one)
  t_write_<v>    mlz_stream_encode_gather_device without tables (plain) / with the tables of variant v, and the stream sizes;
                 t_write_type1_parent: the type 1 Writer of PARENT_LIB in the same loop.  The prefix Writer passes when its median is within
                 the interquartile range of the parent's type 1 figure above that figure's median, or below it.  t_write_prefix4_parent: the
                 type 2 Writer ('":, ') of PARENT_LIB in the same loop; the long-prefix Writer passes against that figure in the same way.

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
VARIANTS = [("type1", None), ("prefix2", b'":'), ("prefix4", b'":, '), ("long_user", b'"user":"')]
LONG, LONG_E = "long_user", 3
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
    P.mlz_stream_encode_gather_device.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(sz), C.c_int, vp, sz]
    P.mlz_stream_encode_gather_device.restype = i64
    P.mlz_stream_encode_gather_device_tables.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_lib.SearchTables), C.POINTER(vp), C.POINTER(sz), C.c_int, vp, sz]
    P.mlz_stream_encode_gather_device_tables.restype = i64
    ph = vp()
    assert P.mlz_init(0, C.byref(ph)) == 0
    parent = (P, ph)

d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
needle = b'"id":"' + np.random.default_rng(1).integers(0, 256, 10, dtype=np.uint8).tobytes()
needle_user = b'"user":"' + np.random.default_rng(2).integers(97, 123, 14, dtype=np.uint8).tobytes()
for o in (3 * BS + BS // 3, 50 * BS + 17, 90 * BS - 8):
    d[o:o + 16] = needle
    d[o + 1000:o + 1000 + len(needle_user)] = needle_user
d = bytes(d)
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = L.mlz_stream_bound_tables(len(d), BS, 0, C.byref(mz.api.search_tables_config(M, bytes(range(256)))))
names = ["plain"] + [v for v, _ in VARIANTS] + (["type1_parent", "prefix4_parent"] if parent else [])
dst = {v: torch.empty(cap, dtype=torch.uint8, device="cuda") for v in names}
size = {}
out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
pos = torch.zeros(64, dtype=torch.int64, device="cuda")


def write(v):
    if v == "type1_parent":
        sp, sl = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(len(d))
        size[v] = parent[0].mlz_stream_encode_gather_device(parent[1], mz.LevelFastest, BS, 4 | M << 8, sp, sl, 1, dst[v].data_ptr(), cap)
        assert size[v] > 0
        return
    if v == "prefix4_parent":
        sp, sl = (C.c_void_p * 1)(src.data_ptr()), (C.c_size_t * 1)(len(d))
        cfg = mz.api.search_tables_config(M, dict(VARIANTS)["prefix4"])
        size[v] = parent[0].mlz_stream_encode_gather_device_tables(parent[1], mz.LevelFastest, BS, 0, C.byref(cfg), sp, sl, 1, dst[v].data_ptr(), cap)
        assert size[v] > 0
        return
    if v == LONG:
        size[v] = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], dst[v].data_ptr(), cap,
                                                  search_match_len=M, search_long_prefix=dict(VARIANTS)[v], search_extras=LONG_E)
        return
    pset = dict(VARIANTS).get(v)
    size[v] = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], dst[v].data_ptr(), cap,
                                              search_match_len=None if v == "plain" else M, search_prefix=pset)


def table_bytes(v):
    """The bytes of the stream's table chunks (0x45), headers included."""
    s = dst[v][:size[v]].cpu().numpy()
    p, total = 0, 0
    while p + 4 <= len(s):
        n = int(s[p + 1]) | int(s[p + 2]) << 8 | int(s[p + 3]) << 16
        if s[p] == 0x45:
            total += 4 + n
        p += 4 + n
    return total


for v in names:
    write(v)
torch.cuda.synchronize()
if parent:
    assert size["type1_parent"] == size["type1"] and torch.equal(dst["type1_parent"][:size["type1"]], dst["type1"][:size["type1"]]), "the type 1 stream changed"
    assert size["prefix4_parent"] == size["prefix4"] and torch.equal(dst["prefix4_parent"][:size["prefix4"]], dst["prefix4"][:size["prefix4"]]), "the type 2 stream changed"
rd = {v: ctx.stream_open_device(dst[v].data_ptr(), size[v]) for v, _ in VARIANTS}
stats = {}


def search(v, **kw):
    total, st = rd[v].search(needle_user if v == LONG else needle, pos.data_ptr(), 64, **kw)
    assert total == 3
    stats[v if not kw else "all"] = st


def decode_all(lib):
    if lib == "parent":
        assert parent[0].mlz_stream_decode_device(parent[1], None, 0, dst["type1"].data_ptr(), size["type1"], out.data_ptr(), len(d)) == len(d)
    else:
        assert ctx.stream_decode_device(dst["type1"].data_ptr(), size["type1"], out.data_ptr(), len(d)) == len(d)


fs = [("t_search_" + v, (lambda v=v: search(v))) for v, _ in VARIANTS]
fs += [("t_search_all", lambda: search("type1", no_tables=True)), ("t_all", lambda: decode_all("this"))]
if parent:
    fs.append(("t_all_parent", lambda: decode_all("parent")))
fs += [("t_write_" + v, (lambda v=v: write(v))) for v in names]
for _ in range(3):
    for _, f in fs:
        f()
        torch.cuda.synchronize()
assert out[:len(d)].cpu().numpy().tobytes() == d
for v, _ in VARIANTS:
    assert stats[v][1] * 10 <= stats[v][0], (v, stats)
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


say("100 MB json-like, LevelFastest, 1 MiB blocks, M = %d, needle %r (%s: %r, E = %d); %d repetitions, the variants alternated" % (M, needle, LONG, needle_user, LONG_E, REPS))
tb = {v: table_bytes(v) for v, _ in VARIANTS}
for v in names:
    extra = ""
    if v in tb:
        extra = "  (+%.2f %% over plain; table chunks %d B = %.2f %% of the stream)" % (100.0 * (size[v] - size["plain"]) / size["plain"], tb[v], 100.0 * tb[v] / size[v])
    say("  stream %-13s %10d B%s" % (v, size[v], extra))
for v, _ in VARIANTS:
    say("  search %-8s: %d data chunks, %d decoded, %d usable tables" % ((v,) + stats[v]))
say("  search without tables: %d decoded" % stats["all"][1])
for k, _ in fs:
    v = sorted(ts[k])
    say("  %-22s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
for v, _ in VARIANTS:
    say("  t_search_%s %s t_all (this library)" % (v, "<" if med["t_search_" + v] < med["t_all"] else ">="))
say("  t_search_%s %.3f ms %s t_search_all %.3f ms" % (LONG, med["t_search_" + LONG], "<" if med["t_search_" + LONG] < med["t_search_all"] else ">=", med["t_search_all"]))
if parent:
    ref, spread = med["t_write_type1_parent"], iqr(ts["t_write_type1_parent"])
    for v in ("prefix2", "prefix4"):
        w = med["t_write_" + v]
        say("  t_write_%s %.3f ms against the parent's type 1 Writer %.3f ms (IQR %.3f): %s" %
            (v, w, ref, spread, "not slower" if w <= ref + spread else "SLOWER by %.3f ms" % (w - ref)))
    ref, spread, w = med["t_write_prefix4_parent"], iqr(ts["t_write_prefix4_parent"]), med["t_write_" + LONG]
    say("  t_write_%s %.3f ms against the parent's type 2 Writer ('\":, ') %.3f ms (IQR %.3f): %s" %
        (LONG, w, ref, spread, "not slower" if w <= ref + spread else "SLOWER by %.3f ms" % (w - ref)))
say("  " + json.dumps({"sizes": size, "table_bytes": tb, "decoded_chunks": {v: stats[v][1] for v, _ in VARIANTS}, "chunks": stats["type1"][0],
                       **{k: round(v, 4) for k, v in med.items()}}))
for r in rd.values():
    r.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
