"""The stored record index on an MI355X (include/minlz_hip_record_index_store.h) against the only source of a record index the parent commit has:
mlz_dev_reader_index_records, which decodes the whole stream (one process, every shape warmed up, REPS timed repetitions with the variants
alternated, medians with interquartile range, a device synchronise inside every timed window).  Input: 100 MB json-like, LevelFastest, 1 MiB
blocks, written by the device Writer; the delimiter is the newline.

  load             mlz_dev_reader_load_record_index of the saved blob on a handle WITHOUT an index (opened outside the timed window)
  parent index     PARENT_LIB's (the parent commit's libminlz_hip.so, loaded into this process beside this tree's; this tree's own where the
                   variable is not set) mlz_dev_reader_index_records on a fresh handle of the same stream (opened outside the window)
  bar              median(load) below median(parent index), beyond both interquartile ranges
recorded without a bar:
  save             mlz_dev_reader_save_record_index of a handle's index
  build_device     mlz_record_index_build_device over the raw bytes, against the parent's open + index_records of the stream (both in the window)
  sizes            the blob's bytes against 8 k (the table in memory), against 2 k and against the stream

usage: [PARENT_LIB=libminlz_hip.so] [FRACTION=n] python tools/record_index_store_time.py [out.txt]"""
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
BS = 1 << 20
FRACTION = int(os.environ.get("FRACTION", "1"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


class Lib:
    """A library loaded by path, with a context of its own: open, index_records and close, through plain ctypes."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.h = C.c_void_p()
        assert self.L.mlz_init(0, C.byref(self.h)) == 0
        self.L.mlz_stream_open_device.restype = C.c_int64
        self.L.mlz_stream_open_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.mlz_dev_reader_index_records.restype = C.c_int64
        self.L.mlz_dev_reader_index_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint8, C.POINTER(C.c_uint64)]
        self.L.mlz_dev_reader_close.restype = None
        self.L.mlz_dev_reader_close.argtypes = [C.c_void_p]

    def open(self, t, n):
        rd = C.c_void_p()
        assert self.L.mlz_stream_open_device(self.h, None, t.data_ptr(), n, C.byref(rd)) >= 0
        return rd

    def index(self, rd):
        info = (C.c_uint64 * 4)()
        r = self.L.mlz_dev_reader_index_records(rd, None, 0, 10, info)
        assert r > 0 and info[3] > 0, (r, list(info))
        return r

    def close(self, rd):
        self.L.mlz_dev_reader_close(rd)


n_bytes = 100_000_000 // FRACTION
d = synth.json_like(n_bytes, seed=1)
src = torch.from_numpy(np.ascontiguousarray(d).copy()).cuda()
ctx = mz.Context(0)
parent = Lib(os.environ.get("PARENT_LIB") or _lib.SO)
whose = "the parent library's" if os.environ.get("PARENT_LIB") else "this tree's own (no PARENT_LIB)"
say("%d MB json-like, LevelFastest, 1 MiB blocks, delimiter 0x0a; %d repetitions, the variants alternated; the yardstick is %s index_records" %
    (n_bytes // 1_000_000, REPS, whose))
cap = api.stream_bound(n_bytes, BS)
stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
n = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [n_bytes], stream.data_ptr(), cap)
keeper = ctx.stream_open_device(stream.data_ptr(), n)
N, info = keeper.index_records(b"\n")
k = info[1]
bound = keeper.record_index_bound()
room = torch.empty(bound, dtype=torch.uint8, device="cuda")
blob_len, sinfo = keeper.save_record_index(room.data_ptr(), bound)
blob = room[:blob_len].clone()
raw_bound = api.record_index_bound(n_bytes)
raw_room = torch.empty(raw_bound, dtype=torch.uint8, device="cuda")
got = {}
fresh, pfresh = {}, {}


def prepare_load():
    fresh["rd"] = ctx.stream_open_device(stream.data_ptr(), n)


def load():
    got["load"] = fresh["rd"].load_record_index(blob.data_ptr(), blob_len)


def finish_load():
    assert got["load"][0] == N and got["load"][1][3] == 0 and ctx.counter(7) == 0
    fresh["rd"].close()


def prepare_parent():
    pfresh["rd"] = parent.open(stream, n)


def parent_index():
    got["parent"] = parent.index(pfresh["rd"])


def finish_parent():
    assert got["parent"] == N
    parent.close(pfresh["rd"])


def save():
    got["save"] = keeper.save_record_index(room.data_ptr(), bound)[0]


def build():
    got["build"] = ctx.record_index_build_device(src.data_ptr(), n_bytes, b"\n", raw_room.data_ptr(), raw_bound)[0]


def parent_open_index():
    rd = parent.open(stream, n)
    got["parent2"] = parent.index(rd)
    pfresh["rd2"] = rd


def finish_parent2():
    parent.close(pfresh["rd2"])


nothing = lambda: None   # noqa: E731
fs = [("load", prepare_load, load, finish_load), ("parent index", prepare_parent, parent_index, finish_parent), ("save", nothing, save, nothing),
      ("build_device", nothing, build, nothing), ("parent open + index", nothing, parent_open_index, finish_parent2)]
for _ in range(3):
    for _, pre, f, post in fs:
        pre()
        f()
        torch.cuda.synchronize()
        post()
ts = {name: [] for name, _, _, _ in fs}
for _ in range(REPS):
    for name, pre, f, post in fs:
        pre()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts[name].append((time.perf_counter() - t0) * 1e3)
        post()
assert got["save"] == blob_len and got["build"] == blob_len and torch.equal(room[:blob_len], blob)
med = {name: statistics.median(v) for name, v in ts.items()}
say("stream %d B of %d decoded; N = %d records, k = %d delimiters; blob %d B in %d sections, %d sparse and %d dense tiles" % (n, n_bytes, N, k, blob_len, sinfo[1], sinfo[2], sinfo[3]))
for name, _, _, _ in fs:
    v = sorted(ts[name])
    say("  %-20s median %8.3f ms   min %8.3f   p90 %8.3f   IQR %7.3f" % (name, med[name], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[name])))
gap, spread = med["parent index"] - med["load"], max(iqr(ts["load"]), iqr(ts["parent index"]))
say("  bar, load: %.3f ms against the parent's index_records %.3f ms: %s" % (med["load"], med["parent index"], "met, %.1f x faster" % (med["parent index"] / med["load"]) if gap > spread else
    "MISSED (the medians are %.3f ms apart, the larger interquartile range is %.3f ms)" % (gap, spread)))
say("  build_device %.3f ms against the parent's open + index_records %.3f ms (%.2f x); save %.3f ms" %
    (med["build_device"], med["parent open + index"], med["parent open + index"] / med["build_device"], med["save"]))
say("  sizes: blob %d B = %.3f x the table in memory (8 k = %d B), %.3f x 2 k (%d B), %.4f x the stream (%d B); %.2f bytes per record" %
    (blob_len, blob_len / (8 * k), 8 * k, blob_len / (2 * k), 2 * k, blob_len / n, n, blob_len / N))
say("  " + json.dumps({**{name: round(v, 4) for name, v in med.items()}, **{name + " iqr": round(iqr(v), 4) for name, v in ts.items()}, "blob": blob_len, "k": k, "N": N,
                       "stream": n, "bar": bool(gap > spread)}))
keeper.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
