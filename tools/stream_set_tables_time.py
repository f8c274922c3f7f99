"""grep over a set of streams that keeps its streams' search tables (mlz_stream_open_batch_device_tables) against the parent commit's grep over
the plain set of the same batch, on an MI355X: one process, the record index built beforehand, a warm-up search so that the tables are found,
REPS timed repetitions with the calls alternated, medians and interquartile ranges, a device synchronise inside every timed window.
JSON-like data, every object ending with a newline; every stream written by the device Writer (LevelFastest) with table type 1, M = 6.

  shapes   1024 streams of one 64 KiB block; 256 streams of 1 MiB in 64 KiB blocks; 16 streams of 8 MiB in 1 MiB blocks.  1 needle planted in
           3 streams, and 16 needles planted in 3 streams each (16 random bytes above 0x7f).
  A        grep_streams on the tabled set: mlz_dev_reader_grep_records + mlz_dev_reader_locate_records
  B        the same two calls on the plain set (mlz_stream_open_batch_device).  With --parent-lib they run in the library given there (a build of
           the parent commit, loaded beside this one), so that the yardstick is not the code under test; without it, in this library, and the
           output says so.
Both legs must select the same records, and A's decoded count is checked against the model on the host (tests/set_tables_model.py) at the
first shape (the model in Python is too slow for the others; there the count is reported).

The bar: A's median below B's by more than both interquartile ranges at every shape.  Reported without a bar: the first search on a handle
(discovery included), the same batch with 0x46 tables (first and steady), search_many on the tabled set against search_streams(prune=True),
a tabled open of a batch without any tables against the plain set, and the chunks decoded of the chunks present.

usage: python tools/stream_set_tables_time.py [--parent-lib libminlz_hip.so] [out.txt]"""
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
from minlz_amd._lib import BlockDesc
from tests import set_tables_model as M

args = sys.argv[1:]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else None

REPS, CAP = 25, 1000
LEVEL = mz.LevelFastest
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (16, 8 << 20, 1 << 20)]   # (streams, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
lines = []
NAMES = {"mlz_stream_open_batch_device": _lib.ABI_EXT["minlz_hip_stream_set.h"], "mlz_dev_reader_locate_records": _lib.ABI_EXT["minlz_hip_stream_set.h"],
         "mlz_dev_reader_index_records": _lib.ABI, "mlz_dev_reader_grep_records": _lib.ABI, "mlz_dev_reader_close": _lib.ABI, "mlz_init": _lib.ABI}


def say(s):
    print(s, flush=True)
    lines.append(s)


# leg B's library: the parent commit's, loaded beside this one, with a context of its own
B, bh = L, ctx.handle
if PARENT:
    B = C.CDLL(PARENT)
    for name, table in NAMES.items():
        getattr(B, name).restype, getattr(B, name).argtypes = table[name]
    bh = C.c_void_p()
    assert B.mlz_init(0, C.byref(bh)) == 0


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def timed(fs):
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
    return ts


def once(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def write_batch(datas, size, bs, **kw):
    """Every stream by the device Writer into a slot of one buffer -> (the buffer, the descriptors, the streams' sizes, the slot)."""
    slot = (api.stream_bound(size, bs, False, **kw) + 255) & ~255
    enc = torch.empty(len(datas) * slot, dtype=torch.uint8, device="cuda")
    res = []
    for i, d in enumerate(datas):
        t = torch.from_numpy(d).cuda()
        res.append(ctx.stream_encode_gather_device(LEVEL, bs, False, [t.data_ptr()], [t.numel()], enc.data_ptr() + i * slot, slot, **kw))
    torch.cuda.synchronize()
    return enc, (BlockDesc * len(datas))(*[BlockDesc(i * slot, res[i], 0, 0) for i in range(len(datas))]), res, slot


class Set:
    """A set opened through the library `lib` (its context `h`), indexed for newlines; grep() = grep_records + locate_records."""

    def __init__(self, lib, h, enc, descs, n, open_name):
        self.lib, self.n = lib, n
        self.rd, out = C.c_void_p(), (C.c_int64 * n)()
        f = getattr(lib, open_name)
        f.restype, f.argtypes = _lib.ABI_EXT["minlz_hip_stream_set_tables.h" if open_name.endswith("_tables") else "minlz_hip_stream_set.h"][open_name]
        assert f(h, None, enc.data_ptr(), descs, n, out, C.byref(self.rd)) > 0 and min(out) > 0
        info = (C.c_uint64 * 4)()
        self.records = lib.mlz_dev_reader_index_records(self.rd, None, 0, 10, info)
        assert self.records > 0
        self.nums = torch.zeros(CAP, dtype=torch.int64, device="cuda")
        self.kinds = torch.zeros(CAP, dtype=torch.uint8, device="cuda")
        self.which = torch.zeros(CAP, dtype=torch.int32, device="cuda")
        self.line = torch.zeros(CAP, dtype=torch.int64, device="cuda")
        self.totals, self.stats = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()

    def grep(self, blob, lens, npat):
        R = self.lib.mlz_dev_reader_grep_records(self.rd, None, 0, blob, lens, npat, 0, 0, self.nums.data_ptr(), self.kinds.data_ptr(), CAP, self.totals, self.stats)
        assert R >= 0
        k = min(R, CAP)
        assert self.lib.mlz_dev_reader_locate_records(self.rd, None, self.nums.data_ptr(), k, self.which.data_ptr(), self.line.data_ptr()) == k
        return R

    def selected(self, R):
        torch.cuda.synchronize()
        return R, self.which[:R].tolist(), self.line[:R].tolist(), tuple(self.stats)

    def close(self):
        self.lib.mlz_dev_reader_close(self.rd)


rng = np.random.default_rng(5)
base = synth.json_like(48 << 20, seed=7)
results = {"B_library": "parent" if PARENT else "this library"}
say("leg B runs in %s" % (("the parent commit's library, " + os.path.basename(PARENT)) if PARENT else "THIS library (no --parent-lib given): the yardstick is the code under test"))
for n, size, bs in SHAPES:
    src_off = [(i * 1_000_003 * 64) % (len(base) - size) for i in range(n)]
    for npat in (1, 16):
        pats = [bytes(rng.integers(128, 256, 16, dtype=np.uint8)) for _ in range(npat)]
        datas = [base[o:o + size].copy() for o in src_off]
        for d in datas:
            d[-1] = 10                                                                      # every object ends with the delimiter
        used = set()
        for p in pats:   # each needle in 3 streams, in a slot of 32 bytes that no other plant has
            for s in rng.choice(n, 3, replace=False):
                o = int(rng.integers(0, size // 32 - 2)) * 32 + 8
                while (int(s), o) in used:
                    o = int(rng.integers(0, size // 32 - 2)) * 32 + 8
                used.add((int(s), o))
                datas[s][o:o + 16] = np.frombuffer(p, np.uint8)
        blob, lens = b"".join(pats), (C.c_uint32 * npat)(*([16] * npat))
        enc, descs, res, slot = write_batch(datas, size, bs, search_match_len=6)
        a = Set(L, ctx.handle, enc, descs, n, "mlz_stream_open_batch_device_tables")
        b = Set(B, bh, enc, descs, n, "mlz_stream_open_batch_device")
        first = once(lambda: a.grep(blob, lens, npat))                                      # the first search on the handle: discovery included
        ga, gb = a.selected(a.grep(blob, lens, npat)), b.selected(b.grep(blob, lens, npat))
        assert ga[:3] == gb[:3] and ga[0] >= 1 and gb[3][1] == gb[3][0], (ga, gb)
        info = (C.c_uint64 * 6)()
        assert L.mlz_dev_reader_set_tables_info(a.rd, info) == 0 and info[5] == 0 and info[1] == n
        if n * size <= 64 << 20 and npat == 1 and size <= 64 << 10:
            enc_h = enc.cpu().numpy()
            m = M.plan([enc_h[i * slot:i * slot + res[i]].tobytes() for i in range(n)], [d.tobytes() for d in datas], pats, records=True)
            assert ga[3][1] == m["decoded"] and tuple(info) == m["info"], (ga[3], m["decoded"], tuple(info), m["info"])
        say("%d streams of %d bytes in blocks of %d (%.1f MB raw, %.1f MB of streams), %d needles; %d repetitions, the calls alternated" % (n, size, bs, n * size / 1e6, sum(res) / 1e6, npat, REPS))
        say("    A decodes %d of %d chunks (%d with a usable table; %d streams pruned, %d decoded whole, %d ends crossed); B decodes %d.  A's first search, discovery included: %.3f ms" %
            (ga[3][1], ga[3][0], ga[3][2], info[1], info[2], info[5], gb[3][1], first))
        ts = timed([("A", lambda: a.grep(blob, lens, npat)), ("B", lambda: b.grep(blob, lens, npat))])
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            v = sorted(ts[k])
            say("    %2d needles %-2s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (npat, k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
        held = med["B"] - med["A"] > max(iqr(ts["A"]), iqr(ts["B"]))
        say("    %2d needles: B / A = %.2f; the bar (A below B by more than both IQRs): %s" % (npat, med["B"] / med["A"], "held" if held else "MISSED"))
        row = dict({k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}, decoded=ga[3][1], chunks=ga[3][0], first_ms=round(first, 3), bar_held=held)
        if npat == 16:
            # without a bar: search_many on the tabled set against the pruned batch search; 0x46 tables; a batch without tables
            pos, which = torch.zeros(CAP, dtype=torch.int64, device="cuda"), torch.zeros(CAP, dtype=torch.int32, device="cuda")
            st = (C.c_uint64 * 4)()
            present = torch.zeros(n * ((npat + 31) // 32), dtype=torch.int32, device="cuda")
            hs = torch.zeros(CAP, dtype=torch.int32, device="cuda")

            def many():
                assert L.mlz_dev_reader_search_many(a.rd, None, 0, blob, lens, npat, None, pos.data_ptr(), which.data_ptr(), CAP, st) >= 3 * npat - 2

            def batch():
                ctx.stream_search_batch_device(enc.data_ptr(), descs, pats, None, None, present.data_ptr(), hs.data_ptr(), pos.data_ptr(), which.data_ptr(), CAP, prune=True)
            ts2 = timed([("many", many), ("batch", batch)])
            say("    search_many on the tabled set (decodes %d of %d chunks: every stream's last bytes are taken) median %.3f ms (IQR %.3f); search_streams(prune=True) %.3f ms (IQR %.3f)" %
                (st[1], st[0], statistics.median(ts2["many"]), iqr(ts2["many"]), statistics.median(ts2["batch"]), iqr(ts2["batch"])))
            row.update(many=round(statistics.median(ts2["many"]), 4), batch_pruned=round(statistics.median(ts2["batch"]), 4))
            penc, pdescs, pres, _ = write_batch(datas, size, bs, search_match_len=6, search_compress=True)
            pa = Set(L, ctx.handle, penc, pdescs, n, "mlz_stream_open_batch_device_tables")
            pfirst = once(lambda: pa.grep(blob, lens, npat))
            expanded = L.mlz_dev_reader_set_tables_info(pa.rd, info)
            tp = timed([("P", lambda: pa.grep(blob, lens, npat))])["P"]
            say("    the same batch written with compressed tables (%.1f MB of streams, %d tables from 0x46 chunks, %d expanded once): first search %.3f ms, steady median %.3f ms (IQR %.3f), decodes %d" %
                (sum(pres) / 1e6, info[4], expanded, pfirst, statistics.median(tp), iqr(tp), pa.stats[1]))
            row.update(packed_first=round(pfirst, 3), packed=round(statistics.median(tp), 4))
            pa.close()
            del penc
            benc, bdescs, bres, _ = write_batch(datas, size, bs)
            ba, bb = Set(L, ctx.handle, benc, bdescs, n, "mlz_stream_open_batch_device_tables"), Set(B, bh, benc, bdescs, n, "mlz_stream_open_batch_device")
            bfirst = once(lambda: ba.grep(blob, lens, npat))
            ts3 = timed([("C", lambda: ba.grep(blob, lens, npat)), ("D", lambda: bb.grep(blob, lens, npat))])
            say("    a batch without tables: the tabled open's first search %.3f ms, steady median %.3f ms (IQR %.3f) against the plain set's %.3f ms (IQR %.3f)" %
                (bfirst, statistics.median(ts3["C"]), iqr(ts3["C"]), statistics.median(ts3["D"]), iqr(ts3["D"])))
            row.update(bare_first=round(bfirst, 3), bare=round(statistics.median(ts3["C"]), 4), bare_plain=round(statistics.median(ts3["D"]), 4))
            ba.close()
            bb.close()
            del benc
        results["%dx%d_%d" % (n, size, npat)] = row
        a.close()
        b.close()
        del enc
say(json.dumps(results))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
