"""The batch Writer with block search tables (mlz_stream_encode_batch_device_tables) against what a caller had to do before it, on an MI355X:
one process, every call warmed up, REPS timed repetitions with the calls alternated, medians and interquartile ranges, a device synchronise
inside every timed window.  JSON-like data, LevelFastest, table type 1 with M = 6.

  shapes   1024 inputs of 64 KiB at blocks of 64 KiB; 256 of 1 MiB at 64 KiB; 4096 of 4 KiB at 4 KiB; 4096 of 4 KiB at blocks of 1 MiB
           (every block is a stream's last and only one: the shape the pre-folded tables are for)
  A        mlz_stream_encode_batch_device_tables, one call
  B        a loop of mlz_stream_encode_gather_device with MLZ_STREAM_SEARCH_TABLES, one call per input: what wrote a tabled batch before
  C        mlz_stream_encode_batch_device, one call: the same streams without tables
With --parent-lib B and C run in the library given there (a build of the parent commit, loaded beside this one), so that the yardstick is
not the code under test; without it, in this library, and the output says so.
Before anything is timed A's streams are compared byte for byte with B's.

The bar: A's median below B's by more than both interquartile ranges, at every shape.  Recorded without a bar: A / C and A - C per 100 MB
(what the tables cost a batch; the single Writer's cost 0.14 ms per 100 MB), and the bytes of table slots A carved (mlz_get_counter 17)
against blocks x 2^(B - 3), what slots sized by the block size would take.  After the timing every batch A wrote is searched pruned
(mlz_stream_search_batch_device_pruned) for a needle planted in 3 inputs: the chunks decoded of the chunks present.

usage: python tools/stream_encode_batch_tables_time.py [--parent-lib libminlz_hip.so] [out.txt]"""
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

args = sys.argv[1:]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else None

REPS, M = 25, 6
LEVEL = mz.LevelFastest
SEARCH_TABLES = 4
SHAPES = [(1024, 64 << 10, 64 << 10), (256, 1 << 20, 64 << 10), (4096, 4 << 10, 4 << 10), (4096, 4 << 10, 1 << 20)]   # (inputs, bytes each, block size)
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# the library of legs B and C: the parent commit's, loaded beside this one, with a context of its own
P, ph = L, ctx.handle
GATHER, BATCH = "mlz_stream_encode_gather_device", "mlz_stream_encode_batch_device"
if PARENT:
    P = C.CDLL(PARENT)
    for name in ("mlz_init", GATHER, BATCH):
        getattr(P, name).restype, getattr(P, name).argtypes = _lib.ABI[name]
    ph = C.c_void_p()
    assert P.mlz_init(0, C.byref(ph)) == 0


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


rng = np.random.default_rng(5)
base = synth.json_like(48 << 20, seed=7)
results = {"BC_library": "parent" if PARENT else "this library"}
say("legs B and C run in %s" % (("the parent commit's library, " + os.path.basename(PARENT)) if PARENT else "THIS library (no --parent-lib given): the yardstick is the code under test"))
for n, size, bs in SHAPES:
    needle = bytes(rng.integers(128, 256, 16, dtype=np.uint8))
    src = np.empty(n * size, np.uint8)
    for i in range(n):
        o = (i * 1_000_003 * 64) % (len(base) - size)
        src[i * size:(i + 1) * size] = base[o:o + size]
    planted = sorted(int(s) for s in rng.choice(n, 3, replace=False))
    for s in planted:
        o = s * size + size // 2 + 8
        src[o:o + 16] = np.frombuffer(needle, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    slot = (api.stream_bound(size, bs, False, search_match_len=M) + 255) & ~255
    outs = {k: torch.zeros(n * slot, dtype=torch.uint8, device="cuda") for k in "ABC"}
    descs = (BlockDesc * n)(*[BlockDesc(i * size, size, i * slot, slot) for i in range(n)])
    cfg = api.batch_tables_config(search_match_len=M)
    lens = {k: (C.c_int64 * n)() for k in "AC"}
    b_len = [0] * n
    one_src, one_len = (C.c_void_p * 1)(), (C.c_size_t * 1)(size)

    def leg_a():
        assert L.mlz_stream_encode_batch_device_tables(ctx.handle, None, LEVEL, bs, 0, C.byref(cfg), d_src.data_ptr(), outs["A"].data_ptr(), descs, n, lens["A"]) == 0

    def leg_b():
        for i in range(n):
            one_src[0] = d_src.data_ptr() + i * size
            b_len[i] = getattr(P, GATHER)(ph, LEVEL, bs, SEARCH_TABLES | M << 8, one_src, one_len, 1, outs["B"].data_ptr() + i * slot, slot)

    def leg_c():
        assert getattr(P, BATCH)(ph, None, LEVEL, bs, 0, d_src.data_ptr(), outs["C"].data_ptr(), descs, n, lens["C"]) == 0

    legs = [("A", leg_a), ("B", leg_b), ("C", leg_c)]
    for _, f in legs:
        f()
    torch.cuda.synchronize()
    # the check first: A's streams are B's, byte for byte
    a_h, b_h = outs["A"].cpu().numpy(), outs["B"].cpu().numpy()
    assert list(lens["A"]) == b_len and min(b_len) > 0, "the streams' sizes differ"
    for i in range(n):
        assert np.array_equal(a_h[i * slot:i * slot + b_len[i]], b_h[i * slot:i * slot + b_len[i]]), "stream %d differs" % i
    blocks = n * ((size + bs - 1) // bs)
    B_bits = max(8, min(23, (bs - 1).bit_length()))
    carved, uniform = ctx.table_slot_bytes, blocks << (B_bits - 3)
    raw_mb = n * size / 1e6
    say("%d inputs of %d bytes at blocks of %d (%.1f MB raw, %.1f MB of streams with tables, %.1f MB without); %d repetitions, the calls alternated; A's bytes are B's" %
        (n, size, bs, raw_mb, sum(b_len) / 1e6, sum(lens["C"]) / 1e6, REPS))
    say("    table slots: %d bytes carved for %d blocks (counter 17); slots of 2^(B - 3) = %d bytes each would take %d (%.1f x)" % (carved, blocks, 1 << (B_bits - 3), uniform, uniform / max(carved, 1)))
    ts = timed(legs)
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in ts:
        v = sorted(ts[k])
        say("    %s median %9.3f ms   min %9.3f   p90 %9.3f   IQR %7.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))], iqr(ts[k])))
    held = med["B"] - med["A"] > max(iqr(ts["A"]), iqr(ts["B"]))
    say("    B / A = %.1f; A / C = %.2f, A - C = %.3f ms = %.3f ms per 100 MB; the bar (A below B by more than both IQRs): %s" %
        (med["B"] / med["A"], med["A"] / med["C"], med["A"] - med["C"], (med["A"] - med["C"]) * 100 / raw_mb, "held" if held else "MISSED"))
    # what A wrote, searched pruned for the planted needle
    spans = [(i * slot, b_len[i]) for i in range(n)]
    total, res, stats = ctx.stream_search_batch_device(outs["A"].data_ptr(), spans, [needle], prune=True)
    assert total == 3 and [i for i, r in enumerate(res) if r] == planted, (total, planted)
    say("    pruned search of A's batch for a needle planted in 3 inputs: %d of %d chunks decoded, %d with a usable table, %d of %d streams skipped" % (stats[1], stats[0], stats[4], stats[5], n))
    results["%dx%d_bs%d" % (n, size, bs)] = dict({k: round(v, 4) for k, v in med.items()}, **{k + "_iqr": round(iqr(v), 4) for k, v in ts.items()}, slot_bytes=carved,
                                                 uniform_slot_bytes=uniform, decoded=int(stats[1]), chunks=int(stats[0]), bar_held=held)
    del outs, d_src
say(json.dumps(results))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
