"""mlz_dev_reader_search_many against a loop of mlz_dev_reader_search calls, on an MI355X (one process, every shape warmed up, the variants
of one pattern count alternated inside every repetition, a device synchronise inside every timed window, medians and interquartile ranges).
Input: the 100 MB json-like stream of tools/stream_search_time.py: LevelFastest, 1 MiB blocks, M = 6, once with type 1 tables and once with
the long-prefix tables (type 4) of '"user":"', E = 3.  Pattern sets of n = 1, 16, 64, 1024 and 4096 needles: 16 random bytes each over the
type 1 stream; over the type 4 stream '"user":"' and 14 letters (22 bytes: a 16-byte needle has no whole group behind that prefix, so the
tables could not serve it).  Two series: all absent, and one needle in sixteen (at least one) planted once in the data.

  a_many      one search_many call (cap 64)
  b_loop      the loop of n mlz_dev_reader_search calls (cap 64 each)
  c_all       one MLZ_SEARCH_NO_TABLES single search: decode everything, scan for one pattern
  many_all    search_many with MLZ_SEARCH_NO_TABLES over the same set: every chunk decoded once and scanned for n patterns.  many_all - c_all
              at n = 1 .. 4096 bounds how the scan's time grows with n.  It is a difference of whole-call times, not the scan kernel alone: it also
              holds the index upload and the per-group prefix and write launches (a kernel trace of its own is outstanding)

For n >= 16, a_many passes when it beats b_loop by more than the two interquartile ranges together.

usage: python tools/stream_search_many_time.py [out.txt]"""
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
from minlz_amd import synth

BS, M, E = 1 << 20, 6, 3
USER = b'"user":"'
NS = [1, 16, 64, 1024, 4096]
REPS = {1: 15, 16: 15, 64: 15, 1024: 7, 4096: 5}
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


rng = np.random.default_rng(7)
d = bytearray(synth.json_like(100_000_000, seed=1).tobytes())
NP = max(NS) // 16
present = {"type1": [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(NP)],
           "long_user": [USER + rng.integers(97, 123, 14, dtype=np.uint8).tobytes() for _ in range(NP)]}
absent = {"type1": [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(max(NS))],
          "long_user": [USER + rng.integers(97, 123, 14, dtype=np.uint8).tobytes() for _ in range(max(NS))]}
places = rng.permutation(len(d) // 4096 - 2)[:2 * NP] * 4096 + 100          # apart from one another, anywhere in the data
for i in range(NP):
    for v, o in (("type1", int(places[2 * i])), ("long_user", int(places[2 * i + 1]))):
        d[o:o + len(present[v][i])] = present[v][i]
d = bytes(d)
src = torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()
cap = mz._lib.lib().mlz_stream_bound(len(d), BS, 0) + (len(d) // BS + 2) * (300 + (1 << 17)) + 1024
rd, keep = {}, []
for v, kw in (("type1", dict(search_match_len=M)), ("long_user", dict(search_match_len=M, search_long_prefix=USER, search_extras=E))):
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    size = ctx.stream_encode_gather_device(mz.LevelFastest, BS, False, [src.data_ptr()], [len(d)], dst.data_ptr(), cap, **kw)
    keep.append(dst)
    rd[v] = ctx.stream_open_device(dst.data_ptr(), size)
pos = torch.zeros(64, dtype=torch.int64, device="cuda")
which = torch.zeros(64, dtype=torch.int32, device="cuda")
counts = torch.zeros(max(NS), dtype=torch.int64, device="cuda")


def pattern_set(v, n, series):
    k = 0 if series == "absent" else max(1, n // 16)
    return present[v][:k] + absent[v][:n - k], k


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


say("100 MB json-like, LevelFastest, 1 MiB blocks, M = %d; type 1 tables (16-byte needles) and type 4 tables of %r, E = %d (22-byte needles)" % (M, USER, E))
result = {}
for v in ("type1", "long_user"):
    for series in ("absent", "present"):
        for n in NS:
            pats, k = pattern_set(v, n, series)
            info = {}

            def a_many():
                total, st = rd[v].search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), 64)
                assert total == k, (total, k)
                info["a"] = st

            def b_loop():
                total, dec = 0, 0
                for p in pats:
                    t, st = rd[v].search(p, pos.data_ptr(), 64)
                    total += t
                    dec += st[1]
                assert total == k
                info["b"] = dec

            def c_all():
                total, st = rd[v].search(pats[0], pos.data_ptr(), 64, no_tables=True)
                info["c"] = st

            def many_all():
                total, st = rd[v].search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), 64, no_tables=True)
                assert total == k
                info["all"] = st

            fs = [("a_many", a_many), ("b_loop", b_loop), ("c_all", c_all), ("many_all", many_all)]
            for _, f in fs:
                f()
                torch.cuda.synchronize()
            ts = {name: [] for name, _ in fs}
            for _ in range(REPS[n]):
                for name, f in fs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            med = {name: statistics.median(t) for name, t in ts.items()}
            spread = {name: iqr(t) for name, t in ts.items()}
            verdict = ""
            if n >= 16:
                verdict = "  a beats b" if med["a_many"] + spread["a_many"] + spread["b_loop"] < med["b_loop"] else "  a DOES NOT beat b"
            say("  %-9s %-7s n=%4d  a_many %8.3f (IQR %6.3f, %3d of %d chunks decoded, %d unserved)  b_loop %9.3f (IQR %7.3f, %d chunk decodes)  c_all %6.3f  many_all %8.3f (IQR %6.3f)  many_all - c_all %7.3f%s"
                % (v, series, n, med["a_many"], spread["a_many"], info["a"][1], info["a"][0], info["a"][3], med["b_loop"], spread["b_loop"], info["b"], med["c_all"], med["many_all"],
                   spread["many_all"], med["many_all"] - med["c_all"], verdict))
            result["%s/%s/%d" % (v, series, n)] = {"a_many": round(med["a_many"], 4), "a_iqr": round(spread["a_many"], 4), "b_loop": round(med["b_loop"], 4), "b_iqr": round(spread["b_loop"], 4),
                                                    "c_all": round(med["c_all"], 4), "many_all": round(med["many_all"], 4), "decoded": info["a"][1], "loop_decodes": info["b"]}
say("  " + json.dumps(result))
for r in rd.values():
    r.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
