"""The device-resident Reader against what a caller had to do without it, on an MI355X (one process, every shape warmed up, REPS timed
repetitions with the variants alternated, medians, a device synchronise inside every timed window):

  t_walk   mlz_stream_decoded_len_device (chunk walk + table read-back)
  t_alt    the same answer without it: the stream copied from HBM to pinned host memory, then mlz_stream_decoded_len
  t_total  mlz_stream_decode_device
  t_floor  mlz_decode_batch_device + mlz_crc_batch_device on the same chunks, descriptors prepared on the host outside the timed window
           (on a copy of the stream whose CRC bytes in front of every block are zeroed, so that each chunk reads as a whole block)

Inputs: (a) the bench stream (100 MB enwik-like, LevelFastest, 8 MiB blocks), (b) its first 64 MiB in 4 KiB blocks, (c) a stream of
1 000 000 empty skippable chunks with a small data chunk after every 1 000.  usage: python tools/stream_device_time.py [out.txt]"""
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
from minlz_amd import stream as S
from minlz_amd._lib import BlockDesc
from tests import stream_device_cases as SC

REPS = 25
L = _lib.lib()
ctx = mz.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(name, s, d):
    n = len(s)
    t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    out = torch.empty(len(d) + 64, dtype=torch.uint8, device="cuda")
    pin = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    # the floor's descriptors: every data chunk as a block `00 uvarint(N) tokens` / `00 00 raw`-free: stored chunks are copied by torch outside the floor
    clone = bytearray(s)
    dec, crc, p, o = [], [], 0, 0
    while p + 4 <= n:
        ty, cl = s[p], s[p + 1] | s[p + 2] << 8 | s[p + 3] << 16
        if ty == 0x02:
            nn, hl = S.uvarint(s, p + 8)
            clone[p + 7] = 0
            dec.append(BlockDesc(p + 7, cl - 3, o, nn))
            crc.append(BlockDesc(o, nn, 0, 0))
            o += nn
        elif ty == 0x01:
            crc.append(BlockDesc(o, cl - 4, 0, 0))
            o += cl - 4
        p += 4 + cl
    tc = torch.from_numpy(np.frombuffer(bytes(clone), np.uint8).copy()).cuda()
    darr, carr = (BlockDesc * max(len(dec), 1))(*dec), (BlockDesc * max(len(crc), 1))(*crc)
    lens = torch.zeros(max(len(dec), 1), dtype=torch.int64, device="cuda")
    crcs = torch.zeros(max(len(crc), 1), dtype=torch.int32, device="cuda")

    def walk():
        r, _ = ctx.stream_decoded_len_device(t.data_ptr(), n)
        assert r == len(d)

    def alt():
        pin.copy_(t, non_blocking=True)
        torch.cuda.synchronize()
        assert L.mlz_stream_decoded_len(pin.data_ptr(), n) == len(d)

    def total():
        assert ctx.stream_decode_device(t.data_ptr(), n, out.data_ptr(), len(d)) == len(d)

    def floor():
        if dec:
            assert L.mlz_decode_batch_device(ctx.handle, None, tc.data_ptr(), out.data_ptr(), darr, len(dec), lens.data_ptr()) == 0
        assert L.mlz_crc_batch_device(ctx.handle, None, out.data_ptr(), carr, len(crc), crcs.data_ptr()) == 0

    fs = [("t_walk", walk), ("t_alt", alt), ("t_total", total), ("t_floor", floor)]
    for _ in range(3):
        for _, f in fs:
            f()
            torch.cuda.synchronize()
    total()
    torch.cuda.synchronize()
    assert out[:len(d)].cpu().numpy().tobytes() == d
    ts = {k: [] for k, _ in fs}
    for _ in range(REPS):
        for k, f in fs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ts.items()}
    say("%s: stream %d B, decoded %d B, %d data chunks (%d compressed), %d repetitions" % (name, n, len(d), len(crc), len(dec), REPS))
    for k, _ in fs:
        v = sorted(ts[k])
        say("  %-8s median %8.3f ms   min %8.3f   p90 %8.3f" % (k, med[k], v[0], v[int(0.9 * (len(v) - 1))]))
    say("  t_total - t_floor = %.3f ms; t_walk %s t_alt" % (med["t_total"] - med["t_floor"], "<=" if med["t_walk"] <= med["t_alt"] else ">"))
    say("  " + json.dumps({"input": name, "stream_bytes": n, **{k: round(v, 4) for k, v in med.items()}}))


a = synth.enwik_like(100_000_000, seed=1).tobytes()
measure("(a) bench stream, 8 MiB blocks", mz.stream_encode(a, mz.LevelFastest, 8 << 20, False, ctx), a)
b = a[:64 << 20]
measure("(b) 64 MiB in 4 KiB blocks", mz.stream_encode(b, mz.LevelFastest, 4 << 10, False, ctx), b)
cs, cd = SC.tiny_chunks(1_000_000, 1_000)
measure("(c) 1 000 000 empty skippable chunks, 1 000 data chunks", cs, cd)
say("decode-side workspace held: %d bytes" % ctx.workspace_bytes()[1])
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
