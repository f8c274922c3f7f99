"""What the GPU tests of the device-resident Writer's search tables and of the pattern search share (tests/test_gpu_stream_search*.py,
tests/test_gpu_stream_writer_cuts.py): inputs on the device, the Writer call with a guarded destination, the search call with guarded
results."""
import numpy as np
import torch

from minlz_amd import synth

SENT = 0x5A5A5A5A5A5A5A5A


def on_device(parts):
    return [torch.from_numpy(np.frombuffer(p, np.uint8).copy()).cuda() if len(p) else torch.empty(0, dtype=torch.uint8, device="cuda") for p in parts]


def gather_into(ctx, parts, cap, level, bs, add_index, **kw):
    """ctx.stream_encode_gather_device over `parts` (bytes objects, one range each) into `cap` bytes of room -> the stream's bytes; nothing
    is written behind the room."""
    assert cap > 0
    srcs = on_device(parts)
    dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    got = ctx.stream_encode_gather_device(level, bs, add_index, [t.data_ptr() if t.numel() else None for t in srcs], [t.numel() for t in srcs], dst.data_ptr(), cap, **kw)
    o = dst.cpu().numpy()
    assert got <= cap and (o[cap:] == 0x5A).all()
    return o[:got].tobytes()


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def data_for(kind, bs, nblk, tail, seed=4, random_block=1):
    d = bytearray(getattr(synth, kind)(bs * nblk + tail, seed).tobytes())
    if random_block is not None:
        d[random_block * bs:(random_block + 1) * bs] = synth.random_bytes(bs, seed=6).tobytes()
    return bytes(d)


class Searcher:
    def __init__(self, ctx, stream):
        self.ctx = ctx
        self.t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
        self.rd = ctx.stream_open_device(self.t.data_ptr(), len(stream))

    def __call__(self, pattern, cap, **kw):
        """-> (total, positions, stats); checks that nothing beyond min(total, cap) was written."""
        out = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search(pattern, out.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        k = min(total, cap)
        assert (o[k:] == SENT).all(), "written beyond the results"
        assert self.ctx.search_plan() == stats[1:]
        return total, o[:k].tolist(), stats

    def close(self):
        self.rd.close()
