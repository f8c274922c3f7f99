"""What the GPU tests of the device-resident Writer's search tables, of the pattern search and of the record calls share
(tests/test_gpu_stream_*.py, tests/test_gpu_sidecar.py): inputs on the device, the Writer call with a guarded destination, an opened
stream, the search call with guarded results."""
import numpy as np
import torch

from minlz_amd import api, synth

SENT = 0x5A5A5A5A5A5A5A5A


def dev_u8(b):
    """bytes -> a uint8 tensor on the device."""
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def dev_u64(values):
    """uint64 values -> an int64 tensor on the device with the same bits."""
    a = np.asarray(values, dtype=np.uint64).view(np.int64)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.empty(0, dtype=torch.int64, device="cuda")


def on_device(parts):
    return [dev_u8(p) for p in parts]


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


def gather(ctx, parts, bs, add_index=False, level=1, cap=None, **tables):
    """The device-resident Writer's stream of `parts` (bytes objects, one range each), without tables or with those the search_* keywords
    of Context.stream_encode_gather_device ask for.  The room is what api.stream_bound says (or `cap`), and nothing is written behind it."""
    if cap is None:
        cap = api.stream_bound(sum(len(p) for p in parts), bs, add_index, **tables)
    return gather_into(ctx, parts, cap, level, bs, add_index, **tables)


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def data_for(kind, bs, nblk, tail, seed=4, random_block=1):
    d = bytearray(getattr(synth, kind)(bs * nblk + tail, seed).tobytes())
    if random_block is not None:
        d[random_block * bs:(random_block + 1) * bs] = synth.random_bytes(bs, seed=6).tobytes()
    return bytes(d)


class Opened:
    """A stream's bytes on the device and the reader opened on them."""

    def __init__(self, ctx, stream):
        self.ctx, self.t = ctx, dev_u8(stream)
        self.rd = ctx.stream_open_device(self.t.data_ptr() if len(stream) else None, len(stream))

    def close(self):
        self.rd.close()


class Searcher(Opened):
    def __call__(self, pattern, cap, null=False, **kw):
        """-> (total, positions, stats); checks that nothing beyond min(total, cap) was written."""
        out = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search(pattern, None if null else out.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        k = min(total, cap)
        assert (o[k:] == SENT).all(), "written beyond the results"
        assert self.ctx.search_plan() == stats[1:]
        return total, o[:k].tolist(), stats
