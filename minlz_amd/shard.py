"""Multi-GPU sharding of a stream's independent blocks.

One process per GPU (torch.distributed, backend "nccl" = RCCL on ROCm; "gloo" in the CPU tests).
Block i of the stream belongs to rank i mod G.  Every rank encodes only its own blocks; the single
exchange is the *gather*: an all_gather of per-block compressed sizes (so every rank knows the
stream layout = the Writer's in-order output and index offsets, writer.go:223-243, index.go:80-104)
and, when one rank has to hold the assembled stream, a gather of the variable-length payloads
padded to a common size.  No reduction, no all-to-all.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import stream as S


def owner(block_index, world):
    return block_index % world


def my_blocks(n_blocks, rank, world):
    return list(range(rank, n_blocks, world))


def cut_blocks(n, block_size):
    return [(o, min(block_size, n - o)) for o in range(0, n, block_size)]


def gather_sizes(local_sizes, n_blocks, rank, world, device="cpu"):
    """all_gather of per-block chunk sizes -> list of n_blocks sizes in stream order."""
    per = (n_blocks + world - 1) // world
    t = torch.zeros(per, dtype=torch.int64, device=device)
    if local_sizes:
        t[:len(local_sizes)] = torch.tensor(local_sizes, dtype=torch.int64, device=device)
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    sizes = [0] * n_blocks
    for r in range(world):
        for j, bi in enumerate(my_blocks(n_blocks, r, world)):
            sizes[bi] = int(parts[r][j].item())
    return sizes


def encode_stream_sharded(data, level, block_size, backend, rank, world, device="cpu", root=0):
    """Every rank passes the same `data`; returns the framed stream on `root` (None elsewhere)."""
    data = bytes(data)
    cuts = cut_blocks(len(data), block_size)
    mine = my_blocks(len(cuts), rank, world)
    blocks = [data[o:o + l] for o, l in (cuts[i] for i in mine)]
    bodies = backend.encode_blocks(blocks, level) if blocks else []
    crcs = backend.crcs(blocks) if blocks else []
    chunks = []
    for blk, body, crc in zip(blocks, bodies, crcs):
        ctype, payload = (S.CHUNK_MINLZ, body) if body is not None else (S.CHUNK_UNCOMPRESSED, blk)
        clen = 4 + len(payload)
        chunks.append(bytes([ctype, clen & 0xFF, (clen >> 8) & 0xFF, (clen >> 16) & 0xFF]) + crc.to_bytes(4, "little") + payload)
    sizes = gather_sizes([len(c) for c in chunks], len(cuts), rank, world, device)
    # payload gather to root: each rank sends its chunks concatenated, padded to the largest rank total
    totals = [sum(sizes[i] for i in my_blocks(len(cuts), r, world)) for r in range(world)]
    pad = max(totals + [1])
    buf = torch.zeros(pad, dtype=torch.uint8, device=device)
    flat = b"".join(chunks)
    if flat:
        buf[:len(flat)] = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(device)
    if dist.get_backend() == "nccl":  # RCCL: all_gather of the padded payloads (gather is built on it)
        parts = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf)
    else:
        parts = [torch.zeros_like(buf) for _ in range(world)] if rank == root else None
        dist.gather(buf, parts, dst=root)
    if rank != root:
        return None
    per_rank = [bytes(parts[r][:totals[r]].cpu().numpy().tobytes()) for r in range(world)]
    cursor = [0] * world
    out = bytearray()
    if cuts:
        out += S.MAGIC + bytes([(block_size - 1).bit_length() - 10])
    for bi in range(len(cuts)):
        r = owner(bi, world)
        out += per_rank[r][cursor[r]:cursor[r] + sizes[bi]]
        cursor[r] += sizes[bi]
    v = S.put_uvarint(len(data))
    out += bytes([S.CHUNK_EOF, len(v), 0, 0]) + v
    return bytes(out)


# =====================================================================================================================
# Device-resident path: one stream cut into contiguous block ranges, one range per rank, payload gather on the device
# =====================================================================================================================
#
# The Writer's concurrent path (writer.go:219-272, :501-560) compresses blocks on worker goroutines and a single
# writer goroutine emits the chunks in order.  Here the workers are the GPUs of a node: rank r keeps blocks
# [r*k, (r+1)*k) of the stream in ITS HBM, encodes them with one device batch call, frames them into a contiguous
# run of chunks on the device, and the only data exchange is the in-order gather of those runs into the root's HBM:
#   all_gather of (chunk size) per block      -> every rank knows the stream layout (8 bytes per block)
#   isend / irecv of the runs                 -> root receives each rank's run at its final offset (RCCL p2p over xGMI;
#                                                gloo in the CPU tests) — no padding, no Python bytes, no host staging
# The gather can be started asynchronously and overlapped with whatever the rank does next (bench.py decodes).

def range_of(rank, world, n_blocks):
    """Contiguous block range [b0, b1) of `rank`: the first ranks take one block more when it does not divide."""
    per, extra = divmod(n_blocks, world)
    b0 = rank * per + min(rank, extra)
    return b0, b0 + per + (1 if rank < extra else 0)


class HipTensorCodec:
    """CUDA tensors through the C ABI's device-resident batch calls (the product path)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def encode(self, src, block_lens, level):
        from ._lib import BlockDesc
        n = len(block_lens)
        stride = (max(block_lens + [0]) + 2 + 255) & ~255
        dev = src.device
        enc = torch.empty(max(n * stride, 1), dtype=torch.uint8, device=dev)
        lens = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        crc32 = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        if n:
            offs = np.concatenate([[0], np.cumsum(block_lens)[:-1]]).tolist()
            desc = (BlockDesc * n)(*[BlockDesc(int(offs[i]), int(block_lens[i]), i * stride, stride) for i in range(n)])
            st = torch.cuda.current_stream(dev).cuda_stream
            self.ctx.encode_batch_device(st, level, src.data_ptr(), enc.data_ptr(), desc, lens.data_ptr())
            self.ctx.crc_batch_device(st, src.data_ptr(), desc, crc32.data_ptr())
        return enc, stride, lens[:n], (crc32[:n].to(torch.int64) & 0xFFFFFFFF)

    def decode(self, enc, blocks, out):
        """blocks: [(src_off, src_len, dst_off, dst_len)] — whole blocks `00 uvarint(N) tokens` / `00 00 raw` inside `enc`, decoded
        to out[dst_off : dst_off + dst_len].  -> int64 tensor on the device: the decoded length of each block or -MLZ_ERR_*."""
        from ._lib import BlockDesc
        n = len(blocks)
        lens = torch.zeros(max(n, 1), dtype=torch.int64, device=enc.device)
        if n:
            desc = (BlockDesc * n)(*[BlockDesc(int(a), int(b), int(c), int(d)) for a, b, c, d in blocks])
            st = torch.cuda.current_stream(enc.device).cuda_stream
            self.ctx.decode_batch_device(st, enc.data_ptr(), out.data_ptr(), desc, lens.data_ptr())
        return lens[:n]

    def crcs(self, base, spans):
        """Masked CRC32C (minlz.go:133-140) of base[off : off + len] for each (off, len) -> int64 tensor on the device."""
        from ._lib import BlockDesc
        n = len(spans)
        crc32 = torch.zeros(max(n, 1), dtype=torch.int32, device=base.device)
        if n:
            desc = (BlockDesc * n)(*[BlockDesc(int(o), int(l), 0, 0) for o, l in spans])
            st = torch.cuda.current_stream(base.device).cuda_stream
            self.ctx.crc_batch_device(st, base.data_ptr(), desc, crc32.data_ptr())
        return crc32[:n].to(torch.int64) & 0xFFFFFFFF

    def decode_stream(self, t, ignore_crc=False):
        """A whole .mz stream that lies on the device (uint8 tensor) -> its decoded bytes, a new uint8 tensor on the same device.  The chunks
        are found on the device (mlz_stream_decoded_len_device sizes the output) and decoded where they lie (mlz_stream_decode_device): no
        payload visits the host.  Raises the Reader's first error in stream order, like api.stream_decode."""
        if t.dtype != torch.uint8 or not t.is_cuda:
            raise ValueError("decode_stream: a uint8 tensor on the device")
        t = t.contiguous()
        st = torch.cuda.current_stream(t.device).cuda_stream
        n, prefix = self.ctx.stream_decoded_len_device(t.data_ptr(), t.numel(), stream=st)
        cap = n if n >= 0 else prefix   # a framing error: the chunks in front of it are decoded and checked first
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=t.device)
        r = self.ctx.stream_decode_device(t.data_ptr(), t.numel(), out.data_ptr(), cap, ignore_crc=ignore_crc, stream=st)
        return out[:r]

    @staticmethod
    def _raise_stream(what, i, code):
        """The error of stream i of a batch: the class of its code, the index in the message and in .index."""
        from . import api
        e = api._ERRS.get(-code, api.MinLZError)("%s: stream %d of the batch: minlz error %d" % (what, i, -code))
        e.code, e.index = -code, i
        raise e

    def decode_streams(self, t, spans, ignore_crc=False):
        """Many .mz streams that lie in one uint8 tensor on the device, stream i at t[off_i : off_i + len_i] for spans[i] = (off_i, len_i) ->
        (out, starts): their decoded bytes packed into one new uint8 tensor on the same device, and the n + 1 places where they start in it
        (a list of ints; the last is out's size).  One batch walk sizes the output (mlz_stream_decoded_len_batch_device), one batch call
        decodes (mlz_stream_decode_batch_device).  Raises the first failing stream's error, which names its index (.index)."""
        if t.dtype != torch.uint8 or not t.is_cuda:
            raise ValueError("decode_streams: a uint8 tensor on the device")
        t = t.contiguous()
        spans = [(int(o), int(n)) for o, n in spans]
        for o, n in spans:
            if o < 0 or n < 0 or o + n > t.numel():
                raise ValueError("decode_streams: a span leaves the tensor")
        if not spans:
            return torch.empty(0, dtype=torch.uint8, device=t.device), [0]
        st = torch.cuda.current_stream(t.device).cuda_stream
        lens = self.ctx.stream_decoded_len_batch_device(t.data_ptr(), spans, stream=st)
        starts = [0]
        for r, prefix in lens:   # a framing error: the chunks in front of it are decoded and checked first
            starts.append(starts[-1] + (r if r >= 0 else prefix))
        out = torch.empty(max(starts[-1], 1), dtype=torch.uint8, device=t.device)
        descs = [(o, n, starts[i], starts[i + 1] - starts[i]) for i, (o, n) in enumerate(spans)]
        res = self.ctx.stream_decode_batch_device(t.data_ptr(), out.data_ptr(), descs, ignore_crc=ignore_crc, stream=st)
        for i, r in enumerate(res):
            if r < 0:
                self._raise_stream("decode_streams", i, r)
        return out[:starts[-1]], starts

    def encode_streams(self, t, spans, level, block_size=1 << 20, add_index=False):
        """Every input t[off_i : off_i + len_i] (a uint8 tensor on the device, spans[i] = (off_i, len_i)) as a .mz stream of its own ->
        (out, stream_spans): one new uint8 tensor on the same device and where each stream lies in it, [(off, len)] (with room between
        them: every stream is written at the place its bound reserves).  One call (mlz_stream_encode_batch_device); the bytes are
        api.stream_encode's.  Raises the first failing stream's error, which names its index (.index)."""
        from . import _lib
        if t.dtype != torch.uint8 or not t.is_cuda:
            raise ValueError("encode_streams: a uint8 tensor on the device")
        t = t.contiguous()
        spans = [(int(o), int(n)) for o, n in spans]
        flags = 1 if add_index else 0
        descs, at = [], 0
        for o, n in spans:
            if o < 0 or n < 0 or o + n > t.numel():
                raise ValueError("encode_streams: a span leaves the tensor")
            cap = int(_lib.lib().mlz_stream_bound(n, block_size, flags))
            if cap < 0:
                raise ValueError("encode_streams: block size %d" % block_size)
            descs.append((o, n, at, cap))
            at += cap
        out = torch.empty(max(at, 1), dtype=torch.uint8, device=t.device)
        if not spans:
            return out[:0], []
        st = torch.cuda.current_stream(t.device).cuda_stream
        res = self.ctx.stream_encode_batch_device(level, block_size, add_index, t.data_ptr(), out.data_ptr(), descs, stream=st)
        for i, r in enumerate(res):
            if r < 0:
                self._raise_stream("encode_streams", i, r)
        return out, [(d[2], r) for d, r in zip(descs, res)]

    def open_stream(self, t):
        """A .mz stream that lies on the device (uint8 tensor) opened for range reads -> DeviceStream (ReadAt, read_ranges).  The chunk walk
        runs once, here; a framing error raises."""
        if t.dtype != torch.uint8 or not t.is_cuda:
            raise ValueError("open_stream: a uint8 tensor on the device")
        return DeviceStream(self.ctx, t.contiguous())


class DeviceStream:
    """A .mz stream on the device opened for random access (HipTensorCodec.open_stream): ReadSeeker.ReadAt (reader.go:1401-1487) with the
    device walk's chunk table in the place of the seek index.  Keeps the stream's tensor alive."""

    def __init__(self, ctx, t):
        self.t = t
        st = torch.cuda.current_stream(t.device).cuda_stream
        self.reader = ctx.stream_open_device(t.data_ptr(), t.numel(), stream=st)
        self.size = self.reader.size
        self.side = None   # the attached sidecar's tensor

    def read_ranges(self, offsets, lengths, ignore_crc=False, return_starts=False):
        """Decoded bytes [offsets[i], offsets[i] + lengths[i]) for every i, back to back in the order given -> one new uint8 tensor.
        return_starts: -> (that tensor, the n + 1 places where the ranges start in it and its size: int64 on the stream's device).
        Two CUDA tensors (int64 or uint64, contiguous, on the stream's device) take the device path (mlz_dev_reader_read_device): the ranges
        stay in device memory and are planned by kernels; the one thing that visits the host is the scalar int(lengths.sum()), which sizes the
        output.  Lists and numpy arrays (and tensors on the CPU) are planned on the host."""
        if torch.is_tensor(offsets) and torch.is_tensor(lengths) and offsets.is_cuda and lengths.is_cuda:
            return self._read_ranges_device(offsets, lengths, ignore_crc, return_starts)
        if torch.is_tensor(offsets):
            offsets = offsets.numpy()
        if torch.is_tensor(lengths):
            lengths = lengths.numpy()
        r = np.empty((len(offsets), 3), dtype=np.uint64)
        r[:, 0] = offsets
        r[:, 1] = lengths
        total = int(r[:, 1].sum())
        r[:, 2] = np.cumsum(r[:, 1]) - r[:, 1]
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.t.device)
        st = torch.cuda.current_stream(self.t.device).cuda_stream
        got = self.reader.read(r, out.data_ptr(), total, ignore_crc=ignore_crc, stream=st)
        if return_starts:
            return out[:got], torch.from_numpy(np.concatenate([r[:, 2], [total]]).astype(np.int64)).to(self.t.device)
        return out[:got]

    def _read_ranges_device(self, offsets, lengths, ignore_crc, return_starts):
        dev = self.t.device
        for a in (offsets, lengths):
            if a.dtype not in (torch.int64, torch.uint64) or a.dim() != 1 or not a.is_contiguous() or a.device != dev:
                raise ValueError("read_ranges: device ranges are contiguous 1-d int64 or uint64 tensors on the stream's device")
        n = offsets.numel()
        if lengths.numel() != n:
            raise ValueError("read_ranges: as many lengths as offsets")
        # (a length that is negative as int64 is beyond every stream: the call finds it whatever this sum comes to)
        total = int(lengths.view(torch.int64).sum()) if n else 0
        if total < 0 or total > n * self.size:
            total = 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        starts = torch.zeros(n + 1, dtype=torch.int64, device=dev) if return_starts else None
        st = torch.cuda.current_stream(dev).cuda_stream
        got = self.reader.read_device(offsets.data_ptr() if n else None, lengths.data_ptr() if n else None, n, out.data_ptr(), total,
                                      d_starts=starts.data_ptr() if return_starts and n else None, ignore_crc=ignore_crc, stream=st)
        return (out[:got], starts) if return_starts else out[:got]

    def search(self, pattern, max_results, ignore_crc=False, no_tables=False):
        """Where `pattern` (1 .. 256 bytes) occurs in the decoded stream -> (the smallest min(total, max_results) positions, ascending: an
        int64 tensor on the stream's device; the total).  Only the blocks whose search tables (types 1 to 4) admit the pattern are decoded."""
        dev = self.t.device
        out = torch.empty(max(max_results, 1), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        total, _ = self.reader.search(pattern, out.data_ptr() if max_results else None, max_results, ignore_crc=ignore_crc, no_tables=no_tables, stream=st)
        return out[:min(total, max_results)], total

    def search_many(self, patterns, max_results, ignore_crc=False, no_tables=False):
        """Where each of `patterns` (a sequence of up to 4096 bytes objects of 1 .. 256 bytes) occurs in the decoded stream, in one pass over
        the blocks that any pattern's search tables admit -> (positions int64, which int32, counts int64, total): the smallest
        min(total, max_results) pairs (position, pattern index) in ascending order, every pattern's own number of occurrences and the
        number of all pairs; tensors on the stream's device."""
        dev = self.t.device
        pats = list(patterns)
        pos = torch.empty(max(max_results, 1), dtype=torch.int64, device=dev)
        which = torch.empty(max(max_results, 1), dtype=torch.int32, device=dev)
        counts = torch.zeros(max(len(pats), 1), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        total, _ = self.reader.search_many(pats, counts.data_ptr(), pos.data_ptr() if max_results else None, which.data_ptr() if max_results else None, max_results,
                                           ignore_crc=ignore_crc, no_tables=no_tables, stream=st)
        k = min(total, max_results)
        return pos[:k], which[:k], counts[:len(pats)], total

    def search_records(self, pattern, delimiter=b"\n", max_records=1024, max_bytes=1 << 20, max_reach=0, ignore_crc=False, no_tables=False):
        """The records (lines, for the default delimiter) of the decoded stream that hold `pattern`, each once, in stream order ->
        (total_records, data, rec_off, rec_start, flags, totals): the first k records' bytes back to back (uint8), where each starts in the
        decoded stream (int64, k values) and in `data` (int64, k + 1 values: the last is data's size), its flags (uint8: 1 = cut left,
        2 = cut right — records longer than max_reach, 0 = 65536) — tensors on the stream's device, trimmed to what was written: k is
        the most records that max_records and max_bytes hold whole — and totals = (records, bytes of all records, occurrences, flagged
        records).  max_records = max_bytes = 0 counts."""
        dev = self.t.device
        data = torch.empty(max(max_bytes, 1), dtype=torch.uint8, device=dev)
        rec_off = torch.empty(max(max_records, 1), dtype=torch.int64, device=dev)
        rec_start = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
        flags = torch.empty(max(max_records, 1), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        total, totals, _ = self.reader.search_records(pattern, delimiter, data.data_ptr() if max_bytes else None, max_bytes, rec_off.data_ptr() if max_records else None,
                                                      rec_start.data_ptr(), flags.data_ptr() if max_records else None, max_records, max_reach=max_reach,
                                                      ignore_crc=ignore_crc, no_tables=no_tables, stream=st)
        k = int((rec_start[1:] != 0).sum())   # (no record is empty: the starts behind the first are positive as far as they were written)
        return total, data[:int(rec_start[k])], rec_off[:k], rec_start[:k + 1], flags[:k], totals

    def index_records(self, delimiter=b"\n", ignore_crc=False):
        """Builds the record index of the decoded stream for the one-byte `delimiter` (one decode of the stream; 8 bytes per delimiter
        stay on the device until close() or another delimiter) -> the number of records N.  read_records, line_numbers and
        read_record_range need it."""
        st = torch.cuda.current_stream(self.t.device).cuda_stream
        return self.reader.index_records(delimiter, ignore_crc=ignore_crc, stream=st)[0]

    def _items(self, a, what):
        if not torch.is_tensor(a) or a.dtype not in (torch.int64, torch.uint64) or a.dim() != 1 or not a.is_contiguous() or a.device != self.t.device:
            raise ValueError(what + ": a contiguous 1-d int64 or uint64 tensor on the stream's device")
        return a

    def read_records(self, idx, ignore_crc=False):
        """The records with the numbers `idx` (int64 or uint64 tensor on the stream's device; any order, repeats allowed), back to back in
        the order given -> (a new uint8 tensor, the n + 1 places where the records start in it and its size: int64).  The one thing that
        visits the host is the records' total size, which sizes the output."""
        idx = self._items(idx, "read_records")
        dev, n = self.t.device, idx.numel()
        starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n == 0:
            self.reader.record_count()   # (without an index this raises, as every call on it does)
            return torch.empty(0, dtype=torch.uint8, device=dev), starts
        st = torch.cuda.current_stream(dev).cuda_stream
        spans = torch.empty(2 * n, dtype=torch.int64, device=dev)
        total = self.reader.record_spans(idx.data_ptr(), n, spans.data_ptr(), spans[n:].data_ptr(), stream=st)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        got = self.reader.read_records(idx.data_ptr(), n, out.data_ptr(), total, d_starts=starts.data_ptr(), ignore_crc=ignore_crc, stream=st)
        return out[:got], starts

    def line_numbers(self, positions):
        """The record number (0-based) of every position of the decoded stream in `positions` (int64 or uint64 tensor on the stream's
        device) -> an int64 tensor; -1 for a position at or beyond the size.  With search_records' rec_off: the line numbers of the
        matching lines."""
        positions = self._items(positions, "line_numbers")
        n = positions.numel()
        out = torch.empty(n, dtype=torch.int64, device=self.t.device)
        st = torch.cuda.current_stream(self.t.device).cuda_stream
        if n == 0:
            self.reader.record_count()
        else:
            self.reader.record_numbers(positions.data_ptr(), n, out.data_ptr(), stream=st)
        return out

    def grep(self, patterns, invert=False, before=0, after=0, max_records=1 << 20, count_only=False, ignore_crc=False, no_tables=False):
        """grep over the decoded stream's lines: the records that hold one of `patterns` (a sequence of up to 4096 bytes objects of
        1 .. 256 bytes without the delimiter; a single bytes object is one pattern), with invert those that hold none, and `before` /
        `after` context records around each, every record once, in stream order.  Builds the record index for b"\n" when the stream has
        none (index_records chooses another delimiter).
        -> (R, numbers, kinds, data, starts): the number of such records; the smallest min(R, max_records) record numbers (int64); 1 for a
        selected record and 0 for one that is context only (uint8); those records' bytes back to back (uint8) and the k + 1 places where
        they start in it and its size (int64) — tensors on the stream's device.
        count_only (grep -c): -> (R, the selected records) and nothing is written or read."""
        from . import api
        dev = self.t.device
        pats = [patterns] if isinstance(patterns, (bytes, bytearray)) else list(patterns)
        st = torch.cuda.current_stream(dev).cuda_stream
        try:
            self.reader.record_count()
        except api.MinLZError:   # (no index yet)
            self.reader.index_records(b"\n", ignore_crc=ignore_crc, stream=st)
        kw = dict(invert=invert, before=before, after=after, ignore_crc=ignore_crc, no_tables=no_tables, stream=st)
        if count_only:
            _, totals, _ = self.reader.grep_records(pats, None, None, 0, **kw)
            return totals[0], totals[1]
        cap = min(max_records, self.reader.record_count())
        numbers = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        kinds = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        R, totals, _ = self.reader.grep_records(pats, numbers.data_ptr() if cap else None, kinds.data_ptr() if cap else None, cap, **kw)
        k = min(R, cap)
        starts = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        data = torch.empty(max(totals[2], 1), dtype=torch.uint8, device=dev)
        got = self.reader.read_records(numbers.data_ptr(), k, data.data_ptr(), totals[2], d_starts=starts.data_ptr(), ignore_crc=ignore_crc, stream=st) if k else 0
        return R, numbers[:k], kinds[:k], data[:got], starts

    def read_record_range(self, first, count, ignore_crc=False):
        """Records first .. first + count - 1 as they lie in the decoded stream, the delimiters between them included -> a new uint8 tensor."""
        off, ln = self.reader.record_range(first, count)
        return self.read_ranges([off], [ln], ignore_crc)

    def build_sidecar(self, cfgs, ignore_crc=False):
        """A sidecar search index of this stream for 1 .. 4 configurations (api.search_config): search tables for every block, whoever
        wrote the stream, in a separate .mz stream -> a new uint8 tensor on the stream's device."""
        dev = self.t.device
        cap = self.reader.sidecar_bound(cfgs)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        got = self.reader.build_sidecar(cfgs, out.data_ptr(), cap, ignore_crc=ignore_crc, stream=st)
        return out[:got].clone()

    def attach_sidecar(self, side, ignore_crc=False):
        """search and search_many use the tables of the sidecar `side` (a uint8 tensor on the stream's device, as build_sidecar returns
        it) from now on; None detaches.  The stream keeps the tensor alive."""
        if side is None:
            self.reader.detach_sidecar()
            self.side = None
            return
        if side.dtype != torch.uint8 or side.dim() != 1 or not side.is_contiguous() or side.device != self.t.device:
            raise ValueError("attach_sidecar: a contiguous 1-d uint8 tensor on the stream's device")
        st = torch.cuda.current_stream(self.t.device).cuda_stream
        self.reader.attach_sidecar(side.data_ptr(), side.numel(), ignore_crc=ignore_crc, stream=st)
        self.side = side

    def ReadAt(self, n, offset, ignore_crc=False):
        """Up to n decoded bytes from `offset`, clamped at the end of the stream -> a new uint8 tensor."""
        if n < 0 or offset < 0 or offset > self.size:
            raise ValueError("ReadAt: offset outside the stream")
        return self.read_ranges([offset], [min(n, self.size - offset)], ignore_crc)

    def close(self):
        self.reader.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frame_run(codec, src, block_lens, level):
    """Encode this rank's blocks and frame them into one contiguous run of stream chunks on the device.
    -> (run: uint8 tensor on src's device, chunk_sizes: list of ints).  Per block `[type][len24][crc32c][body]`,
    type 0x02 + `uvarint(N) tokens` or 0x01 + raw bytes when the block was stored (writer.go:876-910)."""
    enc, stride, lens, crcs = codec.encode(src, block_lens, level)
    lens_h, crcs_h = lens.cpu().tolist(), crcs.cpu().tolist()     # the one host round trip: sizes decide the layout
    sizes, plan, o_src = [], [], 0
    for i, bl in enumerate(block_lens):
        stored = lens_h[i] == bl + 2 or bl == 0
        body = bl if stored else lens_h[i] - 1                      # tokens: the block minus its leading 0x00
        clen = 4 + body
        hdr = bytes([S.CHUNK_UNCOMPRESSED if stored else S.CHUNK_MINLZ, clen & 0xFF, (clen >> 8) & 0xFF, (clen >> 16) & 0xFF]) + int(crcs_h[i]).to_bytes(4, "little")
        plan.append((hdr, stored, body, i, o_src))
        sizes.append(8 + body)
        o_src += bl
    if not plan:
        return torch.empty(0, dtype=torch.uint8, device=src.device), sizes
    # all chunk headers in ONE blocking upload (a pageable temporary must not be handed to an asynchronous copy), and the run
    # assembled by ONE concatenation of views [hdr_0, body_0, hdr_1, body_1, ...] instead of two slice copies per block
    hdrs = torch.frombuffer(bytearray(b"".join(p[0] for p in plan)), dtype=torch.uint8).to(src.device)
    parts = []
    for k, (hdr, stored, body, i, os_) in enumerate(plan):
        parts.append(hdrs[8 * k:8 * k + 8])
        if body:
            parts.append(src[os_:os_ + body] if stored else enc[i * stride + 1:i * stride + 1 + body])
    return torch.cat(parts), sizes


# ---- collectives ----
# RCCL ("nccl") moves device tensors directly.  gloo moves host tensors only: with gloo, device tensors are staged through
# the host on either side of the transfer (that is what a 1-GPU box can run: two ranks, two contexts on one device, gloo).

def _host_staged(t):
    return t.is_cuda and dist.get_backend() == "gloo"


def gather_chunk_sizes(sizes, n_blocks, rank, world, device):
    """all_gather of the per-block chunk sizes of every rank's range -> list of n_blocks ints in stream order."""
    # world == 1 is a LOCAL call unless the process group has exactly one rank too: a rank that encodes a stream of its own inside a
    # larger job (bench.py's config-3 leg on rank 0) must not enter a collective the other ranks never join.  (A one-rank process group
    # still goes through the collective: MINLZ_BENCH_FORCE_DIST runs RCCL's all_gather that way on a 1-GPU box.)
    if world == 1 and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() == 1):
        return list(sizes)
    cdev = "cpu" if dist.get_backend() == "gloo" else device
    per = (n_blocks + world - 1) // world
    t = torch.zeros(max(per, 1), dtype=torch.int64, device=cdev)
    if sizes:
        t[:len(sizes)] = torch.tensor(sizes, dtype=torch.int64, device=cdev)
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    host = torch.stack(parts).cpu().tolist()
    out = []
    for r in range(world):
        b0, b1 = range_of(r, world, n_blocks)
        out += host[r][:b1 - b0]
    return out


class _Transfers:
    """Handles of posted isend / irecv operations plus what has to happen once they are done (host-staged receives are
    copied to their place on the device)."""

    def __init__(self):
        self.ops, self.works, self.after, self.keep = [], [], [], []

    def send(self, t, dst):
        if t.numel() == 0:
            return
        h = t.cpu() if _host_staged(t) else t
        self.keep.append(h)
        self.ops.append(dist.P2POp(dist.isend, h, dst))

    def recv(self, t, src):
        if t.numel() == 0:
            return
        if _host_staged(t):
            h = torch.empty(t.shape, dtype=t.dtype)
            self.after.append((t, h))
            self.ops.append(dist.P2POp(dist.irecv, h, src))
        else:
            self.ops.append(dist.P2POp(dist.irecv, t, src))

    def post(self):
        self.works = dist.batch_isend_irecv(self.ops) if self.ops else []
        return self

    def wait(self):
        for w in self.works:
            w.wait()
        for t, h in self.after:
            t.copy_(h)
        self.works, self.after, self.keep = [], [], []


def start_gather(run, all_sizes, n_blocks, rank, world, root, head=0):
    """Posts the payload gather: root receives rank r's run at its final offset in the stream buffer (allocated here with
    `head` bytes in front for the stream header), the others send theirs.  Returns (stream buffer or None, transfers,
    payload bytes of the whole stream); finish_gather(transfers) before the buffer is read."""
    totals = []
    for r in range(world):
        b0, b1 = range_of(r, world, n_blocks)
        totals.append(sum(all_sizes[b0:b1]))
    payload = sum(totals)
    tr, out = _Transfers(), None
    if rank == root:
        out = torch.empty(head + payload + 16, dtype=torch.uint8, device=run.device)
        o = head
        for r in range(world):
            if r == root:
                out[o:o + totals[r]] = run[:totals[r]]
            else:
                tr.recv(out[o:o + totals[r]], r)
            o += totals[r]
    else:
        tr.send(run[:totals[rank]], root)
    return out, tr.post(), payload


def finish_gather(transfers):
    transfers.wait()


def encode_stream_sharded_device(codec, src, total_len, block_size, level, rank, world, root=0):
    """`src`: this rank's contiguous range of the stream (uint8 tensor on its device; range_of() in whole blocks).
    Returns the framed stream as a uint8 tensor on root's device (None elsewhere)."""
    n_blocks = (total_len + block_size - 1) // block_size
    b0, b1 = range_of(rank, world, n_blocks)
    block_lens = [min(block_size, total_len - i * block_size) for i in range(b0, b1)]
    assert int(src.numel()) == sum(block_lens), (int(src.numel()), sum(block_lens))
    run, sizes = frame_run(codec, src, block_lens, level)
    all_sizes = gather_chunk_sizes(sizes, n_blocks, rank, world, src.device)
    head = 10 if n_blocks else 0
    out, tr, payload = start_gather(run, all_sizes, n_blocks, rank, world, root, head)
    finish_gather(tr)
    if rank != root:
        return None
    if n_blocks:
        out[:10] = torch.frombuffer(bytearray(S.MAGIC + bytes([(block_size - 1).bit_length() - 10])), dtype=torch.uint8).to(out.device)
    v = S.put_uvarint(total_len)
    tail = bytes([S.CHUNK_EOF, len(v), 0, 0]) + v
    out[head + payload:head + payload + len(tail)] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).to(out.device)
    return out[:head + payload + len(tail)]


# =====================================================================================================================
# Reader side: ONE stream decoded by all ranks (reader.go:575-992, DecodeConcurrent)
# =====================================================================================================================
#
# The reference's concurrent Reader walks the chunk headers on one goroutine, hands every block to a worker and writes the
# results in order.  Here the walk is S.walk_chunks (host, a few bytes per chunk); the blocks it finds are dealt to the ranks
# in contiguous ranges, every rank uploads only ITS span of the stream, decodes its blocks with one device batch call and
# checks their CRCs on the device.  What the walk tells every rank — the decoded size of every block, `uvarint(N)` at the
# head of each 0x02 chunk — fixes the layout of the output, so there is NO size exchange on this side:
#   all_reduce(MAX) of one status word        -> every rank reports the same error (first failing block wins by code)
#   (gather=True) isend / irecv of N-sized    -> root receives every rank's decoded range at its final offset; the default
#                 decoded ranges                 leaves the output sharded, which is what SURVEY.md 8(e) recommends
# Input: the stream as host bytes on every rank (a file or object all ranks can read), or on the root only (scatter=True:
# the block table is broadcast and each rank's span of the stream is sent to it).

def plan_decode(blocks, rank, world):
    """blocks: S.walk_chunks(...) entries in stream order -> (b0, b1, span_lo, span_hi, u_lo, u_hi): this rank's block range,
    the byte span of the stream that holds its chunks, and the range of the decoded stream it produces."""
    b0, b1 = range_of(rank, world, len(blocks))
    if b0 == b1:   # an empty range (more ranks than blocks) sits where its predecessors end: the ranks' ranges stay in order and cover the stream
        if b0 == 0:
            return b0, b1, 0, 0, 0, 0
        pv = blocks[b0 - 1]
        return b0, b1, pv.payload_off + pv.payload_len, pv.payload_off + pv.payload_len, pv.u_off + pv.n, pv.u_off + pv.n
    lo = blocks[b0].chunk_off
    hi = blocks[b1 - 1].payload_off + blocks[b1 - 1].payload_len
    return b0, b1, lo, hi, blocks[b0].u_off, blocks[b1 - 1].u_off + blocks[b1 - 1].n


def decode_span_device(codec, span, blocks, span_lo, u_lo, device, ignore_crc=False, owned=False):
    """Decodes the blocks whose chunks lie in `span` (the stream bytes [span_lo, ...): host bytes / numpy, or a uint8 tensor;
    one already on `device` is copied first unless owned=True says this call may modify it) on `device`.
    -> (decoded uint8 tensor of this range, status: 0 or an MLZ_ERR_* code)."""
    from . import api
    n_out = sum(b.n for b in blocks)
    out = torch.empty(max(n_out, 1), dtype=torch.uint8, device=device)
    if not blocks:
        return out[:0], 0
    if isinstance(span, torch.Tensor):
        # (a pinned host tensor uploads at link speed; a tensor already on the target device type is CLONED unless the caller says
        #  the buffer is this call's to modify — the CRC bytes are zeroed in place below, and a view of the caller's stream would be damaged)
        enc = span.to(device) if span.device.type != torch.device(device).type else (span if owned else span.clone())
    else:
        enc = torch.from_numpy(np.array(span, dtype=np.uint8, copy=True)).to(device)
    # The decode call wants whole blocks: `00 uvarint(N) tokens` (0x02 / 0x03 chunks: the chunk body behind one zero byte) or
    # `00 00 raw` (0x01 chunks).  The bytes in front of a chunk's payload are its CRC, which the walk has already read: they
    # are overwritten with zeros in the DEVICE copy (one index_fill), so every block is decoded in place, no repacking.
    descs, zero_at, crc_out, crc_in, want_out, want_in = [], [], [], [], [], []
    for b in blocks:
        p = b.payload_off - span_lo
        if b.kind == S.CHUNK_UNCOMPRESSED:
            zero_at += [p - 2, p - 1]
            descs.append((p - 2, b.payload_len + 2, b.u_off - u_lo, b.n))
        else:
            zero_at.append(p - 1)
            descs.append((p - 1, b.payload_len + 1, b.u_off - u_lo, b.n))
        if b.kind == S.CHUNK_MINLZ_COMPCRC:       # CRC over the token bytes (reader.go:341-344)
            crc_in.append((p + b.hdr_len, b.payload_len - b.hdr_len)); want_in.append(b.crc)
        else:
            crc_out.append((b.u_off - u_lo, b.n)); want_out.append(b.crc)
    enc.index_fill_(0, torch.tensor(zero_at, dtype=torch.int64).to(enc.device), 0)
    lens = codec.decode(enc, descs, out)
    ok = lens == torch.tensor([b.n for b in blocks], dtype=torch.int64).to(lens.device)
    if not ignore_crc:
        # (both CRC sets are queued behind the decode before the single host read-back below)
        for base, spans, want in ((out, crc_out, want_out), (enc, crc_in, want_in)):
            if spans:
                ok = torch.cat([ok, codec.crcs(base, spans) == torch.tensor(want, dtype=torch.int64).to(lens.device)])
    status = 0
    if not bool(ok.all()):
        okh, lh = ok.cpu().tolist(), lens.cpu().tolist()
        badlen = [l for l, o in zip(lh, okh[:len(lh)]) if not o]
        status = (-badlen[0] if badlen[0] < 0 else api.ErrCorrupt.code) if badlen else api.ErrCRC.code
    return out[:n_out], status


def decode_stream_sharded_device(codec, stream, rank, world, device, root=0, gather=False, scatter=False, ignore_crc=False):
    """One .mz stream decoded by all ranks.  `stream`: bytes-like, on every rank (or on `root` only with scatter=True).
    Returns (local, (u_lo, u_hi), total): this rank's decoded range as a uint8 tensor on `device` and where it sits in the
    decoded stream of `total` bytes; with gather=True the root's `local` is the WHOLE decoded stream (range (0, total)).
    Raises the reference's errors (ErrCorrupt, ErrCRC, ...) on every rank when any rank's blocks fail."""
    from . import api
    blocks = total = None
    err = 0
    if not scatter or rank == root:
        try:
            blocks, total = S.walk_chunks(stream.numpy() if isinstance(stream, torch.Tensor) else stream)
        except api.MinLZError as e:
            err = e.code
            blocks, total = [], 0
    if scatter and world > 1:
        box = [(blocks, total, err)]
        dist.broadcast_object_list(box, src=root)
        blocks, total, err = box[0]
    if err:
        api._raise(-err)
    b0, b1, lo, hi, u_lo, u_hi = plan_decode(blocks, rank, world)
    if scatter and world > 1:
        # each rank's span of the stream travels from the root's host memory to that rank (sizes are known from the table)
        # (RCCL moves device memory: the root uploads the other ranks' spans and sends them from its HBM; gloo sends host tensors)
        tr = _Transfers()
        cdev = "cpu" if dist.get_backend() == "gloo" else device
        if rank == root:
            sv = stream.numpy() if isinstance(stream, torch.Tensor) else np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream
            for r in range(world):
                if r != root:
                    _, _, rlo, rhi, _, _ = plan_decode(blocks, r, world)
                    tr.send(torch.from_numpy(np.array(sv[rlo:rhi], copy=True)).to(cdev), r)
            span = sv[lo:hi]
        else:
            buf = torch.empty(hi - lo, dtype=torch.uint8, device=cdev)
            tr.recv(buf, root)
        tr.post().wait()
        if rank != root:
            span = buf
    elif isinstance(stream, torch.Tensor):
        span = stream[lo:hi]          # a CPU tensor (pinned: the upload runs at link speed)
    else:
        sv = np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream
        span = sv[lo:hi]
    # A rank whose decode raises (a HIP failure surfaced by the codec) must still reach the all_reduce below, or the others hang:
    # the exception becomes this rank's status word and is re-raised — as the same error on every rank — behind the exchange.
    try:
        local, status = decode_span_device(codec, span, blocks[b0:b1], lo, u_lo, device, ignore_crc,
                                           owned=scatter and world > 1 and rank != root)
    except api.MinLZError as e:
        local, status = torch.empty(0, dtype=torch.uint8, device=device), (e.code or api.ErrHIP.code)
    except RuntimeError:
        local, status = torch.empty(0, dtype=torch.uint8, device=device), api.ErrHIP.code
    if world > 1:
        st = torch.tensor([status], dtype=torch.int64, device="cpu" if dist.get_backend() == "gloo" else device)
        dist.all_reduce(st, op=dist.ReduceOp.MAX)
        status = int(st.item())
    if status:
        api._raise(-status)
    if gather and world > 1:
        tr = _Transfers()
        if rank == root:
            whole = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
            for r in range(world):
                _, _, _, _, rlo, rhi = plan_decode(blocks, r, world)
                if r == root:
                    whole[rlo:rhi] = local
                else:
                    tr.recv(whole[rlo:rhi], r)
            tr.post().wait()
            return whole[:total], (0, total), total
        tr.send(local, root)
        tr.post().wait()
    return local, (u_lo, u_hi), total
