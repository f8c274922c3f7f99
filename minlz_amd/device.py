"""The tensor layer over the C ABI: CUDA tensors through the device-resident calls of api.Context and api.DeviceReader.

HipTensorCodec is the block and stream codec on tensors (the product path, what bench.py times); DeviceStream is a .mz stream in HBM
opened for range reads, searches and record reads, DeviceStreamSet many of them opened as one.  Every call runs on the current stream of
the tensor's device.
"""
import numpy as np
import torch

from . import api
from ._lib import BlockDesc


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _u8(t, what, dev=None):
    """A uint8 tensor on the device, made contiguous; with `dev`: one that is contiguous, 1-d and on that device already."""
    if dev is not None:
        if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
            raise ValueError(what + ": a contiguous 1-d uint8 tensor on the stream's device")
        return t
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError(what + ": a uint8 tensor on the device")
    return t.contiguous()


def _items(a, dev, what, message=": a contiguous 1-d int64 or uint64 tensor on the stream's device"):
    if not torch.is_tensor(a) or a.dtype not in (torch.int64, torch.uint64) or a.dim() != 1 or not a.is_contiguous() or a.device != dev:
        raise ValueError(what + message)
    return a


def _room(n, dtype, dev, fill=torch.empty):
    """Room for n items, at least one -> (the tensor, its address or None when n is 0: what the ABI takes with a capacity of 0)."""
    t = fill(max(n, 1), dtype=dtype, device=dev)
    return t, (t.data_ptr() if n else None)


def _spans(t, spans, what):
    spans = [(int(o), int(n)) for o, n in spans]
    for o, n in spans:
        if o < 0 or n < 0 or o + n > t.numel():
            raise ValueError(what + ": a span leaves the tensor")
    return spans


class HipTensorCodec:
    """CUDA tensors through the C ABI's device-resident batch calls (the product path)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def encode(self, src, block_lens, level):
        n = len(block_lens)
        stride = (max(block_lens + [0]) + 2 + 255) & ~255
        dev = src.device
        enc = torch.empty(max(n * stride, 1), dtype=torch.uint8, device=dev)
        lens = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        crc32 = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        if n:
            offs = np.concatenate([[0], np.cumsum(block_lens)[:-1]]).tolist()
            desc = (BlockDesc * n)(*[BlockDesc(int(offs[i]), int(block_lens[i]), i * stride, stride) for i in range(n)])
            st = _stream(dev)
            self.ctx.encode_batch_device(st, level, src.data_ptr(), enc.data_ptr(), desc, lens.data_ptr())
            self.ctx.crc_batch_device(st, src.data_ptr(), desc, crc32.data_ptr())
        return enc, stride, lens[:n], (crc32[:n].to(torch.int64) & 0xFFFFFFFF)

    def decode(self, enc, blocks, out):
        """blocks: [(src_off, src_len, dst_off, dst_len)] — whole blocks `00 uvarint(N) tokens` / `00 00 raw` inside `enc`, decoded
        to out[dst_off : dst_off + dst_len].  -> int64 tensor on the device: the decoded length of each block or -MLZ_ERR_*."""
        n = len(blocks)
        lens = torch.zeros(max(n, 1), dtype=torch.int64, device=enc.device)
        if n:
            desc = (BlockDesc * n)(*[BlockDesc(int(a), int(b), int(c), int(d)) for a, b, c, d in blocks])
            self.ctx.decode_batch_device(_stream(enc.device), enc.data_ptr(), out.data_ptr(), desc, lens.data_ptr())
        return lens[:n]

    def crcs(self, base, spans):
        """Masked CRC32C (minlz.go:133-140) of base[off : off + len] for each (off, len) -> int64 tensor on the device."""
        n = len(spans)
        crc32 = torch.zeros(max(n, 1), dtype=torch.int32, device=base.device)
        if n:
            desc = (BlockDesc * n)(*[BlockDesc(int(o), int(l), 0, 0) for o, l in spans])
            self.ctx.crc_batch_device(_stream(base.device), base.data_ptr(), desc, crc32.data_ptr())
        return crc32[:n].to(torch.int64) & 0xFFFFFFFF

    def decode_stream(self, t, ignore_crc=False):
        """A whole .mz stream that lies on the device (uint8 tensor) -> its decoded bytes, a new uint8 tensor on the same device.  The chunks
        are found on the device (mlz_stream_decoded_len_device sizes the output) and decoded where they lie (mlz_stream_decode_device): no
        payload visits the host.  Raises the Reader's first error in stream order, like api.stream_decode."""
        t = _u8(t, "decode_stream")
        st = _stream(t.device)
        n, prefix = self.ctx.stream_decoded_len_device(t.data_ptr(), t.numel(), stream=st)
        cap = n if n >= 0 else prefix   # a framing error: the chunks in front of it are decoded and checked first
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=t.device)
        r = self.ctx.stream_decode_device(t.data_ptr(), t.numel(), out.data_ptr(), cap, ignore_crc=ignore_crc, stream=st)
        return out[:r]

    @staticmethod
    def _raise_stream(what, i, code):
        """The error of stream i of a batch: the class of its code, the index in the message and in .index."""
        e = api._error(-code, "%s: stream %d of the batch: " % (what, i))
        e.code, e.index = -code, i
        raise e

    def decode_streams(self, t, spans, ignore_crc=False):
        """Many .mz streams that lie in one uint8 tensor on the device, stream i at t[off_i : off_i + len_i] for spans[i] = (off_i, len_i) ->
        (out, starts): their decoded bytes packed into one new uint8 tensor on the same device, and the n + 1 places where they start in it
        (a list of ints; the last is out's size).  One batch walk sizes the output (mlz_stream_decoded_len_batch_device), one batch call
        decodes (mlz_stream_decode_batch_device).  Raises the first failing stream's error, which names its index (.index)."""
        t = _u8(t, "decode_streams")
        spans = _spans(t, spans, "decode_streams")
        if not spans:
            return torch.empty(0, dtype=torch.uint8, device=t.device), [0]
        st = _stream(t.device)
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

    def encode_streams(self, t, spans, level, block_size=1 << 20, add_index=False, search_match_len=None, search_prefix=None, search_long_prefix=None, search_extras=0):
        """Every input t[off_i : off_i + len_i] (a uint8 tensor on the device, spans[i] = (off_i, len_i)) as a .mz stream of its own ->
        (out, stream_spans): one new uint8 tensor on the same device and where each stream lies in it, [(off, len)] (with room between
        them: every stream is written at the place its bound reserves).  One call (mlz_stream_encode_batch_device); the bytes are
        api.stream_encode's.  With the search_* keywords (those of Context.stream_encode_gather_device) every stream carries block search
        tables of that configuration, which search_streams(prune=True) reads; the bytes are then the gather Writer's for that input alone.
        Raises the first failing stream's error, which names its index (.index)."""
        t = _u8(t, "encode_streams")
        tables = dict(search_match_len=search_match_len, search_prefix=search_prefix, search_long_prefix=search_long_prefix, search_extras=search_extras)
        descs, at = [], 0
        for o, n in _spans(t, spans, "encode_streams"):
            try:
                cap = api.stream_bound(n, block_size, add_index, **tables)
            except api.MinLZError:
                raise ValueError("encode_streams: block size %d" % block_size)
            descs.append((o, n, at, cap))
            at += cap
        out = torch.empty(max(at, 1), dtype=torch.uint8, device=t.device)
        if not descs:
            return out[:0], []
        res = self.ctx.stream_encode_batch_device(level, block_size, add_index, t.data_ptr(), out.data_ptr(), descs, stream=_stream(t.device), **tables)
        for i, r in enumerate(res):
            if r < 0:
                self._raise_stream("encode_streams", i, r)
        return out, [(d[2], r) for d, r in zip(descs, res)]

    def search_streams(self, t, spans, patterns, max_results=0, present=True, ignore_crc=False, ignore_case=False, on_error="raise", prune=False):
        """Which of many .mz streams that lie in one uint8 tensor on the device (stream i at t[off_i : off_i + len_i] for spans[i]) hold which
        of `patterns` (1 .. 4096 bytes objects of 1 .. 256 bytes), and where, in one call (mlz_stream_search_batch_device) ->
        (counts, present, hit_stream, hit_pos, hit_which, pattern_counts, total), tensors on t's device: every stream's occurrences (int64, n
        values); present[i, p] = pattern p occurs in stream i (bool, n x patterns; None with present=False), exact whatever max_results is;
        the smallest min(total, max_results) triples in (stream, position inside the stream's decoded bytes, pattern) order (int32, int64,
        int32); every pattern's occurrences (int64); the number of all triples.
        on_error "raise": the first failing stream's error, which names its index (.index), as decode_streams; "keep": that stream's
        negative code in counts, its row of present False, and the other streams' results as without it.
        prune: decode only the chunks that the streams' inline block search tables cannot rule out (mlz_stream_search_batch_device_pruned);
        the same results for streams whose tables are truthful."""
        if on_error not in ("raise", "keep"):
            raise ValueError("search_streams: on_error is \"raise\" or \"keep\"")
        t = _u8(t, "search_streams")
        dev = t.device
        spans, pats = _spans(t, spans, "search_streams"), list(patterns)
        n, words = len(spans), (len(pats) + 31) // 32
        pos, d_pos = _room(max_results, torch.int64, dev)
        hs, d_hs = _room(max_results, torch.int32, dev)
        which, d_which = _room(max_results, torch.int32, dev)
        pc, _ = _room(len(pats), torch.int64, dev, torch.zeros)
        bits, d_bits = _room(n * words if present else 0, torch.int32, dev, torch.zeros)
        total, res, _ = self.ctx.stream_search_batch_device(t.data_ptr(), spans, pats, None, pc.data_ptr(), d_bits, d_hs, d_pos, d_which, max_results, ignore_crc=ignore_crc,
                                                            ignore_case=ignore_case, stream=_stream(dev), prune=prune)
        for i, r in enumerate(res):
            if r < 0 and on_error == "raise":
                self._raise_stream("search_streams", i, r)
        counts = torch.tensor(res, dtype=torch.int64).to(dev)
        k = min(total, max_results)
        p = None
        if present:
            shifts = torch.arange(32, dtype=torch.int32, device=dev)
            p = ((bits[:n * words].view(n, words, 1) >> shifts) & 1).view(n, words * 32)[:, :len(pats)].bool()
        return counts, p, hs[:k], pos[:k], which[:k], pc[:len(pats)], total

    def build_record_index(self, data, delimiter=b"\n"):
        """The record index blob (include/minlz_hip_record_index_store.h) of the raw bytes `data` (uint8 tensor on the device) for the one-byte
        `delimiter`, made without a stream: what DeviceStream.load_record_index takes for the stream these bytes are encoded into -> a new
        uint8 tensor on data's device."""
        data = _u8(data, "build_record_index")
        cap = api.record_index_bound(data.numel())
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
        got, _ = self.ctx.record_index_build_device(data.data_ptr() if data.numel() else None, data.numel(), delimiter, out.data_ptr(), cap, stream=_stream(data.device))
        return out[:got].clone()

    def open_stream(self, t):
        """A .mz stream that lies on the device (uint8 tensor) opened for range reads -> DeviceStream (ReadAt, read_ranges).  The chunk walk
        runs once, here; a framing error raises."""
        return DeviceStream(self.ctx, _u8(t, "open_stream"))

    def open_streams(self, t, spans, on_error="raise", tables=False):
        """Many .mz streams that lie in one uint8 tensor on the device (stream i at t[off_i : off_i + len_i] for spans[i]) opened as ONE
        DeviceStreamSet: a DeviceStream over their decoded bytes one behind the other, in the order of the spans (one call,
        mlz_stream_open_batch_device).  on_error "raise": the first stream with a framing error raises its error, which names its index
        (.index); "skip": such a stream is left out (size 0), and .errors names it.  tables: the set's searches and greps prune by every
        stream's inline search tables (mlz_stream_open_batch_device_tables), with the same results."""
        if on_error not in ("raise", "skip"):
            raise ValueError("open_streams: on_error is \"raise\" or \"skip\"")
        t = _u8(t, "open_streams")
        s = DeviceStreamSet(self.ctx, t, _spans(t, spans, "open_streams"), tables=tables)
        if on_error == "raise" and s.errors:
            i = min(s.errors)
            s.close()
            self._raise_stream("open_streams", i, s.errors[i])
        return s


class DeviceStream:
    """A .mz stream on the device opened for random access (HipTensorCodec.open_stream): ReadSeeker.ReadAt (reader.go:1401-1487) with the
    device walk's chunk table in the place of the seek index.  Keeps the stream's tensor alive."""

    def __init__(self, ctx, t):
        self.t, self.dev = t, t.device
        self.reader = ctx.stream_open_device(t.data_ptr(), t.numel(), stream=_stream(t.device))
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
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        got = self.reader.read(r, out.data_ptr(), total, ignore_crc=ignore_crc, stream=_stream(self.dev))
        if return_starts:
            return out[:got], torch.from_numpy(np.concatenate([r[:, 2], [total]]).astype(np.int64)).to(self.dev)
        return out[:got]

    def _read_ranges_device(self, offsets, lengths, ignore_crc, return_starts):
        for a in (offsets, lengths):
            _items(a, self.dev, "read_ranges", ": device ranges are contiguous 1-d int64 or uint64 tensors on the stream's device")
        n = offsets.numel()
        if lengths.numel() != n:
            raise ValueError("read_ranges: as many lengths as offsets")
        # (a length that is negative as int64 is beyond every stream: the call finds it whatever this sum comes to)
        total = int(lengths.view(torch.int64).sum()) if n else 0
        if total < 0 or total > n * self.size:
            total = 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        starts = torch.zeros(n + 1, dtype=torch.int64, device=self.dev) if return_starts else None
        got = self.reader.read_device(offsets.data_ptr() if n else None, lengths.data_ptr() if n else None, n, out.data_ptr(), total,
                                      d_starts=starts.data_ptr() if return_starts and n else None, ignore_crc=ignore_crc, stream=_stream(self.dev))
        return (out[:got], starts) if return_starts else out[:got]

    def search(self, pattern, max_results, ignore_crc=False, no_tables=False, ignore_case=False):
        """Where `pattern` (1 .. 256 bytes) occurs in the decoded stream -> (the smallest min(total, max_results) positions, ascending: an
        int64 tensor on the stream's device; the total).  Only the blocks whose search tables (types 1 to 4) admit the pattern are decoded.
        ignore_case (here, in search_many, search_records and grep): grep -i in the C locale, A .. Z equal a .. z; the stream stays as it is."""
        out, d_out = _room(max_results, torch.int64, self.dev)
        total, _ = self.reader.search(pattern, d_out, max_results, ignore_crc=ignore_crc, no_tables=no_tables, stream=_stream(self.dev), ignore_case=ignore_case)
        return out[:min(total, max_results)], total

    def search_many(self, patterns, max_results, ignore_crc=False, no_tables=False, ignore_case=False):
        """Where each of `patterns` (a sequence of up to 4096 bytes objects of 1 .. 256 bytes) occurs in the decoded stream, in one pass over
        the blocks that any pattern's search tables admit -> (positions int64, which int32, counts int64, total): the smallest
        min(total, max_results) pairs (position, pattern index) in ascending order, every pattern's own number of occurrences and the
        number of all pairs; tensors on the stream's device."""
        pats = list(patterns)
        pos, d_pos = _room(max_results, torch.int64, self.dev)
        which, d_which = _room(max_results, torch.int32, self.dev)
        counts, _ = _room(len(pats), torch.int64, self.dev, torch.zeros)
        total, _ = self.reader.search_many(pats, counts.data_ptr(), d_pos, d_which, max_results, ignore_crc=ignore_crc, no_tables=no_tables, stream=_stream(self.dev),
                                           ignore_case=ignore_case)
        k = min(total, max_results)
        return pos[:k], which[:k], counts[:len(pats)], total

    def search_records(self, pattern, delimiter=b"\n", max_records=1024, max_bytes=1 << 20, max_reach=0, ignore_crc=False, no_tables=False, ignore_case=False):
        """The records (lines, for the default delimiter) of the decoded stream that hold `pattern`, each once, in stream order ->
        (total_records, data, rec_off, rec_start, flags, totals): the first k records' bytes back to back (uint8), where each starts in the
        decoded stream (int64, k values) and in `data` (int64, k + 1 values: the last is data's size), its flags (uint8: 1 = cut left,
        2 = cut right — records longer than max_reach, 0 = 65536) — tensors on the stream's device, trimmed to what was written: k is
        the most records that max_records and max_bytes hold whole — and totals = (records, bytes of all records, occurrences, flagged
        records).  max_records = max_bytes = 0 counts.  With ignore_case the records' bytes are the stream's original ones."""
        data, d_data = _room(max_bytes, torch.uint8, self.dev)
        rec_off, d_rec_off = _room(max_records, torch.int64, self.dev)
        rec_start = torch.zeros(max_records + 1, dtype=torch.int64, device=self.dev)
        flags, d_flags = _room(max_records, torch.uint8, self.dev)
        total, totals, _ = self.reader.search_records(pattern, delimiter, d_data, max_bytes, d_rec_off, rec_start.data_ptr(), d_flags, max_records, max_reach=max_reach,
                                                      ignore_crc=ignore_crc, no_tables=no_tables, stream=_stream(self.dev), ignore_case=ignore_case)
        k = int((rec_start[1:] != 0).sum())   # (no record is empty: the starts behind the first are positive as far as they were written)
        return total, data[:int(rec_start[k])], rec_off[:k], rec_start[:k + 1], flags[:k], totals

    def index_records(self, delimiter=b"\n", ignore_crc=False):
        """Builds the record index of the decoded stream for the one-byte `delimiter` (one decode of the stream; 8 bytes per delimiter
        stay on the device until close() or another delimiter) -> the number of records N.  read_records, line_numbers and
        read_record_range need it."""
        return self.reader.index_records(delimiter, ignore_crc=ignore_crc, stream=_stream(self.dev))[0]

    def read_records(self, idx, ignore_crc=False):
        """The records with the numbers `idx` (int64 or uint64 tensor on the stream's device; any order, repeats allowed), back to back in
        the order given -> (a new uint8 tensor, the n + 1 places where the records start in it and its size: int64).  The one thing that
        visits the host is the records' total size, which sizes the output."""
        idx = _items(idx, self.dev, "read_records")
        dev, n = self.dev, idx.numel()
        starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n == 0:
            self.reader.record_count()   # (without an index this raises, as every call on it does)
            return torch.empty(0, dtype=torch.uint8, device=dev), starts
        st = _stream(dev)
        spans = torch.empty(2 * n, dtype=torch.int64, device=dev)
        total = self.reader.record_spans(idx.data_ptr(), n, spans.data_ptr(), spans[n:].data_ptr(), stream=st)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        got = self.reader.read_records(idx.data_ptr(), n, out.data_ptr(), total, d_starts=starts.data_ptr(), ignore_crc=ignore_crc, stream=st)
        return out[:got], starts

    def line_numbers(self, positions):
        """The record number (0-based) of every position of the decoded stream in `positions` (int64 or uint64 tensor on the stream's
        device) -> an int64 tensor; -1 for a position at or beyond the size.  With search_records' rec_off: the line numbers of the
        matching lines."""
        positions = _items(positions, self.dev, "line_numbers")
        n = positions.numel()
        out = torch.empty(n, dtype=torch.int64, device=self.dev)
        if n == 0:
            self.reader.record_count()
        else:
            self.reader.record_numbers(positions.data_ptr(), n, out.data_ptr(), stream=_stream(self.dev))
        return out

    def grep(self, patterns, invert=False, before=0, after=0, max_records=1 << 20, count_only=False, ignore_crc=False, no_tables=False, ignore_case=False):
        """grep over the decoded stream's lines: the records that hold one of `patterns` (a sequence of up to 4096 bytes objects of
        1 .. 256 bytes without the delimiter; a single bytes object is one pattern), with invert those that hold none, and `before` /
        `after` context records around each, every record once, in stream order.  Builds the record index for b"\n" when the stream has
        none (index_records chooses another delimiter).
        -> (R, numbers, kinds, data, starts): the number of such records; the smallest min(R, max_records) record numbers (int64); 1 for a
        selected record and 0 for one that is context only (uint8); those records' bytes back to back (uint8) and the k + 1 places where
        they start in it and its size (int64) — tensors on the stream's device.
        count_only (grep -c): -> (R, the selected records) and nothing is written or read."""
        R, totals, numbers, kinds = self._grep_numbers(patterns, 0 if count_only else max_records, invert=invert, before=before, after=after, ignore_crc=ignore_crc,
                                                       no_tables=no_tables, ignore_case=ignore_case)
        return self._grep_lines(R, totals, numbers, kinds, count_only, ignore_crc)

    def _grep_lines(self, R, totals, numbers, kinds, count_only, ignore_crc):
        """grep's second half: what _grep_numbers or _grep_regex_numbers found -> what grep returns (the records' bytes by read_records)."""
        if count_only:
            return totals[0], totals[1]
        dev, k = self.dev, numbers.numel()
        starts = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        data = torch.empty(max(totals[2], 1), dtype=torch.uint8, device=dev)
        got = self.reader.read_records(numbers.data_ptr(), k, data.data_ptr(), totals[2], d_starts=starts.data_ptr(), ignore_crc=ignore_crc, stream=_stream(dev)) if k else 0
        return R, numbers, kinds, data[:got], starts

    def _grep_numbers(self, patterns, max_records, **kw):
        """grep's first half -> (R, the call's totals, the smallest min(R, max_records) record numbers, their kinds); builds the index for b"\n"
        when the stream has none."""
        pats = [patterns] if isinstance(patterns, (bytes, bytearray)) else list(patterns)
        return self._grep_call(lambda d_numbers, d_kinds, cap, st: self.reader.grep_records(pats, d_numbers, d_kinds, cap, stream=st, **kw), max_records, kw.get("ignore_crc", False))

    def _grep_call(self, call, max_records, ignore_crc):
        """The index for b"\n" when the stream has none, room for min(max_records, N) numbers and kinds, call(d_numbers, d_kinds, cap, stream) ->
        (R, the call's totals, the numbers, the kinds)."""
        dev, st = self.dev, _stream(self.dev)
        try:
            self.reader.record_count()
        except api.MinLZError:   # (no index yet)
            self.reader.index_records(b"\n", ignore_crc=ignore_crc, stream=st)
        cap = min(max_records, self.reader.record_count())
        numbers, d_numbers = _room(cap, torch.int64, dev)
        kinds, d_kinds = _room(cap, torch.uint8, dev)
        R, totals, _ = call(d_numbers, d_kinds, cap, st)
        k = min(R, cap)
        return R, totals, numbers[:k], kinds[:k]

    def _grep_regex_numbers(self, exprs, max_records, ignore_case=False, ignore_crc=False, **kw):
        """_grep_numbers for regular expressions (a bytes object, a sequence of them, or an api.Regex, which stays the caller's)."""
        regex = exprs if isinstance(exprs, api.Regex) else api.Regex(exprs, ignore_case=ignore_case)
        try:
            return self._grep_call(lambda d_numbers, d_kinds, cap, st: self.reader.grep_regex(regex, d_numbers, d_kinds, cap, ignore_crc=ignore_crc, stream=st, **kw), max_records, ignore_crc)
        finally:
            if regex is not exprs:
                regex.close()

    def grep_regex(self, exprs, invert=False, before=0, after=0, max_records=1 << 20, count_only=False, ignore_crc=False, ignore_case=False, prune=False):
        """grep -E over the decoded stream's lines: grep() with the selected records decided by regular expressions over bytes — `exprs` is a
        bytes object, a sequence of up to 256 of them (a record is selected when it holds a match of any) or a compiled api.Regex (whose own
        ignore_case then holds); the syntax is the subset of Python's `re` that include/minlz_hip_regex.h lists, ^ and $ are a record's start
        and end, and an empty line is selected exactly when the expression matches the empty string (b"^$").  Every chunk is decoded once: no
        search table prunes for an expression — unless prune is set: then only the chunks are decoded that the search tables admit for the
        expression's required literals (api.Regex.literals), widened to whole lines, with the same result.  Lines longer than api.REGEX_MAX_RECORD raise ErrUnsupported.
        -> what grep returns: (R, numbers, kinds, data, starts), or with count_only (R, the selected records)."""
        R, totals, numbers, kinds = self._grep_regex_numbers(exprs, 0 if count_only else max_records, ignore_case=ignore_case, ignore_crc=ignore_crc, invert=invert, before=before,
                                                             after=after, prune=prune)
        return self._grep_lines(R, totals, numbers, kinds, count_only, ignore_crc)

    def read_record_range(self, first, count, ignore_crc=False):
        """Records first .. first + count - 1 as they lie in the decoded stream, the delimiters between them included -> a new uint8 tensor."""
        off, ln = self.reader.record_range(first, count)
        return self.read_ranges([off], [ln], ignore_crc)

    def build_sidecar(self, cfgs, ignore_crc=False, compress=False):
        """A sidecar search index of this stream for 1 .. 4 configurations (api.search_config): search tables for every block, whoever
        wrote the stream, in a separate .mz stream -> a new uint8 tensor on the stream's device.  compress: table chunks are written
        compressed (0x46) where that is smaller."""
        cap = self.reader.sidecar_bound(cfgs)
        out = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        got = self.reader.build_sidecar(cfgs, out.data_ptr(), cap, ignore_crc=ignore_crc, stream=_stream(self.dev), compress=compress)
        return out[:got].clone()

    def attach_sidecar(self, side, ignore_crc=False):
        """search and search_many use the tables of the sidecar `side` (a uint8 tensor on the stream's device, as build_sidecar returns
        it) from now on; None detaches.  The stream keeps the tensor alive."""
        if side is None:
            self.reader.detach_sidecar()
        else:
            side = _u8(side, "attach_sidecar", self.dev)
            self.reader.attach_sidecar(side.data_ptr(), side.numel(), ignore_crc=ignore_crc, stream=_stream(self.dev))
        self.side = side

    def extract_sidecar(self, strip=False):
        """The search tables this stream carries inline, copied as they are into a sidecar (the reference's ExtractSidecar; nothing is
        decoded or rebuilt) -> a new uint8 tensor on the stream's device, whose references name this stream's offsets.  strip: -> (side, main)
        where `main` is this stream without its search and index chunks and with a fresh seek index, and the references name main's offsets:
        open `main` and attach `side` to search it."""
        side_cap, main_cap = self.reader.extract_sidecar_bound()
        side = torch.empty(side_cap, dtype=torch.uint8, device=self.dev)
        main = torch.empty(main_cap, dtype=torch.uint8, device=self.dev) if strip else None
        got = self.reader.extract_sidecar(side.data_ptr(), side_cap, main.data_ptr() if strip else None, main_cap if strip else 0, stream=_stream(self.dev))
        return (side[:got.side_len].clone(), main[:got.main_len].clone()) if strip else side[:got.side_len].clone()

    def save_record_index(self):
        """The stream's record index (index_records, or a load) as a record index blob: about 2 bytes per record, bound to this stream ->
        a new uint8 tensor on the stream's device.  load_record_index of a later open of the same stream takes it in the place of the decode."""
        cap = self.reader.record_index_bound()
        out = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        got, _ = self.reader.save_record_index(out.data_ptr(), cap, stream=_stream(self.dev))
        return out[:got].clone()

    def load_record_index(self, blob, ignore_crc=False):
        """The record index blob `blob` (a uint8 tensor on the stream's device: save_record_index's, or HipTensorCodec.build_record_index's
        over the stream's raw bytes) becomes the stream's record index without a decode -> the number of records N.  A blob that is
        malformed or belongs to another stream raises, and the stream keeps the index it had."""
        blob = _u8(blob, "load_record_index", self.dev)
        return self.reader.load_record_index(blob.data_ptr(), blob.numel(), ignore_crc=ignore_crc, stream=_stream(self.dev))[0]

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


class DeviceStreamSet(DeviceStream):
    """Many .mz streams on the device opened as ONE DeviceStream (HipTensorCodec.open_streams): its decoded bytes are the streams' decoded
    bytes one behind the other, and read_ranges, search, search_many, search_records, index_records, read_records, line_numbers, grep and grep_regex
    work on that concatenation — a range, an occurrence or a record may cross from one stream into the next.  The calls here turn positions
    and record numbers back into (stream, position or record inside the stream), on the device.  No search tables and no sidecar — unless the set was opened
    with tables=True (.tables): then search, search_many, search_records, grep, grep_streams, grep_regex(prune=True) and
    grep_streams_regex(prune=True) decode only the chunks that the streams' inline search tables admit (include/minlz_hip_stream_set_tables.h:
    the greps prune as each stream alone would when every stream ends with the delimiter; the position searches also take every stream's last
    bytes), no_tables=True turns that off per call, and tables_info() describes the last plan.  Still no sidecar.
    .sizes: every stream's decoded size (0 for a failed one); .errors: {index: negative code} of the streams left out for a framing error;
    .bases: the n + 1 places where the streams start in the set (a list of ints; the last is .size)."""

    def __init__(self, ctx, t, spans, tables=False):
        self.t, self.dev, self.spans, self.tables = t, t.device, spans, bool(tables)
        self.reader, res = ctx.stream_open_batch_device(t.data_ptr() if spans else None, spans, stream=_stream(t.device), tables=self.tables)
        self.size = self.reader.size
        self.side = None
        self.sizes = [max(r, 0) for r in res]
        self.errors = {i: r for i, r in enumerate(res) if r < 0}
        self.bases = self.reader.stream_bases()

    def tables_info(self):
        """The last plan on a set opened with tables=True (api.DeviceReader.set_tables_info) -> (classes, streams pruned, streams decoded
        whole, chunks with a usable table, those from compressed table chunks, stream ends treated as crossed, 0x46 tables that stand expanded)."""
        return self.reader.set_tables_info()

    def _located(self, call, items, what):
        items = _items(items, self.dev, what)
        n = items.numel()
        which = torch.full((max(n, 1),), -1, dtype=torch.int32, device=self.dev)
        local = torch.zeros(max(n, 1), dtype=torch.int64, device=self.dev)
        if n:
            call(items.data_ptr(), n, which.data_ptr(), local.data_ptr(), stream=_stream(self.dev))
        return which[:n], local[:n]

    def locate(self, positions):
        """(which, local): the stream of every position of the set in `positions` (int64 or uint64 tensor on the device) and the position
        inside that stream's decoded bytes — int32 and int64 tensors; -1 and 0 for a position at or beyond the size.  With the offsets of
        search / search_many and a pattern of L bytes: local + L > sizes[which] is an occurrence that crosses a stream's end."""
        return self._located(self.reader.locate, positions, "locate")

    def locate_records(self, rec_no):
        """(which, local_no): the stream in which every record of `rec_no` (int64 or uint64 tensor on the device) starts and its number
        inside that stream — int32 and int64 tensors; -1 and 0 at or beyond the record count.  Needs the record index."""
        if _items(rec_no, self.dev, "locate_records").numel() == 0:
            self.reader.record_count()
        return self._located(self.reader.locate_records, rec_no, "locate_records")

    def read_stream_ranges(self, which, offsets, lengths, ignore_crc=False, return_starts=False):
        """read_ranges with every range relative to its stream: bytes [offsets[i], offsets[i] + lengths[i]) of stream which[i], back to back in
        the order given -> one new uint8 tensor (return_starts: and the n + 1 places where the ranges start in it).  which: an int32 or int64
        tensor on the device; offsets, lengths: int64 or uint64.  A range that leaves its stream raises."""
        for a in (offsets, lengths):
            _items(a, self.dev, "read_stream_ranges")
        if not torch.is_tensor(which) or which.dtype not in (torch.int32, torch.int64) or which.dim() != 1 or which.device != self.dev:
            raise ValueError("read_stream_ranges: which is a 1-d int32 or int64 tensor on the stream's device")
        n = offsets.numel()
        if lengths.numel() != n or which.numel() != n:
            raise ValueError("read_stream_ranges: as many streams and lengths as offsets")
        if which.dtype == torch.int64:   # (a number that does not fit is beyond every count: it stays so)
            which = which.clamp(-1, 0x7FFFFFFF).to(torch.int32)
        which = which.contiguous()
        total = int(lengths.view(torch.int64).sum()) if n else 0
        if total < 0 or total > n * max(self.sizes + [0]):
            total = 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        starts = torch.zeros(n + 1, dtype=torch.int64, device=self.dev) if return_starts else None
        got = self.reader.read_streams_device(which.data_ptr() if n else None, offsets.data_ptr() if n else None, lengths.data_ptr() if n else None, n, out.data_ptr(), total,
                                              d_starts=starts.data_ptr() if return_starts and n else None, ignore_crc=ignore_crc, stream=_stream(self.dev))
        return (out[:got], starts) if return_starts else out[:got]

    def stream_records(self):
        """(first, joined): first[i] = the records of the set that start in front of stream i (n + 1 ints; the last is the record count);
        joined = the streams whose last record runs on into the next stream.  With joined == 0 stream i's own records are the set's
        records first[i] .. first[i + 1] - 1.  Needs the record index."""
        return self.reader.stream_records(stream=_stream(self.dev))

    def grep_streams(self, patterns, invert=False, before=0, after=0, max_records=1 << 20, ignore_crc=False, no_tables=False, ignore_case=False):
        """grep -H -n over the set: grep's selected and context records as (which, line_in_stream, kind) — the stream each record starts in
        (int32), its number inside that stream (int64, from 0) and 1 for a selected record, 0 for context only (uint8); tensors on the
        device, in the set's order.  grep followed by locate_records; nothing per record visits the host."""
        _, _, numbers, kinds = self._grep_numbers(patterns, max_records, invert=invert, before=before, after=after, ignore_crc=ignore_crc, no_tables=no_tables,
                                                  ignore_case=ignore_case)
        which, line = self.locate_records(numbers)
        return which, line, kinds

    def grep_streams_regex(self, exprs, invert=False, before=0, after=0, max_records=1 << 20, ignore_crc=False, ignore_case=False, prune=False):
        """grep -E -H -n over the set: grep_streams with the selected records decided by regular expressions (exprs as in grep_regex)
        -> (which, line_in_stream, kind).  grep_regex's first half followed by locate_records."""
        _, _, numbers, kinds = self._grep_regex_numbers(exprs, max_records, ignore_case=ignore_case, ignore_crc=ignore_crc, invert=invert, before=before, after=after, prune=prune)
        which, line = self.locate_records(numbers)
        return which, line, kinds

    def build_sidecar(self, cfgs, ignore_crc=False, compress=False):
        raise api.ErrUnsupported("build_sidecar: a set of streams takes no sidecar")

    def attach_sidecar(self, side, ignore_crc=False):
        raise api.ErrUnsupported("attach_sidecar: a set of streams takes no sidecar")

    def extract_sidecar(self, strip=False):
        raise api.ErrUnsupported("extract_sidecar: a set of streams takes no sidecar")
