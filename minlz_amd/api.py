"""Block API mirror of the reference (encode.go:74-244, decode.go:50-156) over the C ABI."""
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import BlockDesc

LevelSuperFast, LevelUncompressed, LevelFastest, LevelBalanced = -1, 0, 1, 2  # encode.go:25-43 (LevelSmallest = 3 is CPU-only)
MaxBlockSize = 8 << 20  # minlz.go:84

OPT_DECODE_ALGO, OPT_ENCODE_FAR, OPT_TIMING = 1, 2, 100
OPT_L2_FREE, OPT_GEN_SPIN, OPT_GEN_PACKED, OPT_DEVICE_GROUP, OPT_L2_GAP = 14, 9, 13, 17, 19   # include/minlz_hip.h


class MinLZError(Exception):
    code = 0


class ErrCorrupt(MinLZError):
    """minlz: corrupt input (decode.go:31)"""
    code = 1


class ErrTooLarge(MinLZError):
    """minlz: decoded block is too large (decode.go:35)"""
    code = 2


class ErrUnsupported(MinLZError):
    """minlz: unsupported input (decode.go:37)"""
    code = 3


class ErrInvalidLevel(MinLZError):
    """minlz: invalid compression level (decode.go:39)"""
    code = 4


class ErrCRC(MinLZError):
    """minlz: corrupt input, crc mismatch (decode.go:33)"""
    code = 5


class ErrHIP(MinLZError):
    code = 7


_ERRS = {1: ErrCorrupt, 2: ErrTooLarge, 3: ErrUnsupported, 4: ErrInvalidLevel, 5: ErrCRC, 7: ErrHIP}


def _raise(code, ctx=None):
    code = -code if code < 0 else code
    msg = ""
    if ctx is not None and code == 7:
        msg = _lib.lib().mlz_last_error(ctx.handle).decode()
    raise _ERRS.get(code, MinLZError)("minlz error %d %s" % (code, msg))


class Context:
    """One HIP device context (mlz_ctx). Thread-safe on the C side."""

    def __init__(self, device=-1, devices=None):
        """device: one HIP device (mlz_init).  devices: a list of ordinals (repeats allowed) or "all" — one context that deals the blocks of
        batches and streams to all of them from this process (mlz_init_devices)."""
        self.handle = C.c_void_p()
        L = _lib.lib()
        if devices is None:
            r = L.mlz_init(device, C.byref(self.handle))
        elif isinstance(devices, str):
            assert devices == "all"
            r = L.mlz_init_devices(None, 0, C.byref(self.handle))
        else:
            arr = (C.c_int * len(devices))(*devices)
            r = L.mlz_init_devices(arr, len(devices), C.byref(self.handle))
        if r != 0:
            raise ErrHIP("mlz_init failed (%d): no HIP device?" % r)

    def device_count(self):
        return int(_lib.lib().mlz_device_count(self.handle))

    def close(self):
        if self.handle:
            _lib.lib().mlz_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt, value):
        r = _lib.lib().mlz_set_option(self.handle, opt, int(value))
        if r:
            _raise(r, self)

    def device_name(self):
        buf = C.create_string_buffer(256)
        _lib.lib().mlz_device_name(self.handle, buf, 256)
        return buf.value.decode()

    def timers(self):
        arr = (C.c_float * 16)()
        n = _lib.lib().mlz_get_timers(self.handle, arr, 16)
        return {_lib.lib().mlz_timer_name(i).decode(): arr[i] for i in range(n) if arr[i] >= 0}

    def combine_stats(self):
        """(batches run, requests served) by the combining queue of the single-block host calls."""
        L = _lib.lib()
        return int(L.mlz_get_counter(self.handle, 0)), int(L.mlz_get_counter(self.handle, 1))

    def workspace_bytes(self):
        """(encode side, decode side): device workspace the context holds — grow-only, i.e. the high-water mark of its calls (mlz_get_counter 3, 4)."""
        L = _lib.lib()
        return int(L.mlz_get_counter(self.handle, 3)), int(L.mlz_get_counter(self.handle, 4))

    def general_blocks(self):
        """Blocks of the last decode call that took the path for streams of other encoders (mlz_get_counter 2)."""
        return int(_lib.lib().mlz_get_counter(self.handle, 2))

    def general_team(self):
        """Workgroups per block (1, 2 or 4) the general-block pass of the last decode call settled with; 0 = no general block (mlz_get_counter 6)."""
        return int(_lib.lib().mlz_get_counter(self.handle, 6))

    def release_stream(self, stream):
        """mlz_release_stream: call before destroying a stream that carried a *_batch_device call of this context."""
        r = _lib.lib().mlz_release_stream(self.handle, stream)
        if r:
            _raise(r, self)

    def stream_encode_gather_device(self, level, block_size, add_index, d_srcs, lens, d_dst, dst_cap, search_match_len=None, search_prefix=None,
                                    search_long_prefix=None, search_extras=0):
        """mlz_stream_encode_gather_device: ranges of one stream resident on the context's devices -> the framed stream in d_dst (device memory).
        search_match_len: None = no search tables; 0 = block search tables with the reference's default match length (6); 1 .. 8 = with that one.
        search_prefix (with search_match_len): an iterable of byte values; the tables then index only the positions behind one of them
        (mlz_stream_encode_gather_device_tables: 1 to 8 distinct values give table type 2, in sorted order, more give type 3).
        search_long_prefix (with search_match_len, not with search_prefix): 1 .. 256 bytes; the tables then index the search_extras + 1
        windows behind every occurrence of that byte string (mlz_stream_encode_gather_device_long_prefix, table type 4; search_extras 0 .. 15,
        match length + extras <= 16).
        Returns the stream size."""
        n = len(d_srcs)
        sp = (C.c_void_p * n)(*d_srcs); sl = (C.c_size_t * n)(*lens)
        if search_long_prefix is not None:
            if search_prefix is not None:
                raise ValueError("search_long_prefix and search_prefix exclude each other")
            if search_match_len is None:
                raise ValueError("search_long_prefix needs search_match_len")
            cfg = search_long_prefix_config(search_match_len, search_long_prefix, search_extras)
            r = _lib.lib().mlz_stream_encode_gather_device_long_prefix(self.handle, level, block_size, STREAM_ADD_INDEX if add_index else 0, C.byref(cfg), sp, sl, n,
                                                                       d_dst, dst_cap)
            if r < 0:
                _raise(r, self)
            return int(r)
        if search_extras:
            raise ValueError("search_extras needs search_long_prefix")
        if search_prefix is not None:
            if search_match_len is None:
                raise ValueError("search_prefix needs search_match_len")
            cfg = search_tables_config(search_match_len, search_prefix)
            r = _lib.lib().mlz_stream_encode_gather_device_tables(self.handle, level, block_size, STREAM_ADD_INDEX if add_index else 0, C.byref(cfg), sp, sl, n, d_dst, dst_cap)
            if r < 0:
                _raise(r, self)
            return int(r)
        flags = (STREAM_ADD_INDEX if add_index else 0) | (0 if search_match_len is None else STREAM_SEARCH_TABLES | (search_match_len & 15) << 8)
        r = _lib.lib().mlz_stream_encode_gather_device(self.handle, level, block_size, flags, sp, sl, n, d_dst, dst_cap)
        if r < 0:
            _raise(r, self)
        return int(r)

    # ---- device-resident batch calls: pointers are raw device addresses (e.g. tensor.data_ptr()) ----
    def encode_batch_device(self, stream, level, d_src, d_dst, descs, d_out_len):
        arr = (BlockDesc * len(descs))(*descs) if not isinstance(descs, C.Array) else descs
        r = _lib.lib().mlz_encode_batch_device(self.handle, stream, level, d_src, d_dst, arr, len(arr), d_out_len)
        if r:
            _raise(r, self)

    def crc_batch_device(self, stream, d_base, descs, d_out_u32):
        arr = (BlockDesc * len(descs))(*descs) if not isinstance(descs, C.Array) else descs
        r = _lib.lib().mlz_crc_batch_device(self.handle, stream, d_base, arr, len(arr), d_out_u32)
        if r:
            _raise(r, self)

    def decode_batch_device(self, stream, d_src, d_dst, descs, d_out_len):
        arr = (BlockDesc * len(descs))(*descs) if not isinstance(descs, C.Array) else descs
        r = _lib.lib().mlz_decode_batch_device(self.handle, stream, d_src, d_dst, arr, len(arr), d_out_len)
        if r:
            _raise(r, self)

    def stream_decoded_len_device(self, d_src, n, stream=None):
        """mlz_stream_decoded_len_device: the chunk walk of a stream in device memory -> (result, prefix_len).  `result` is the raw return
        value (the decoded size, or -MLZ_ERR_* for a framing error: nothing is raised, so that a caller can size the output for the prefix)."""
        prefix = C.c_uint64(0)
        r = _lib.lib().mlz_stream_decoded_len_device(self.handle, stream, d_src, n, C.byref(prefix))
        return int(r), int(prefix.value)

    def stream_decode_device(self, d_src, n, d_dst, dst_cap, ignore_crc=False, stream=None):
        """mlz_stream_decode_device: NewReader(src) read to EOF, source and destination in device memory -> decoded size."""
        r = _lib.lib().mlz_stream_decode_device(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d_src, n, d_dst, dst_cap)
        if r < 0:
            _raise(r, self)
        return int(r)

    # ---- batches of streams in device memory: one call for many streams; per-stream results come back as lists, nothing is raised per stream ----
    @staticmethod
    def _stream_descs(descs):
        if isinstance(descs, C.Array):
            return descs
        return (BlockDesc * max(len(descs), 1))(*[BlockDesc(*[int(v) for v in (tuple(d) + (0, 0))[:4]]) for d in descs])

    def stream_decoded_len_batch_device(self, d_src, spans, stream=None):
        """mlz_stream_decoded_len_batch_device: the chunk walk of every stream (src_off, src_len) of the buffer at d_src ->
        [(result, prefix_len)], each as stream_decoded_len_device gives it for that stream alone."""
        n = len(spans)
        out = (C.c_int64 * max(n, 1))()
        prefix = (C.c_uint64 * max(n, 1))()
        r = _lib.lib().mlz_stream_decoded_len_batch_device(self.handle, stream, d_src, self._stream_descs(spans), n, out, prefix)
        if r:
            _raise(r, self)
        return [(int(out[i]), int(prefix[i])) for i in range(n)]

    def stream_decode_batch_device(self, d_src, d_dst, descs, ignore_crc=False, stream=None):
        """mlz_stream_decode_batch_device: every stream (src_off, src_len, dst_off, dst_cap) of the buffer at d_src decoded to its place in the
        buffer at d_dst -> [result]: the decoded size or -MLZ_ERR_* of each stream, as mlz_stream_decode_device returns it for that stream alone."""
        n = len(descs)
        out = (C.c_int64 * max(n, 1))()
        r = _lib.lib().mlz_stream_decode_batch_device(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d_src, d_dst, self._stream_descs(descs), n, out)
        if r:
            _raise(r, self)
        return [int(out[i]) for i in range(n)]

    def stream_encode_batch_device(self, level, block_size, add_index, d_src, d_dst, descs, stream=None, flags=0):
        """mlz_stream_encode_batch_device: every input (src_off, src_len, dst_off, dst_cap) of the buffer at d_src written as a stream of its own to
        its place in the buffer at d_dst -> [result]: the stream's size or -MLZ_ERR_* of each.  flags: further MLZ_STREAM_* bits, as they are."""
        n = len(descs)
        out = (C.c_int64 * max(n, 1))()
        r = _lib.lib().mlz_stream_encode_batch_device(self.handle, stream, level, block_size, (STREAM_ADD_INDEX if add_index else 0) | flags, d_src, d_dst,
                                                      self._stream_descs(descs), n, out)
        if r:
            _raise(r, self)
        return [int(out[i]) for i in range(n)]

    def batch_long_streams(self):
        """Streams that the context's last stream batch call walked by the region kernels: more than 4096 chunk headers (mlz_get_counter 12)."""
        return int(_lib.lib().mlz_get_counter(self.handle, 12))


    def stream_open_device(self, d_src, n, stream=None):
        """mlz_stream_open_device: a stream in device memory opened for range reads -> DeviceReader.  The caller keeps d_src alive and unchanged
        while the reader is open.  A stream with a framing error raises that error (no reader)."""
        h = C.c_void_p()
        r = _lib.lib().mlz_stream_open_device(self.handle, stream, d_src, n, C.byref(h))
        if r < 0:
            _raise(r, self)
        return DeviceReader(self, h, int(r))

    def range_plan(self):
        """(chunks decoded or copied, decoded bytes put into the scratch) by the context's last DeviceReader.read (mlz_get_counter 7, 8)."""
        L = _lib.lib()
        return int(L.mlz_get_counter(self.handle, 7)), int(L.mlz_get_counter(self.handle, 8))

    def search_plan(self):
        """(chunks decoded or copied, chunks with a usable search table) of the context's last DeviceReader.search, search_many or grep_records (mlz_get_counter 10, 11)."""
        L = _lib.lib()
        return int(L.mlz_get_counter(self.handle, 10)), int(L.mlz_get_counter(self.handle, 11))

    def range_plan_host_bytes(self):
        """Bytes of plan data that crossed between host and device, both directions together, in the context's last DeviceReader.read_device
        (mlz_get_counter 9): a header and two records per TOUCHED CHUNK, nothing per range."""
        return int(_lib.lib().mlz_get_counter(self.handle, 9))


class DeviceReader:
    """mlz_dev_reader: the device-resident ReadSeeker of one stream (Context.stream_open_device).  A context manager; close() frees it."""

    def __init__(self, ctx, handle, size):
        self.ctx, self.handle, self.size = ctx, handle, size

    def read(self, ranges, d_dst, dst_cap, ignore_crc=False, stream=None):
        """mlz_dev_reader_read.  ranges: (off, len, dst_off) triples, or a C-contiguous uint64 array of shape (k, 3): decoded bytes
        [off, off + len) go to d_dst[dst_off, dst_off + len).  -> the sum of the lengths."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        a = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 3)
        r = _lib.lib().mlz_dev_reader_read(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, a.ctypes.data if a.size else None, a.shape[0], d_dst, dst_cap)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def read_device(self, d_off, d_len, n, d_dst, dst_cap, d_starts=None, ignore_crc=False, stream=None):
        """mlz_dev_reader_read_device.  d_off, d_len: device addresses of n uint64 offsets and lengths; decoded bytes [off[i], off[i] + len[i])
        go to d_dst packed in the order given; d_starts (device address of n + 1 uint64, or None) receives where each range starts and the
        total.  -> the sum of the lengths."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_read_device(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d_off, d_len, n, d_dst, dst_cap, d_starts)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def search(self, pattern, d_offsets, cap, ignore_crc=False, no_tables=False, stream=None):
        """mlz_dev_reader_search.  pattern: 1 .. 256 bytes; d_offsets: device address of room for `cap` uint64 (None with cap == 0), which
        receives the smallest min(total, cap) positions of the pattern in the decoded stream, ascending.
        Uses the stream's block search tables of type 1, 2, 3 or 4 (with a prefix table: the pattern's windows that follow a prefix byte; a
        pattern without one is served by decoding every chunk, and the usable-table count is then 0).
        -> (total, (data chunks, chunks decoded or copied, chunks with a usable search table))."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        p = bytes(pattern)
        stats = (C.c_uint64 * 4)()
        flags = (STREAM_IGNORE_CRC if ignore_crc else 0) | (SEARCH_NO_TABLES if no_tables else 0)
        r = _lib.lib().mlz_dev_reader_search(self.handle, stream, flags, p, len(p), d_offsets, cap, stats)
        if r < 0:
            _raise(r, self.ctx)
        return int(r), (int(stats[0]), int(stats[1]), int(stats[2]))

    def search_many(self, patterns, d_counts, d_offsets, d_which, cap, ignore_crc=False, no_tables=False, stream=None):
        """mlz_dev_reader_search_many.  patterns: a sequence of up to 4096 bytes objects of 1 .. 256 bytes; d_counts: device address of room
        for len(patterns) uint64 (or None), which receives every pattern's number of occurrences; d_offsets, d_which: device addresses of
        room for `cap` uint64 and `cap` uint32 (None with cap == 0), which receive the smallest min(total, cap) pairs (position, pattern
        index) in ascending order.  The chunks that any pattern's tables admit are decoded once and scanned once for all patterns.
        -> (total pairs, (data chunks, chunks decoded or copied, chunks with a usable search table, patterns the tables could not serve))."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        pats = [bytes(p) for p in patterns]
        blob = b"".join(pats)
        lens = np.asarray([len(p) for p in pats], dtype=np.uint32)
        stats = (C.c_uint64 * 4)()
        flags = (STREAM_IGNORE_CRC if ignore_crc else 0) | (SEARCH_NO_TABLES if no_tables else 0)
        r = _lib.lib().mlz_dev_reader_search_many(self.handle, stream, flags, blob if pats else None, lens.ctypes.data if pats else None, len(pats), d_counts, d_offsets,
                                                  d_which, cap, stats)
        if r < 0:
            _raise(r, self.ctx)
        return int(r), tuple(int(v) for v in stats)

    def search_records(self, pattern, delimiter, d_dst, dst_cap, d_rec_off, d_rec_start, d_rec_flags, rec_cap, max_reach=0, ignore_crc=False, no_tables=False, stream=None):
        """mlz_dev_reader_search_records: the records (maximal runs without the byte `delimiter`) that hold `pattern` (1 .. 256 bytes without
        the delimiter), each once, in stream order.  d_dst: device address of room for dst_cap bytes (None with dst_cap == 0), which
        receives the first k records' bytes, packed; d_rec_off: room for rec_cap uint64 (None with rec_cap == 0), each record's start in
        the decoded stream; d_rec_start: room for rec_cap + 1 uint64 or None, each record's start in d_dst and the bytes written;
        d_rec_flags: room for rec_cap bytes or None, bit 0 = cut left, bit 1 = cut right.  k: the most records that both caps hold whole.
        max_reach: how far the call looks to either side of an occurrence (0 = 65536, at most 2^20); longer records come out cut.
        -> (records, (records, bytes of all records, occurrences, records with a flag), (data chunks, chunks decoded or copied by the
        search phase, chunks with a usable search table))."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        p = bytes(pattern)
        d = bytes(delimiter) if not isinstance(delimiter, int) else bytes([delimiter])
        if len(d) != 1:
            raise ValueError("search_records: a delimiter of one byte")
        totals, stats = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        flags = (STREAM_IGNORE_CRC if ignore_crc else 0) | (SEARCH_NO_TABLES if no_tables else 0)
        r = _lib.lib().mlz_dev_reader_search_records(self.handle, stream, flags, p, len(p), d[0], max_reach, d_dst, dst_cap, d_rec_off, d_rec_start, d_rec_flags, rec_cap,
                                                     totals, stats)
        if r < 0:
            _raise(r, self.ctx)
        return int(r), tuple(int(v) for v in totals), (int(stats[0]), int(stats[1]), int(stats[2]))

    def index_records(self, delimiter=b"\n", ignore_crc=False, stream=None):
        """mlz_dev_reader_index_records: builds the record index for the one-byte `delimiter` — the positions of all delimiters of the
        decoded stream, 8 bytes each in device memory the handle owns — by one decode of the stream.  Record r is the bytes between
        delimiter r - 1 and delimiter r; empty records count; a stream that ends without a delimiter has one more record.  The same
        delimiter again costs nothing; another one replaces the index.
        -> (N, (N, delimiters, bytes of index held, chunks this call decoded))."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        d = bytes(delimiter) if not isinstance(delimiter, int) else bytes([delimiter])
        if len(d) != 1:
            raise ValueError("index_records: a delimiter of one byte")
        info = (C.c_uint64 * 4)()
        r = _lib.lib().mlz_dev_reader_index_records(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d[0], info)
        if r < 0:
            _raise(r, self.ctx)
        return int(r), tuple(int(v) for v in info)

    def record_count(self):
        """mlz_dev_reader_record_count: the records of the indexed stream; raises without an index."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_record_count(self.handle)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def record_spans(self, d_idx, n, d_off, d_len, stream=None):
        """mlz_dev_reader_record_spans.  d_idx: device address of n uint64 record numbers (any order, repeats allowed); d_off, d_len:
        device addresses of room for n uint64 each, which receive every record's first byte in the decoded stream and its length.
        -> the sum of the lengths.  A number >= record_count() raises."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_record_spans(self.handle, stream, d_idx, n, d_off, d_len)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def read_records(self, d_idx, n, d_dst, dst_cap, d_starts=None, ignore_crc=False, stream=None):
        """mlz_dev_reader_read_records: the records d_idx[0 .. n) (device address of uint64 record numbers) packed into d_dst in the order
        given; d_starts (device address of n + 1 uint64, or None) receives where each record starts in d_dst and the total.  Only the
        chunks the records touch are decoded, each once.  -> the bytes written.  A number >= record_count() or a total above dst_cap
        raises, and nothing has been written then."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_read_records(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d_idx, n, d_dst, dst_cap, d_starts)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def record_numbers(self, d_pos, n, d_no, stream=None):
        """mlz_dev_reader_record_numbers.  d_pos: device address of n uint64 positions of the decoded stream; d_no: room for n uint64, which
        receive each position's record number (0-based; a delimiter has the number of the record it ends; 2^64 - 1 for a position at or
        beyond the size).  -> how many positions lie inside the stream."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_record_numbers(self.handle, stream, d_pos, n, d_no)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def grep_records(self, patterns, d_rec_no, d_rec_kind, rec_cap, invert=False, before=0, after=0, ignore_crc=False, no_tables=False, stream=None):
        """mlz_dev_reader_grep_records: grep over the record index.  patterns: a sequence of up to 4096 bytes objects of 1 .. 256 bytes
        without the index's delimiter (none: nothing matches, and under invert every record is selected); a record is selected when it
        holds one of them, with invert when it holds none; before, after: context records in front of and behind every selected one.
        d_rec_no: device address of room for rec_cap uint64 (None with rec_cap == 0), which receives the smallest min(R, rec_cap) numbers
        of the selected and context records, ascending; d_rec_kind: room for rec_cap bytes or None, 1 = selected, 0 = context only.
        -> (R, (R, selected records, bytes of the written records: read_records' dst_cap, bytes of all R records), (data chunks, chunks
        decoded or copied, chunks with a usable search table, patterns the tables could not serve))."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        pats = [bytes(p) for p in patterns]
        blob = b"".join(pats)
        lens = np.asarray([len(p) for p in pats], dtype=np.uint32)
        totals, stats = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        flags = (STREAM_IGNORE_CRC if ignore_crc else 0) | (SEARCH_NO_TABLES if no_tables else 0) | (GREP_INVERT if invert else 0)
        r = _lib.lib().mlz_dev_reader_grep_records(self.handle, stream, flags, blob if pats else None, lens.ctypes.data if pats else None, len(pats), before, after, d_rec_no,
                                                   d_rec_kind, rec_cap, totals, stats)
        if r < 0:
            _raise(r, self.ctx)
        return int(r), tuple(int(v) for v in totals), tuple(int(v) for v in stats)

    def record_range(self, first, count):
        """mlz_dev_reader_record_range: records first .. first + count - 1 as one byte range, the delimiters between them included
        -> (off, len), to be read with read().  first + count > record_count() raises."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        off, ln = C.c_uint64(), C.c_uint64()
        r = _lib.lib().mlz_dev_reader_record_range(self.handle, first, count, C.byref(off), C.byref(ln))
        if r < 0:
            _raise(r, self.ctx)
        return int(off.value), int(ln.value)

    @staticmethod
    def _configs(cfgs):
        cfgs = list(cfgs)
        arr = (_lib.SearchConfig * max(len(cfgs), 1))()
        for i, q in enumerate(cfgs):
            arr[i] = q
        return arr, len(cfgs)

    def sidecar_bound(self, cfgs):
        """mlz_dev_reader_sidecar_bound: room that always suffices for build_sidecar with these configurations (api.search_config)."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        arr, n = self._configs(cfgs)
        r = _lib.lib().mlz_dev_reader_sidecar_bound(self.handle, arr, n)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def build_sidecar(self, cfgs, d_dst, cap, ignore_crc=False, stream=None):
        """mlz_dev_reader_build_sidecar: the sidecar of this stream for 1 .. 4 configurations (api.search_config) — search tables for every
        data chunk in a separate stream that names the chunks by remote references — into `cap` bytes at device address d_dst -> its size."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        arr, n = self._configs(cfgs)
        r = _lib.lib().mlz_dev_reader_build_sidecar(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, arr, n, d_dst, cap)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def attach_sidecar(self, d_side, n, ignore_crc=False, stream=None):
        """mlz_dev_reader_attach_sidecar: search and search_many use the tables of the sidecar at device address d_side (n bytes) from now
        on.  The caller keeps those bytes alive and unchanged.  A sidecar that does not belong to this stream raises, and nothing changes."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_attach_sidecar(self.handle, stream, STREAM_IGNORE_CRC if ignore_crc else 0, d_side, n)
        if r < 0:
            _raise(r, self.ctx)

    def detach_sidecar(self):
        """The searches use the stream's inline tables again."""
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        r = _lib.lib().mlz_dev_reader_attach_sidecar(self.handle, None, 0, None, 0)
        if r < 0:
            _raise(r, self.ctx)

    def close(self):
        if self.handle:
            _lib.lib().mlz_dev_reader_close(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self.ctx.handle:   # (a reader that outlived its context has nothing left to free it with: the context owned the device)
                self.close()
        except Exception:
            pass


_default = None
_default_lock = threading.Lock()


def default_context():
    global _default
    with _default_lock:
        if _default is None:
            _default = Context()
        return _default


def _np(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(b, dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data if a.size else None


def MaxEncodedLen(n):
    """encode.go:234-244"""
    return _lib.lib().mlz_max_encoded_len(n) if n >= 0 else -1


def DecodedLen(src):
    """decode.go:107-110"""
    a = _np(src)
    r = _lib.lib().mlz_decoded_len(_ptr(a), a.size)
    if r < 0:
        _raise(r)
    return r


def IsMinLZ(src):
    """decode.go:114-117 -> (ok, size); raises like the reference returns err."""
    a = _np(src)
    r = _lib.lib().mlz_decoded_len(_ptr(a), a.size)
    if r < 0:
        _raise(r)
    return (a.size > 0 and a[0] == 0), r


def Encode(src, level=LevelFastest, ctx=None):
    """minlz.Encode(nil, src, level), encode.go:74-139."""
    ctx = ctx or default_context()
    a = _np(src)
    cap_ = MaxEncodedLen(a.size)
    if cap_ < 0:
        raise ErrTooLarge()
    out = np.empty(cap_, dtype=np.uint8)
    r = _lib.lib().mlz_encode(ctx.handle, level, _ptr(a), a.size, out.ctypes.data, cap_)
    if r < 0:
        _raise(r, ctx)
    return out[:r].tobytes()


def AppendEncoded(dst, src, level=LevelFastest, ctx=None):
    """encode.go:144-162"""
    return bytes(dst) + Encode(src, level, ctx)


def TryEncode(src, level=LevelFastest, ctx=None):
    """encode.go:168-206: None when incompressible."""
    a = _np(src)
    if MaxEncodedLen(a.size) < 0 or a.size < 16 or level not in (LevelSuperFast, LevelFastest, LevelBalanced):
        return None
    e = Encode(a, level, ctx)
    if len(e) >= 2 and e[0] == 0 and e[1] == 0:
        return None
    return e if len(e) < a.size else None


def Decode(src, ctx=None, guard=0):
    """minlz.Decode(nil, src), decode.go:50-78."""
    ctx = ctx or default_context()
    a = _np(src)
    n = DecodedLen(a)
    out = np.full(n + guard, 0xA5, dtype=np.uint8)
    if a.size and a[0] != 0 and not (a.size == 1):
        raise ErrUnsupported("Snappy/S2 fallback block")
    r = _lib.lib().mlz_decode(ctx.handle, _ptr(a), a.size, out.ctypes.data, n)
    if guard and not (out[n:] == 0xA5).all():
        raise AssertionError("decoder wrote past dst")
    if r < 0:
        _raise(r, ctx)
    return out[:r].tobytes()


def AppendDecoded(dst, src, ctx=None):
    """decode.go:85-103"""
    return bytes(dst) + Decode(src, ctx)


def crc(b, ctx=None):
    """crc(b) of minlz.go:133-140 (masked CRC32C), computed on the device."""
    ctx = ctx or default_context()
    a = _np(b)
    r = _lib.lib().mlz_crc(ctx.handle, _ptr(a), a.size)
    if r < 0:
        _raise(r, ctx)
    return int(r)


def encode_block(src, level=LevelFastest, ctx=None):
    """encodeBlock(dst, src) / WriterCustomEncoder contract (writer.go:1293-1304): tokens only; b'' = incompressible."""
    ctx = ctx or default_context()
    a = _np(src)
    out = np.empty(a.size + 16, dtype=np.uint8)
    r = _lib.lib().mlz_encode_block(ctx.handle, level, _ptr(a), a.size, out.ctypes.data, out.size)
    if r < 0:
        _raise(r, ctx)
    return out[:r].tobytes()


def decode_block(body, dlen, ctx=None):
    """minLZDecode(dst[:dlen], body) (decode.go:178): returns (code, bytes)."""
    ctx = ctx or default_context()
    a = _np(body)
    out = np.zeros(max(dlen, 1), dtype=np.uint8)
    r = _lib.lib().mlz_decode_block(ctx.handle, _ptr(a), a.size, out.ctypes.data, dlen)
    if r < 0:
        _raise(r, ctx)
    return r, out[:dlen].tobytes()


def encode_batch(blocks, level=LevelFastest, ctx=None):
    """mlz_encode_batch over a list of byte blocks -> list of encoded blocks."""
    ctx = ctx or default_context()
    arrs = [_np(b) for b in blocks]
    n = len(arrs)
    outs = [np.empty(max(MaxEncodedLen(a.size), 1), dtype=np.uint8) for a in arrs]
    vp, sz = C.c_void_p, C.c_size_t
    srcp = (vp * n)(*[_ptr(a) for a in arrs]); srcl = (sz * n)(*[a.size for a in arrs])
    dstp = (vp * n)(*[o.ctypes.data for o in outs]); dstc = (sz * n)(*[o.size for o in outs])
    ol = (C.c_int64 * n)()
    r = _lib.lib().mlz_encode_batch(ctx.handle, level, n, srcp, srcl, dstp, dstc, ol)
    if r:
        _raise(r, ctx)
    res = []
    for i in range(n):
        if ol[i] < 0:
            _raise(ol[i], ctx)
        res.append(outs[i][:ol[i]].tobytes())
    return res


def decode_batch(blocks, ctx=None):
    ctx = ctx or default_context()
    arrs = [_np(b) for b in blocks]
    n = len(arrs)
    lens = [DecodedLen(a) for a in arrs]
    outs = [np.empty(max(l, 1), dtype=np.uint8) for l in lens]
    vp, sz = C.c_void_p, C.c_size_t
    srcp = (vp * n)(*[_ptr(a) for a in arrs]); srcl = (sz * n)(*[a.size for a in arrs])
    dstp = (vp * n)(*[o.ctypes.data for o in outs]); dstc = (sz * n)(*lens)
    ol = (C.c_int64 * n)()
    r = _lib.lib().mlz_decode_batch(ctx.handle, n, srcp, srcl, dstp, dstc, ol)
    if r:
        _raise(r, ctx)
    res = []
    for i in range(n):
        if ol[i] < 0:
            _raise(ol[i], ctx)
        res.append(outs[i][:ol[i]].tobytes())
    return res


STREAM_ADD_INDEX, STREAM_IGNORE_CRC, STREAM_SEARCH_TABLES, SEARCH_NO_TABLES, GREP_INVERT = 1, 2, 4, 8, 16


def search_tables_config(match_len, prefix):
    """An mlz_search_tables for a set of prefix byte values: 1 to 8 distinct values -> table type 2 (sorted), more -> type 3 (the mask; an
    empty set too: the empty mask is valid and indexes nothing)."""
    vals = sorted({int(v) for v in prefix})
    if vals and (vals[0] < 0 or vals[-1] > 255):
        raise ValueError("search_prefix: byte values")
    cfg = _lib.SearchTables()
    cfg.match_len = match_len & 255
    if 1 <= len(vals) <= 8:
        cfg.table_type, cfg.n_prefix = 2, len(vals)
        for i, v in enumerate(vals):
            cfg.prefix[i] = v
    else:
        cfg.table_type = 3
        for v in vals:
            cfg.prefix[v >> 3] |= 1 << (v & 7)
    return cfg


def search_long_prefix_config(match_len, prefix, extras=0):
    """An mlz_search_long_prefix (table type 4): a prefix of 1 .. 256 bytes, match length 0 (= 6) .. 8, extras 0 .. 15 with match length +
    extras <= 16.  ValueError outside these ranges."""
    pfx = bytes(prefix)
    match_len, extras = int(match_len), int(extras)
    if not 1 <= len(pfx) <= 256:
        raise ValueError("search_long_prefix: 1 .. 256 bytes")
    if not 0 <= match_len <= 8:
        raise ValueError("search_match_len: 0 .. 8")
    if not 0 <= extras <= 15 or (match_len or 6) + extras > 16:
        raise ValueError("search_extras: 0 .. 15, match length + extras <= 16")
    cfg = _lib.SearchLongPrefix()
    cfg.match_len, cfg.extras, cfg.prefix_len = match_len, extras, len(pfx)
    for i, v in enumerate(pfx):
        cfg.prefix[i] = v
    return cfg


def search_config(table_type, match_len=None, prefix=b"", extras=0):
    """An mlz_search_config, one table configuration of a sidecar (DeviceReader.build_sidecar).  table_type 1: no prefix; 2: `prefix` holds
    1 .. 8 byte values, kept in the order given; 3: `prefix` holds the byte values of the set (any number; the 256-bit mask is made here);
    4: `prefix` is the long prefix of 1 .. 256 bytes, `extras` 0 .. 15 with match length + extras <= 16.  match_len None or 0 = 6."""
    table_type, match_len, extras, pfx = int(table_type), int(match_len or 0), int(extras), bytes(prefix)
    if not 1 <= table_type <= 4:
        raise ValueError("search_config: table type 1 .. 4")
    if not 0 <= match_len <= 8:
        raise ValueError("search_match_len: 0 .. 8")
    if table_type != 4 and extras:
        raise ValueError("search_extras: table type 4 only")
    cfg = _lib.SearchConfig()
    cfg.table_type, cfg.match_len, cfg.extras = table_type, match_len, extras
    if table_type == 2:
        if not 1 <= len(pfx) <= 8:
            raise ValueError("search_config: type 2 takes 1 .. 8 byte values")
        cfg.prefix_len = len(pfx)
        for i, v in enumerate(pfx):
            cfg.prefix[i] = v
    elif table_type == 3:
        for v in pfx:
            cfg.prefix[v >> 3] |= 1 << (v & 7)
    elif table_type == 4:
        if not 1 <= len(pfx) <= 256:
            raise ValueError("search_long_prefix: 1 .. 256 bytes")
        if not 0 <= extras <= 15 or (match_len or 6) + extras > 16:
            raise ValueError("search_extras: 0 .. 15, match length + extras <= 16")
        cfg.prefix_len = len(pfx)
        for i, v in enumerate(pfx):
            cfg.prefix[i] = v
    return cfg


def stream_encode(src, level=LevelFastest, block_size=2 << 20, add_index=False, ctx=None):
    """mlz_stream_encode: NewWriter(...).EncodeBuffer(src) + Close() in one call -> the .mz stream bytes."""
    ctx = ctx or default_context()
    a = _np(src)
    flags = STREAM_ADD_INDEX if add_index else 0
    cap = _lib.lib().mlz_stream_bound(a.size, block_size, flags)
    if cap < 0:
        _raise(cap, ctx)
    out = np.empty(cap, dtype=np.uint8)
    r = _lib.lib().mlz_stream_encode(ctx.handle, level, block_size, flags, _ptr(a), a.size, out.ctypes.data, out.size)
    if r < 0:
        _raise(r, ctx)
    return out[:r].tobytes()


def stream_decode(src, ignore_crc=False, ctx=None):
    """mlz_stream_decode: NewReader(src) read to EOF -> decoded bytes."""
    ctx = ctx or default_context()
    a = _np(src)
    n = _lib.lib().mlz_stream_decoded_len(_ptr(a), a.size)
    if n < 0:   # a framing error: the chunks in front of it are decoded first, and their first error wins (stream order)
        n = _lib.lib().mlz_stream_decoded_prefix_len(_ptr(a), a.size)
    out = np.empty(max(n, 1), dtype=np.uint8)
    r = _lib.lib().mlz_stream_decode(ctx.handle, STREAM_IGNORE_CRC if ignore_crc else 0, _ptr(a), a.size, out.ctypes.data, n)
    if r < 0:
        _raise(r, ctx)
    return out[:r].tobytes()
