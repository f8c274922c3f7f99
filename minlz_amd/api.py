"""Block API mirror of the reference (encode.go:74-244, decode.go:50-156) over the C ABI."""
import collections
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import BlockDesc

# ---- the constants of include/minlz_hip.h (tests/test_abi.py holds every one against its #define) ----
LevelSuperFast, LevelUncompressed, LevelFastest, LevelBalanced = -1, 0, 1, 2  # encode.go:25-43 (LevelSmallest = 3 is CPU-only)
MaxBlockSize = 8 << 20  # minlz.go:84

ERR_CORRUPT, ERR_TOO_LARGE, ERR_UNSUPPORTED, ERR_INVALID_LEVEL, ERR_CRC, ERR_DST_TOO_SMALL, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5, 6, 7, 8

STREAM_ADD_INDEX, STREAM_IGNORE_CRC, STREAM_SEARCH_TABLES, SEARCH_NO_TABLES, GREP_INVERT = 1, 2, 4, 8, 16
IGNORE_CASE = 32                  # MLZ_SEARCH_IGNORE_CASE: the searches' ignore_case=True
COMPRESS_TABLES = 64              # MLZ_STREAM_SEARCH_COMPRESS: the device Writer's search_compress=True
SEARCH_MAX_PATTERNS = 4096
REGEX_IGNORE_CASE = 1             # MLZ_REGEX_IGNORE_CASE (include/minlz_hip_regex.h): Regex(..., ignore_case=True)
REGEX_MAX_RECORD = 1 << 20        # MLZ_REGEX_MAX_RECORD: the longest record grep_regex accepts

OPT_DECODE_ALGO, OPT_ENCODE_FAR, OPT_DEBUG_STATUS, OPT_PROFILE, OPT_PROFILE_READ, OPT_TILE_TIMELINE_READ, OPT_GENERAL_ALGO = 1, 2, 3, 4, 5, 7, 8
OPT_GEN_SPIN, OPT_HOST_GROUP_ENC, OPT_HOST_GROUP_DEC, OPT_TIMER_MASK, OPT_GEN_PACKED, OPT_L2_FREE, OPT_DEVICE_GROUP = 9, 10, 11, 12, 13, 14, 17
OPT_FAR_SLICES_L2, OPT_L2_GAP, OPT_GEN_SETTLE_CAP, OPT_FUSED_SERIALIZER, OPT_LEVEL0_KERNEL, OPT_FOLD_LAYOUT = 18, 19, 20, 21, 23, 24
OPT_TIMING = 100  # MLZ_TIMER_ENABLE

# mlz_get_counter(ctx, which): the header numbers them without names
COUNTER_COMBINE_BATCHES = 0       # batches run by the combining queue of the single-block host calls
COUNTER_COMBINE_REQUESTS = 1      # requests that queue served
COUNTER_GENERAL_BLOCKS = 2        # blocks of the last decode call that went through the general-block path
COUNTER_ENCODE_WORKSPACE = 3      # bytes of device workspace held for encoding (grow-only)
COUNTER_DECODE_WORKSPACE = 4      # bytes of device workspace held for decoding (grow-only)
COUNTER_GENERAL_FALLBACKS = 5     # decode calls whose general blocks fell back to the tile chain
COUNTER_GENERAL_TEAM = 6          # workgroups per block (1, 2 or 4) of the last decode call's general-block pass; 0 = no general block
COUNTER_RANGE_CHUNKS = 7          # chunks the last range read decoded or copied
COUNTER_RANGE_SCRATCH_BYTES = 8   # decoded bytes it put into the scratch
COUNTER_RANGE_HOST_BYTES = 9      # bytes of plan data that crossed between host and device in the last read_device
COUNTER_SEARCH_CHUNKS = 10        # chunks the last search decoded or copied
COUNTER_SEARCH_TABLES = 11        # chunks with a usable search table in the last search
COUNTER_BATCH_LONG_STREAMS = 12   # streams the last stream batch call sent through the region walk (more than 4096 chunk headers)


class MinLZError(Exception):
    code = 0


class ErrCorrupt(MinLZError):
    """minlz: corrupt input (decode.go:31)"""
    code = ERR_CORRUPT


class ErrTooLarge(MinLZError):
    """minlz: decoded block is too large (decode.go:35)"""
    code = ERR_TOO_LARGE


class ErrUnsupported(MinLZError):
    """minlz: unsupported input (decode.go:37)"""
    code = ERR_UNSUPPORTED


class ErrInvalidLevel(MinLZError):
    """minlz: invalid compression level (decode.go:39)"""
    code = ERR_INVALID_LEVEL


class ErrCRC(MinLZError):
    """minlz: corrupt input, crc mismatch (decode.go:33)"""
    code = ERR_CRC


class ErrHIP(MinLZError):
    code = ERR_HIP


# mlz_sidecar_extract_result (include/minlz_hip_sidecar_extract.h), what DeviceReader.extract_sidecar returns
SidecarExtract = collections.namedtuple("SidecarExtract", "side_len main_len blocks info_chunks tables tables_compressed passed_bytes dropped_bytes")

_ERRS = {e.code: e for e in (ErrCorrupt, ErrTooLarge, ErrUnsupported, ErrInvalidLevel, ErrCRC, ErrHIP)}


def _error(code, before="", after=""):
    """The exception of the (positive) error code: its class, "minlz error <code>" between the two texts."""
    return _ERRS.get(code, MinLZError)("%sminlz error %d%s" % (before, code, after))


def _raise(code, ctx=None):
    code = -code if code < 0 else code
    raise _error(code, after=" " + (_lib.lib().mlz_last_error(ctx.handle).decode() if ctx is not None and code == ERR_HIP else ""))


# ---- argument marshalling, each form once ----

def _flags(add_index=False, ignore_crc=False, no_tables=False, invert=False, ignore_case=False):
    return ((STREAM_ADD_INDEX if add_index else 0) | (STREAM_IGNORE_CRC if ignore_crc else 0) | (SEARCH_NO_TABLES if no_tables else 0) | (GREP_INVERT if invert else 0) |
            (IGNORE_CASE if ignore_case else 0))


def _patterns(patterns):
    """A sequence of bytes objects -> (their bytes back to back, their uint32 lengths, their number): the three arguments of the ABI."""
    pats = [bytes(p) for p in patterns]
    return (b"".join(pats), (C.c_uint32 * len(pats))(*[len(p) for p in pats]), len(pats)) if pats else (None, None, 0)


def _delimiter(d, what):
    d = bytes(d) if not isinstance(d, int) else bytes([d])
    if len(d) != 1:
        raise ValueError(what + ": a delimiter of one byte")
    return d[0]


def _block_descs(descs):
    """A BlockDesc array as it is, or a sequence of BlockDesc or of tuples (src_off, src_len[, dst_off, dst_cap]) -> the array of as many."""
    if isinstance(descs, C.Array):
        return descs
    return (BlockDesc * len(descs))(*[d if isinstance(d, BlockDesc) else BlockDesc(*[int(v) for v in (tuple(d) + (0, 0))[:4]]) for d in descs])


def _stats():
    return (C.c_uint64 * 4)()


def _ints(a, n=4):
    return tuple(int(a[i]) for i in range(n))


class Regex:
    """mlz_regex: regular expressions over bytes (a bytes object, or a sequence of up to 256 of them: grep -E -e a -e b) compiled on the host
    into one search automaton, for DeviceReader.grep_regex.  The syntax is the subset of Python's `re` on bytes that
    include/minlz_hip_regex.h lists; ignore_case: re.IGNORECASE on bytes.  Needs no context and no GPU.  A context manager; close() frees it.
    A syntax error raises MinLZError and a refused construct or a limit ErrUnsupported, with the expression's index and the offset."""

    def __init__(self, exprs, ignore_case=False):
        self.handle = C.c_void_p()
        exprs = [bytes(exprs)] if isinstance(exprs, (bytes, bytearray, memoryview)) else [bytes(e) for e in exprs]
        where = (C.c_uint64 * 2)()
        blob, lens, n = _patterns(exprs)
        r = _lib.lib().mlz_regex_compile(blob, lens, n, REGEX_IGNORE_CASE if ignore_case else 0, C.byref(self.handle), where)
        if r < 0:
            self.handle = C.c_void_p()
            raise _error(-r, "Regex: ", " in expression %d at offset %d" % (where[0], where[1]))

    def _open(self):
        if not self.handle:
            raise ValueError("Regex is closed")
        return self.handle

    def info(self):
        """mlz_regex_info -> (states, byte classes, bytes of class map and table as the kernel holds them, whether the empty record matches)."""
        info = _stats()
        _lib.lib().mlz_regex_info(self._open(), info)
        return int(info[0]), int(info[1]), int(info[2]), bool(info[3] & 1)

    def literals(self):
        """mlz_regex_literals (include/minlz_hip_regex_prune.h) -> (the required literals, a sorted list of bytes objects of which every matching record
        holds one, empty: none; whether they are folded: under ignore_case the record with A - Z folded to a - z holds one)."""
        info = _stats()
        n = _lib.lib().mlz_regex_literals(self._open(), None, 0, None, 0, info)
        lens, buf = (C.c_uint32 * max(n, 1))(), (C.c_uint8 * max(int(info[1]), 1))()
        _lib.lib().mlz_regex_literals(self._open(), buf, int(info[1]), lens, n, info)
        blob, at, out = bytes(buf), 0, []
        for i in range(n):
            out.append(blob[at:at + lens[i]])
            at += lens[i]
        return out, bool(info[3] & 1)

    def test(self, record):
        """mlz_regex_test: does `record` hold a match, by the rule the kernel runs."""
        rec = bytes(record)
        return _lib.lib().mlz_regex_test(self._open(), rec, len(rec)) == 1

    def close(self):
        if self.handle:
            _lib.lib().mlz_regex_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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

    def _call(self, name, *args):
        """The ABI function `name` on this context -> its result; a negative one raises its error."""
        r = getattr(_lib.lib(), name)(self.handle, *args)
        if r < 0:
            _raise(r, self)
        return int(r)

    def device_count(self):
        return self._call("mlz_device_count")

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
        self._call("mlz_set_option", opt, int(value))

    def device_name(self):
        buf = C.create_string_buffer(256)
        _lib.lib().mlz_device_name(self.handle, buf, 256)
        return buf.value.decode()

    def timers(self):
        arr = (C.c_float * 16)()
        n = _lib.lib().mlz_get_timers(self.handle, arr, 16)
        return {_lib.lib().mlz_timer_name(i).decode(): arr[i] for i in range(n) if arr[i] >= 0}

    def counter(self, which):
        """mlz_get_counter: one of COUNTER_*."""
        return int(_lib.lib().mlz_get_counter(self.handle, which))

    def combine_stats(self):
        """(batches run, requests served) by the combining queue of the single-block host calls."""
        return self.counter(COUNTER_COMBINE_BATCHES), self.counter(COUNTER_COMBINE_REQUESTS)

    def workspace_bytes(self):
        """(encode side, decode side): device workspace the context holds — grow-only, i.e. the high-water mark of its calls (mlz_get_counter 3, 4)."""
        return self.counter(COUNTER_ENCODE_WORKSPACE), self.counter(COUNTER_DECODE_WORKSPACE)

    def general_blocks(self):
        """Blocks of the last decode call that took the path for streams of other encoders (mlz_get_counter 2)."""
        return self.counter(COUNTER_GENERAL_BLOCKS)

    def general_team(self):
        """Workgroups per block (1, 2 or 4) the general-block pass of the last decode call settled with; 0 = no general block (mlz_get_counter 6)."""
        return self.counter(COUNTER_GENERAL_TEAM)

    def batch_long_streams(self):
        """Streams that the context's last stream batch call walked by the region kernels: more than 4096 chunk headers (mlz_get_counter 12)."""
        return self.counter(COUNTER_BATCH_LONG_STREAMS)

    def range_plan(self):
        """(chunks decoded or copied, decoded bytes put into the scratch) by the context's last DeviceReader.read (mlz_get_counter 7, 8)."""
        return self.counter(COUNTER_RANGE_CHUNKS), self.counter(COUNTER_RANGE_SCRATCH_BYTES)

    def search_plan(self):
        """(chunks decoded or copied, chunks with a usable search table) of the context's last DeviceReader.search, search_many, grep_records or grep_regex (mlz_get_counter 10, 11)."""
        return self.counter(COUNTER_SEARCH_CHUNKS), self.counter(COUNTER_SEARCH_TABLES)

    def search_compressed_tables(self):
        """Of the chunks with a usable search table in the context's last search, those whose table came from a compressed table chunk, 0x46
        (mlz_get_counter 14)."""
        return self.counter(_lib.COUNTER_SEARCH_COMPRESSED)

    @property
    def tables_written_compressed(self):
        """Table chunks the context's last stream_encode_gather_device or build_sidecar wrote compressed, as 0x46 (mlz_get_counter 15)."""
        return self.counter(_lib.COUNTER_TABLES_COMPRESSED)

    @property
    def table_slot_bytes(self):
        """Bytes of workspace the context's last stream_encode_batch_device with search tables carved for its blocks' tables: 2^(B - r0 - 3) per
        block of a stream that had room, r0 = the folds the block's length makes certain (mlz_get_counter 17)."""
        return self.counter(_lib.COUNTER_TABLE_SLOT_BYTES)

    def range_plan_host_bytes(self):
        """Bytes of plan data that crossed between host and device, both directions together, in the context's last DeviceReader.read_device
        (mlz_get_counter 9): a header and two records per TOUCHED CHUNK, nothing per range."""
        return self.counter(COUNTER_RANGE_HOST_BYTES)

    def release_stream(self, stream):
        """mlz_release_stream: call before destroying a stream that carried a *_batch_device call of this context."""
        self._call("mlz_release_stream", stream)

    def stream_encode_gather_device(self, level, block_size, add_index, d_srcs, lens, d_dst, dst_cap, search_match_len=None, search_prefix=None,
                                    search_long_prefix=None, search_extras=0, search_compress=False):
        """mlz_stream_encode_gather_device: ranges of one stream resident on the context's devices -> the framed stream in d_dst (device memory).
        search_match_len: None = no search tables; 0 = block search tables with the reference's default match length (6); 1 .. 8 = with that one.
        search_prefix (with search_match_len): an iterable of byte values; the tables then index only the positions behind one of them
        (mlz_stream_encode_gather_device_tables: 1 to 8 distinct values give table type 2, in sorted order, more give type 3).
        search_long_prefix (with search_match_len, not with search_prefix): 1 .. 256 bytes; the tables then index the search_extras + 1
        windows behind every occurrence of that byte string (mlz_stream_encode_gather_device_long_prefix, table type 4; search_extras 0 .. 15,
        match length + extras <= 16).
        search_compress (MLZ_STREAM_SEARCH_COMPRESS, with any of these tables): a table's chunk is written compressed (0x46) where that is
        smaller; the property tables_written_compressed then says how many were.
        Returns the stream size."""
        n = len(d_srcs)
        suffix, flags, cfg = _writer_tables(search_match_len, search_prefix, search_long_prefix, search_extras)
        flags |= COMPRESS_TABLES if search_compress else 0
        return self._call("mlz_stream_encode_gather_device" + suffix, level, block_size, _flags(add_index=add_index) | flags, *cfg,
                          (C.c_void_p * n)(*d_srcs), (C.c_size_t * n)(*lens), n, d_dst, dst_cap)

    # ---- device-resident batch calls: pointers are raw device addresses (e.g. tensor.data_ptr()) ----
    # (the three block calls are the benchmark's step: the ctypes call and its check stand here themselves, nothing between them and the caller)
    def encode_batch_device(self, stream, level, d_src, d_dst, descs, d_out_len):
        arr = descs if isinstance(descs, C.Array) else _block_descs(descs)
        r = _lib.lib().mlz_encode_batch_device(self.handle, stream, level, d_src, d_dst, arr, len(arr), d_out_len)
        if r:
            _raise(r, self)

    def crc_batch_device(self, stream, d_base, descs, d_out_u32):
        arr = descs if isinstance(descs, C.Array) else _block_descs(descs)
        r = _lib.lib().mlz_crc_batch_device(self.handle, stream, d_base, arr, len(arr), d_out_u32)
        if r:
            _raise(r, self)

    def decode_batch_device(self, stream, d_src, d_dst, descs, d_out_len):
        arr = descs if isinstance(descs, C.Array) else _block_descs(descs)
        r = _lib.lib().mlz_decode_batch_device(self.handle, stream, d_src, d_dst, arr, len(arr), d_out_len)
        if r:
            _raise(r, self)

    def search_bitmaps_compress_device(self, d_src, d_dst, descs, d_len, stream=None):
        """mlz_search_bitmaps_compress_device (include/minlz_hip_search_compress.h): every bitmap (src_off, src_len, dst_off, dst_cap) of the
        buffer at d_src -> the huff0 section of its compressed chunk at its place in the buffer at d_dst, by kernels; d_len: device memory
        of one int64 per item, which receives the section's length or the item's own -MLZ_ERR_*.  Returns when the kernels have run."""
        arr = _block_descs(descs)
        self._call("mlz_search_bitmaps_compress_device", stream, d_src, d_dst, arr, len(arr), d_len)

    def stream_decoded_len_device(self, d_src, n, stream=None):
        """mlz_stream_decoded_len_device: the chunk walk of a stream in device memory -> (result, prefix_len).  `result` is the raw return
        value (the decoded size, or -MLZ_ERR_* for a framing error: nothing is raised, so that a caller can size the output for the prefix)."""
        prefix = C.c_uint64(0)
        r = _lib.lib().mlz_stream_decoded_len_device(self.handle, stream, d_src, n, C.byref(prefix))
        return int(r), int(prefix.value)

    def stream_decode_device(self, d_src, n, d_dst, dst_cap, ignore_crc=False, stream=None):
        """mlz_stream_decode_device: NewReader(src) read to EOF, source and destination in device memory -> decoded size."""
        return self._call("mlz_stream_decode_device", stream, _flags(ignore_crc=ignore_crc), d_src, n, d_dst, dst_cap)

    # ---- batches of streams in device memory: one call for many streams; per-stream results come back as lists, nothing is raised per stream ----
    def stream_decoded_len_batch_device(self, d_src, spans, stream=None):
        """mlz_stream_decoded_len_batch_device: the chunk walk of every stream (src_off, src_len) of the buffer at d_src ->
        [(result, prefix_len)], each as stream_decoded_len_device gives it for that stream alone."""
        arr = _block_descs(spans)
        n = len(arr)
        out = (C.c_int64 * max(n, 1))()
        prefix = (C.c_uint64 * max(n, 1))()
        self._call("mlz_stream_decoded_len_batch_device", stream, d_src, arr, n, out, prefix)
        return [(int(out[i]), int(prefix[i])) for i in range(n)]

    def stream_decode_batch_device(self, d_src, d_dst, descs, ignore_crc=False, stream=None):
        """mlz_stream_decode_batch_device: every stream (src_off, src_len, dst_off, dst_cap) of the buffer at d_src decoded to its place in the
        buffer at d_dst -> [result]: the decoded size or -MLZ_ERR_* of each stream, as mlz_stream_decode_device returns it for that stream alone."""
        arr = _block_descs(descs)
        n = len(arr)
        out = (C.c_int64 * max(n, 1))()
        self._call("mlz_stream_decode_batch_device", stream, _flags(ignore_crc=ignore_crc), d_src, d_dst, arr, n, out)
        return [int(out[i]) for i in range(n)]

    def stream_encode_batch_device(self, level, block_size, add_index, d_src, d_dst, descs, stream=None, flags=0, search_match_len=None, search_prefix=None,
                                   search_long_prefix=None, search_extras=0):
        """mlz_stream_encode_batch_device: every input (src_off, src_len, dst_off, dst_cap) of the buffer at d_src written as a stream of its own to
        its place in the buffer at d_dst -> [result]: the stream's size or -MLZ_ERR_* of each.  flags: further MLZ_STREAM_* bits, as they are.
        The search_* keywords are stream_encode_gather_device's: with search_match_len every stream carries block search tables of that one
        configuration (mlz_stream_encode_batch_device_tables, include/minlz_hip_encode_batch_tables.h), byte for byte those of the gather
        Writer on that input alone; api.stream_bound with the same keywords is a stream's room; table_slot_bytes then says what the tables
        took of workspace."""
        arr = _block_descs(descs)
        n = len(arr)
        out = (C.c_int64 * max(n, 1))()
        cfg = batch_tables_config(search_match_len, search_prefix, search_long_prefix, search_extras)
        if cfg is None:
            self._call("mlz_stream_encode_batch_device", stream, level, block_size, _flags(add_index=add_index) | flags, d_src, d_dst, arr, n, out)
        else:
            self._call("mlz_stream_encode_batch_device_tables", stream, level, block_size, _flags(add_index=add_index) | flags, C.byref(cfg), d_src, d_dst, arr, n, out)
        return [int(out[i]) for i in range(n)]

    def stream_search_batch_device(self, d_src, spans, patterns, d_stream_counts=None, d_pattern_counts=None, d_present=None, d_hit_stream=None, d_hit_pos=None,
                                   d_hit_which=None, cap=0, ignore_crc=False, ignore_case=False, stream=None, flags=0, prune=False):
        """mlz_stream_search_batch_device: every stream (src_off, src_len) of the buffer at d_src searched for `patterns` (1 .. 4096 bytes objects
        of 1 .. 256 bytes) in one call.  Device addresses or None: d_stream_counts (n uint64), d_pattern_counts (one uint64 per pattern),
        d_present (n rows of ceil(patterns / 32) uint32: bit p of row i = pattern p occurs in stream i), d_hit_stream / d_hit_pos / d_hit_which
        (room for `cap` uint32 / uint64 / uint32: the smallest min(total, cap) triples in (stream, position, pattern) order).
        flags: further MLZ_* bits, as they are.
        prune: mlz_stream_search_batch_device_pruned (include/minlz_hip_search_batch_prune.h) — only the chunks that the streams' inline block
        search tables cannot rule out are decoded; four more stats: chunks with a usable table in a pruned stream, streams of which nothing
        was decoded, configuration classes found, streams decoded whole.
        -> (total triples over the healthy streams, [result]: the occurrences in each stream or its -MLZ_ERR_*, stats): stats = (data chunks,
        chunks decoded over all passes, streams that failed in the decode, scan passes), and with prune=True four values more (chunks with a
        usable table in a pruned stream, streams of which no chunk was decoded although they hold bytes, configuration classes found, streams
        that hold bytes and are decoded whole).  counter(16) then is the bytes the plan brought to the host, the classes' configurations apart."""
        arr = _block_descs(spans)
        n = len(arr)
        out, stats = (C.c_int64 * max(n, 1))(), (C.c_uint64 * 8)() if prune else _stats()
        r = self._call("mlz_stream_search_batch_device_pruned" if prune else "mlz_stream_search_batch_device", stream, _flags(ignore_crc=ignore_crc, ignore_case=ignore_case) | flags, d_src, arr, n, *_patterns(patterns), out,
                       d_stream_counts, d_pattern_counts, d_present, d_hit_stream, d_hit_pos, d_hit_which, cap, stats)
        return r, [int(out[i]) for i in range(n)], _ints(stats, 8 if prune else 4)

    def record_index_build_device(self, d_raw, n, delimiter, d_dst, dst_cap, stream=None):
        """mlz_record_index_build_device (include/minlz_hip_record_index_store.h): the record index blob of the n raw bytes at device address d_raw for
        the one-byte `delimiter`, unbound, into dst_cap bytes at d_dst (record_index_bound(n) always suffices) — the index of a stream made while
        the same bytes go to the device Writer.  -> (the blob's bytes, (bytes, sections, sparse tiles, dense tiles))."""
        info = _stats()
        r = self._call("mlz_record_index_build_device", stream, d_raw, n, _delimiter(delimiter, "record_index_build_device"), d_dst, dst_cap, info)
        return r, _ints(info)

    def stream_open_device(self, d_src, n, stream=None):
        """mlz_stream_open_device: a stream in device memory opened for range reads -> DeviceReader.  The caller keeps d_src alive and unchanged
        while the reader is open.  A stream with a framing error raises that error (no reader)."""
        h = C.c_void_p()
        return DeviceReader(self, h, self._call("mlz_stream_open_device", stream, d_src, n, C.byref(h)))

    def stream_open_batch_device(self, d_src, spans, stream=None, tables=False):
        """mlz_stream_open_batch_device (include/minlz_hip_stream_set.h): every stream (src_off, src_len) of the buffer at d_src opened as ONE
        reader over the streams' decoded bytes one behind the other -> (DeviceReader, [result]: the decoded size or the framing error
        -MLZ_ERR_* of each stream; a failed one is left out of the reader).  The caller keeps d_src alive and unchanged while it is open.
        tables: mlz_stream_open_batch_device_tables (include/minlz_hip_stream_set_tables.h) — the reader's searches prune by every stream's
        inline search tables, with the same results."""
        arr = _block_descs(spans)
        n = len(arr)
        out = (C.c_int64 * max(n, 1))()
        h = C.c_void_p()
        size = self._call("mlz_stream_open_batch_device_tables" if tables else "mlz_stream_open_batch_device", stream, d_src, arr, n, out, C.byref(h))
        return DeviceReader(self, h, size), [int(out[i]) for i in range(n)]


class DeviceReader:
    """mlz_dev_reader: the device-resident ReadSeeker of one stream (Context.stream_open_device) or of a set of streams
    (Context.stream_open_batch_device).  A context manager; close() frees it."""

    def __init__(self, ctx, handle, size):
        self.ctx, self.handle, self.size = ctx, handle, size

    def _open(self):
        if not self.handle:
            raise ValueError("DeviceReader is closed")
        return self.handle

    def _call(self, name, *args):
        """The ABI function `name` on this reader -> its result; a closed reader is refused, a negative result raises its error."""
        handle = self._open()
        r = getattr(_lib.lib(), name)(handle, *args)
        if r < 0:
            _raise(r, self.ctx)
        return int(r)

    def read(self, ranges, d_dst, dst_cap, ignore_crc=False, stream=None):
        """mlz_dev_reader_read.  ranges: (off, len, dst_off) triples, or a C-contiguous uint64 array of shape (k, 3): decoded bytes
        [off, off + len) go to d_dst[dst_off, dst_off + len).  -> the sum of the lengths."""
        a = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 3)
        return self._call("mlz_dev_reader_read", stream, _flags(ignore_crc=ignore_crc), _ptr(a), a.shape[0], d_dst, dst_cap)

    def read_device(self, d_off, d_len, n, d_dst, dst_cap, d_starts=None, ignore_crc=False, stream=None):
        """mlz_dev_reader_read_device.  d_off, d_len: device addresses of n uint64 offsets and lengths; decoded bytes [off[i], off[i] + len[i])
        go to d_dst packed in the order given; d_starts (device address of n + 1 uint64, or None) receives where each range starts and the
        total.  -> the sum of the lengths."""
        return self._call("mlz_dev_reader_read_device", stream, _flags(ignore_crc=ignore_crc), d_off, d_len, n, d_dst, dst_cap, d_starts)

    def search(self, pattern, d_offsets, cap, ignore_crc=False, no_tables=False, stream=None, ignore_case=False):
        """mlz_dev_reader_search.  pattern: 1 .. 256 bytes; d_offsets: device address of room for `cap` uint64 (None with cap == 0), which
        receives the smallest min(total, cap) positions of the pattern in the decoded stream, ascending.
        Uses the stream's block search tables of type 1, 2, 3 or 4 (with a prefix table: the pattern's windows that follow a prefix byte; a
        pattern without one is served by decoding every chunk, and the usable-table count is then 0).
        ignore_case (here and in the three calls below): grep -i in the C locale — the result is that of the call on the stream and the
        pattern with A .. Z folded to a .. z; the stream is not changed.  Windows of the pattern with more than three letters cannot be
        pruned by the tables.
        -> (total, (data chunks, chunks decoded or copied, chunks with a usable search table))."""
        p, stats = bytes(pattern), _stats()
        r = self._call("mlz_dev_reader_search", stream, _flags(ignore_crc=ignore_crc, no_tables=no_tables, ignore_case=ignore_case), p, len(p), d_offsets, cap, stats)
        return r, _ints(stats, 3)

    def search_many(self, patterns, d_counts, d_offsets, d_which, cap, ignore_crc=False, no_tables=False, stream=None, ignore_case=False):
        """mlz_dev_reader_search_many.  patterns: a sequence of up to 4096 bytes objects of 1 .. 256 bytes; d_counts: device address of room
        for len(patterns) uint64 (or None), which receives every pattern's number of occurrences; d_offsets, d_which: device addresses of
        room for `cap` uint64 and `cap` uint32 (None with cap == 0), which receive the smallest min(total, cap) pairs (position, pattern
        index) in ascending order.  The chunks that any pattern's tables admit are decoded once and scanned once for all patterns.
        -> (total pairs, (data chunks, chunks decoded or copied, chunks with a usable search table, patterns the tables could not serve))."""
        stats = _stats()
        r = self._call("mlz_dev_reader_search_many", stream, _flags(ignore_crc=ignore_crc, no_tables=no_tables, ignore_case=ignore_case), *_patterns(patterns), d_counts, d_offsets, d_which, cap, stats)
        return r, _ints(stats)

    def search_records(self, pattern, delimiter, d_dst, dst_cap, d_rec_off, d_rec_start, d_rec_flags, rec_cap, max_reach=0, ignore_crc=False, no_tables=False, stream=None,
                       ignore_case=False):
        """mlz_dev_reader_search_records: the records (maximal runs without the byte `delimiter`) that hold `pattern` (1 .. 256 bytes without
        the delimiter), each once, in stream order.  d_dst: device address of room for dst_cap bytes (None with dst_cap == 0), which
        receives the first k records' bytes, packed; d_rec_off: room for rec_cap uint64 (None with rec_cap == 0), each record's start in
        the decoded stream; d_rec_start: room for rec_cap + 1 uint64 or None, each record's start in d_dst and the bytes written;
        d_rec_flags: room for rec_cap bytes or None, bit 0 = cut left, bit 1 = cut right.  k: the most records that both caps hold whole.
        max_reach: how far the call looks to either side of an occurrence (0 = 65536, at most 2^20); longer records come out cut.
        ignore_case: the records come out with their original bytes; a delimiter that is an ASCII letter raises.
        -> (records, (records, bytes of all records, occurrences, records with a flag), (data chunks, chunks decoded or copied by the
        search phase, chunks with a usable search table))."""
        self._open()
        p, totals, stats = bytes(pattern), _stats(), _stats()
        r = self._call("mlz_dev_reader_search_records", stream, _flags(ignore_crc=ignore_crc, no_tables=no_tables, ignore_case=ignore_case), p, len(p), _delimiter(delimiter, "search_records"),
                       max_reach, d_dst, dst_cap, d_rec_off, d_rec_start, d_rec_flags, rec_cap, totals, stats)
        return r, _ints(totals), _ints(stats, 3)

    def index_records(self, delimiter=b"\n", ignore_crc=False, stream=None):
        """mlz_dev_reader_index_records: builds the record index for the one-byte `delimiter` — the positions of all delimiters of the
        decoded stream, 8 bytes each in device memory the handle owns — by one decode of the stream.  Record r is the bytes between
        delimiter r - 1 and delimiter r; empty records count; a stream that ends without a delimiter has one more record.  The same
        delimiter again costs nothing; another one replaces the index.
        -> (N, (N, delimiters, bytes of index held, chunks this call decoded))."""
        self._open()
        info = _stats()
        r = self._call("mlz_dev_reader_index_records", stream, _flags(ignore_crc=ignore_crc), _delimiter(delimiter, "index_records"), info)
        return r, _ints(info)

    def record_count(self):
        """mlz_dev_reader_record_count: the records of the indexed stream; raises without an index."""
        return self._call("mlz_dev_reader_record_count")

    def record_spans(self, d_idx, n, d_off, d_len, stream=None):
        """mlz_dev_reader_record_spans.  d_idx: device address of n uint64 record numbers (any order, repeats allowed); d_off, d_len:
        device addresses of room for n uint64 each, which receive every record's first byte in the decoded stream and its length.
        -> the sum of the lengths.  A number >= record_count() raises."""
        return self._call("mlz_dev_reader_record_spans", stream, d_idx, n, d_off, d_len)

    def read_records(self, d_idx, n, d_dst, dst_cap, d_starts=None, ignore_crc=False, stream=None):
        """mlz_dev_reader_read_records: the records d_idx[0 .. n) (device address of uint64 record numbers) packed into d_dst in the order
        given; d_starts (device address of n + 1 uint64, or None) receives where each record starts in d_dst and the total.  Only the
        chunks the records touch are decoded, each once.  -> the bytes written.  A number >= record_count() or a total above dst_cap
        raises, and nothing has been written then."""
        return self._call("mlz_dev_reader_read_records", stream, _flags(ignore_crc=ignore_crc), d_idx, n, d_dst, dst_cap, d_starts)

    def record_numbers(self, d_pos, n, d_no, stream=None):
        """mlz_dev_reader_record_numbers.  d_pos: device address of n uint64 positions of the decoded stream; d_no: room for n uint64, which
        receive each position's record number (0-based; a delimiter has the number of the record it ends; 2^64 - 1 for a position at or
        beyond the size).  -> how many positions lie inside the stream."""
        return self._call("mlz_dev_reader_record_numbers", stream, d_pos, n, d_no)

    def grep_records(self, patterns, d_rec_no, d_rec_kind, rec_cap, invert=False, before=0, after=0, ignore_crc=False, no_tables=False, stream=None, ignore_case=False):
        """mlz_dev_reader_grep_records: grep over the record index.  patterns: a sequence of up to 4096 bytes objects of 1 .. 256 bytes
        without the index's delimiter (none: nothing matches, and under invert every record is selected); a record is selected when it
        holds one of them, with invert when it holds none; before, after: context records in front of and behind every selected one.
        ignore_case: grep -i; an index built on an ASCII letter raises.
        d_rec_no: device address of room for rec_cap uint64 (None with rec_cap == 0), which receives the smallest min(R, rec_cap) numbers
        of the selected and context records, ascending; d_rec_kind: room for rec_cap bytes or None, 1 = selected, 0 = context only.
        -> (R, (R, selected records, bytes of the written records: read_records' dst_cap, bytes of all R records), (data chunks, chunks
        decoded or copied, chunks with a usable search table, patterns the tables could not serve))."""
        totals, stats = _stats(), _stats()
        r = self._call("mlz_dev_reader_grep_records", stream, _flags(ignore_crc=ignore_crc, no_tables=no_tables, invert=invert, ignore_case=ignore_case), *_patterns(patterns), before, after,
                       d_rec_no, d_rec_kind, rec_cap, totals, stats)
        return r, _ints(totals), _ints(stats)

    def grep_regex(self, regex, d_rec_no, d_rec_kind, rec_cap, invert=False, before=0, after=0, ignore_crc=False, stream=None, prune=False, no_tables=False):
        """mlz_dev_reader_grep_regex: grep_records with the selected records decided by `regex` (a Regex): a record is selected when its
        bytes, the delimiter excluded, hold a match (an empty record: when the expression matches the empty string), with invert when they
        hold none.  d_rec_no, d_rec_kind, rec_cap, before and after as in grep_records.  Every chunk is decoded once; an index with a
        record longer than REGEX_MAX_RECORD raises ErrUnsupported before that.
        prune: mlz_dev_reader_grep_regex_pruned (include/minlz_hip_regex_prune.h), the same results from the chunks that the search tables admit
        for the expression's required literals (Regex.literals) and those that complete their records; no_tables (with prune only) decodes every chunk.
        -> (R, (R, selected records, bytes of the written records, bytes of all R records), (data chunks, chunks decoded, 0, 0)); with prune the
        last two are the chunks with a usable table and the chunks the plan took before it was widened to whole records."""
        self._open()
        totals, stats = _stats(), _stats()
        if no_tables and not prune:
            raise ValueError("grep_regex: no_tables goes with prune=True")
        r = self._call("mlz_dev_reader_grep_regex_pruned" if prune else "mlz_dev_reader_grep_regex", stream, _flags(ignore_crc=ignore_crc, invert=invert, no_tables=no_tables), regex._open(),
                       before, after, d_rec_no, d_rec_kind, rec_cap, totals, stats)
        return r, _ints(totals), _ints(stats)

    def record_range(self, first, count):
        """mlz_dev_reader_record_range: records first .. first + count - 1 as one byte range, the delimiters between them included
        -> (off, len), to be read with read().  first + count > record_count() raises."""
        off, ln = C.c_uint64(), C.c_uint64()
        self._call("mlz_dev_reader_record_range", first, count, C.byref(off), C.byref(ln))
        return int(off.value), int(ln.value)

    # ---- a set of streams behind the reader (include/minlz_hip_stream_set.h); a reader of one stream answers as a set of one ----
    def stream_count(self):
        """mlz_dev_reader_stream_count: the streams the reader was opened with, failed ones included."""
        return self._call("mlz_dev_reader_stream_count")

    def stream_bases(self):
        """mlz_dev_reader_stream_bases -> the count + 1 bases: stream i's decoded bytes are [bases[i], bases[i + 1]) of the reader."""
        out = (C.c_uint64 * (self.stream_count() + 1))()
        self._call("mlz_dev_reader_stream_bases", out)
        return [int(v) for v in out]

    def locate(self, d_pos, n, d_which, d_local, stream=None):
        """mlz_dev_reader_locate.  d_pos: device address of n uint64 positions of the reader; d_which, d_local: room for n uint32 and n uint64,
        which receive each position's stream and the position inside it (0xFFFFFFFF and 0 at or beyond the size).  -> the positions inside."""
        return self._call("mlz_dev_reader_locate", stream, d_pos, n, d_which, d_local)

    def read_streams_device(self, d_which, d_off, d_len, n, d_dst, dst_cap, d_starts=None, ignore_crc=False, stream=None):
        """mlz_dev_reader_read_streams_device: read_device with range i = bytes [off[i], off[i] + len[i]) of stream which[i] (device addresses
        of n uint32, uint64, uint64).  A range that leaves its stream raises, and nothing has been written then.  -> the sum of the lengths."""
        return self._call("mlz_dev_reader_read_streams_device", stream, _flags(ignore_crc=ignore_crc), d_which, d_off, d_len, n, d_dst, dst_cap, d_starts)

    def stream_records(self, stream=None):
        """mlz_dev_reader_stream_records -> (first, joined): first[i] = the records that start in front of stream i (count + 1 values, the last
        is the record count); joined = the streams whose last record runs on into the next stream.  Raises without a record index."""
        first, joined = (C.c_uint64 * (self.stream_count() + 1))(), C.c_uint64()
        self._call("mlz_dev_reader_stream_records", stream, first, C.byref(joined))
        return [int(v) for v in first], int(joined.value)

    def locate_records(self, d_rec_no, n, d_which, d_local_no, stream=None):
        """mlz_dev_reader_locate_records.  d_rec_no: device address of n uint64 record numbers; d_which, d_local_no: room for n uint32 and n
        uint64, which receive the stream each record starts in and its number inside that stream (0xFFFFFFFF and 0 at or beyond the record
        count).  -> the numbers in range.  Raises without a record index."""
        return self._call("mlz_dev_reader_locate_records", stream, d_rec_no, n, d_which, d_local_no)

    def set_tables_info(self):
        """mlz_dev_reader_set_tables_info (include/minlz_hip_stream_set_tables.h): the last plan on a set opened with tables=True ->
        (classes found, streams pruned by a class, streams with bytes decoded whole, chunks with a usable table in pruned streams, those of
        them from a compressed table chunk, stream ends treated as crossed, and behind these six the 0x46 tables that stand expanded in the
        reader's arenas, which stays as it is from the second search on): a 7-tuple.  Any other reader raises (error 8)."""
        out = (C.c_uint64 * 6)()
        expanded = self._call("mlz_dev_reader_set_tables_info", out)
        return tuple(int(v) for v in out) + (expanded,)

    @staticmethod
    def _configs(cfgs):
        cfgs = list(cfgs)
        arr = (_lib.SearchConfig * max(len(cfgs), 1))()
        for i, q in enumerate(cfgs):
            arr[i] = q
        return arr, len(cfgs)

    def sidecar_bound(self, cfgs):
        """mlz_dev_reader_sidecar_bound: room that always suffices for build_sidecar with these configurations (api.search_config)."""
        return self._call("mlz_dev_reader_sidecar_bound", *self._configs(cfgs))

    def build_sidecar(self, cfgs, d_dst, cap, ignore_crc=False, stream=None, compress=False):
        """mlz_dev_reader_build_sidecar: the sidecar of this stream for 1 .. 4 configurations (api.search_config) — search tables for every
        data chunk in a separate stream that names the chunks by remote references — into `cap` bytes at device address d_dst -> its size.
        compress (MLZ_STREAM_SEARCH_COMPRESS): a table's chunk is written compressed (0x46) where that is smaller."""
        return self._call("mlz_dev_reader_build_sidecar", stream, _flags(ignore_crc=ignore_crc) | (COMPRESS_TABLES if compress else 0), *self._configs(cfgs), d_dst, cap)

    def attach_sidecar(self, d_side, n, ignore_crc=False, stream=None):
        """mlz_dev_reader_attach_sidecar: search and search_many use the tables of the sidecar at device address d_side (n bytes) from now
        on.  The caller keeps those bytes alive and unchanged.  A sidecar that does not belong to this stream raises, and nothing changes."""
        self._call("mlz_dev_reader_attach_sidecar", stream, _flags(ignore_crc=ignore_crc), d_side, n)

    def detach_sidecar(self):
        """The searches use the stream's inline tables again."""
        self._call("mlz_dev_reader_attach_sidecar", None, 0, None, 0)

    def extract_sidecar_bound(self):
        """mlz_dev_reader_extract_sidecar_bound (include/minlz_hip_sidecar_extract.h) -> (side_cap, main_cap) that always suffice for extract_sidecar."""
        main = C.c_uint64(0)
        side = self._call("mlz_dev_reader_extract_sidecar_bound", C.byref(main))
        return side, int(main.value)

    def extract_sidecar(self, d_side, side_cap, d_main=None, main_cap=0, stream=None):
        """mlz_dev_reader_extract_sidecar: the search chunks this stream carries (0x44, 0x45, 0x46), copied as they are into a sidecar at device
        address d_side with one remote reference per data chunk; nothing is decoded.  With d_main the stream is also written there without its
        search and index chunks, with a fresh seek index, and the references name the offsets in d_main (which must not overlap the stream or
        d_side); without it they name the offsets in this stream.  -> SidecarExtract.  Room that is too small raises MinLZError (error 6) whose
        `needed` is (side_len, main_len)."""
        out = _lib.SidecarExtractResult()
        handle = self._open()
        r = _lib.lib().mlz_dev_reader_extract_sidecar(handle, stream, 0, d_side, side_cap, d_main, main_cap, C.byref(out))
        if r < 0:
            try:
                _raise(r, self.ctx)
            except MinLZError as e:
                e.needed = (int(out.side_len), int(out.main_len))
                raise
        return SidecarExtract(*(int(getattr(out, name)) for name in SidecarExtract._fields))

    def record_index_bound(self):
        """mlz_dev_reader_record_index_bound (include/minlz_hip_record_index_store.h): bytes that always suffice for save_record_index; raises without an index."""
        return self._call("mlz_dev_reader_record_index_bound")

    def save_record_index(self, d_dst, dst_cap, stream=None):
        """mlz_dev_reader_save_record_index: the handle's record index as a record index blob (about 2 bytes per record, bound to this stream) into
        dst_cap bytes at device address d_dst -> (the blob's bytes, (bytes, sections, sparse tiles, dense tiles))."""
        self._open()
        info = _stats()
        r = self._call("mlz_dev_reader_save_record_index", stream, d_dst, dst_cap, info)
        return r, _ints(info)

    def load_record_index(self, d_blob, n, ignore_crc=False, stream=None):
        """mlz_dev_reader_load_record_index: the record index blob of n bytes at device address d_blob becomes this handle's record index; nothing is
        decoded.  A blob that is malformed, fails a CRC or belongs to another stream raises, and the handle keeps the index it had.
        -> (N, (N, delimiters, bytes of index held, 0))."""
        self._open()
        info = _stats()
        r = self._call("mlz_dev_reader_load_record_index", stream, _flags(ignore_crc=ignore_crc), d_blob, n, info)
        return r, _ints(info)

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
    return (a.size > 0 and a[0] == 0), DecodedLen(a)


def Encode(src, level=LevelFastest, ctx=None):
    """minlz.Encode(nil, src, level), encode.go:74-139."""
    ctx = ctx or default_context()
    a = _np(src)
    cap_ = MaxEncodedLen(a.size)
    if cap_ < 0:
        raise ErrTooLarge()
    out = np.empty(cap_, dtype=np.uint8)
    return out[:ctx._call("mlz_encode", level, _ptr(a), a.size, out.ctypes.data, cap_)].tobytes()


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
    a = _np(b)
    return (ctx or default_context())._call("mlz_crc", _ptr(a), a.size)


def record_index_bound(n):
    """mlz_record_index_bound (include/minlz_hip_record_index_store.h): bytes that always suffice for Context.record_index_build_device over n raw
    bytes; host only."""
    r = _lib.lib().mlz_record_index_bound(n)
    if r < 0:
        _raise(r)
    return int(r)


def record_index_parse(blob):
    """mlz_record_index_parse: the header chunk and the directory of a record index blob in host memory, checked against its length; needs no
    context and no GPU -> a dict: flags, delimiter, size, k, N, longest (None when the blob does not know it), tag, data_chunks, nsections, bound.
    An unknown magic raises ErrUnsupported, a malformed blob ErrCorrupt, a stale header CRC ErrCRC."""
    a = _np(blob)
    info = (C.c_uint64 * 8)()
    r = _lib.lib().mlz_record_index_parse(_ptr(a) if a.size else info, a.size, info)
    if r < 0:
        _raise(r)
    flags, delimiter, size, k, N, longest, tag, chunks = (int(v) for v in info)
    return dict(flags=flags, delimiter=delimiter, size=size, k=k, N=N, longest=longest if flags & 2 else None, tag=tag, data_chunks=chunks, nsections=int(r), bound=bool(flags & 1))


def expand_search_table(body, ignore_crc=False):
    """mlz_search_table_expand (include/minlz_hip_search_compressed.h): the payload of a compressed block search table chunk (0x46) ->
    (R, the table's bytes), on the host; needs no context and no GPU.  A chunk that is refused raises ErrCorrupt, a stale CRC ErrCRC."""
    a = _np(body)
    R = C.c_uint32()
    out = np.empty(1 << 20, dtype=np.uint8)     # the largest table: 2^23 bits
    r = _lib.lib().mlz_search_table_expand(_ptr(a), a.size, out.ctypes.data, out.size, C.byref(R), _flags(ignore_crc=ignore_crc))
    if r < 0:
        _raise(r)
    return int(R.value), out[:r].tobytes()


def compress_search_bitmap(bitmap, cap=None):
    """mlz_search_bitmap_compress (include/minlz_hip_search_compress.h): a search table's bitmap (a power of two of 32 bytes to 1 MiB) -> the
    huff0 section of its compressed chunk (0x46): `h0_bs h0_tc | table descriptions | sub-blocks`, what stands behind the CRC.  On the
    host; needs no context and no GPU.  cap: the room offered (default: the largest section, n + 18).  A refused size raises MinLZError
    (code ERR_ARG), a cap below the section's length MinLZError (code ERR_DST_TOO_SMALL)."""
    a = _np(bitmap)
    out = np.empty(a.size + 18 if cap is None else max(int(cap), 1), dtype=np.uint8)
    r = _lib.lib().mlz_search_bitmap_compress(_ptr(a), a.size, out.ctypes.data, out.size if cap is None else int(cap))
    if r < 0:
        _raise(r)
    return out[:r].tobytes()


def encode_block(src, level=LevelFastest, ctx=None):
    """encodeBlock(dst, src) / WriterCustomEncoder contract (writer.go:1293-1304): tokens only; b'' = incompressible."""
    a = _np(src)
    out = np.empty(a.size + 16, dtype=np.uint8)
    return out[:(ctx or default_context())._call("mlz_encode_block", level, _ptr(a), a.size, out.ctypes.data, out.size)].tobytes()


def decode_block(body, dlen, ctx=None):
    """minLZDecode(dst[:dlen], body) (decode.go:178): returns (code, bytes)."""
    a = _np(body)
    out = np.zeros(max(dlen, 1), dtype=np.uint8)
    return (ctx or default_context())._call("mlz_decode_block", _ptr(a), a.size, out.ctypes.data, dlen), out[:dlen].tobytes()


def _host_batch(ctx, name, lead, blocks, caps):
    """The host-pointer batch call `name` (arguments `lead` in front of the count) over `blocks`, block i into caps(block i) bytes of room
    -> the results' bytes; the first block that failed raises its error."""
    ctx = ctx or default_context()
    arrs = [_np(b) for b in blocks]
    n = len(arrs)
    caps = [caps(a) for a in arrs]
    outs = [np.empty(max(c, 1), dtype=np.uint8) for c in caps]
    vp, sz = C.c_void_p, C.c_size_t
    ol = (C.c_int64 * n)()
    ctx._call(name, *lead, n, (vp * n)(*[_ptr(a) for a in arrs]), (sz * n)(*[a.size for a in arrs]), (vp * n)(*[o.ctypes.data for o in outs]), (sz * n)(*caps), ol)
    for v in ol:
        if v < 0:
            _raise(v, ctx)
    return [o[:v].tobytes() for o, v in zip(outs, ol)]


def encode_batch(blocks, level=LevelFastest, ctx=None):
    """mlz_encode_batch over a list of byte blocks -> list of encoded blocks."""
    return _host_batch(ctx, "mlz_encode_batch", (level,), blocks, lambda a: max(MaxEncodedLen(a.size), 1))


def decode_batch(blocks, ctx=None):
    return _host_batch(ctx, "mlz_decode_batch", (), blocks, DecodedLen)


# ---- search table configurations ----

def _put_prefix(cfg, pfx, mask=False):
    """The prefix field of a configuration: the bytes as they come, or (mask) the 256-bit set of their values."""
    for i, v in enumerate(pfx):
        if mask:
            cfg.prefix[v >> 3] |= 1 << (v & 7)
        else:
            cfg.prefix[i] = v
    return len(pfx)


def _check_ranges(match_len, long_prefix=None, extras=0):
    """The ranges of the match length and, for a long prefix (table type 4), of its length and the extras."""
    if long_prefix is not None and not 1 <= len(long_prefix) <= 256:
        raise ValueError("search_long_prefix: 1 .. 256 bytes")
    if not 0 <= match_len <= 8:
        raise ValueError("search_match_len: 0 .. 8")
    if long_prefix is not None and (not 0 <= extras <= 15 or (match_len or 6) + extras > 16):
        raise ValueError("search_extras: 0 .. 15, match length + extras <= 16")


def search_tables_config(match_len, prefix):
    """An mlz_search_tables for a set of prefix byte values: 1 to 8 distinct values -> table type 2 (sorted), more -> type 3 (the mask; an
    empty set too: the empty mask is valid and indexes nothing)."""
    vals = sorted({int(v) for v in prefix})
    if vals and (vals[0] < 0 or vals[-1] > 255):
        raise ValueError("search_prefix: byte values")
    cfg = _lib.SearchTables()
    cfg.match_len = match_len & 255
    if 1 <= len(vals) <= 8:
        cfg.table_type, cfg.n_prefix = 2, _put_prefix(cfg, vals)
    else:
        cfg.table_type = 3
        _put_prefix(cfg, vals, mask=True)
    return cfg


def search_long_prefix_config(match_len, prefix, extras=0):
    """An mlz_search_long_prefix (table type 4): a prefix of 1 .. 256 bytes, match length 0 (= 6) .. 8, extras 0 .. 15 with match length +
    extras <= 16.  ValueError outside these ranges."""
    pfx, match_len, extras = bytes(prefix), int(match_len), int(extras)
    _check_ranges(match_len, pfx, extras)
    cfg = _lib.SearchLongPrefix()
    cfg.match_len, cfg.extras, cfg.prefix_len = match_len, extras, _put_prefix(cfg, pfx)
    return cfg


def search_config(table_type, match_len=None, prefix=b"", extras=0):
    """An mlz_search_config, one table configuration of a sidecar (DeviceReader.build_sidecar).  table_type 1: no prefix; 2: `prefix` holds
    1 .. 8 byte values, kept in the order given; 3: `prefix` holds the byte values of the set (any number; the 256-bit mask is made here);
    4: `prefix` is the long prefix of 1 .. 256 bytes, `extras` 0 .. 15 with match length + extras <= 16.  match_len None or 0 = 6."""
    table_type, match_len, extras, pfx = int(table_type), int(match_len or 0), int(extras), bytes(prefix)
    if not 1 <= table_type <= 4:
        raise ValueError("search_config: table type 1 .. 4")
    _check_ranges(match_len)
    if table_type != 4 and extras:
        raise ValueError("search_extras: table type 4 only")
    cfg = _lib.SearchConfig()
    cfg.table_type, cfg.match_len, cfg.extras = table_type, match_len, extras
    if table_type == 2 and not 1 <= len(pfx) <= 8:
        raise ValueError("search_config: type 2 takes 1 .. 8 byte values")
    if table_type == 4:
        _check_ranges(match_len, pfx, extras)
    if table_type == 3:
        _put_prefix(cfg, pfx, mask=True)
    elif table_type != 1:
        cfg.prefix_len = _put_prefix(cfg, pfx)
    return cfg


def _writer_tables(search_match_len, search_prefix, search_long_prefix, search_extras):
    """The Writer's search keywords -> (which C entry points: the suffix of mlz_stream_bound and mlz_stream_encode_gather_device, their
    search flags, their config argument: a tuple of one or none)."""
    if search_long_prefix is not None:
        if search_prefix is not None:
            raise ValueError("search_long_prefix and search_prefix exclude each other")
        if search_match_len is None:
            raise ValueError("search_long_prefix needs search_match_len")
        return "_long_prefix", 0, (C.byref(search_long_prefix_config(search_match_len, search_long_prefix, search_extras)),)
    if search_extras:
        raise ValueError("search_extras needs search_long_prefix")
    if search_prefix is not None:
        if search_match_len is None:
            raise ValueError("search_prefix needs search_match_len")
        return "_tables", 0, (C.byref(search_tables_config(search_match_len, search_prefix)),)
    return "", 0 if search_match_len is None else STREAM_SEARCH_TABLES | (search_match_len & 15) << 8, ()


def batch_tables_config(search_match_len=None, search_prefix=None, search_long_prefix=None, search_extras=0):
    """The Writer's search keywords -> the mlz_search_config of Context.stream_encode_batch_device, None without tables.  The table type is
    chosen as the gather Writer chooses it: no prefix -> 1; 1 to 8 distinct prefix byte values -> 2 (sorted), more or none -> 3; a long
    prefix -> 4."""
    suffix, _, _ = _writer_tables(search_match_len, search_prefix, search_long_prefix, search_extras)   # (the keywords' own checks)
    if search_match_len is None:
        return None
    if suffix == "_long_prefix":
        return search_config(4, search_match_len, search_long_prefix, search_extras)
    if suffix == "":
        return search_config(1, search_match_len)
    t = search_tables_config(search_match_len, search_prefix)
    cfg = _lib.SearchConfig()
    cfg.table_type, cfg.match_len, cfg.prefix_len = t.table_type, t.match_len, t.n_prefix
    for i in range(32):
        cfg.prefix[i] = t.prefix[i]
    return cfg


def stream_bound(n, block_size, add_index=False, search_match_len=None, search_prefix=None, search_long_prefix=None, search_extras=0, search_compress=False):
    """mlz_stream_bound, _tables or _long_prefix: the room that always suffices for a stream of n bytes written with these settings (the
    search keywords are Context.stream_encode_gather_device's; search_compress changes nothing: a compressed table chunk is only written
    where it is smaller).  Host only; raises for a block size or a configuration the Writer refuses."""
    suffix, flags, cfg = _writer_tables(search_match_len, search_prefix, search_long_prefix, search_extras)
    flags |= COMPRESS_TABLES if search_compress else 0
    r = getattr(_lib.lib(), "mlz_stream_bound" + suffix)(n, block_size, _flags(add_index=add_index) | flags, *cfg)
    if r < 0:
        _raise(r)
    return int(r)


def stream_encode(src, level=LevelFastest, block_size=2 << 20, add_index=False, ctx=None):
    """mlz_stream_encode: NewWriter(...).EncodeBuffer(src) + Close() in one call -> the .mz stream bytes."""
    ctx = ctx or default_context()
    a = _np(src)
    out = np.empty(stream_bound(a.size, block_size, add_index), dtype=np.uint8)
    return out[:ctx._call("mlz_stream_encode", level, block_size, _flags(add_index=add_index), _ptr(a), a.size, out.ctypes.data, out.size)].tobytes()


def stream_decode(src, ignore_crc=False, ctx=None):
    """mlz_stream_decode: NewReader(src) read to EOF -> decoded bytes."""
    ctx = ctx or default_context()
    a = _np(src)
    n = _lib.lib().mlz_stream_decoded_len(_ptr(a), a.size)
    if n < 0:   # a framing error: the chunks in front of it are decoded first, and their first error wins (stream order)
        n = _lib.lib().mlz_stream_decoded_prefix_len(_ptr(a), a.size)
    out = np.empty(max(n, 1), dtype=np.uint8)
    return out[:ctx._call("mlz_stream_decode", _flags(ignore_crc=ignore_crc), _ptr(a), a.size, out.ctypes.data, n)].tobytes()
