"""ctypes binding of the C ABI declared in include/minlz_hip.h and its extension headers include/minlz_hip_search_batch.h, include/minlz_hip_search_batch_prune.h, include/minlz_hip_stream_set.h, include/minlz_hip_stream_set_tables.h, include/minlz_hip_regex.h, include/minlz_hip_regex_prune.h, include/minlz_hip_search_compressed.h, include/minlz_hip_search_compress.h, include/minlz_hip_sidecar_extract.h, include/minlz_hip_record_index_store.h and include/minlz_hip_encode_batch_tables.h.

There is no CPU fallback here: if libminlz_hip.so is missing or HIP is unavailable, calls raise.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MINLZ_HIP_LIB: development override used by tools/ to time experimental builds of the same library
SO = os.environ.get("MINLZ_HIP_LIB") or os.path.join(HERE, "libminlz_hip.so")


class Range(C.Structure):
    """mlz_range: decoded bytes [off, off + len) -> d_dst[dst_off, dst_off + len)."""
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64), ("dst_off", C.c_uint64)]


class SearchTables(C.Structure):
    """mlz_search_tables: table type 1, 2 (n_prefix byte values in prefix) or 3 (prefix = a 256-bit mask), match length (0 = 6)."""
    _fields_ = [("table_type", C.c_uint8), ("match_len", C.c_uint8), ("n_prefix", C.c_uint8), ("reserved", C.c_uint8), ("prefix", C.c_uint8 * 32)]


class SearchLongPrefix(C.Structure):
    """mlz_search_long_prefix: table type 4, a prefix of 1 .. 256 bytes, match length (0 = 6) and extras (0 .. 15, match_len + extras <= 16)."""
    _fields_ = [("match_len", C.c_uint8), ("extras", C.c_uint8), ("prefix_len", C.c_uint16), ("reserved", C.c_uint8 * 4), ("prefix", C.c_uint8 * 256)]


class SearchConfig(C.Structure):
    """mlz_search_config: one table configuration of a sidecar, any table type 1 .. 4."""
    _fields_ = [("table_type", C.c_uint8), ("match_len", C.c_uint8), ("extras", C.c_uint8), ("reserved", C.c_uint8), ("prefix_len", C.c_uint16),
                ("reserved2", C.c_uint8 * 2), ("prefix", C.c_uint8 * 256)]


class SidecarExtractResult(C.Structure):
    """mlz_sidecar_extract_result (include/minlz_hip_sidecar_extract.h)."""
    _fields_ = [(name, C.c_uint64) for name in ("side_len", "main_len", "blocks", "info_chunks", "tables", "tables_compressed", "passed_bytes", "dropped_bytes")]


class BlockDesc(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint64), ("dst_off", C.c_uint64), ("dst_cap", C.c_uint64)]


vp, sz, i32, i64, u8, u32, u64, cstr = C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_uint8, C.c_uint32, C.c_uint64, C.c_char_p
P = C.POINTER

# The ABI: every function include/minlz_hip.h declares, in its order -> (restype, argtypes).  tests/test_abi.py holds the names and the
# argument counts against the header.
ABI = {
    "mlz_init": (i32, [i32, P(vp)]),
    "mlz_destroy": (None, [vp]),
    "mlz_init_devices": (i32, [P(i32), i32, P(vp)]),
    "mlz_device_count": (i32, [vp]),
    "mlz_device_ctx": (vp, [vp, i32]),
    "mlz_last_error": (cstr, [vp]),
    "mlz_version": (i32, []),
    "mlz_device_name": (i32, [vp, cstr, sz]),
    "mlz_max_encoded_len": (i64, [u64]),
    "mlz_decoded_len": (i64, [vp, sz]),
    "mlz_encode": (i64, [vp, i32, vp, sz, vp, sz]),
    "mlz_decode": (i64, [vp, vp, sz, vp, sz]),
    "mlz_encode_block": (i64, [vp, i32, vp, sz, vp, sz]),
    "mlz_decode_block": (i32, [vp, vp, sz, vp, sz]),
    "mlz_encode_batch": (i32, [vp, i32, i32, P(vp), P(sz), P(vp), P(sz), P(i64)]),
    "mlz_decode_batch": (i32, [vp, i32, P(vp), P(sz), P(vp), P(sz), P(i64)]),
    "mlz_release_stream": (i32, [vp, vp]),
    "mlz_encode_batch_device": (i32, [vp, vp, i32, vp, vp, P(BlockDesc), i32, vp]),
    "mlz_decode_batch_device": (i32, [vp, vp, vp, vp, P(BlockDesc), i32, vp]),
    "mlz_crc": (i64, [vp, vp, sz]),
    "mlz_crc_batch_device": (i32, [vp, vp, vp, P(BlockDesc), i32, vp]),
    "mlz_stream_bound": (i64, [u64, u32, u32]),
    "mlz_stream_encode": (i64, [vp, i32, u32, u32, vp, sz, vp, sz]),
    "mlz_stream_decoded_len": (i64, [vp, sz]),
    "mlz_stream_decoded_prefix_len": (i64, [vp, sz]),
    "mlz_stream_decode": (i64, [vp, u32, vp, sz, vp, sz]),
    "mlz_stream_encode_gather_device": (i64, [vp, i32, u32, u32, P(vp), P(sz), i32, vp, sz]),
    "mlz_stream_bound_tables": (i64, [u64, u32, u32, P(SearchTables)]),
    "mlz_stream_encode_gather_device_tables": (i64, [vp, i32, u32, u32, P(SearchTables), P(vp), P(sz), i32, vp, sz]),
    "mlz_stream_bound_long_prefix": (i64, [u64, u32, u32, P(SearchLongPrefix)]),
    "mlz_stream_encode_gather_device_long_prefix": (i64, [vp, i32, u32, u32, P(SearchLongPrefix), P(vp), P(sz), i32, vp, sz]),
    "mlz_stream_decoded_len_device": (i64, [vp, vp, vp, sz, P(u64)]),
    "mlz_stream_decode_device": (i64, [vp, vp, u32, vp, sz, vp, sz]),
    "mlz_stream_decoded_len_batch_device": (i32, [vp, vp, vp, P(BlockDesc), i32, P(i64), P(u64)]),
    "mlz_stream_decode_batch_device": (i32, [vp, vp, u32, vp, vp, P(BlockDesc), i32, P(i64)]),
    "mlz_stream_encode_batch_device": (i32, [vp, vp, i32, u32, u32, vp, vp, P(BlockDesc), i32, P(i64)]),
    "mlz_stream_open_device": (i64, [vp, vp, vp, sz, P(vp)]),
    "mlz_dev_reader_size": (i64, [vp]),
    "mlz_dev_reader_read": (i64, [vp, vp, u32, vp, sz, vp, sz]),
    "mlz_dev_reader_read_device": (i64, [vp, vp, u32, vp, vp, sz, vp, sz, vp]),
    "mlz_dev_reader_close": (None, [vp]),
    "mlz_dev_reader_search": (i64, [vp, vp, u32, vp, sz, vp, sz, P(u64)]),
    "mlz_dev_reader_search_many": (i64, [vp, vp, u32, vp, vp, sz, vp, vp, vp, sz, P(u64)]),
    "mlz_dev_reader_search_records": (i64, [vp, vp, u32, vp, sz, u8, u32, vp, sz, vp, vp, vp, sz, P(u64), P(u64)]),
    "mlz_dev_reader_index_records": (i64, [vp, vp, u32, u8, P(u64)]),
    "mlz_dev_reader_record_count": (i64, [vp]),
    "mlz_dev_reader_record_spans": (i64, [vp, vp, vp, sz, vp, vp]),
    "mlz_dev_reader_read_records": (i64, [vp, vp, u32, vp, sz, vp, sz, vp]),
    "mlz_dev_reader_record_numbers": (i64, [vp, vp, vp, sz, vp]),
    "mlz_dev_reader_record_range": (i64, [vp, u64, u64, P(u64), P(u64)]),
    "mlz_dev_reader_grep_records": (i64, [vp, vp, u32, vp, vp, sz, u64, u64, vp, vp, sz, P(u64), P(u64)]),
    "mlz_dev_reader_sidecar_bound": (i64, [vp, P(SearchConfig), i32]),
    "mlz_dev_reader_build_sidecar": (i64, [vp, vp, u32, P(SearchConfig), i32, vp, sz]),
    "mlz_dev_reader_attach_sidecar": (i64, [vp, vp, u32, vp, sz]),
    "mlz_set_option": (i32, [vp, i32, i64]),
    "mlz_get_timers": (i32, [vp, P(C.c_float), i32]),
    "mlz_timer_name": (cstr, [i32]),
    "mlz_get_counter": (i64, [vp, i32]),
}
SYMBOLS = list(ABI)

# The functions of the extension headers beside include/minlz_hip.h, header by header -> {name: (restype, argtypes)}, bound like the ABI's
# (tests/test_stream_search_batch_host.py and tests/test_stream_set_host.py hold the tables against the headers' prototypes)
ABI_EXT = {
    "minlz_hip_search_batch.h": {
        "mlz_stream_search_batch_device": (i64, [vp, vp, u32, vp, P(BlockDesc), i32, vp, vp, sz, P(i64), vp, vp, vp, vp, vp, vp, sz, P(u64)]),
    },
    "minlz_hip_search_batch_prune.h": {
        "mlz_stream_search_batch_device_pruned": (i64, [vp, vp, u32, vp, P(BlockDesc), i32, vp, vp, sz, P(i64), vp, vp, vp, vp, vp, vp, sz, P(u64)]),
    },
    "minlz_hip_stream_set.h": {
        "mlz_stream_open_batch_device": (i64, [vp, vp, vp, P(BlockDesc), i32, P(i64), P(vp)]),
        "mlz_dev_reader_stream_count": (i64, [vp]),
        "mlz_dev_reader_stream_bases": (i64, [vp, P(u64)]),
        "mlz_dev_reader_locate": (i64, [vp, vp, vp, sz, vp, vp]),
        "mlz_dev_reader_read_streams_device": (i64, [vp, vp, u32, vp, vp, vp, sz, vp, sz, vp]),
        "mlz_dev_reader_stream_records": (i64, [vp, vp, P(u64), P(u64)]),
        "mlz_dev_reader_locate_records": (i64, [vp, vp, vp, sz, vp, vp]),
    },
    "minlz_hip_stream_set_tables.h": {
        "mlz_stream_open_batch_device_tables": (i64, [vp, vp, vp, P(BlockDesc), i32, P(i64), P(vp)]),
        "mlz_dev_reader_set_tables_info": (i64, [vp, P(u64)]),
    },
    "minlz_hip_regex.h": {
        "mlz_regex_compile": (i32, [vp, vp, sz, u32, P(vp), P(u64)]),
        "mlz_regex_free": (None, [vp]),
        "mlz_regex_info": (i32, [vp, P(u64)]),
        "mlz_regex_test": (i32, [vp, vp, sz]),
        "mlz_dev_reader_grep_regex": (i64, [vp, vp, u32, vp, u64, u64, vp, vp, sz, P(u64), P(u64)]),
    },
    "minlz_hip_regex_prune.h": {
        "mlz_regex_literals": (i32, [vp, vp, sz, P(u32), sz, P(u64)]),
        "mlz_dev_reader_grep_regex_pruned": (i64, [vp, vp, u32, vp, u64, u64, vp, vp, sz, P(u64), P(u64)]),
    },
    "minlz_hip_search_compressed.h": {
        "mlz_search_table_expand": (i64, [vp, sz, vp, sz, P(u32), u32]),
    },
    "minlz_hip_search_compress.h": {
        "mlz_search_bitmap_compress": (i64, [vp, sz, vp, sz]),
        "mlz_search_bitmaps_compress_device": (i32, [vp, vp, vp, vp, P(BlockDesc), i32, vp]),
    },
    "minlz_hip_sidecar_extract.h": {
        "mlz_dev_reader_extract_sidecar_bound": (i64, [vp, P(u64)]),
        "mlz_dev_reader_extract_sidecar": (i64, [vp, vp, u32, vp, sz, vp, sz, P(SidecarExtractResult)]),
    },
    "minlz_hip_record_index_store.h": {
        "mlz_dev_reader_record_index_bound": (i64, [vp]),
        "mlz_dev_reader_save_record_index": (i64, [vp, vp, vp, sz, P(u64)]),
        "mlz_dev_reader_load_record_index": (i64, [vp, vp, u32, vp, sz, P(u64)]),
        "mlz_record_index_bound": (i64, [u64]),
        "mlz_record_index_build_device": (i64, [vp, vp, vp, sz, u8, vp, sz, P(u64)]),
        "mlz_record_index_parse": (i64, [vp, sz, P(u64)]),
    },
    "minlz_hip_encode_batch_tables.h": {
        "mlz_stream_bound_config": (i64, [u64, u32, u32, P(SearchConfig)]),
        "mlz_search_table_prefold": (i64, [u64, u32, u32]),
        "mlz_stream_encode_batch_device_tables": (i32, [vp, vp, i32, u32, u32, P(SearchConfig), vp, vp, P(BlockDesc), i32, P(i64)]),
    },
}

# mlz_get_counter(ctx, 14): of the chunks with a usable search table in the last search (counter 11), those whose table came from a compressed
# table chunk, 0x46 (api.Context.search_compressed_tables; the names of the counters 0 .. 12 stand in api)
COUNTER_SEARCH_COMPRESSED = 14
# mlz_get_counter(ctx, 15): table chunks the last device Writer or build_sidecar call wrote compressed, as 0x46 (api.Context.tables_written_compressed)
COUNTER_TABLES_COMPRESSED = 15
# mlz_get_counter(ctx, 17): bytes of table slots the last stream_encode_batch_device with search tables carved (api.Context.table_slot_bytes)
COUNTER_TABLE_SLOT_BYTES = 17

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError("minlz_amd: %s not built (run python -c 'import __graft_entry__ as g; g.build()')" % SO)
        L = C.CDLL(SO)
        # Under the development override a library from before an extension header loads without that header's functions (tools/ time the
        # parent commit's library against this tree's); calling one of them then raises AttributeError.  The tree's own library has them all.
        old = bool(os.environ.get("MINLZ_HIP_LIB"))
        for name, (restype, argtypes) in list(ABI.items()) + [kv for table in ABI_EXT.values() for kv in table.items()]:
            if old and name not in ABI and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib
