"""ctypes binding of the C ABI declared in include/minlz_hip.h.

There is no CPU fallback here: if libminlz_hip.so is missing or HIP is unavailable, calls raise.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MINLZ_HIP_LIB: development override used by tools/ to time experimental builds of the same library
SO = os.environ.get("MINLZ_HIP_LIB") or os.path.join(HERE, "libminlz_hip.so")

# every symbol include/minlz_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "mlz_init", "mlz_destroy", "mlz_last_error", "mlz_version", "mlz_device_name", "mlz_max_encoded_len",
    "mlz_decoded_len", "mlz_encode", "mlz_decode", "mlz_encode_block", "mlz_decode_block", "mlz_encode_batch",
    "mlz_decode_batch", "mlz_encode_batch_device", "mlz_decode_batch_device", "mlz_set_option", "mlz_get_timers",
    "mlz_timer_name", "mlz_crc", "mlz_crc_batch_device", "mlz_stream_bound", "mlz_stream_encode", "mlz_stream_decoded_len",
    "mlz_stream_decode", "mlz_get_counter", "mlz_init_devices", "mlz_device_count", "mlz_device_ctx",
    "mlz_stream_encode_gather_device", "mlz_release_stream", "mlz_stream_decoded_prefix_len",
    "mlz_stream_decoded_len_device", "mlz_stream_decode_device",
    "mlz_stream_decoded_len_batch_device", "mlz_stream_decode_batch_device", "mlz_stream_encode_batch_device",
    "mlz_stream_open_device", "mlz_dev_reader_size", "mlz_dev_reader_read", "mlz_dev_reader_close",
    "mlz_dev_reader_read_device", "mlz_dev_reader_search", "mlz_dev_reader_search_many",
    "mlz_stream_bound_tables", "mlz_stream_encode_gather_device_tables",
    "mlz_stream_bound_long_prefix", "mlz_stream_encode_gather_device_long_prefix",
    "mlz_dev_reader_sidecar_bound", "mlz_dev_reader_build_sidecar", "mlz_dev_reader_attach_sidecar",
    "mlz_dev_reader_search_records",
    "mlz_dev_reader_index_records", "mlz_dev_reader_record_count", "mlz_dev_reader_record_spans", "mlz_dev_reader_read_records",
    "mlz_dev_reader_record_numbers", "mlz_dev_reader_record_range",
    "mlz_dev_reader_grep_records",
]


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


class BlockDesc(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint64), ("dst_off", C.c_uint64), ("dst_cap", C.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        raise RuntimeError("minlz_amd: %s not built (run python -c 'import __graft_entry__ as g; g.build()')" % SO)
    L = C.CDLL(SO)
    vp, sz, i64, i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int
    L.mlz_init.argtypes = [i32, C.POINTER(vp)]; L.mlz_init.restype = i32
    L.mlz_destroy.argtypes = [vp]; L.mlz_destroy.restype = None
    L.mlz_init_devices.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]; L.mlz_init_devices.restype = i32
    L.mlz_device_count.argtypes = [vp]; L.mlz_device_count.restype = i32
    L.mlz_device_ctx.argtypes = [vp, i32]; L.mlz_device_ctx.restype = vp
    L.mlz_last_error.argtypes = [vp]; L.mlz_last_error.restype = C.c_char_p
    L.mlz_version.argtypes = []; L.mlz_version.restype = i32
    L.mlz_device_name.argtypes = [vp, C.c_char_p, sz]; L.mlz_device_name.restype = i32
    L.mlz_max_encoded_len.argtypes = [C.c_uint64]; L.mlz_max_encoded_len.restype = i64
    L.mlz_decoded_len.argtypes = [vp, sz]; L.mlz_decoded_len.restype = i64
    L.mlz_encode.argtypes = [vp, i32, vp, sz, vp, sz]; L.mlz_encode.restype = i64
    L.mlz_decode.argtypes = [vp, vp, sz, vp, sz]; L.mlz_decode.restype = i64
    L.mlz_encode_block.argtypes = [vp, i32, vp, sz, vp, sz]; L.mlz_encode_block.restype = i64
    L.mlz_decode_block.argtypes = [vp, vp, sz, vp, sz]; L.mlz_decode_block.restype = i32
    L.mlz_encode_batch.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i64)]
    L.mlz_encode_batch.restype = i32
    L.mlz_decode_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i64)]
    L.mlz_decode_batch.restype = i32
    L.mlz_encode_batch_device.argtypes = [vp, vp, i32, vp, vp, C.POINTER(BlockDesc), i32, vp]; L.mlz_encode_batch_device.restype = i32
    L.mlz_decode_batch_device.argtypes = [vp, vp, vp, vp, C.POINTER(BlockDesc), i32, vp]; L.mlz_decode_batch_device.restype = i32
    L.mlz_set_option.argtypes = [vp, i32, i64]; L.mlz_set_option.restype = i32
    L.mlz_release_stream.argtypes = [vp, vp]; L.mlz_release_stream.restype = i32
    L.mlz_get_timers.argtypes = [vp, C.POINTER(C.c_float), i32]; L.mlz_get_timers.restype = i32
    L.mlz_timer_name.argtypes = [i32]; L.mlz_timer_name.restype = C.c_char_p
    L.mlz_get_counter.argtypes = [vp, i32]; L.mlz_get_counter.restype = i64
    L.mlz_crc.argtypes = [vp, vp, sz]; L.mlz_crc.restype = i64
    L.mlz_crc_batch_device.argtypes = [vp, vp, vp, C.POINTER(BlockDesc), i32, vp]; L.mlz_crc_batch_device.restype = i32
    u32, u64 = C.c_uint32, C.c_uint64
    L.mlz_stream_bound.argtypes = [u64, u32, u32]; L.mlz_stream_bound.restype = i64
    L.mlz_stream_encode.argtypes = [vp, i32, u32, u32, vp, sz, vp, sz]; L.mlz_stream_encode.restype = i64
    L.mlz_stream_decoded_len.argtypes = [vp, sz]; L.mlz_stream_decoded_len.restype = i64
    L.mlz_stream_decoded_prefix_len.argtypes = [vp, sz]; L.mlz_stream_decoded_prefix_len.restype = i64
    L.mlz_stream_encode_gather_device.argtypes = [vp, i32, u32, u32, C.POINTER(vp), C.POINTER(sz), i32, vp, sz]
    L.mlz_stream_encode_gather_device.restype = i64
    L.mlz_stream_bound_tables.argtypes = [u64, u32, u32, C.POINTER(SearchTables)]; L.mlz_stream_bound_tables.restype = i64
    L.mlz_stream_encode_gather_device_tables.argtypes = [vp, i32, u32, u32, C.POINTER(SearchTables), C.POINTER(vp), C.POINTER(sz), i32, vp, sz]
    L.mlz_stream_encode_gather_device_tables.restype = i64
    L.mlz_stream_bound_long_prefix.argtypes = [u64, u32, u32, C.POINTER(SearchLongPrefix)]; L.mlz_stream_bound_long_prefix.restype = i64
    L.mlz_stream_encode_gather_device_long_prefix.argtypes = [vp, i32, u32, u32, C.POINTER(SearchLongPrefix), C.POINTER(vp), C.POINTER(sz), i32, vp, sz]
    L.mlz_stream_encode_gather_device_long_prefix.restype = i64
    L.mlz_stream_decode.argtypes = [vp, u32, vp, sz, vp, sz]; L.mlz_stream_decode.restype = i64
    L.mlz_stream_decoded_len_device.argtypes = [vp, vp, vp, sz, C.POINTER(u64)]; L.mlz_stream_decoded_len_device.restype = i64
    L.mlz_stream_decode_device.argtypes = [vp, vp, u32, vp, sz, vp, sz]; L.mlz_stream_decode_device.restype = i64
    L.mlz_stream_decoded_len_batch_device.argtypes = [vp, vp, vp, C.POINTER(BlockDesc), i32, C.POINTER(i64), C.POINTER(u64)]
    L.mlz_stream_decoded_len_batch_device.restype = i32
    L.mlz_stream_decode_batch_device.argtypes = [vp, vp, u32, vp, vp, C.POINTER(BlockDesc), i32, C.POINTER(i64)]; L.mlz_stream_decode_batch_device.restype = i32
    L.mlz_stream_encode_batch_device.argtypes = [vp, vp, i32, u32, u32, vp, vp, C.POINTER(BlockDesc), i32, C.POINTER(i64)]
    L.mlz_stream_encode_batch_device.restype = i32
    L.mlz_stream_open_device.argtypes = [vp, vp, vp, sz, C.POINTER(vp)]; L.mlz_stream_open_device.restype = i64
    L.mlz_dev_reader_size.argtypes = [vp]; L.mlz_dev_reader_size.restype = i64
    L.mlz_dev_reader_read.argtypes = [vp, vp, u32, vp, sz, vp, sz]; L.mlz_dev_reader_read.restype = i64
    L.mlz_dev_reader_close.argtypes = [vp]; L.mlz_dev_reader_close.restype = None
    L.mlz_dev_reader_read_device.argtypes = [vp, vp, u32, vp, vp, sz, vp, sz, vp]; L.mlz_dev_reader_read_device.restype = i64
    L.mlz_dev_reader_search.argtypes = [vp, vp, u32, vp, sz, vp, sz, C.POINTER(u64)]; L.mlz_dev_reader_search.restype = i64
    L.mlz_dev_reader_search_many.argtypes = [vp, vp, u32, vp, vp, sz, vp, vp, vp, sz, C.POINTER(u64)]; L.mlz_dev_reader_search_many.restype = i64
    L.mlz_dev_reader_sidecar_bound.argtypes = [vp, C.POINTER(SearchConfig), i32]; L.mlz_dev_reader_sidecar_bound.restype = i64
    L.mlz_dev_reader_build_sidecar.argtypes = [vp, vp, u32, C.POINTER(SearchConfig), i32, vp, sz]; L.mlz_dev_reader_build_sidecar.restype = i64
    L.mlz_dev_reader_attach_sidecar.argtypes = [vp, vp, u32, vp, sz]; L.mlz_dev_reader_attach_sidecar.restype = i64
    L.mlz_dev_reader_search_records.argtypes = [vp, vp, u32, vp, sz, C.c_uint8, u32, vp, sz, vp, vp, vp, sz, C.POINTER(u64), C.POINTER(u64)]
    L.mlz_dev_reader_search_records.restype = i64
    L.mlz_dev_reader_index_records.argtypes = [vp, vp, u32, C.c_uint8, C.POINTER(u64)]; L.mlz_dev_reader_index_records.restype = i64
    L.mlz_dev_reader_record_count.argtypes = [vp]; L.mlz_dev_reader_record_count.restype = i64
    L.mlz_dev_reader_record_spans.argtypes = [vp, vp, vp, sz, vp, vp]; L.mlz_dev_reader_record_spans.restype = i64
    L.mlz_dev_reader_read_records.argtypes = [vp, vp, u32, vp, sz, vp, sz, vp]; L.mlz_dev_reader_read_records.restype = i64
    L.mlz_dev_reader_record_numbers.argtypes = [vp, vp, vp, sz, vp]; L.mlz_dev_reader_record_numbers.restype = i64
    L.mlz_dev_reader_record_range.argtypes = [vp, u64, u64, C.POINTER(u64), C.POINTER(u64)]; L.mlz_dev_reader_record_range.restype = i64
    L.mlz_dev_reader_grep_records.argtypes = [vp, vp, u32, vp, vp, sz, u64, u64, vp, vp, sz, C.POINTER(u64), C.POINTER(u64)]
    L.mlz_dev_reader_grep_records.restype = i64
    _lib = L
    return L
