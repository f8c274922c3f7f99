"""The Python binding without a GPU: the public surface, the closed reader, api.stream_bound against the C functions and the three
configuration builders against the bytes they have always produced."""
import ctypes as C
import inspect
import types

import pytest

import minlz_amd
from minlz_amd import _build, _lib, api, shard


def surface(module):
    return {n for n in dir(module) if not n.startswith("_") and not isinstance(getattr(module, n), types.ModuleType)}


API_SURFACE = """AppendDecoded AppendEncoded BlockDesc Context Decode DecodedLen DeviceReader Encode ErrCRC ErrCorrupt ErrHIP ErrInvalidLevel ErrTooLarge
ErrUnsupported GREP_INVERT IsMinLZ LevelBalanced LevelFastest LevelSuperFast LevelUncompressed MaxBlockSize MaxEncodedLen MinLZError OPT_DECODE_ALGO
OPT_DEVICE_GROUP OPT_ENCODE_FAR OPT_GEN_PACKED OPT_GEN_SPIN OPT_L2_FREE OPT_L2_GAP OPT_TIMING SEARCH_NO_TABLES STREAM_ADD_INDEX STREAM_IGNORE_CRC
STREAM_SEARCH_TABLES TryEncode crc decode_batch decode_block default_context encode_batch encode_block search_config search_long_prefix_config
search_tables_config stream_decode stream_encode""".split()
SHARD_SURFACE = """DeviceStream HipTensorCodec cut_blocks decode_span_device decode_stream_sharded_device encode_stream_sharded
encode_stream_sharded_device finish_gather frame_run gather_chunk_sizes gather_sizes my_blocks owner plan_decode range_of start_gather""".split()


def test_public_surface_is_kept():
    """The public names the package, api and shard had before the binding was folded: all still there."""
    assert len(API_SURFACE) == 47 and len(SHARD_SURFACE) == 16
    assert set(API_SURFACE) <= surface(api)
    assert set(API_SURFACE) <= surface(minlz_amd)        # (the package re-exports api)
    assert set(SHARD_SURFACE) <= surface(shard)


def test_every_method_of_a_closed_reader_refuses():
    """Every public method of DeviceReader but close(), whatever it is given, raises the one ValueError on a closed handle and does not reach
    the library (which is not even loaded for this)."""
    rd = api.DeviceReader(None, C.c_void_p(), 0)
    methods = [(n, f) for n, f in inspect.getmembers(api.DeviceReader, inspect.isfunction) if not n.startswith("_") and n != "close"]
    assert len(methods) >= 16
    loaded, _lib.lib = _lib.lib, lambda: pytest.fail("a closed reader reached the library")
    try:
        for name, f in methods:
            required = [p for p in list(inspect.signature(f).parameters.values())[1:] if p.default is p.empty]
            with pytest.raises(ValueError, match="^DeviceReader is closed$"):
                f(rd, *[() for _ in required])
        rd.close()
    finally:
        _lib.lib = loaded


TABLES = [dict(), dict(search_match_len=0), dict(search_match_len=6), dict(search_match_len=8), dict(search_match_len=6, search_prefix=b"\n \t"),
          dict(search_match_len=0, search_prefix=range(40)), dict(search_match_len=5, search_long_prefix=b'"id":', search_extras=3)]


@pytest.mark.parametrize("kw", TABLES, ids=lambda kw: "-".join("%s" % (v if isinstance(v, int) else len(v)) for v in kw.values()) or "plain")
def test_stream_bound_is_the_c_function(kw):
    """api.stream_bound = mlz_stream_bound, _tables or _long_prefix of the configuration, called directly; host-only functions."""
    _build.build()
    L = _lib.lib()
    m = kw.get("search_match_len")
    bs = 64 << 10
    for n in (0, 1, bs, 3 * bs + 7):
        for add_index in (False, True):
            if "search_long_prefix" in kw:
                want = L.mlz_stream_bound_long_prefix(n, bs, int(add_index), C.byref(api.search_long_prefix_config(m, kw["search_long_prefix"], kw["search_extras"])))
            elif "search_prefix" in kw:
                want = L.mlz_stream_bound_tables(n, bs, int(add_index), C.byref(api.search_tables_config(m, kw["search_prefix"])))
            else:
                want = L.mlz_stream_bound(n, bs, int(add_index) | (0 if m is None else 4 | m << 8))
            assert want > 0 and api.stream_bound(n, bs, add_index, **kw) == want
    with pytest.raises(api.MinLZError):
        api.stream_bound(3 * bs + 7, 1000, **kw)


def head(hexes, rest=b"", size=264):
    return (bytes.fromhex(hexes) + bytes(rest)).ljust(size, b"\0")


# (builder, arguments) -> bytes(cfg), or the ValueError's message
CONFIGS = [
    (api.search_tables_config, (0, [0x20]), head("02000100 20", size=36)),
    (api.search_tables_config, (6, [10, 32, 32, 9]), head("02060300 090a20", size=36)),
    (api.search_tables_config, (8, list(range(8))), head("02080800 0001020304050607", size=36)),
    (api.search_tables_config, (4, list(range(40))), head("03040000 ffffffffff", size=36)),
    (api.search_tables_config, (0, []), head("03000000", size=36)),
    (api.search_tables_config, (6, [256]), "search_prefix: byte values"),
    (api.search_tables_config, (6, [-1]), "search_prefix: byte values"),
    (api.search_long_prefix_config, (0, b"key=", 0), head("0000 0400 00000000", b"key=")),
    (api.search_long_prefix_config, (8, bytes(range(256)), 8), head("0808 0001 00000000", range(256))),
    (api.search_long_prefix_config, (1, b"x", 15), head("010f 0100 00000000", b"x")),
    (api.search_long_prefix_config, (6, b"", 0), "search_long_prefix: 1 .. 256 bytes"),
    (api.search_long_prefix_config, (6, bytes(257), 0), "search_long_prefix: 1 .. 256 bytes"),
    (api.search_long_prefix_config, (9, b"ab", 0), "search_match_len: 0 .. 8"),
    (api.search_long_prefix_config, (6, b"ab", 16), "search_extras: 0 .. 15, match length + extras <= 16"),
    (api.search_long_prefix_config, (0, b"ab", 11), "search_extras: 0 .. 15, match length + extras <= 16"),
    (api.search_config, (1,), head("01000000 0000 0000")),
    (api.search_config, (1, 8), head("01080000 0000 0000")),
    (api.search_config, (2, 6, b"\n \t"), head("02060000 0300 0000", b"\n \t")),
    (api.search_config, (3, None, bytes(range(0, 256, 5))), head("03000000 0000 0000" + "2184104208" * 6 + "2184")),
    (api.search_config, (3, 4, b""), head("03040000 0000 0000")),
    (api.search_config, (4, 5, b'"id":', 3), head("04050300 0500 0000", b'"id":')),
    (api.search_config, (4, 0, bytes(range(256)), 10), head("04000a00 0001 0000", range(256))),
    (api.search_config, (0,), "search_config: table type 1 .. 4"),
    (api.search_config, (5,), "search_config: table type 1 .. 4"),
    (api.search_config, (1, 9), "search_match_len: 0 .. 8"),
    (api.search_config, (2, 6, b"ab", 1), "search_extras: table type 4 only"),
    (api.search_config, (2, 6, b""), "search_config: type 2 takes 1 .. 8 byte values"),
    (api.search_config, (2, 6, b"123456789"), "search_config: type 2 takes 1 .. 8 byte values"),
    (api.search_config, (4, 6, b""), "search_long_prefix: 1 .. 256 bytes"),
    (api.search_config, (4, 6, b"ab", 16), "search_extras: 0 .. 15, match length + extras <= 16"),
    (api.search_config, (4, 8, b"ab", 9), "search_extras: 0 .. 15, match length + extras <= 16"),
]


@pytest.mark.parametrize("builder,args,want", CONFIGS, ids=["%s%d" % (c[0].__name__, i) for i, c in enumerate(CONFIGS)])
def test_config_builders_keep_their_bytes(builder, args, want):
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            builder(*args)
        assert str(e.value) == want
    else:
        assert bytes(builder(*args)) == want
