"""The model of compressed block search tables (tests/search_compressed_model.py) held against an independent RFC 8878 implementation,
libzstd, in both directions, and against itself: the writer's Huffman sections decode in libzstd, libzstd's literals sections decode in the
reader (live, and from tests/golden/huff0_zstd_sections.bin, which tests/golden/make_huff0_zstd_sections.py recorded), every disposition
round-trips, and real tables of tests/search_model.py survive build and parse."""
import ctypes
import os
import random
import struct

import numpy as np
import pytest

from tests import search_compressed_model as CM
from tests import search_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "huff0_zstd_sections.bin")
CFG = (1, 6, 16, b"")


def libzstd():
    for name in ("libzstd.so.1", "libzstd.so"):
        try:
            z = ctypes.CDLL(name)
        except OSError:
            continue
        z.ZSTD_decompress.restype = z.ZSTD_compress.restype = z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        return z
    return None


def skewed(n, seed, top=255):
    rng = random.Random(seed)
    return bytes(min(top, int(rng.expovariate(0.03))) for _ in range(n))


def zstd_frame(section, n):
    """A Huffman section (tree description, jump table, four streams) of n literals as a zstd frame: a single-segment header, one
    compressed block whose literals section is of type 2 with four streams and whose sequences section says "none"."""
    comp = len(section)
    if n < 1024 and comp < 1024:
        lit = (2 | 1 << 2 | n << 4 | comp << 14).to_bytes(3, "little")
    elif n < 16384 and comp < 16384:
        lit = (2 | 2 << 2 | n << 4 | comp << 18).to_bytes(4, "little")
    else:
        lit = (2 | 3 << 2 | n << 4 | comp << 22).to_bytes(5, "little")
    block = lit + section + b"\x00"
    return struct.pack("<IB", 0xFD2FB528, 0xA0) + struct.pack("<I", n) + (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block


def zstd_section(frame):
    """A frame libzstd made -> (Huffman section, literals) of its first block, or None when the block is not "compressed literals, four
    streams, an FSE-compressed tree description, zero sequences"."""
    assert frame[:4] == struct.pack("<I", 0xFD2FB528)
    fhd = frame[4]
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs]
    bh = int.from_bytes(frame[p:p + 3], "little")
    p += 3
    if (bh >> 1) & 3 != 2:
        return None
    end = p + (bh >> 3)
    b0 = frame[p]
    if b0 & 3 != 2 or (b0 >> 2) & 3 == 0:
        return None
    sf = (b0 >> 2) & 3
    nb, width = {1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(frame[p:p + nb], "little")
    n, comp = (v >> 4) & ((1 << width) - 1), v >> (4 + width)
    p += nb
    section = frame[p:p + comp]
    if p + comp + 1 != end or frame[p + comp] != 0 or section[0] >= 128:
        return None
    return section, n


def decode_section(section, n):
    sym, nb, log, used = CM.read_huff_table(section, 0)
    return CM.decode_4x(section[used:], n, (sym, nb, log))


@pytest.mark.parametrize("n", [32, 512, 8 << 10, 128 << 10])
@pytest.mark.parametrize("form, top", [("direct", 128), ("fse", 128), ("fse", 255)])
def test_writer_decodes_in_libzstd(n, form, top):
    """The model's table description (direct and FSE-compressed weights, symbols above 127 in the latter), jump table and streams, wrapped
    into a zstd frame, are what libzstd decodes to the exact bytes."""
    z = libzstd()
    if z is None:
        pytest.skip("libzstd does not load")
    data = skewed(n, n + top, top)
    desc, code, length, _ = CM.huff_table(np.bincount(np.frombuffer(data, np.uint8), minlength=256), form)
    assert (desc[0] >= 128) == (form == "direct")
    frame = zstd_frame(desc + CM.encode_4x(data, code, length), n)
    out = ctypes.create_string_buffer(n)
    got = z.ZSTD_decompress(out, n, frame, len(frame))
    assert not z.ZSTD_isError(got) and got == n and out.raw == data
    assert decode_section(desc + CM.encode_4x(data, code, length), n) == data


def golden_sections():
    raw = open(GOLDEN, "rb").read()
    p, out = 0, []
    while p < len(raw):
        n, comp = struct.unpack_from("<II", raw, p)
        out.append((raw[p + 8:p + 8 + comp], raw[p + 8 + comp:p + 8 + comp + n]))
        p += 8 + comp + n
    return out


def test_reader_decodes_recorded_libzstd_sections():
    """Literals sections libzstd made (four streams, FSE-compressed weights), recorded: the reader gives the bytes they were made from."""
    got = golden_sections()
    assert len(got) >= 4
    for section, data in got:
        assert section[0] < 128 and decode_section(section, len(data)) == data


def test_reader_decodes_live_libzstd_sections():
    z = libzstd()
    if z is None:
        pytest.skip("libzstd does not load")
    seen = 0
    for seed, n in enumerate([600, 1000, 2500, 4000, 8000]):
        data = skewed(n, 100 + seed)
        cap = z.ZSTD_compressBound(n)
        out = ctypes.create_string_buffer(cap)
        got = z.ZSTD_compress(out, cap, data, n, 1)
        assert not z.ZSTD_isError(got)
        sec = zstd_section(out.raw[:got])
        if sec is None:
            continue
        assert sec[1] == n and decode_section(sec[0], n) == data
        seen += 1
    assert seen >= 3


def bitmap_of(n, dens, seed):
    return np.packbits(np.random.default_rng(seed).random(8 * n) < dens).tobytes()


@pytest.mark.parametrize("n, R", [(32, 8), (512, 4), (8192, 0)])
def test_every_disposition_round_trips(n, R):
    bm = bitmap_of(n, 0.05, n)
    for kinds in (None, ["huff"], ["raw"], ["sparse"]):
        assert CM.parse_compressed_table(CM.build_compressed_table(CFG, R, bm, kinds=kinds), CFG) == (R, bm)
    for v in (0, 0xFF, 0x5A):
        assert CM.parse_compressed_table(CM.build_compressed_table(CFG, R, bytes([v]) * n, kinds=["rle"]), CFG) == (R, bytes([v]) * n)
    if n >= 512:
        nsub = 16
        sub = n // nsub
        parts = [bitmap_of(sub, 0.04, 7), bitmap_of(sub, 0.05, 8), bitmap_of(sub, 0.4, 9), bytes(sub), b"\xff" * sub, bitmap_of(sub, 0.002, 10), bytes(sub)]
        parts += [bitmap_of(sub, 0.1, 20 + i) for i in range(nsub - len(parts))]
        kinds = [("huff", 0), ("huff", 0), "huff", "rle", "rle", "sparse", "sparse"] + ["huff", "raw"] * 5
        bm = b"".join(parts)
        payload = CM.build_compressed_table(CFG, R, bm, h0_bs=(sub - 1).bit_length(), kinds=kinds[:nsub])
        assert CM.parse_compressed_table(payload, CFG) == (R, bm)


def test_partition_is_the_reference_policy():
    assert [CM.default_bs(n) for n in (32, 8192, 32 << 10, 64 << 10, 512 << 10, 1 << 20)] == [5, 13, 15, 15, 15, 16]


def sparse_of(n, bits):
    b = bytearray(n)
    for p in bits:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


@pytest.mark.parametrize("bits", [[], [0], [2047], [0, 2047], [0, 256], [3, 259], [0, 511], [5, 516, 1027], [254, 255, 256], [255], [510]])
def test_sparse_edges(bits):
    """Bit 0, the last bit, gaps of exactly 255 and 510 (one and two bytes of 255 and then 0), no bits at all (length 0)."""
    bm = sparse_of(256, bits)
    enc = CM.encode_sparse(bm)
    if not bits:
        assert enc == b""
    if bits == [0, 256]:
        assert enc == bytes([0, 255, 0])
    if bits == [0, 511]:
        assert enc == bytes([0, 255, 255, 0])
    assert CM.decode_sparse(enc, 256) == bm
    assert CM.parse_compressed_table(CM.build_compressed_table(CFG, 5, bm, kinds=["sparse"]), CFG) == (5, bm)


def test_sparse_errors():
    with pytest.raises(CM.Invalid):
        CM.decode_sparse(bytes([255] * 8 + [8]), 256)          # position 2048 of 2048 bits
    with pytest.raises(CM.Invalid):
        CM.decode_sparse(bytes([1, 255]), 256)
    assert CM.decode_sparse(bytes([255] * 8 + [7]), 256) == sparse_of(256, [2047])


@pytest.mark.parametrize("T, prefix, extras", [(1, b"", 0), (2, b'":', 0), (4, b'"id":', 2)])
def test_real_tables_survive(T, prefix, extras):
    """parse(build(bitmap)) == bitmap for tables search_model builds over text, R = 0 and R > 0."""
    from minlz_amd import synth
    cfg3 = SM.config(T, 6, prefix, extras)
    data = synth.json_like(3 * 65536, 5).tobytes()
    seen = set()
    for B, blk in ((16, data[:65536]), (16, data[65536:65536 + 3000]), (12, data[:4096])):
        table, R = SM.build_table(cfg3, blk, data[len(blk):len(blk) + 64], B)
        if table is None:
            continue
        cfg = (cfg3[0], cfg3[1], B, cfg3[2])
        for bs in (None, max(5, (len(table) - 1).bit_length() - 4)):
            payload = CM.build_compressed_table(cfg, R, table, h0_bs=bs)
            assert CM.parse_compressed_table(payload, cfg) == (R, table)
        seen.add(R > 0)
    assert seen == {False, True} or T != 1


def test_corrupt_set_is_refused():
    bm = bitmap_of(8192, 0.05, 3)
    names = [name for name, _ in CM.corrupt_set(CFG, 0, bm)]
    assert len(names) == len(set(names)) == 19
    for name, payload in CM.corrupt_set(CFG, 0, bm):
        with pytest.raises(CM.Invalid):
            CM.parse_compressed_table(payload, CFG)


def test_recompress_stream_leaves_the_rest():
    from minlz_amd import synth
    import oracle as O
    data = synth.json_like(5 * 4096 + 100, 2).tobytes()
    stream = O.stream_encode(data, 1, 4096)
    with45, tables = SM.splice(stream, data, SM.config(1, 6), 12)
    with46 = CM.recompress_stream(with45)
    a, b = SM.chunks_of(with45), SM.chunks_of(with46)
    assert len(a) == len(b) and sum(t is not None for t in tables) >= 3
    k = 0
    for (pa, ta, na), (pb, tb, nb) in zip(a, b):
        if ta == SM.CHUNK_TABLE:
            assert tb == CM.CHUNK_COMPRESSED
            R, bm = CM.parse_compressed_table(with46[pb + 4:pb + 4 + nb], (1, 6, 12, b""))
            while tables[k] is None:
                k += 1
            assert (bm, R) == tables[k]
            k += 1
        else:
            assert with45[pa:pa + 4 + na] == with46[pb:pb + 4 + nb]
