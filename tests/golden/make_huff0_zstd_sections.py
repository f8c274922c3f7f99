"""Records tests/golden/huff0_zstd_sections.bin: Huffman literals sections as libzstd writes them (ZSTD_compress, level 1) for seeded
skewed bytes.  Every recorded block is checked to be "compressed literals (type 2), four streams, zero sequences, an FSE-compressed tree
description (header byte < 128)", so that its literals are the input itself.  Record: `u32 n | u32 section bytes | section | the n bytes`.
Run from the repository's root: python tests/golden/make_huff0_zstd_sections.py"""
import ctypes
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import test_search_compressed_model as T  # noqa: E402

z = T.libzstd()
out = []
for seed, n in enumerate([600, 900, 1500, 2500]):
    data = T.skewed(n, 100 + seed)
    cap = z.ZSTD_compressBound(n)
    buf = ctypes.create_string_buffer(cap)
    got = z.ZSTD_compress(buf, cap, data, n, 1)
    assert not z.ZSTD_isError(got)
    sec = T.zstd_section(buf.raw[:got])
    assert sec is not None, "not type 2 / four streams / zero sequences / header byte < 128"
    section, m = sec
    assert m == n and section[0] < 128
    out.append(struct.pack("<II", n, len(section)) + section + data)
open(T.GOLDEN, "wb").write(b"".join(out))
print(len(b"".join(out)), "bytes")
