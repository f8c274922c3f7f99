"""What the tests of the compressed block search tables' write side share (tests/test_search_table_compress_host.py and
tests/test_gpu_stream_search_compress.py): the bitmaps (designed contents and real tables), the model's section of a bitmap, and the
rewrite of a stream or sidecar by the writer's rule: a 0x45 chunk becomes the model's 0x46 chunk where that is strictly smaller.
tests/search_compressed_model.py is the model; nothing here looks at the library."""
import functools

import numpy as np

from tests import search_compressed_model as CM
from tests import search_model as SM

CFG0 = (1, 6, b"")
SIZES = (32, 64, 512, 8 << 10, 32 << 10, 64 << 10, 512 << 10, 1 << 20)


def cfg_of(n, R=0, cfg3=CFG0):
    """A configuration (T, M, B, field) whose table of R reductions has n bytes."""
    return cfg3[0], cfg3[1], (n - 1).bit_length() + 3 + R, cfg3[2]


def huff_or_none(hist):
    """huff_table(hist), or None where no form of the description carries the weights (the model asserts there)."""
    try:
        return CM.huff_table(hist)
    except AssertionError as e:
        assert "no form" in str(e)
        return None


def model_kinds(bm):
    """The model's choice per sub-block with its defaults ("rle", "raw", "sparse", "huff"), where a sub-block without a description is
    "raw or sparse"; -> (kinds, whether any sub-block had no description)."""
    sub = 1 << CM.default_bs(len(bm))
    kinds, without = [], False
    for i in range(0, len(bm), sub):
        b = np.frombuffer(bm[i:i + sub], np.uint8)
        hist = np.bincount(b, minlength=256)
        if np.count_nonzero(hist) == 1:
            kinds.append("rle")
            continue
        sizes = {"raw": sub, "sparse": len(CM.encode_sparse(b.tobytes())) + 3}
        t = huff_or_none(hist)
        if t is None:
            without = True
        else:
            sizes["huff"] = len(t[0]) + 9 + (int(t[2][b].sum()) + 7) // 8 + 3
        kinds.append(min(sizes, key=sizes.get))
    return kinds, without


@functools.lru_cache(maxsize=None)
def model_payload(cfg, R, bm):
    """build_compressed_table with its defaults; a sub-block whose weights no description carries is raw or sparse."""
    try:
        return CM.build_compressed_table(cfg, R, bm)
    except AssertionError as e:
        assert "no form" in str(e)
        return CM.build_compressed_table(cfg, R, bm, kinds=model_kinds(bm)[0])


def model_section(bm, cfg=None, R=0):
    """The huff0 section of the bitmap: the model's 0x46 payload behind the CRC."""
    cfg = cfg or cfg_of(len(bm), R)
    return model_payload(cfg, R, bytes(bm))[3 + len(cfg[3]) + 5:]


def fixed_fields(bm, cfg=None, R=0):
    """`T M B field R crc` of the bitmap's chunk (0x45 and 0x46 alike)."""
    import oracle as O
    cfg = cfg or cfg_of(len(bm), R)
    return bytes([cfg[0], cfg[1], cfg[2]]) + bytes(cfg[3]) + bytes([R]) + O.crc(bytes(bm)).to_bytes(4, "little")


def bits_of(n, positions):
    b = bytearray(n)
    for p in positions:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


def density(n, dens, seed):
    return np.packbits(np.random.default_rng(seed).random(8 * n) < dens).tobytes()


def fibonacci(n=32 << 10, symbols=20):
    """n bytes whose counts grow like Fibonacci numbers over `symbols` byte values (the rest is one more value): a Huffman tree deeper than
    11, which the writer must flatten."""
    counts = [1, 1]
    while len(counts) < symbols:
        counts.append(counts[-1] + counts[-2])
    assert sum(counts) < n
    vals = np.concatenate([np.full(c, 9 * s + 1, np.uint8) for s, c in enumerate(counts)] + [np.full(n - sum(counts), 250, np.uint8)])
    np.random.default_rng(7).shuffle(vals)
    return vals.tobytes()


def skewed(n, scale, seed, permute=False):
    """All 256 byte values, geometric probabilities (more than 128 listed weights: only FSE can carry them, if anything)."""
    rng = np.random.default_rng(seed)
    p = np.exp(-np.arange(256) / scale)
    if permute:
        p = rng.permutation(p)
    return rng.choice(256, n, p=p / p.sum()).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def designed():
    """[(name, bitmap)]: every size of SIZES, every kind, both description forms, the sparse escapes, a flattened tree, sub-blocks that
    differ in kind, sixteen tables."""
    rng = np.random.default_rng(42)
    out = []
    for n in SIZES:
        out.append(("zeros %d" % n, bytes(n)))
        out.append(("one bit %d" % n, bits_of(n, [8 * n // 2 + 3])))
        out.append(("density 0.05 %d" % n, density(n, 0.05, n)))
    out.append(("ones 64", b"\xff" * 64))
    out.append(("ones 65536", b"\xff" * 65536))
    p0 = 1000
    out.append(("escapes 8192", bits_of(8192, np.cumsum([p0, 255, 256, 257, 511, 1, 2 * 255 + 1, 3 * 255]).tolist())))   # zeros between: 254, 255, 256, 510, 0, 510, 764
    out.append(("escapes 64", bits_of(64, [0, 255, 511])))
    out.append(("last bit 512", bits_of(512, [17, 8 * 512 - 1])))
    out.append(("last bit of sub-block 0 of 2", bits_of(64 << 10, [8 * (32 << 10) - 1, 8 * (32 << 10) + 300])))
    out.append(("alphabet 0..3 8192", rng.integers(0, 4, 8192, dtype=np.uint8).tobytes()))
    out.append(("alphabet 0..3 32", rng.integers(0, 4, 32, dtype=np.uint8).tobytes()))
    out.append(("two values 512", rng.choice(np.array([7, 200], np.uint8), 512).tobytes()))
    out.append(("two values 32768", rng.choice(np.array([0, 255], np.uint8), 32768, p=[0.9, 0.1]).tobytes()))
    out.append(("fibonacci 32768", fibonacci()))
    out.append(("uniform 512", rng.integers(0, 256, 512, dtype=np.uint8).tobytes()))
    out.append(("uniform 65536", rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()))
    out.append(("skewed 256 values 32768", skewed(32768, 40.0, 3)))
    out.append(("skewed 256 values 8192", skewed(8192, 12.0, 4)))
    out.append(("skewed permuted 32768", skewed(32768, 24.0, 5, permute=True)))
    out.append(("kinds differ 65536", density(32 << 10, 0.004, 1) + density(32 << 10, 0.12, 2)))
    out.append(("kinds differ 524288", b"".join([bytes(32 << 10), density(32 << 10, 0.002, 3), density(32 << 10, 0.5, 4), density(32 << 10, 0.1, 5)] * 4)))
    out.append(("sixteen tables 524288", b"".join(density(32 << 10, 0.04 + 0.01 * i, 50 + i) for i in range(16))))
    out.append(("sixteen sub-blocks 1048576", b"".join(density(64 << 10, 0.01 * (i + 1), 70 + i) if i % 5 else bytes([i]) * (64 << 10) for i in range(16))))
    assert all(len(b) in SIZES for _, b in out) and {len(b) for _, b in out} == set(SIZES)
    return out


@functools.lru_cache(maxsize=None)
def real_tables():
    """[(name, cfg (T, M, B, field), R, bitmap)]: what search_model builds over text-like and JSON-like blocks of 64 KiB and 1 MiB for types
    1, 2 and 4, and the table of an all-zero block."""
    from minlz_amd import synth
    out = []
    shapes = [("type 1", SM.config(1, 6)), ("type 2", SM.config(2, 6, b'":, ')), ("type 4", SM.config(4, 6, b'"user":"', 3))]
    for kind in ("text_like", "json_like"):
        for bs in (64 << 10, 1 << 20):
            data = getattr(synth, kind)(bs + 64, 5).tobytes()
            for name, cfg3 in shapes if kind == "json_like" else shapes[:1]:
                B = SM.table_bits(bs)
                table, R = SM.build_table(cfg3, data[:bs], data[bs:], B)
                assert table is not None
                out.append(("%s %s %d" % (kind, name, bs), (cfg3[0], cfg3[1], B, cfg3[2]), R, table))
    table, R = SM.build_table(CFG0, bytes(64 << 10), None, 16)
    out.append(("zero block", (1, 6, 16, b""), R, table))
    return out


def rewrite(stream):
    """The stream (or sidecar) as the writer's rule leaves it: every 0x45 chunk replaced by the model's 0x46 chunk of the same table where
    that is strictly smaller, every other byte as it is.  -> (stream, 0x46 chunks written)."""
    stream = bytes(stream)
    out, wrote = [], 0
    for p, t, n in SM.chunks_of(stream):
        raw = stream[p:p + 4 + n]
        if t == SM.CHUNK_TABLE:
            body = raw[4:]
            cfg, at = CM.table_config(body)
            comp = SM.frame(CM.CHUNK_COMPRESSED, model_payload(cfg, body[at], body[at + 5:]))
            if len(comp) < len(raw):
                raw, wrote = comp, wrote + 1
        out.append(raw)
    return b"".join(out), wrote


def with_index(stream, n_decoded):
    """A stream without a seek index -> the same stream with the index the model's Index appends: an entry per data chunk at the offset
    where the block's chunks start (its table chunk, 0x45 or 0x46, when it has one), as search_model.splice rebuilds it."""
    from minlz_amd import index as I
    stream = bytes(stream)
    idx = I.Index()
    idx.reset(1 << (stream[9] + 10))
    idx.add(0, 0)
    u, start = 0, None
    sizes = [n for n, _ in SM.data_grid(stream)]
    k = 0
    for p, t, n in SM.chunks_of(stream):
        if t in (SM.CHUNK_TABLE, CM.CHUNK_COMPRESSED) and start is None:
            start = p
        elif t in (0x01, 0x02, 0x03):
            idx.add(p if start is None else start, u)
            u += sizes[k]
            k += 1
            start = None
    assert u == n_decoded
    return stream + idx.append_to(n_decoded, len(stream))
