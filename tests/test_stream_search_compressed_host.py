"""Compressed block search tables (chunk 0x46) without a GPU: the rules the expansion kernels share with the host
(minlz_amd/csrc/mlz_search_compressed.h: the parse, the weights and the decode table of a table description, the stream decode loop, the
sparse walk), run as plain loops by tools/search_compressed_check.cpp, plain and under AddressSanitizer and UBSan, and through
mlz_search_table_expand (include/minlz_hip_search_compressed.h) by ctypes; tests/search_compressed_model.py says what must come out."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, api
from tests import search_compressed_model as CM
from tests import search_host as H
from tests import search_model as SM

SRC = "search_compressed_check.cpp"
HEADER = "minlz_hip_search_compressed.h"
CFG = (1, 6, 16, b"")


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def bitmap_of(n, dens, seed):
    return np.packbits(np.random.default_rng(seed).random(8 * n) < dens).tobytes()


def sparse_of(n, bits):
    b = bytearray(n)
    for p in bits:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


def every_disposition(n=8192, R=0, cfg=CFG):
    """One chunk of 16 sub-blocks: two huff0 tables (direct and FSE-compressed weights), one of them shared by two sub-blocks, a raw one,
    RLE 0x00 and 0xff, a sparse one with a gap above 255 and its last bit set, an empty sparse one."""
    sub = n // 16
    few = bytes(np.random.default_rng(5).choice(np.array([0, 1, 2, 4, 8, 16, 32, 64, 128], np.uint8), size=sub, p=[.6, .05, .05, .05, .05, .05, .05, .05, .05]))
    parts = [few, bitmap_of(sub, 0.05, 8), bitmap_of(sub, 0.06, 9), bitmap_of(sub, 0.5, 10), bytes(sub), b"\xff" * sub,
             sparse_of(sub, [1, 300, 8 * sub - 1]), bytes(sub)]
    kinds = ["huff", ("huff", 1), ("huff", 1), "raw", "rle", "rle", "sparse", "sparse"]
    parts += [bitmap_of(sub, 0.02 * (i + 1), 20 + i) for i in range(8)]
    kinds += ["huff", "sparse", "raw", "huff"] * 2
    bm = b"".join(parts)
    payload = CM.build_compressed_table(cfg, R, bm, h0_bs=(sub - 1).bit_length(), kinds=kinds, forms={0: "direct", 1: "fse"})
    return payload, bm


def valid_cases():
    """[(payload, cfg)] the model made: every partition of the GPU tests' shapes in small, every disposition, every table type's field."""
    out = []
    for n, R, bs in ((32, 8, 5), (512, 4, 5), (512, 4, 9), (8192, 0, 13), (8192, 0, 9), (2048, 2, None), (128 << 10, 0, 17), (128 << 10, 0, 15), (128 << 10, 0, 13)):
        for dens in (0.004, 0.08, 0.45):
            out.append((CM.build_compressed_table((1, 6, R + 3 + (n - 1).bit_length(), b""), R, bitmap_of(n, dens, n + R), h0_bs=bs), (1, 6, R + 3 + (n - 1).bit_length(), b"")))
    out.append((every_disposition()[0], CFG))
    for cfg3 in (SM.config(2, 5, b'":'), SM.config(3, 4, SM.NON_ALNUM), SM.config(4, 6, b'"id":', 2)):
        cfg = (cfg3[0], cfg3[1], 13, cfg3[2])
        out.append((CM.build_compressed_table(cfg, 1, bitmap_of(512, 0.1, 77)), cfg))
    for v in (0, 0xFF):
        out.append((CM.build_compressed_table(CFG, 0, bytes([v]) * 8192, h0_bs=10), CFG))
    return out


def verdict(payload, cfg, ignore_crc=False):
    try:
        R, bm = CM.parse_compressed_table(payload, cfg, ignore_crc)
    except CM.Invalid:
        return "0"
    return "1 %d %d %d" % (R, len(bm), O.crc(bm))


def rec(payload, flags=0):
    return struct.pack("<II", flags, len(payload)) + payload


def test_checker_equals_model_on_valid_chunks(checkers):
    cases = valid_cases()
    lines = H.both(checkers, [rec(p) for p, _ in cases])
    assert lines == [verdict(p, cfg) for p, cfg in cases] and all(line.startswith("1 ") for line in lines)


def test_checker_refuses_the_corrupt_set(checkers):
    """Each case is one edit of a valid chunk: the program's verdict is the model's, a refusal, and no sanitizer reports anything (a report
    ends the program with a failure).  Under "the CRC is not compared" only the stale CRC is let through, as in the model."""
    bm = bitmap_of(8192, 0.05, 3)
    cases = CM.corrupt_set(CFG, 0, bm)
    assert len(cases) == 19
    lines = H.both(checkers, [rec(p) for _, p in cases])
    assert lines == ["0"] * len(cases) == [verdict(p, CFG) for _, p in cases]
    loose = H.both(checkers, [rec(p, 1) for _, p in cases])
    assert loose == [verdict(p, CFG, True) for _, p in cases]
    assert [name for (name, _), line in zip(cases, loose) if line != "0"] == ["stale CRC"]


def test_checker_on_truncations_and_noise(checkers):
    """Every prefix of a valid chunk and chunks with one byte changed: refused or expanded as the model says, never a sanitizer report."""
    payload, _ = every_disposition(2048, 2)
    rng = np.random.default_rng(11)
    cases = [payload[:k] for k in range(0, len(payload), 7)]
    for _ in range(300):
        b = bytearray(payload)
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        cases.append(bytes(b))
    assert H.both(checkers, [rec(p) for p in cases]) == [verdict(p, CFG) for p in cases]
    assert H.both(checkers, [rec(p, 1) for p in cases]) == [verdict(p, CFG, True) for p in cases]


def test_sanitized_build_exists_where_the_others_do(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizers' runtimes: " + H.LINK_ERROR.get(SRC, "")[-200:])


def test_exported():
    """The library exports the symbol; the header declares exactly the entry of _lib.ABI_EXT under its name, with as many parameters, and
    minlz_hip.h does not."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == ["mlz_search_table_expand"]
    restype, argtypes = _lib.ABI_EXT[HEADER]["mlz_search_table_expand"]
    assert L.mlz_search_table_expand and restype is _lib.i64 and len(argtypes) == protos[0][1].count(",") + 1
    assert not re.search(r"\bmlz_search_table_expand\s*\(", open(os.path.join(inc, "minlz_hip.h")).read())
    assert _lib.COUNTER_SEARCH_COMPRESSED == 14


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text("""#include "%s"
int main(void) {
    uint8_t out[32];
    uint32_t R = 0;
    const uint8_t rle[] = {1, 6, 8, 0, 0x44, 0xb2, 0x58, 0x8a, 5, 0, 17, 0};
    if (mlz_search_table_expand(0, 0, out, 32, &R, 0) != -MLZ_ERR_ARG) return 1;
    if (mlz_search_table_expand(rle, sizeof rle, out, 32, &R, 4) != -MLZ_ERR_ARG) return 2;
    if (mlz_search_table_expand(rle, sizeof rle, out, 31, &R, MLZ_STREAM_IGNORE_CRC) != -MLZ_ERR_DST_TOO_SMALL) return 3;
    if (mlz_search_table_expand(rle, sizeof rle, out, 32, &R, MLZ_STREAM_IGNORE_CRC) != 32 || R != 0 || out[0] || out[31]) return 4;
    if (mlz_search_table_expand(rle, sizeof rle - 1, out, 32, 0, MLZ_STREAM_IGNORE_CRC) != -MLZ_ERR_CORRUPT) return 5;
    return 0;
}
""" % HEADER)
    inc = os.path.join(H.ROOT, "include")
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (nothing here touches a device)


def test_expand_equals_model():
    """api.expand_search_table (mlz_search_table_expand through the one ABI table) on the chunks the model made, and on the corrupt set."""
    for payload, cfg in valid_cases():
        assert api.expand_search_table(payload) == CM.parse_compressed_table(payload, cfg)
    bm = bitmap_of(8192, 0.05, 3)
    for name, payload in CM.corrupt_set(CFG, 0, bm):
        with pytest.raises(api.ErrCRC if name == "stale CRC" else api.ErrCorrupt):
            api.expand_search_table(payload)
        if name == "stale CRC":
            assert api.expand_search_table(payload, ignore_crc=True) == (0, bm)
    with pytest.raises(api.ErrCorrupt):
        api.expand_search_table(SM.table_chunk((1, 6, b""), 16, bm, 0)[4:])     # a 0x45 body read as 0x46


def test_search_checker_plans_through_compressed_tables(tmp_path_factory):
    """tools/stream_search_check.cpp restates the locate rule: on a stream whose tables the model recompressed (all of them, and mixed with
    0x45 chunks in both orders) its plan is the 0x45 twin's; a 0x46 chunk with a stale CRC is a table that is not there."""
    from minlz_amd import synth
    run = H.build_checker(tmp_path_factory, "stream_search_check.cpp")
    bs = 64 << 10
    d = bytearray(synth.json_like(6 * bs, 5).tobytes())
    nd = b"#4711-a/Zqxjkv"
    d[4 * bs - 5:4 * bs - 5 + len(nd)] = nd
    d = bytes(d)
    twin, tables = SM.splice(O.stream_encode(d, 1, bs), d, SM.config(1, 6), 16)
    order = [("46",), ("45",), ("45", "46"), ("46", "45")]
    streams = [twin, CM.recompress_stream(twin), CM.recompress_stream(twin, choose=lambda i: order[i % 4]), CM.recompress_stream(twin, crc=lambda i: 7 if i == 2 else None)]
    lines = run([H.rec_stream(10, s_, p) for s_ in streams for p in (nd, d[bs + 100:bs + 120])])[0]
    assert lines[0] == lines[2] == lines[4] and lines[1] == lines[3] == lines[5]
    usable = sum(t is not None for t in tables)
    assert H.parse_stream_line(lines[0])[0][3] == usable and len(H.parse_stream_line(lines[0])[1]) < 6
    holed = list(tables)
    holed[2] = None
    for line, p in zip(lines[6:], (nd, d[bs + 100:bs + 120])):
        head, plan = H.parse_stream_line(line)
        assert head[3] == usable - 1 and plan == SM.plan(holed, [n for n, _ in SM.data_grid(twin)], p, (1, 6, b""), 16)


def tiny_chunk(cfg, R):
    """A 0x46 chunk whose fixed fields are the configuration's but whose bitmap would have fewer than 32 bytes (R > B - 8): no valid chunk,
    and no candidate either, so that it takes no room in the arena in front of the tables behind it."""
    T, M, B, field = cfg
    return SM.frame(CM.CHUNK_COMPRESSED, bytes([T, M, B]) + bytes(field) + bytes([R]) + bytes(4) + bytes([5, 0, CM.RLE, 0]))


def with_tiny_in_front(stream, cfg):
    """The stream with tiny chunks (bitmaps of 2 and of 16 bytes) in front of the first table chunk."""
    cks = SM.chunks_of(stream)
    p = next(p for p, t, _ in cks if t in (SM.CHUNK_TABLE, CM.CHUNK_COMPRESSED))
    return stream[:p] + tiny_chunk(cfg, cfg[2] - 4) + tiny_chunk(cfg, cfg[2] - 7) + stream[p:]


def test_search_checker_no_arena_and_tiny_tables(tmp_path_factory):
    """The rule of a locate round (cst_settle) in tools/stream_search_check.cpp: without an arena (flag 4) the compressed tables count as
    none and nothing behind them is taken instead, while 0x45 tables of the same stream stay in use; 0x46 chunks with bitmaps below 32
    bytes in front of block 0 are no candidates, and the valid tables behind them are used."""
    from minlz_amd import synth
    run = H.build_checker(tmp_path_factory, "stream_search_check.cpp")
    bs = 64 << 10
    d = bytearray(synth.json_like(6 * bs, 5).tobytes())
    nd = b"#4711-a/Zqxjkv"
    d[4 * bs - 5:4 * bs - 5 + len(nd)] = nd
    d = bytes(d)
    twin, tables = SM.splice(O.stream_encode(d, 1, bs), d, SM.config(1, 6), 16)
    sizes = [n for n, _ in SM.data_grid(twin)]
    order = [("46",), ("45",), ("46", "45"), ("45", "46")]
    mixed = CM.recompress_stream(twin, choose=lambda i: order[i % 4])
    kept = [t if order[i % 4][0] == "45" else None for i, t in enumerate(tables)]      # (a 0x45 behind a 0x46 is not taken instead)
    assert sum(t is not None for t in kept) == 3
    tiny = with_tiny_in_front(CM.recompress_stream(twin), (1, 6, 16, b""))
    lines = run([H.rec_stream(10, mixed, nd, 4), H.rec_stream(10, mixed, nd), H.rec_stream(10, twin, nd), H.rec_stream(10, tiny, nd)])[0]
    head, plan = H.parse_stream_line(lines[0])
    assert head[3] == 3 and plan == SM.plan(kept, sizes, nd, (1, 6, b""), 16)
    assert lines[1] == lines[2] == lines[3] and H.parse_stream_line(lines[2])[0][3] == 6
    with pytest.raises(CM.Invalid):
        CM.parse_compressed_table(tiny_chunk((1, 6, 16, b""), 12)[4:], (1, 6, 16, b""))


def test_sidecar_checker_reads_compressed_tables(tmp_path_factory):
    """tools/sidecar_check.cpp restates the attach rule: a sidecar of two configurations that the model recompressed (all tables, and
    mixed with 0x45 tables in both orders) plans as its 0x45 twin; a broken 0x46 table of one configuration leaves the other's in use, and
    one that has a 0x45 behind it is passed over for that one."""
    from minlz_amd import synth
    from tests import sidecar_model as SideM
    from tests.test_sidecar_host import parse_line, rec_attach
    run = H.build_checker(tmp_path_factory, "sidecar_check.cpp")
    san = H.build_checker(tmp_path_factory, "sidecar_check.cpp", sanitized=True)
    bs = 64 << 10
    d = bytearray(synth.json_like(6 * bs, 5).tobytes())
    nd = b'"user":"#4711-a/Zqxjkv'
    d[4 * bs - 5:4 * bs - 5 + len(nd)] = nd
    d = bytes(d)
    main = O.stream_encode(d, 1, bs)
    side = SideM.build(main, d, [SM.config(1, 6), SM.config(2, 6, b'":, ')])
    assert sum(1 for _, t, _ in SM.chunks_of(side) if t == 0x45) == 12            # table 2 k + c: chunk k, configuration c
    order = [("46",), ("45",), ("46", "45"), ("45", "46")]
    sides = [side, CM.recompress_stream(side), CM.recompress_stream(side, choose=lambda i: order[i % 4]),
             CM.recompress_stream(side, crc=lambda i: 7 if i == 6 else None),                                      # chunk 3, configuration 0: broken, nothing behind it
             CM.recompress_stream(side, crc=lambda i: 7 if i == 6 else None, choose=lambda i: ("46", "45") if i == 6 else ("46",))]
    only_first = b"#4711-a/Zq"                                                    # no window behind a prefix byte: configuration 1 cannot serve it
    recs = [rec_attach(s_, main, p) for s_ in sides for p in (nd, only_first)]
    lines = run(recs)[0]
    if san is not None:
        assert san(recs)[0] == lines
    got = [parse_line(line) for line in lines]
    assert got[0] == got[2] == got[4] == got[8] and got[1] == got[3] == got[5] == got[9]
    assert got[0][0] == (2, 6) and got[1][0] == (2, 6) and len(got[1][1]) < 6
    assert got[6][0] == (2, 6) and got[7][0] == (2, 5) and set(got[1][1]) <= set(got[7][1])
