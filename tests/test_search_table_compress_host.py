"""The write side of compressed block search tables (chunk 0x46) without a GPU: mlz_search_bitmap_compress
(include/minlz_hip_search_compress.h, api.compress_search_bitmap) must give the model's default writer's section byte for byte
(tests/search_compressed_model.py: build_compressed_table), the model's reader and the library's reader must give the bitmap back, and
tools/search_compress_check.cpp runs the same code as plain loops, plain and under AddressSanitizer and UBSan."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, api
from tests import search_compress_cases as K
from tests import search_compressed_model as CM
from tests import search_host as H

SRC = "search_compress_check.cpp"
HEADER = "minlz_hip_search_compress.h"
NAMES = ["mlz_search_bitmap_compress", "mlz_search_bitmaps_compress_device"]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def three_ways(bm, cfg=None, R=0, name=""):
    """The contract of one bitmap; -> the section."""
    cfg = cfg or K.cfg_of(len(bm), R)
    want = K.model_section(bm, cfg, R)
    got = api.compress_search_bitmap(bm)
    assert got == want, (name, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))
    payload = K.fixed_fields(bm, cfg, R) + got
    assert CM.parse_compressed_table(payload, cfg) == (R, bm), name
    assert api.expand_search_table(payload) == (R, bm), name
    assert len(got) <= len(bm) + 2 + 16
    return got


def kinds_of(section, n):
    """The kind bytes of a section's sub-blocks (a table index for a tabled one)."""
    cfg = K.cfg_of(n)
    payload = bytes([cfg[0], cfg[1], cfg[2], 0]) + bytes(4) + section
    bs, tc = section[0], section[1]
    p, sub = 10, 1 << section[0]
    for _ in range(tc):
        p += CM.read_huff_table(payload, p)[3]
    out = []
    for _ in range(n // sub):
        k = payload[p]
        out.append(k)
        p += 1
        if k < 16 or k == CM.SPARSE:
            ln, used = CM.get_uvarint(payload, p)
            p += used + ln
        else:
            p += sub if k == CM.RAW else 1
    assert p == len(payload) and bs == CM.default_bs(n)
    return out


def test_designed_bitmaps():
    seen = set()
    for name, bm in K.designed():
        section = three_ways(bm, name=name)
        assert section[0] == CM.default_bs(len(bm))
        seen.update(min(k, 0) if k < 16 else k for k in kinds_of(section, len(bm)))
    assert seen == {0, CM.RAW, CM.RLE, CM.SPARSE}


def test_real_tables():
    sizes = {}
    for name, cfg, R, bm in K.real_tables():
        sizes[name] = (len(bm), len(three_ways(bm, cfg, R, name)))
    # the JSON-like 1 MiB block's tables compress (the zero block's is RLE): these are the chunks the Writer would write as 0x46
    for name in ("json_like type 1 1048576", "json_like type 2 1048576", "json_like type 4 1048576", "text_like type 1 65536", "zero block"):
        assert sizes[name][1] < sizes[name][0], (name, sizes[name])


def test_description_forms_and_kinds():
    d = dict(K.designed())
    s = api.compress_search_bitmap(d["alphabet 0..3 8192"])
    assert s[:2] == bytes([13, 1]) and s[2] >= 128                     # one table, direct weights
    s = api.compress_search_bitmap(d["skewed 256 values 32768"])
    assert s[:2] == bytes([15, 1]) and 0 < s[2] < 128                   # more than 128 listed weights: FSE-compressed
    assert kinds_of(api.compress_search_bitmap(d["uniform 65536"]), 65536) == [CM.RAW, CM.RAW]
    assert kinds_of(api.compress_search_bitmap(d["zeros 64"]), 64) == [CM.RLE]
    assert kinds_of(api.compress_search_bitmap(d["ones 65536"]), 65536) == [CM.RLE] * 2
    assert kinds_of(api.compress_search_bitmap(d["escapes 8192"]), 8192) == [CM.SPARSE]
    assert kinds_of(api.compress_search_bitmap(d["kinds differ 65536"]), 65536) == [CM.SPARSE, 0]
    assert kinds_of(api.compress_search_bitmap(d["sixteen tables 524288"]), 512 << 10) == list(range(16))
    assert len(set(kinds_of(api.compress_search_bitmap(d["kinds differ 524288"]), 512 << 10))) >= 6
    assert len(kinds_of(api.compress_search_bitmap(d["sixteen sub-blocks 1048576"]), 1 << 20)) == 16


def test_flattened_tree():
    """Fibonacci-like counts: the plain Huffman tree is deeper than 11, so the model's code_lengths took shift > 0; the bytes are equal."""
    bm = K.fibonacci()
    hist = np.bincount(np.frombuffer(bm, np.uint8), minlength=256)
    assert np.count_nonzero(hist) >= 14
    assert max(CM.code_lengths(hist, limit=255).values()) > 11 and max(CM.code_lengths(hist).values()) <= 11
    section = three_ways(bm, name="fibonacci")
    assert kinds_of(section, len(bm)) == [0]


def test_sparse_escapes_bytes():
    """Distances 254, 255, 256 and 510 between set bits, written out: a 255 per full 255 zeros, then the rest."""
    bm = K.bits_of(8192, np.cumsum([1000, 255, 256, 257, 511]).tolist())
    s = api.compress_search_bitmap(bm)
    body = bytes([255] * 3 + [1000 - 765, 254, 255, 0, 255, 1, 255, 255, 0])
    assert s == bytes([13, 0, CM.SPARSE, len(body)]) + body == K.model_section(bm)


def test_refusals():
    for n in (0, 31, 48, 1 << 21):
        with pytest.raises(api.MinLZError, match="minlz error %d" % api.ERR_ARG):
            api.compress_search_bitmap(bytes(n))
    for name, bm in K.designed()[:12]:
        n = len(api.compress_search_bitmap(bm))
        assert len(api.compress_search_bitmap(bm, cap=n)) == n
        with pytest.raises(api.MinLZError, match="minlz error %d" % api.ERR_DST_TOO_SMALL):
            api.compress_search_bitmap(bm, cap=n - 1)


def test_chunk_rule():
    """"section < n" selects exactly the bitmaps whose 0x46 chunk (the model's) is smaller than their 0x45 chunk, and both happen."""
    from tests import search_model as SM
    took = set()
    cases = [(name, K.cfg_of(len(bm)), 0, bm) for name, bm in K.designed()] + list(K.real_tables())
    for name, cfg, R, bm in cases:
        c46 = SM.frame(CM.CHUNK_COMPRESSED, K.model_payload(cfg, R, bm))
        c45 = SM.table_chunk((cfg[0], cfg[1], cfg[3]), cfg[2], bm, R)
        smaller = len(api.compress_search_bitmap(bm)) < len(bm)
        assert smaller == (len(c46) < len(c45)), name
        took.add(smaller)
    assert took == {True, False}


def rec(kind, data):
    return struct.pack("<II", kind, len(data)) + data


def test_checker_equals_model(checkers):
    """The header's write side as plain loops: the section's length and CRC are the model's, and the program itself expands every section
    again (an exit status of 4 is a bitmap that did not come back; a sanitizer report ends it too)."""
    cases = [bm for _, bm in K.designed() if len(bm) <= 64 << 10] + [bm for _, _, _, bm in K.real_tables() if len(bm) <= 64 << 10]
    lines = H.both(checkers, [rec(1, bm) for bm in cases] + [rec(1, bytes(48))])
    assert lines[-1] == "refused"
    for bm, line in zip(cases, lines):
        want = K.model_section(bm)
        assert line.split()[:2] == [str(len(want)), str(O.crc(want))]
    d = dict(K.designed())
    assert lines[cases.index(K.fibonacci())].split()[8] == "1"                      # flattened
    assert lines[cases.index(d["skewed 256 values 32768"])].split()[7] == "1"       # FSE


def test_checker_random_histograms(checkers):
    """A few thousand pseudo-random histograms and bitmaps, each round-tripped through the read side by the program.  Every kind and both
    description forms occur, trees are flattened; the last figure says whether any histogram left both description forms unusable
    (such a sub-block is raw or sparse)."""
    line = H.both(checkers, [rec(2, struct.pack("<II", 1, 3000))])[0].split()
    assert line[:2] == ["searched", "3000"]
    raw, rle, sparse, huff, direct, fse, flattened, without = (int(v) for v in line[2:])
    assert min(raw, sparse, huff, direct, fse, flattened) > 0 and direct + fse == huff
    print("sub-blocks without a usable description:", without)


def test_checker_descriptions_of_weight_vectors(checkers):
    """Weight vectors handed to cst_w_description directly, more than 128 of them each, so that only the FSE form can carry them: every
    section it returns decodes to the weights again in the read side.  Over weights 0 .. 11, all a tree of this writer can give, the
    search finds no vector it refuses (the longest section is printed: 124 bytes of the 128 allowed).  Flat vectors over 0 .. 12 make it
    refuse (an FSE section of 128 bytes or more returns 0), and the caller's choice is then cst_w_pick without a description, which the
    program checks over a grid of sizes: raw or sparse by the sizes alone."""
    line = H.both(checkers, [rec(3, struct.pack("<II", 7, 20000))])[0].split()
    assert line[0] == "weights" and line[1] == "20000" and line[6] == "wide" and int(line[3]) <= 128 and int(line[9]) <= 128
    print("weights 0 .. 11: longest FSE description", line[3], "refused", line[5], "; flat weights 0 .. 12: longest", line[9], "refused", line[11])
    assert int(line[11]) > 0


def test_no_description_is_raw_or_sparse():
    """Where the model's huff_table asserts (more than 128 listed weights and an FSE section of 128 bytes or more), the helper's section
    has no table for that sub-block, and the library agrees; a histogram of that kind, if this search finds one."""
    found = 0
    for seed in range(40):
        bm = K.skewed(8192, 6.0 + seed, 100 + seed, permute=True)
        kinds, without = K.model_kinds(bm)
        if without:
            found += 1
            assert kinds[0] in ("raw", "sparse")
        three_ways(bm, name="permuted %d" % seed)
    print("histograms without a usable description:", found)


def test_sanitized_build_exists_where_the_others_do(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizers' runtimes: " + H.LINK_ERROR.get(SRC, "")[-200:])


def test_exported():
    """The library exports the symbols; the header declares exactly the entries of _lib.ABI_EXT under its name, each with as many
    parameters; minlz_hip.h declares neither."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert getattr(L, name) and len(argtypes) == params.count(",") + 1 and name not in _lib.ABI
        assert not re.search(r"\b%s\s*\(" % name, open(os.path.join(inc, "minlz_hip.h")).read())


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text("""#include "%s"
int main(void) {
    uint8_t bm[32] = {0}, out[64];
    if (mlz_search_bitmap_compress(bm, 32, out, sizeof out) != 4 || out[0] != 5 || out[1] != 0 || out[2] != 17 || out[3] != 0) return 1;
    if (mlz_search_bitmap_compress(bm, 32, out, 3) != -MLZ_ERR_DST_TOO_SMALL) return 2;
    if (mlz_search_bitmap_compress(bm, 31, out, sizeof out) != -MLZ_ERR_ARG) return 3;
    if (mlz_search_bitmap_compress(0, 32, out, sizeof out) != -MLZ_ERR_ARG) return 4;
    bm[31] = 0x80;
    if (mlz_search_bitmap_compress(bm, 32, out, sizeof out) != 6 || out[2] != 18 || out[3] != 2 || out[4] != 255 || out[5] != 0) return 5;
    if (mlz_search_bitmaps_compress_device(0, 0, 0, 0, 0, 0, 0) != -MLZ_ERR_ARG) return 6;
    return 0;
}
""" % HEADER)
    inc = os.path.join(H.ROOT, "include")
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (nothing here touches a device)
