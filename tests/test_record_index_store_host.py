"""The stored record index without a GPU (include/minlz_hip_record_index_store.h): the rules its kernels share
(minlz_amd/csrc/mlz_stream_record_index_store.h), run as plain loops by tools/record_index_store_check.cpp — plain and under AddressSanitizer and
UBSan — against the model (tests/record_index_store_model.py) at blob shifts 0, 1 and 2; the model's blob through the oracle's stream reader;
the golden fixture; mlz_record_index_parse through ctypes; the header against the binding's table."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, api
from tests import record_index_store_cases as K
from tests import record_index_store_model as M
from tests import search_host as H

SRC = "record_index_store_check.cpp"
HEADER = "minlz_hip_record_index_store.h"
NAMES = ["mlz_dev_reader_record_index_bound", "mlz_dev_reader_save_record_index", "mlz_dev_reader_load_record_index", "mlz_record_index_bound",
         "mlz_record_index_build_device", "mlz_record_index_parse"]
GOLDEN = os.path.join(H.ROOT, "tests", "golden", "record_index_v1.bin")
BINDING, LONGEST = (0x1234, 9), 40000
SHIFTS = (0, 1, 2)


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


@pytest.fixture(scope="module")
def base():
    return M.pack(K.BASE_D, K.BASE_SIZE, K.DELIM, bound=BINDING, longest=LONGEST)


@pytest.fixture(scope="module")
def small():
    return M.pack(K.SMALL_D, K.SMALL_SIZE, K.DELIM)


def rec_save(D, size, shift, bound=None, longest=None, delim=K.DELIM):
    flags = (M.BOUND if bound else 0) | (M.LONGEST if longest is not None else 0)
    tag, chunks = bound or (0, 0)
    return struct.pack("<IIIIIIQQQ", 1, delim, shift, flags, tag, chunks, size, M.UNKNOWN if longest is None else longest, len(D)) + np.asarray(D, np.uint64).tobytes()


def rec_load(blob, shift, size, bound=(0, 0), ignore_crc=False):
    return struct.pack("<IIIIIQQ", 2, shift, 1 if ignore_crc else 0, bound[0], bound[1], size, len(blob)) + blob


def test_sanitized_build_links(checkers):
    assert checkers[1] is not None, H.LINK_ERROR.get(SRC)


def test_save_and_load_rules_against_the_model(checkers, base):
    """Every shape, the two-section stream and the corruptions' base, at blob shifts 0, 1 and 2: the save path's bytes are the model's, the
    counts of sparse and dense tiles are the model's, and the load path over those bytes gives D back (the program checks that itself)."""
    cases = K.shapes() + [K.two_sections()]
    recs = [rec_save(D, size, shift) for _, size, D in cases for shift in SHIFTS] + [rec_save(K.BASE_D, K.BASE_SIZE, shift, BINDING, LONGEST) for shift in SHIFTS]
    lines = H.both(checkers, recs)
    want = [(name, M.pack(D, size, K.DELIM), size, D) for name, size, D in cases for _ in SHIFTS] + [("base", base, K.BASE_SIZE, K.BASE_D)] * 3
    assert len(lines) == len(want)
    for line, (name, blob, size, D) in zip(lines, want):
        n, ns, sparse, dense, hexed = line.split()
        counts = np.diff(np.searchsorted(D, np.arange(M.ntiles(size) + 1, dtype=np.uint64) * np.uint64(M.TILE)))
        assert bytes.fromhex(hexed) == blob, name
        assert (int(n), int(ns), int(sparse), int(dense)) == (len(blob), M.nsections(size), int((counts <= M.SPARSE_MAX).sum()), int((counts > M.SPARSE_MAX).sum())), name
        assert len(blob) <= api.record_index_bound(size), name


def test_load_rules_refuse_what_the_model_refuses(checkers, base, small):
    """Every corruption at shifts 0, 1 and 2: the model's unpack names the expected error, and the load path as the kernels run it ends in
    the same code without a read outside the blob (the program's own bounds checks, and the sanitizer's: the buffer ends with the blob)."""
    recs, want = [], []
    for name, which, blob, ignore_crc, code in K.corruptions(base, small):
        size, bound = (K.BASE_SIZE, BINDING) if which == "base" else (K.SMALL_SIZE, (0, 0))
        with pytest.raises(M.StoreError) as e:
            M.unpack(blob, ignore_crc, expect=(size,) + bound)
        assert e.value.code == code, name
        for shift in SHIFTS:
            recs.append(rec_load(blob, shift, size, bound, ignore_crc))
            want.append((name, "error %d" % code))
    # and what loads: the base as it is, for its handle and (unbound blobs only) for any handle of its size; the delimiter is the header's
    other = M.reheader(base, delimiter=0x3B)
    recs += [rec_load(base, 1, K.BASE_SIZE, BINDING), rec_load(small, 2, K.SMALL_SIZE, (77, 3)), rec_load(other, 0, K.BASE_SIZE, BINDING)]
    N = len(K.BASE_D) + 1
    want += [("base", "ok %d %d 10 %d : %s" % (N, len(K.BASE_D), LONGEST, " ".join(str(int(v)) for v in K.BASE_D))),
             ("small", "ok 4 3 10 %d : %s" % (M.UNKNOWN, " ".join(str(int(v)) for v in K.SMALL_D))),
             ("another delimiter", "ok %d %d 59 %d : %s" % (N, len(K.BASE_D), LONGEST, " ".join(str(int(v)) for v in K.BASE_D)))]
    lines = H.both(checkers, recs)
    assert [(name, line) for (name, _), line in zip(want, lines)] == want


def test_the_oracle_reads_a_blob_as_an_empty_stream(base, small):
    """A blob is a valid stream without data: the oracle's stream reader decodes it to zero bytes without an error."""
    for _, size, D in K.shapes() + [K.two_sections()]:
        assert O.stream_decode(M.pack(D, size, K.DELIM), 64) == b""
    assert O.stream_decode(base, 64) == b"" and O.stream_decode(small, 64) == b""


def test_golden_fixture(base):
    """tests/golden/record_index_v1.bin pins the format: it is pack() of the corruptions' base — a sparse tile with an odd count, an empty
    tile, a dense tile and a dense tile cut by the size — and unpacks to it."""
    blob = open(GOLDEN, "rb").read()
    assert blob == base
    D, h = M.unpack(blob, expect=(K.BASE_SIZE,) + BINDING)
    counts = np.diff(np.searchsorted(D, np.arange(5, dtype=np.uint64) * np.uint64(M.TILE)))
    assert (D == K.BASE_D).all() and counts.tolist() == [5, 0, 65536, 14995]
    assert h == dict(flags=3, delimiter=K.DELIM, size=K.BASE_SIZE, k=len(K.BASE_D), N=len(K.BASE_D) + 1, longest=LONGEST, tag=BINDING[0], data_chunks=BINDING[1], nsections=1)
    assert M.pack(D, h["size"], h["delimiter"], bound=(h["tag"], h["data_chunks"]), longest=h["longest"]) == blob


def parse_code(blob):
    info = (C.c_uint64 * 8)()
    a = np.frombuffer(bytes(blob) + b"\0", np.uint8)   # (a byte behind the blob, so that an empty one has an address)
    return _lib.lib().mlz_record_index_parse(a.ctypes.data, len(blob), info), [int(v) for v in info]


def test_parse_through_ctypes(base, small):
    """mlz_record_index_parse on host memory: the model's header, field by field, for every shape; api.record_index_parse's dict; each error
    code — the model's parse names the same one; NULL arguments."""
    for name, size, D in K.shapes() + [K.two_sections()]:
        blob = M.pack(D, size, K.DELIM)
        h = M.parse(blob)[0]
        r, info = parse_code(blob)
        assert r == h["nsections"] and info == [h[f] for f in ("flags", "delimiter", "size", "k", "N", "longest", "tag", "data_chunks")], name
    got = api.record_index_parse(base)
    assert got == dict(flags=3, delimiter=K.DELIM, size=K.BASE_SIZE, k=len(K.BASE_D), N=len(K.BASE_D) + 1, longest=LONGEST, tag=BINDING[0], data_chunks=BINDING[1], nsections=1, bound=True)
    assert api.record_index_parse(small)["longest"] is None and not api.record_index_parse(small)["bound"]
    seen = set()
    for name, which, blob, ignore_crc, code in K.corruptions(base, small):
        try:
            M.parse(blob)
            want = 1      # (a blob whose fault lies in its sections or in what it is loaded into: the header and the directory pass)
        except M.StoreError as e:
            want = -e.code
        r, _ = parse_code(blob)
        assert r == want, name
        seen.add(r)
    assert seen == {1, -M.ERR_CORRUPT, -M.ERR_UNSUPPORTED, -M.ERR_CRC}
    assert parse_code(b"")[0] == -M.ERR_CORRUPT
    with pytest.raises(api.ErrUnsupported):
        api.record_index_parse(M.reheader(base, magic=b"MLZRIDX9"))
    with pytest.raises(api.ErrCorrupt):
        api.record_index_parse(base[:-1])
    with pytest.raises(api.ErrCRC):
        api.record_index_parse(base[:30] + bytes([base[30] ^ 1]) + base[31:])
    L = _lib.lib()
    info = (C.c_uint64 * 8)()
    assert L.mlz_record_index_parse(None, 0, info) == -M.ERR_ARG and L.mlz_record_index_parse(b"x", 1, None) == -M.ERR_ARG


def test_bounds():
    """mlz_record_index_bound: what the header states, and above the model's blob where every byte is a delimiter and where none is."""
    for size in (0, 1, 65536, 65537, 3 * 65536 + 5):
        full = M.pack(np.arange(size, dtype=np.uint64), size, K.DELIM)
        assert len(full) <= api.record_index_bound(size) and len(M.pack([], size, K.DELIM)) <= api.record_index_bound(size)
    # the issue's bound, overhead + min(2 k + 2 tiles, 8192 tiles) with the overhead spelled out (85 bytes of frame, 32 per section, 4 per
    # tile), holds for every shape, and a tile of exactly 4096 delimiters meets 2 k: the sparse form's last size
    for _, size, D in K.shapes() + [K.two_sections()]:
        nt, ns, k = M.ntiles(size), M.nsections(size), len(D)
        assert len(M.pack(D, size, K.DELIM)) <= 85 + 32 * ns + 4 * nt + min(2 * k + 2 * nt, 8192 * nt)
    assert len(M.pack(np.arange(0, 65536, 16, dtype=np.uint64), 65536, K.DELIM)) == 85 + 32 + 4 + 2 * 4096
    assert _lib.lib().mlz_record_index_bound((1 << 32) - (1 << 17) + 1) == -api.ERR_TOO_LARGE and api.record_index_bound((1 << 32) - (1 << 17)) > 0
    with pytest.raises(api.ErrTooLarge):
        api.record_index_bound(1 << 32)
    assert _lib.lib().mlz_dev_reader_record_index_bound(None) == -M.ERR_ARG


def test_exported(tmp_path):
    """The library exports the symbols; the header declares exactly the entries of _lib.ABI_EXT under its name, each with as many parameters
    as the entry has argument types, and minlz_hip.h declares none of them; the header compiles as C99 on its own, and a client gets the
    refusals that come before any device call."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert getattr(L, name) and restype is _lib.i64 and len(argtypes) == params.count(",") + 1 and name not in _lib.ABI
    main_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "minlz_hip.h")).read(), flags=re.S)
    assert not any(re.search(r"\b%s\s*\(" % n, main_h) for n in NAMES)
    src = tmp_path / "client.c"
    src.write_text("""#include "%s"
int main(void) {
    uint64_t info[8];
    uint8_t room[4] = {0, 0, 0, 0};
    if (mlz_dev_reader_record_index_bound(0) != -MLZ_ERR_ARG) return 1;
    if (mlz_dev_reader_save_record_index(0, 0, room, 4, info) != -MLZ_ERR_ARG) return 2;
    if (mlz_dev_reader_load_record_index(0, 0, 0, room, 4, info) != -MLZ_ERR_ARG) return 3;
    if (mlz_record_index_bound(0) < 85) return 4;
    if (mlz_record_index_build_device(0, 0, room, 4, 10, room, 4, info) != -MLZ_ERR_ARG) return 5;
    if (mlz_record_index_parse(room, 4, info) != -MLZ_ERR_CORRUPT) return 6;
    return 0;
}
""" % HEADER)
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0
