"""mlz_dev_reader_extract_sidecar without a GPU (include/minlz_hip_sidecar_extract.h): the model of the call (tests/sidecar_extract_model.py, the
reference's ExtractSidecar for one stream) pinned by routes that do not go through it — the sidecar parser, the oracle's Reader, the seek index's
loader, the sidecar builder —, the rules the call shares with its kernels (minlz_amd/csrc/mlz_stream_sidecar_extract.h) run as plain loops by
tools/sidecar_extract_check.cpp, plain and under AddressSanitizer and UBSan, and the header against the binding's table."""
import os
import re
import struct
import subprocess

import pytest

import oracle as O
from minlz_amd import _lib, synth
from minlz_amd import index as I
from tests import search_host as H
from tests import search_model as SMod
from tests import sidecar_extract_cases as XC
from tests import sidecar_extract_model as XM
from tests import sidecar_model as SM

SRC = "sidecar_extract_check.cpp"
HEADER = "minlz_hip_sidecar_extract.h"
NAMES = ["mlz_dev_reader_extract_sidecar_bound", "mlz_dev_reader_extract_sidecar"]
BS = 64 << 10


def test_exported(tmp_path):
    """The library exports the symbols; the header declares exactly the entries of _lib.ABI_EXT under its name, each with as many parameters
    as the entry has argument types, and minlz_hip.h declares none of them; the result struct is the binding's, field by field; the header
    compiles as C99 on its own, and a client that passes NULLs gets -MLZ_ERR_ARG from both calls without a device."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    raw = open(os.path.join(inc, HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert getattr(L, name) and restype is _lib.i64 and len(argtypes) == params.count(",") + 1 and name not in _lib.ABI
    main_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "minlz_hip.h")).read(), flags=re.S)
    assert not any(re.search(r"\b%s\s*\(" % n, main_h) for n in NAMES)
    body = re.search(r"typedef struct \{(.*?)\} mlz_sidecar_extract_result;", text, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t([^;]*);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.SidecarExtractResult._fields_] and struct.calcsize("8Q") == 8 * len(fields)
    src = tmp_path / "client.c"
    src.write_text("""#include "%s"
int main(void) {
    mlz_sidecar_extract_result out;
    uint64_t main_bound = 7;
    uint8_t room[4];
    if (sizeof out != 64) return 1;
    if (mlz_dev_reader_extract_sidecar_bound(0, &main_bound) != -MLZ_ERR_ARG || main_bound != 0) return 2;
    if (mlz_dev_reader_extract_sidecar_bound(0, 0) != -MLZ_ERR_ARG) return 3;
    if (mlz_dev_reader_extract_sidecar(0, 0, 0, room, 4, 0, 0, &out) != -MLZ_ERR_ARG) return 4;
    return 0;
}
""" % HEADER)
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (every refusal here comes before any device call)


# ---- the model, pinned by independent routes ----

def type1_stream(nblk=9, tail=777, index=False, bs=BS):
    """The oracle's stream of JSON-like text, framed by the model writer with a type 1 table in front of every block."""
    d = synth.json_like(bs * nblk + tail, 5).tobytes()
    stream, tables = SMod.splice(O.stream_encode(d, 1, bs), d, XC.T1, SMod.table_bits(bs), stored_too=True, index=index)
    assert all(t is not None for t in tables)
    return stream, d


@pytest.fixture(scope="module")
def streams():
    """name -> (stream, decoded bytes)"""
    d = synth.text_like(20000, 3).tobytes()
    return {
        "type 1": type1_stream(),
        "type 1 with an index": type1_stream(index=True),
        "hand framed": XC.hand_framed(),
        "hand framed, a table behind the EOF": XC.hand_framed(post_eof_table=True),
        "no tables": (O.stream_encode(d, 1, 4 << 10), d),
        "header and EOF": (XC.HEADER_AND_EOF, b""),
    }


def check_refs(side, main_stream, data):
    """Every reference of the sidecar lands on a data chunk header of `main_stream` and names its decoded size, in order."""
    mb = SM.max_block_of(side[:10])
    refs = [SM.parse_refs(side[p + 4:p + 4 + n], mb) for p, t, n in SMod.chunks_of(side) if t == SM.CHUNK_REF]
    assert all(r is not None and len(r) == 1 for r in refs)
    dcs = SM.main_chunks(main_stream)
    assert [r[0] for r in refs] == dcs and all(main_stream[p] in (1, 2, 3) for p, _ in dcs) and sum(n for _, n in dcs) == len(data)


def test_model_against_the_parser_the_reader_and_the_index(streams):
    """Both modes of every stream: sidecar_model.parse accepts the sidecar against the stream its references name and finds the tables the
    source carries; every reference lands on a data chunk header with the right decoded size; the oracle's Reader decodes the stripped
    main to the data and the sidecar to nothing; index.py loads the appended index, and Find of every block start returns that block's
    new offset or the nearest kept entry at or before it; the counts are those of the chunks."""
    for name, (stream, d) in streams.items():
        kinds = [t for _, t, _ in SMod.chunks_of(stream)]
        inline = SMod.read_tables(stream)
        for strip in (False, True):
            side, main, c = XM.extract(stream, strip)
            target = main if strip else stream
            assert (main is None) == (not strip)
            cfgs, Bs, tables = SM.parse(side, target)
            check_refs(side, target, d)
            assert O.stream_decode(side, 0) == b""
            if inline[0] is not None:
                assert cfgs == [inline[0]] and Bs == [inline[1]] and tables == [inline[2]], name
            assert (c.side_len, c.main_len, c.blocks) == (len(side), len(main) if strip else 0, sum(k in (1, 2, 3) for k in kinds))
            assert (c.info_chunks, c.tables, c.tables_compressed) == (kinds.count(0x44), kinds.count(0x45) + kinds.count(0x46), kinds.count(0x46))
            side_kinds = [t for _, t, _ in SMod.chunks_of(side)]
            assert set(side_kinds) <= {0xFF, 0x44, 0x45, 0x46, 0x47, 0x20} and side_kinds.count(0x20) == 1 and side_kinds.count(0xFF) == 1
            if not strip:
                assert c.passed_bytes == c.dropped_bytes == 0
                continue
            assert O.stream_decode(main, len(d)) == d, name
            main_kinds = [t for _, t, _ in SMod.chunks_of(main)]
            assert not {0x44, 0x45, 0x46} & set(main_kinds) and main_kinds.count(0x40) == 1 and main_kinds.count(0x99) == 0
            assert [k for k in main_kinds if k not in (0x20, 0x40)] == [k for k in kinds if k not in (0x44, 0x45, 0x46, 0x40, 0x99, 0x20)], name
            passed = sum(4 + n for _, t, n in SMod.chunks_of(stream) if t not in (0xFF, 1, 2, 3, 0x20, 0x40, 0x99, 0x44, 0x45, 0x46))
            assert (c.passed_bytes, c.dropped_bytes) == (passed, sum(4 + n for _, t, n in SMod.chunks_of(stream) if t in (0x40, 0x99)))
            p_eof = next(p for p, t, _ in SMod.chunks_of(main) if t == 0x20)
            idx = I.Index()
            rest = idx.load(main[p_eof + 4 + main[p_eof + 1]:])
            assert idx.total_uncompressed == len(d) and idx.total_compressed == -1
            assert rest == main[len(main) - len(rest):] and main_kinds[main_kinds.index(0x20) + 1] == 0x40
            u, kept = 0, dict((uo, co) for co, uo in idx.offsets)
            for p, n in SM.main_chunks(main):
                co, uo = idx.find(u)
                assert (co, uo) == (p, u) if u in kept else (uo < u and uo in kept and co == kept[uo] and co < p), (name, u)
                u += n


def test_strip_equals_the_builder_for_type_1():
    """Two routes to the same tables: the model writer frames a type 1 stream with a table in front of every block, extract-with-strip moves
    them out, and the sidecar is what sidecar_model.build makes for the stripped stream from the decoded data, byte for byte — every block,
    the last one included: both models give a block the bytes of the block behind it as its overlap and the last block none, and the blocks
    here are longer than the overlap, so the rule that differs (what follows a next block that is shorter than the overlap) never applies."""
    for index in (False, True):
        stream, d = type1_stream(index=index)
        side, main, c = XM.extract(stream, True)
        want, tables = SM.build(main, d, [XC.T1], with_tables=True)
        assert all(t is not None for t in tables[0]) and c.tables == len(tables[0]) == 10
        assert side == want, XC.first_difference(side, want)
        # mode a carries the same chunks; only the references differ
        side_a = XM.extract(stream, False)[0]
        strip_refs = lambda s: b"".join(s[p:p + 4 + n] for p, t, n in SMod.chunks_of(s) if t != SM.CHUNK_REF)
        assert strip_refs(side_a) == strip_refs(side) and side_a != side


def test_model_refusals():
    stream, d = type1_stream(nblk=2)
    for bad, kind in ((b"", "corrupt"), (stream + stream, "unsupported"), (stream + b"\x20\x00\x00\x00", "unsupported"),
                      (stream[:10] + SMod.frame(0x01, bytes(4)) + stream[10:], "corrupt")):
        with pytest.raises(XM.ExtractError) as e:
            XM.extract(bad, True)
        assert e.value.kind == kind


# ---- tools/sidecar_extract_check.cpp ----

@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def test_rules_against_the_serial_restatement(checkers):
    """The classify, scan, piece, layout and emit rules against ExtractSidecar restated chunk by chunk, on pseudo-random chunk tables and gap
    contents: 200 streams whole in memory in both modes (every descriptor run as a memcpy, every output byte written exactly once), and
    virtual streams whose data chunk offsets lie on both sides of 2^14, 2^21, 2^28 and 2^35, with max - actual of 0, 127 and 128, an empty
    gap, a gap of 300 padding chunks, a table with no data chunk behind it and two tables in front of one block; plain and as a stand-alone
    program under AddressSanitizer and UBSan (nothing is preloaded), which must print the same."""
    lines = H.both(checkers, [struct.pack("<III", 1, 7, 200), struct.pack("<II", 2, 9), struct.pack("<III", 1, 1234, 50)])
    assert checkers[1] is not None, H.LINK_ERROR.get(SRC)
    assert lines == ["real ok 200", "virtual ok", "real ok 50"]


def test_rules_give_the_model_bytes(checkers, streams):
    """Every stream of the model tests through the rules as the call runs them (scan per gap, layout, emit per gap, the pieces copied), with the
    model's EOF chunk and index as the foot: the sidecar, the stripped main and the counts are the model's."""
    recs, want = [], []
    for name, (stream, d) in streams.items():
        for strip in (0, 1):
            side, main, c = XM.extract(stream, bool(strip))
            foot = b""
            if strip:
                p_eof = next(p for p, t, _ in SMod.chunks_of(main) if t == 0x20)
                p_idx = p_eof + 4 + main[p_eof + 1]
                foot = main[p_eof:p_idx + 4 + int.from_bytes(main[p_idx + 1:p_idx + 4], "little")]
            recs.append(struct.pack("<IIIQ", 3, strip, len(foot), len(stream)) + foot + stream)
            want.append("side %s main %s %d %d %d %d %d %d" % (side.hex(), main.hex() if strip else "-", c.blocks, c.info_chunks, c.tables, c.tables_compressed,
                                                             c.passed_bytes, c.dropped_bytes))
    lines = H.both(checkers, recs)
    assert len(lines) == len(want)
    for line, w, name in zip(lines, want, [n for n in streams for _ in (0, 1)]):
        assert line == w, name
