"""A set of streams behind one handle without a GPU: tools/stream_set_check.cpp runs the rules the calls of include/minlz_hip_stream_set.h
share with their kernels (minlz_amd/csrc/mlz_stream_set.h: bases, the stream of a position, the range check, first[], joined, the stream
of a record) as plain loops, and the Python model (tests/stream_set_model.py: bytes.split and bisect) says what must come out."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from minlz_amd import _lib
from tests import search_host as H
from tests import stream_set_model as M

SRC = "stream_set_check.cpp"
HEADER = "minlz_hip_stream_set.h"
NAMES = ["mlz_stream_open_batch_device", "mlz_dev_reader_stream_count", "mlz_dev_reader_stream_bases", "mlz_dev_reader_locate",
         "mlz_dev_reader_read_streams_device", "mlz_dev_reader_stream_records", "mlz_dev_reader_locate_records"]
U64 = 2 ** 64 - 1
NL = 10


def test_exported(tmp_path):
    """The library exports the symbols; include/minlz_hip_stream_set.h declares exactly the entries of _lib.ABI_EXT under its name, each with
    as many parameters as the entry has argument types; the header compiles as C99 on its own (it includes minlz_hip.h); a client that
    passes NULLs gets -MLZ_ERR_ARG from every call without a device."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert getattr(L, name) and restype is _lib.i64 and len(argtypes) == params.count(",") + 1 and name not in _lib.ABI
    main_h = open(os.path.join(inc, "minlz_hip.h")).read()
    assert HEADER in main_h and not any(re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", main_h, flags=re.S)) for n in NAMES)
    calls = ["mlz_stream_open_batch_device(0, 0, 0, 0, 0, 0, 0)", "mlz_stream_open_batch_device(0, 0, 0, 0, 1, 0, &rd)", "mlz_dev_reader_stream_count(0)",
             "mlz_dev_reader_stream_bases(0, 0)", "mlz_dev_reader_locate(0, 0, 0, 0, 0, 0)", "mlz_dev_reader_read_streams_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)",
             "mlz_dev_reader_stream_records(0, 0, 0, 0)", "mlz_dev_reader_locate_records(0, 0, 0, 0, 0, 0)"]
    src = tmp_path / "client.c"
    src.write_text('#include "%s"\nint main(void) {\n    mlz_dev_reader* rd = 0;\n%s    return rd != 0;\n}\n' %
                   (HEADER, "".join("    if (%s != -MLZ_ERR_ARG) return %d;\n" % (c, i + 1) for i, c in enumerate(calls))))
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (every refusal comes before any device call: no GPU is needed)


def rec(size, delim, data, positions, ranges, rec_nos):
    assert sum(size) == len(data)
    return (struct.pack("<I", len(size)) + np.asarray(size, np.uint64).tobytes() + struct.pack("<I", delim) + data +
            struct.pack("<I", len(positions)) + np.asarray(positions, np.uint64).tobytes() +
            struct.pack("<I", len(ranges)) + b"".join(struct.pack("<IQQ", *r) for r in ranges) +
            struct.pack("<I", len(rec_nos)) + np.asarray(rec_nos, np.uint64).tobytes())


def want_line(size, delim, data, positions, ranges, rec_nos):
    base = M.bases(size)
    first = M.first(base, data, delim)
    g = [M.range_global(base, *r) for r in ranges]
    return " | ".join([
        " ".join(map(str, base)),
        " ".join("%d:%d" % M.locate(base, p) for p in positions),
        " ".join("-" if v is None else str(v) for v in g),
        " ".join(map(str, first)),
        "%d %d" % (M.joined(base, data, delim), first[-1]),
        " ".join("%d:%d" % M.locate_record(base, data, delim, r) for r in rec_nos)])


def probes(size, data, delim, rng):
    """The designed positions, ranges and record numbers of a case, and a few random ones."""
    base, n = M.bases(size), len(size)
    total = base[-1]
    pos = {0, 1, total, U64, U64 - 1}
    for b in base:
        pos |= {b, b + 1}
        if b:
            pos.add(b - 1)
    if total:
        pos |= {total - 1} | {int(v) for v in rng.integers(0, total, 8)}
    ranges = [(n, 0, 0), (n + 1, 0, 1), (0xFFFFFFFF, 0, 0)]
    for i in sorted({0, n - 1, n // 2} | {int(v) for v in rng.integers(0, n, 6)}) if n else []:
        s = size[i]
        ranges += [(i, 0, 0), (i, 0, s), (i, s, 0), (i, s, 1), (i, 0, s + 1), (i, s + 1, 0), (i, U64, 0), (i, U64, 1), (i, U64, U64), (i, 1, U64), (i, 0, U64),
                   (i, s // 2, s - s // 2), (i, s // 2, s - s // 2 + 1)]
    nrec = M.first(base, data, delim)[-1]
    recs = {0, 1, nrec, nrec + 1, U64} | ({nrec - 1} if nrec else set()) | {int(v) for v in rng.integers(0, nrec + 1, 12)} | set(M.first(base, data, delim))
    return sorted(pos), ranges, sorted(recs)


def text(rng, n, ends_with_delim):
    d = bytearray(rng.choice(np.frombuffer(b"ab\n\n.", np.uint8), n).tobytes())
    if n:
        d[-1] = NL if ends_with_delim else ord("x")
    return bytes(d)


def designed(rng):
    E = b""
    yield [E], "one empty stream"
    yield [E, E, E], "only empty streams"
    yield [b"x"], "one byte"
    yield [b"\n"], "a stream that is one delimiter"
    yield [b"\n", b"\n", E, b"\n"], "delimiters alone"
    yield [E, E, b"ab\ncd\n", E, E, E, b"x", b"\n", E, b"tail", E, E], "runs of empty streams at the start, in the middle and at the end"
    yield [b"a\n", b"b\n", b"c\n"], "every stream ends with the delimiter"
    yield [b"a", b"b", b"c"], "no stream does: one record"
    yield [b"a\nb", b"c\nd\n", b"e", E, b"f\n", b"g"], "joined over an empty stream, and a last stream without a delimiter"
    yield [b"ab", b"\n", b"cd"], "a stream that is one delimiter between two unterminated ones"
    yield [b"\n\n\n", b"x\n\n", b"\n"], "empty records"
    yield [b"0123456789" * 30, b"\n" * 7, b"z"], "a long record"
    yield [text(rng, int(s), bool(t)) for s, t in zip(rng.choice([0, 0, 1, 2, 3, 17, 200], 300), rng.integers(0, 2, 300))], "300 streams: the bisections have depth"
    yield [text(rng, int(s), True) for s in rng.choice([0, 1, 5, 40], 300)], "300 terminated streams: joined == 0"


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(77)
    recs, want, notes = [], [], []
    everything = [(d, note, ()) for d, note in designed(rng)]
    for _ in range(120):
        n = int(rng.integers(1, 12))
        datas = [text(rng, int(rng.choice([0, 0, 1, 2, 9, 64, 300])), bool(rng.integers(0, 2))) for _ in range(n)]
        failed = tuple(int(i) for i in np.flatnonzero(rng.random(n) < 0.2))
        everything.append((datas, "random", failed))
    for datas, note, failed in everything:
        for delim in ((NL, ord("a")) if note != "random" else (NL,)):
            size, data = M.sizes(datas, failed), M.concat(datas, failed)
            pos, ranges, rno = probes(size, data, delim, rng)
            recs.append(rec(size, delim, data, pos, ranges, rno))
            want.append(want_line(size, delim, data, pos, ranges, rno))
            notes.append((note, delim, failed))
    return recs, want, notes


def _check(lines, want, notes):
    assert len(lines) == len(want)
    for line, w, note in zip(lines, want, notes):
        assert " ".join(line.split()) == " ".join(w.split()), note


def test_rules_agree_with_the_model(tmp_path_factory, cases):
    """Streams of 0 and 1 byte, runs of empty and of failed streams at the start, in the middle and at the end, only empty streams, streams
    that end and do not end with the delimiter, a stream that is one delimiter; positions bases[i] - 1, bases[i], size - 1, size and
    2^64 - 1; ranges with off = size_i and len = 0, off + len = size_i + 1, off = 2^64 - 1 and which = count; 300 streams."""
    recs, want, notes = cases
    _check(H.build_checker(tmp_path_factory, SRC)(recs)[0], want, notes)
    joined = [int(w.split("|")[4].split()[0]) for w in want]
    assert len(recs) > 140 and 0 in joined and max(joined) > 100 and any(n[2] for n in notes)
    assert any(" %d:0" % M.NO_STREAM in w.split("|")[1] for w in want) and any("-" in w.split("|")[2].split() for w in want)


def test_rules_under_the_sanitizers(tmp_path_factory, cases):
    """The check tool built once with -fsanitize=address,undefined as a stand-alone program, on the same case file: no read outside the
    count + 1 bases or the delimiter table, no arithmetic that wraps where the range check is meant not to."""
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    recs, want, notes = cases
    lines, err = run(recs)
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check(lines, want, notes)
