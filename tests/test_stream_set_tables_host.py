"""A set of streams that keeps its streams' search tables, without a GPU: the header against the binding, and tools/stream_set_tables_check.cpp,
which runs the rules the plan shares with its kernels (minlz_amd/csrc/mlz_stream_set_tables.h: the classes, cross, the tail chunks, the marking
that stops at or passes a stream's end) as plain loops over case records; tests/set_tables_model.py says what must come out."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from minlz_amd import _lib
from tests import search_host as H
from tests import search_model as SMod
from tests import set_tables_model as M

SRC = "stream_set_tables_check.cpp"
HEADER = "minlz_hip_stream_set_tables.h"
NAMES = ["mlz_stream_open_batch_device_tables", "mlz_dev_reader_set_tables_info"]


def test_exported(tmp_path):
    """The library exports the symbols; the header declares exactly the entries of _lib.ABI_EXT under its name, each with as many parameters as
    the entry has argument types; minlz_hip.h names the header and declares nothing of it; the header compiles as C99 on its own; a client
    that passes NULLs gets -MLZ_ERR_ARG from every call without a device."""
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
    assert '#include "minlz_hip_stream_set.h"' in open(os.path.join(inc, HEADER)).read()
    calls = ["mlz_stream_open_batch_device_tables(0, 0, 0, 0, 0, 0, 0)", "mlz_stream_open_batch_device_tables(0, 0, 0, 0, 1, 0, &rd)", "mlz_dev_reader_set_tables_info(0, 0)",
             "mlz_dev_reader_set_tables_info(0, out)"]
    src = tmp_path / "client.c"
    src.write_text('#include "%s"\nint main(void) {\n    mlz_dev_reader* rd = 0;\n    uint64_t out[6];\n%s    return rd != 0;\n}\n' %
                   (HEADER, "".join("    if (%s != -MLZ_ERR_ARG) return %d;\n" % (c, i + 1) for i, c in enumerate(calls))))
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (every refusal comes before any device call: no GPU is needed)


# ---- the rules ----

def case(streams, records, nw, L, t_min):
    """streams: dicts(key=(T, M, B, ok, flen, hash), part, mode, delim: its last byte is the delimiter, chunks=[(n, a, s)])."""
    out = struct.pack("<IIIII", len(streams), int(records), nw, L, t_min)
    for s in streams:
        T, Mm, B, ok, flen, h = s["key"]
        out += struct.pack("<BBBBBHQIII", T, Mm, B, ok, s["part"], flen, h, s["mode"], int(s["delim"]), len(s["chunks"]))
        out += b"".join(struct.pack("<QII", *c) for c in s["chunks"])
    return out


def classes_of(streams):
    """The distinct keys of the streams that take part and are usable, in order: (class per stream or 255, their number)."""
    seen, cls = [], []
    for s in streams:
        T, Mm, B, ok, flen, h = s["key"]
        if not s["part"] or not ok:
            cls.append(255)
            continue
        k = (T, Mm, B, flen, h)
        if k not in seen:
            seen.append(k)
        cls.append(seen.index(k) if seen.index(k) < M.MAX_CLASSES else 255)
    return cls, len(seen)


def want_line(streams, records, nw, L, t_min):
    sizes = [[c[0] for c in s["chunks"]] for s in streams]
    modes = [s["mode"] for s in streams]
    total = [sum(x) for x in sizes]
    cross = M.cross_flags(total, [bool(t) and s["delim"] for t, s in zip(total, streams)] if records else None)
    verdicts = [SMod.admits([c[1] for c in s["chunks"]], [c[2] for c in s["chunks"]], sz, nw, L, t_min) if nw else [True] * len(sz) for s, sz in zip(streams, sizes)]
    cls, ncls = classes_of(streams)
    tails = [int(M.tail(sz, k, L)) for sz, m in zip(sizes, modes) for k in range(len(sz))]
    return " | ".join([" ".join(map(str, cls + [ncls])), " ".join(str(int(c)) for c in cross), " ".join(map(str, tails)),
                       " ".join(map(str, M.marks(sizes, modes, cross, verdicts, L)))])


KEYS = [(1, 6, 12, 1, 0, 11), (1, 4, 12, 1, 0, 22), (2, 6, 12, 1, 8, 33), (4, 4, 12, 1, 5, 44), (1, 5, 12, 1, 0, 55), (1, 6, 12, 1, 0, 66), (1, 6, 12, 0, 0, 0)]


def probe_of(rng, nw, table):
    """A table's probe of nw groups: (the leading groups present, the trailing ones); (nw, nw) without a table or when all are present."""
    if not table:
        return nw, nw
    has = rng.random(nw) < 0.6
    a = int(np.argmin(has)) if not has.all() else nw
    if a == nw:
        return nw, nw
    return a, int(np.argmin(has[::-1]))


def stream_of(rng, sizes, mode, delim, nw, key=None, part=1):
    return dict(key=KEYS[int(rng.integers(0, len(KEYS)))] if key is None else key, part=part, mode=mode, delim=delim,
                chunks=[(int(n),) + probe_of(rng, nw, rng.random() < 0.8) for n in sizes])


def designed(rng):
    P, W = M.PRUNE, M.WHOLE
    for records in (0, 1):
        for L, nw in ((1, 1), (2, 1), (7, 2), (12, 7)):
            s = lambda sizes, mode=P, delim=False: stream_of(rng, sizes, mode, delim, nw, key=KEYS[0])
            yield [s([9, 3]), s([]), s([4, 20])], records, nw, L, "an empty stream between two streams"
            yield [s([9, 3]), s([0, 0]), s([4, 20])], records, nw, L, "a stream of chunks without bytes between two streams"
            yield [s([30, 5, 0]), s([2, 0]), s([40])], records, nw, L, "a last chunk of 0 bytes"
            yield [s([1]), s([1]), s([1]), s([1])], records, nw, L, "streams of one 1-byte chunk"
            yield [s([1], delim=True), s([1]), s([1], delim=True), s([1])], records, nw, L, "cross alternating over 1-byte streams"
            yield [s([8, 8], delim=True) for _ in range(5)], records, nw, L, "cross false everywhere (a record-bound call)"
            yield [s([8, 8]) for _ in range(5)], records, nw, L, "cross true everywhere"
            yield [s([8, 3], delim=bool(i & 1)) for i in range(7)], records, nw, L, "cross alternating"
            yield [s([5, 5], W), s([3, 3]), s([2], W, True), s([6, 6])], records, nw, L, "whole and pruned streams in turn"
            yield [s([2, 2, 2, 2, 2]), s([1, 1, 1]), s([2])], records, nw, L, "L - 1 spans several chunks and whole streams"
            yield [stream_of(rng, [4], P, False, nw, part=0, key=KEYS[0]) | dict(chunks=[], mode=M.SKIP), s([6]), s([])], records, nw, L, "a stream left out at the start"
    yield [stream_of(rng, [4, 4], P, False, 2, key=k) for k in KEYS + KEYS[:2]], 0, 2, 7, "six usable configurations: the first four are classes"
    yield [stream_of(rng, [4, 4], P, False, 0, key=KEYS[0]) for _ in range(3)], 0, 0, 3, "a pattern the class gives no window: every chunk is a candidate"


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(2024)
    recs, want, notes = [], [], []
    everything = [c for c in designed(rng)]
    for _ in range(2400):
        L = int(rng.integers(1, 13))
        nw = int(rng.integers(1, max(2, L)))
        t_min = int(rng.integers(0, 2))
        records = int(rng.integers(0, 2))
        streams = []
        for _ in range(int(rng.integers(1, 10))):
            mode = int(rng.choice([M.SKIP, M.WHOLE, M.PRUNE, M.PRUNE]))
            sizes = [] if mode == M.SKIP else [int(v) for v in rng.choice([0, 1, 2, 3, 5, 11, 40], int(rng.integers(0, 6)))]
            streams.append(stream_of(rng, sizes, mode, bool(rng.integers(0, 2)), nw, part=int(mode != M.SKIP)))
        everything.append((streams, records, nw, L, "random") if len(everything) % 2 else (streams, records, nw, L, t_min, "random"))
    for c in everything:
        streams, records, nw, L = c[:4]
        t_min = c[4] if len(c) == 6 else 1
        recs.append(case(streams, records, nw, L, t_min))
        want.append(want_line(streams, records, nw, L, t_min))
        notes.append((c[-1], records, nw, L, t_min))
    return recs, want, notes


def _check(lines, want, notes):
    assert len(lines) == len(want)
    for line, w, note in zip(lines, want, notes):
        assert " ".join(line.split()) == " ".join(w.split()), note


def test_rules_agree_with_the_model(tmp_path_factory, cases):
    """At least 2000 pseudo-random cases of 1 to 9 streams with 0 to 5 chunks of 0 to 40 bytes against pattern lengths 1 to 12, and the designed
    ones: an empty stream between two streams, a last chunk of 0 bytes, streams of one 1-byte chunk, cross true, false and alternating."""
    recs, want, notes = cases
    assert len(recs) > 2000
    _check(H.build_checker(tmp_path_factory, SRC)(recs)[0], want, notes)
    crosses = [w.split("|")[1].split() for w in want]
    assert any("1" in c for c in crosses) and any(c and "1" not in c for c in crosses) and any("1" in w.split("|")[2].split() for w in want)


def test_rules_under_the_sanitizers(tmp_path_factory, cases):
    """The check tool built once with -fsanitize=address,undefined as a stand-alone program, on the same case file: no read outside the
    chunk list, the streams, the bases or the delimiter table."""
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    recs, want, notes = cases
    lines, err = run(recs)
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check(lines, want, notes)
