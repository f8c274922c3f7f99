"""What the host tests share (tests/test_stream_*_host.py, tests/test_sidecar_host.py): the build of a tools/*_check.cpp with g++, plain
and sanitized, and the run of its case file, and the records and result lines of tools/stream_search_check.cpp (the record kinds are the
program's)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_ERROR = {}          # source -> the end of g++'s messages where a sanitized build did not link


def build_checker(tmp_path_factory, source, sanitized=False, flags=()):
    """Compiles tools/<source> -> run(records, argv=()) -> (the program's stdout lines, its stderr): the program gets argv and then the
    path of a file that holds the records (bytes objects) back to back; an exit status other than 0 fails with the stderr.  sanitized: the same stand-alone program under AddressSanitizer and UBSan (nothing is preloaded), or None where this g++ does
    not link their runtimes (LINK_ERROR[source] then says why)."""
    exe = str(tmp_path_factory.mktemp(source.partition(".")[0] + ("_san" if sanitized else "")) / "check")
    opt = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2", "-std=c++17"]
    r = subprocess.run(["g++"] + opt + list(flags) + ["-o", exe, os.path.join(ROOT, "tools", source)], capture_output=True, text=True)
    if sanitized and r.returncode != 0:
        LINK_ERROR[source] = r.stderr[-2000:]
        return None
    assert r.returncode == 0, r.stderr[-2000:]

    def run(records, argv=()):
        path = os.path.join(os.path.dirname(exe), "cases.bin")
        with open(path, "wb") as f:
            for rec in records:
                f.write(rec)
        r = subprocess.run([exe] + list(argv) + [path], capture_output=True, text=True, timeout=900)
        os.unlink(path)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines(), r.stderr
    return run


def checkers(tmp_path_factory, source):
    """The plain build, and the same program under AddressSanitizer and UBSan where this g++ links their runtimes (else None)."""
    return build_checker(tmp_path_factory, source), build_checker(tmp_path_factory, source, sanitized=True)


def both(checkers, records, argv=()):
    """The plain program's lines; the sanitized build runs the same cases and must print the same."""
    plain, san = checkers
    lines = plain(records, argv)[0]
    if san is not None:
        assert san(records, argv)[0] == lines
    return lines


# ---- tools/stream_search_check.cpp ----

def rec_hash(triples):
    return struct.pack("<II", 1, len(triples)) + b"".join(struct.pack("<QII", v, B, M) for v, B, M in triples)


def rec_rule(a, s, sizes, nw, L, t_min=None):
    """Kind 2: the type 1 rule; with t_min kind 7: the rule of every type."""
    head = struct.pack("<IIII", 2, len(sizes), nw, L) if t_min is None else struct.pack("<IIIII", 7, len(sizes), nw, L, t_min)
    return head + np.asarray(a, np.uint32).tobytes() + np.asarray(s, np.uint32).tobytes() + np.asarray(sizes, np.uint64).tobytes()


def rec_stream(kind, stream, pattern, flags=0):
    """Kind 3: a search that knows type 1, 6: types 1 to 3, 10: types 1 to 4."""
    return struct.pack("<IQII", kind, len(stream), len(pattern), flags) + stream + pattern


def rec_reduce(B, pops, limit=None):
    """Kind 4: the writer's reduction rule with type 1's limit; with a limit kind 8."""
    return (struct.pack("<II", 4, B) if limit is None else struct.pack("<III", 8, B, limit)) + np.asarray(pops, np.uint32).tobytes()


def rec_layout(sizes, jobs, pattern, data, group_bytes):
    return (struct.pack("<IIIIQQ", 5, len(sizes), len(jobs), len(pattern), group_bytes, len(data)) + np.asarray(sizes, np.uint64).tobytes() +
            np.asarray(jobs, np.uint32).tobytes() + pattern + data)


def rec_windows(T, M, field, pattern):
    return struct.pack("<IIII", 9, T, M, len(pattern)) + bytes(field).ljust(32, b"\0") + pattern


def rec_groups(M, field, pattern):
    return struct.pack("<IIII", 11, M, len(pattern), len(field)) + bytes(field) + pattern


def parse_stream_line(line):
    """The line of a rec_stream -> (head, plan).  head of kind 3: (M, B, usable); 6: (T, M, B, usable, nw, t_min); 10: the same and gsize."""
    head, _, rest = line.partition(":")
    return tuple(int(v) for v in head.split()), [int(v) for v in rest.split()]
