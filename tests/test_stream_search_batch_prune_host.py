"""mlz_stream_search_batch_device_pruned without a GPU: the header and its binding, and tools/stream_search_batch_prune_check.cpp, which runs the
host code the call shares with its kernels (minlz_amd/csrc/mlz_stream_search_batch_prune.h) lane by lane, against the Python model
(tests/search_batch_prune_model.py).  The streams are made on the CPU: search_model.splice over the oracle's streams, table types 1 to 4,
blocks of 16 KiB and 64 KiB, 1 to 6 chunks."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from tests import search_batch_prune_model as PM
from tests import search_host as H
from tests import search_model as SMod

SRC = "stream_search_batch_prune_check.cpp"
HEADER = "minlz_hip_search_batch_prune.h"
NAME = "mlz_stream_search_batch_device_pruned"
IGNORE_CRC, IGNORE_CASE = 2, 32
QUOTE = b'"'


def test_exported(tmp_path):
    """The library exports the symbol; the header declares it and nothing else, with as many parameters as its entry in _lib.ABI_EXT has
    argument types (those of the unpruned call); a C99 client compiles against it, and n_patterns == 0 is refused without a GPU."""
    L = _lib.lib()
    assert getattr(L, NAME)
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == [NAME]
    restype, argtypes = _lib.ABI_EXT[HEADER][NAME]
    assert restype is _lib.i64 and len(argtypes) == protos[0][1].count(",") + 1 == 18 and NAME not in _lib.ABI
    assert argtypes == _lib.ABI_EXT["minlz_hip_search_batch.h"]["mlz_stream_search_batch_device"][1]
    src = tmp_path / "client.c"
    src.write_text('#include "%s"\nint main(void) { return %s(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == -MLZ_ERR_ARG ? 0 : 1; }\n' % (HEADER, NAME))
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0


# ---- the batches ----

def rec(streams, pats, flags=0):
    return (struct.pack("<III", len(streams), len(pats), flags) + np.asarray([len(s) for s in streams], np.uint64).tobytes() +
            np.asarray([len(p) for p in pats], np.uint32).tobytes() + b"".join(pats) + b"".join(streams))


def parse(line):
    head, _, rest = line.partition(":")
    classes, whole, skipped, tabbed, decoded, bad_keys, home = (int(v) for v in head.split())
    return dict(classes=classes, whole=whole, skipped=skipped, tabbed=tabbed, decoded=decoded, bad_keys=bad_keys, home=home, plans=[[int(v) for v in part.split()] for part in rest.split("|")])


def json_data(bs, k, nblk=5):
    return synth.json_like(nblk * bs + 100 * k, 92 + k).tobytes()


def put(d, o, p):
    return d[:o] + p + d[o + len(p):]


def tabled(data, bs, cfg, **kw):
    return SMod.splice(O.stream_encode(data, 1, bs), data, cfg, SMod.table_bits(bs), **kw)[0]


def stale_crc(stream, which):
    """The stream with the stated CRC of its `which`-th table chunk flipped."""
    cfg, _, _ = SMod.read_tables(stream)
    at = [p for p, t, _ in SMod.chunks_of(stream) if t == SMod.CHUNK_TABLE][which]
    b = bytearray(stream)
    b[at + 4 + 4 + len(cfg[2])] ^= 0x10
    return bytes(b)


CONFIGS = [SMod.config(1, 6), SMod.config(1, 4), SMod.config(2, 6, QUOTE), SMod.config(3, 6, b'":,{}[] \n'), SMod.config(4, 4, b'":', 2), SMod.config(1, 5)]


def _needle(seed, L=16, head=b""):
    """Random bytes above 0x7f (no prefix byte of CONFIGS among them) behind `head`."""
    return head + bytes(np.random.default_rng(seed).integers(128, 256, L - len(head), dtype=np.uint8))


def _batches():
    """-> [(what, [(stream, data)], patterns, flags, the streams whose class must prune and serve)]"""
    out = []
    for bs in (16 << 10, 64 << 10):
        across, absent, short = _needle(1), _needle(2), _needle(3, 5)
        # type 1, M = 6: a needle across the border at 2 * bs, 5 chunks, and 6 with a tail chunk of 100 bytes (k = 1)
        d = [put(json_data(bs, k), 2 * bs - 8, across) for k in range(3)]
        one = put(json_data(bs, 0, 1)[:bs], 3000, across)
        plain = [(tabled(x, bs, CONFIGS[0]), x) for x in d] + [(O.stream_encode(b"", 1, bs), b""), (tabled(one, bs, CONFIGS[0]), one),
                                                                (O.stream_encode(d[0], 1, bs), d[0]),                               # no info chunk
                                                                (tabled(d[1], bs, CONFIGS[0], skip=range(8)), d[1])]                # an info chunk and no table
        out.append(("type 1 bs %d" % bs, plain, [across, absent], 0, [0, 1, 2]))
        out.append(("type 1 bs %d, one pattern" % bs, plain, [across], 0, [0, 1, 2]))
        out.append(("a pattern shorter than M, bs %d" % bs, plain, [across, short], 0, []))
        # a pattern at a stream's last bytes whose continuation stands at the next stream's first bytes
        left, right = d[0][:3 * bs + 77] + across[:9], across[9:] + d[1][:4 * bs]
        out.append(("stream border bs %d" % bs, [(tabled(left, bs, CONFIGS[0]), left), (tabled(right, bs, CONFIGS[0]), right)], [across], 0, [0, 1]))
        # six configurations in one batch: a needle every one of them serves ('"' is a prefix byte of types 2 and 3, '":' the prefix of type 4)
        served = _needle(4, 16, b'":')
        six = []
        for k, cfg in enumerate(CONFIGS):
            x = put(json_data(bs, k), 2 * bs - 8, served)
            six.append((tabled(x, bs, cfg), x))
        out.append(("six classes bs %d" % bs, six, [served, _needle(5, 16, b'":')], 0, [0, 1, 2, 3]))
        out.append(("six classes reversed bs %d" % bs, six[::-1], [served], 0, [0, 1, 2, 3]))
        # types 2 to 4 with a random needle: unserved
        out.append(("prefix types, a random needle bs %d" % bs, six[2:5], [across], 0, []))
        # two streams that differ only in the prefix field
        x = put(json_data(bs, 2), 2 * bs - 8, served)
        two = [(tabled(x, bs, SMod.config(2, 6, QUOTE)), x), (tabled(x, bs, SMod.config(2, 6, b":")), x)]
        out.append(("two prefix fields bs %d" % bs, two, [served], 0, [0, 1]))
        # a stale table CRC: its chunk is admitted; with IGNORE_CRC the table is used
        broken = [(stale_crc(plain[0][0], 3), d[0]), plain[1]]
        out.append(("stale CRC bs %d" % bs, broken, [across], 0, [0, 1]))
        out.append(("stale CRC ignored bs %d" % bs, broken, [across], IGNORE_CRC, [0, 1]))
        # folding: an id in three cases
        ident = b"\x81K\x93\xa7\xf2q\xc5\x88\xd4V\x9e\xb1\xe3\xf7\x8a\x90"                # (three letters, at most two in a window of 6)
        y = put(put(put(json_data(bs, 0), 1000, ident), 2 * bs - 5, ident.lower()), 2 * bs + 500, ident.upper())
        out.append(("fold bs %d" % bs, [(tabled(y, bs, CONFIGS[0]), y), plain[1]], [ident], IGNORE_CASE, [0, 1]))
        out.append(("fold, a word bs %d" % bs, [(tabled(y, bs, CONFIGS[0]), y)], [b"stream"], IGNORE_CASE, []))
        # folding over three classes: every class's records index the call's one array of variant hashes
        z = put(put(json_data(bs, 0), 5000, ident.upper()), 2 * bs - 3, ident.lower())
        three = [(tabled(y, bs, CONFIGS[0]), y), (tabled(z, bs, SMod.config(1, 8)), z), (tabled(y, bs, SMod.config(1, 7)), y), (tabled(z, bs, CONFIGS[0]), z)]
        out.append(("fold, three classes bs %d" % bs, three, [ident, b"\x82\x95Z\xa1\xb3\xc4\xd5\xe6w\xf1\x83\x94\xa5\xb6\xc7\xd8"], IGNORE_CASE, [0, 1, 2, 3]))
    return out


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture(scope="module")
def models(batches):
    return [PM.plan([s for s, _ in streams], pats, ignore_crc=bool(flags & IGNORE_CRC), fold=bool(flags & IGNORE_CASE)) for _, streams, pats, flags, _ in batches]


def test_the_model_prunes_and_is_sound(batches, models):
    """A condition on the inputs, asserted on the model alone: every stream whose class prunes and serves the patterns loses at least one
    chunk; and every chunk that holds a byte of a brute-force occurrence is in the plan."""
    from tests import fold_model as FM
    for (what, streams, pats, flags, pruned), m in zip(batches, models):
        fold = bool(flags & IGNORE_CASE)
        for i in pruned:
            assert m["pruning"][i] and len(m["plans"][i]) < sum(1 for v in m["sizes"][i] if v), (what, i, m["plans"][i])
        for i, (_, d) in enumerate(streams):
            for p in pats:
                pos = SMod.brute(FM.fold(d), FM.fold(p)) if fold else SMod.brute(d, p)
                assert SMod.chunks_touched(m["sizes"][i], pos, len(p)) <= set(m["plans"][i]), (what, i)
    by = {b[0]: m for b, m in zip(batches, models)}
    bs = 64 << 10
    for size in (16 << 10, bs):                                                                             # the planted border, and little else
        assert all({1, 2} <= set(p) and len(p) <= 4 for p in by["type 1 bs %d, one pattern" % size]["plans"][:3])
    assert by["type 1 bs %d" % (16 << 10)]["plans"][3:] == [[], [0], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5]]
    assert by["six classes bs %d" % bs]["classes"] == 6 and by["six classes bs %d" % bs]["whole"] == 2
    assert by["six classes bs %d" % bs]["pruning"] == [True] * 4 + [False] * 2
    assert by["two prefix fields bs %d" % bs]["classes"] == 2 and by["two prefix fields bs %d" % bs]["whole"] == 0     # (two classes, and each serves the needle: it holds '"' and ':')
    assert by["a pattern shorter than M, bs %d" % bs]["whole"] == 6 and by["prefix types, a random needle bs %d" % bs]["whole"] == 3
    assert 3 in by["stale CRC bs %d" % bs]["plans"][0] and 3 not in by["stale CRC ignored bs %d" % bs]["plans"][0]
    left, right = by["stream border bs %d" % bs]["plans"]
    assert 0 not in right                                                                                   # the continuation marks nothing of the next stream
    assert {0, 1, 2} <= set(by["fold bs %d" % bs]["plans"][0]) and by["fold, a word bs %d" % bs]["whole"] == 1


def _check(lines, batches, models):
    assert len(lines) == len(batches)
    for line, (what, streams, _, _, _), m in zip(lines, batches, models):
        got = parse(line)
        assert got["bad_keys"] == 0, what
        # the plan's traffic by the call's own count: at most 32 bytes per stream and one byte per data chunk (a stale table costs a round more)
        n, nck = len(streams), sum(len(x) for x in m["sizes"])
        assert got["home"] <= 32 * n + nck and (got["home"] >= 16 * n or nck == 0), (what, got["home"], n, nck)
        assert got["plans"] == m["plans"], what
        assert (got["classes"], got["whole"], got["skipped"], got["tabbed"], got["decoded"]) == (m["classes"], m["whole"], m["skipped"], m["tabbed"], m["decoded"]), what


def test_the_shared_code_plans_what_the_model_plans(tmp_path_factory, batches, models):
    run = H.build_checker(tmp_path_factory, SRC)
    _check(run([rec([s for s, _ in streams], pats, flags) for _, streams, pats, flags, _ in batches])[0], batches, models)


def test_the_shared_code_under_the_sanitizers(tmp_path_factory, batches, models):
    """The check tool as a stand-alone program under AddressSanitizer and UBSan: no hop, probe or mark leaves the batch's bytes or a stream's chunks."""
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    lines, err = run([rec([s for s, _ in streams], pats, flags) for _, streams, pats, flags, _ in batches])
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check(lines, batches, models)
