"""The staging rule of the scratch decode without a GPU: tools/stream_scratch_check.cpp runs minlz_amd/csrc/mlz_stream_scratch.h over staged
lists and then executes the result as loops (per group a scratch of exactly scratch_max bytes, the group's copies, the compressed chunks'
bytes, every job's bytes compared), plain and under AddressSanitizer and UBSan; the figures it prints are compared with a count in Python."""
import struct

import numpy as np
import pytest

from tests import search_host as H
from tests.search_host import both

SRC = "stream_scratch_check.cpp"
PIECE = 64 << 10
STORED, COMPRESSED, COMPRESSED_CRC = 1, 2, 3


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def staged(chunks, groups, pad=0, seed=1):
    """chunks: [(type, n)] of a stream; groups: per group the chunks it holds, side by side from scratch[pad] on (a chunk may be a job of two
    groups).  -> (the record, the line the program must print).  A stored chunk's body is its bytes; a compressed chunk's body is other
    bytes of half the length."""
    rng = np.random.default_rng(seed)
    stream, body_off, data = bytearray(b"\xff\x06\x00\x00MinLz\x06"), [], []
    for t, n in chunks:
        stream += bytes(8)
        body_off.append(len(stream))
        data.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        stream += data[-1] if t == STORED else rng.integers(0, 256, n // 2 + 1, dtype=np.uint8).tobytes()
    jobs, gend, ends, pieces, smax = [], [], [], 0, 0
    for g in groups:
        o = pad
        for k in g:
            t, n = chunks[k]
            jobs.append((k, o))
            pieces += (n + PIECE - 1) // PIECE if t == STORED else 0
            o += n
            smax = max(smax, o)
        gend.append(len(jobs))
        ends.append(pieces)
    rec = struct.pack("<IIIQ", 1, len(jobs), len(groups), len(stream))
    rec += b"".join(struct.pack("<IQQQ", chunks[k][0], chunks[k][1], body_off[k], at) for k, at in jobs)
    rec += np.asarray(gend, np.uint64).tobytes() + bytes(stream) + b"".join(data[k] for k, _ in jobs)
    return rec, "places %d ends%s max %d" % (pieces, "".join(" %d" % e for e in ends), smax)


C, X, S = COMPRESSED, COMPRESSED_CRC, STORED
CASES = {
    "no stored chunk": ([(C, 700), (X, 300), (C, 5000)], [[0, 1], [2]]),
    "only stored chunks": ([(S, 700), (S, 300), (S, 5000)], [[0, 1], [2]]),
    "stored first in groups 1 and 2": ([(C, 900), (C, 400), (S, 333), (C, 800), (S, 1), (X, 450)], [[0, 1], [2, 3], [4, 5]]),
    "stored last in groups 1 and 2": ([(S, 900), (C, 400), (C, 333), (S, 800), (X, 64), (S, 450)], [[0, 1], [2, 3], [4, 5]]),
    "a piece, a piece and a byte, a byte": ([(S, PIECE), (C, 100), (S, PIECE + 1), (S, 1), (C, 7)], [[0, 1], [2], [3, 4]]),
    "three pieces and a rest in the second group": ([(C, 300), (S, 3 * PIECE + 77), (C, 12)], [[0], [1, 2]]),
    # the sidecar build: the next group's first chunk lies behind a group's last one, and is staged in both
    "sidecar: a stored overlap chunk": ([(C, 600), (C, 500), (S, PIECE + 40), (C, 300), (S, 90)], [[0, 1, 2], [2, 3, 4], [4]]),
    "sidecar: a compressed overlap chunk": ([(S, 600), (C, 500), (C, 400), (S, 300)], [[0, 1, 2], [2, 3]]),
    "no job at all": ([], []),
    "an empty chunk beside a stored one": ([(S, 0), (S, 10), (C, 0)], [[0, 1, 2]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_staged_lists(checkers, name):
    chunks, groups = CASES[name]
    # from scratch[0] on as the record index and the sidecar build lay a group, and behind a pad as the searches do
    recs = [staged(chunks, groups, pad, seed) for seed, pad in enumerate((0, 256))]
    assert both(checkers, [r for r, _ in recs]) == [w for _, w in recs]


def test_the_program_sees_a_wrong_list(checkers):
    """The check is not vacuous: a stored chunk whose body offset is one too low does not put its bytes into the scratch."""
    rec, _ = staged([(C, 100), (S, 200)], [[0], [1]])
    head = struct.calcsize("<IIIQ") + struct.calcsize("<IQQQ") + struct.calcsize("<IQ")
    (off,) = struct.unpack_from("<Q", rec, head)
    bad = rec[:head] + struct.pack("<Q", off - 1) + rec[head + 8:]
    with pytest.raises(AssertionError, match="not in the scratch"):
        checkers[0]([bad])


def whole(chunks, groups, size):
    """chunks: [(n, out_off)] of a chunk table; groups: per group how many of the chunks WITH bytes it holds, in order.  -> (the record,
    the line the program must print): the count below is whole_stream_list's rule in Python."""
    dc = [k for k, (n, _) in enumerate(chunks) if n]
    gend = list(np.cumsum(groups, dtype=np.int64)) if groups else []
    rec = struct.pack("<IIIQ", 3, len(chunks), len(gend), size)
    rec += b"".join(struct.pack("<QQ", n, off) for n, off in chunks) + np.asarray(gend, np.uint64).tobytes()
    spans, at, pos, i = [], [], 0, 0
    for e in gend:
        first, o = chunks[dc[i]][1] if i < e else pos, 0
        for k in dc[i:e]:
            if chunks[k][1] != first + o:
                return rec, "status 1"
            at.append(o)
            o += chunks[k][0]
        i = e
        spans.append((first, o))
        if o == 0 or first != pos or pos + o > size:
            return rec, "status 2"
        pos += o
    if pos != size:
        return rec, "status 2"
    return rec, "status 0 groups%s at%s" % ("".join(" %d+%d" % s for s in spans), "".join(" %d" % a for a in at))


# (chunks as (n, out_off), the groups' job counts, the decoded size) -> the status
WHOLE = {
    "one group": ([(700, 0), (300, 700), (5000, 1000)], [3], 6000, 0),
    "three groups, empty chunks between and at both ends": ([(0, 0), (90, 0), (10, 90), (0, 100), (0, 100), (400, 100), (0, 500), (7, 500), (1, 507), (0, 508)], [2, 1, 2], 508, 0),
    "an out_off one too high inside a group": ([(700, 0), (300, 701), (50, 1001)], [2, 1], 1051, 1),
    "a gap between two groups": ([(700, 0), (300, 700), (50, 1001)], [2, 1], 1051, 2),
    "the first group does not start at 0": ([(700, 1), (300, 701)], [1, 1], 1001, 2),
    "the last group ends short of the size": ([(700, 0), (300, 700)], [1, 1], 1001, 2),
    "the last group ends beyond the size": ([(700, 0), (300, 700)], [1, 1], 999, 2),
    "a group without a chunk": ([(700, 0), (300, 700)], [1, 0, 1], 1000, 2),
    "no chunk with bytes, size 0": ([(0, 0), (0, 0)], [], 0, 0),
    "no chunk with bytes, size 5": ([(0, 0)], [], 5, 2),
}


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_stream_list(checkers, name):
    chunks, groups, size, status = WHOLE[name]
    rec, want = whole(chunks, groups, size)
    assert want.startswith("status %d" % status)
    assert both(checkers, [rec]) == [want]


def test_chunks_with_bytes(checkers):
    sizes = [0, 5, 0, 0, 1, 1 << 40, 0]
    recs = [struct.pack("<II", 2, len(s)) + np.asarray(s, np.uint64).tobytes() for s in (sizes, [], [0, 0])]
    assert both(checkers, recs) == ["with bytes 1 4 5", "with bytes", "with bytes"]
