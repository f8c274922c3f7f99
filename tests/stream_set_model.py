"""The contract of a set of streams opened as one handle (include/minlz_hip_stream_set.h), in plain Python over a list of byte strings
(every stream's decoded bytes) and a set of failed indices (streams with a framing error: left out, size 0): bases, locate, the range
check, first[], joined and locate_records, by bytes.split and bisect.  tests/test_stream_set_host.py holds the shared C++ rules
(minlz_amd/csrc/mlz_stream_set.h) against it, tests/test_gpu_stream_set.py the library."""
import bisect

NO_STREAM = 0xFFFFFFFF


def sizes(datas, failed=()):
    return [0 if i in failed else len(d) for i, d in enumerate(datas)]


def concat(datas, failed=()):
    return b"".join(b"" if i in failed else d for i, d in enumerate(datas))


def bases(size):
    out = [0]
    for s in size:
        out.append(out[-1] + s)
    return out


def locate(base, p):
    """(stream, position inside it) of position p of the handle: the last i with base[i] <= p; (NO_STREAM, 0) for p >= size."""
    if p >= base[-1]:
        return NO_STREAM, 0
    i = bisect.bisect_right(base, p) - 1
    assert i < len(base) - 1 and base[i + 1] > p
    return i, p - base[i]


def range_global(base, which, off, length):
    """The first byte in the handle of range (which, off, length), or None where the range is refused."""
    if which >= len(base) - 1:
        return None
    s = base[which + 1] - base[which]
    if off > s or off + length > s:
        return None
    return base[which] + off


def records(data, delim):
    """data.split(delimiter) with one trailing empty piece dropped: the records of the record index."""
    pieces = data.split(bytes([delim]))
    if pieces[-1] == b"":
        pieces.pop()
    return pieces


def record_starts(data, delim):
    out, at = [], 0
    for r in records(data, delim):
        out.append(at)
        at += len(r) + 1
    return out


def first(base, data, delim):
    """first[i] = the records of `data` (the handle's bytes) that start below base[i]; first[count] = the record count."""
    starts = record_starts(data, delim)
    out = [bisect.bisect_left(starts, b) for b in base]
    assert out[-1] == len(starts)
    return out


def joined(base, data, delim):
    """Streams that have bytes, do not end with the delimiter and have a stream with bytes behind them."""
    return sum(1 for i in range(len(base) - 1) if base[i + 1] > base[i] and data[base[i + 1] - 1] != delim and base[i + 1] < base[-1])


def locate_record(base, data, delim, r):
    """(the stream in which record r starts, its number inside that stream); (NO_STREAM, 0) for r >= the record count."""
    starts = record_starts(data, delim)
    if r >= len(starts):
        return NO_STREAM, 0
    i, _ = locate(base, starts[r])
    return i, r - bisect.bisect_left(starts, base[i])


def grep_n(datas, failed, delim, match):
    """grep -n per stream, for a set whose joined is 0: [(stream, line number inside the stream (from 0), record)] of the records for
    which match(record) holds, in order."""
    out = []
    for i, d in enumerate(datas):
        if i in failed:
            continue
        out += [(i, k, r) for k, r in enumerate(records(d, delim)) if match(r)]
    return out
