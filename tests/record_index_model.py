"""The contract of the record index (include/minlz_hip.h: mlz_dev_reader_index_records and the calls that read it) in numpy, for
tests/test_stream_record_index_host.py and tests/test_gpu_stream_record_index.py: the delimiters' positions, N, the spans, the numbers."""
import numpy as np

NO_RECORD = (1 << 64) - 1


def delimiters(data, delim):
    """D: the positions of all bytes equal to the delimiter, ascending (int64)."""
    a = np.frombuffer(data if isinstance(data, bytes) else bytes(data), np.uint8)
    return np.flatnonzero(a == delim[0]).astype(np.int64)


def _count(D, size):
    k = len(D)
    return (k + 1 if size > 0 and (k == 0 or D[-1] != size - 1) else k), k


def count(data, delim):
    """-> (N, k): N = k + 1 when the data has bytes and its last one is no delimiter, else k."""
    return _count(delimiters(data, delim), len(data))


def spans(data, delim):
    """-> (start, length) of every record, two int64 arrays of N values: start(0) = 0, start(r) = D[r-1] + 1; end(r) = D[r], end(k) = size."""
    D = delimiters(data, delim)
    N, k = _count(D, len(data))
    start = np.concatenate([[0], D + 1])[:N].astype(np.int64)
    end = np.concatenate([D, [len(data)]])[:N].astype(np.int64)
    return start, end - start


def numbers(data, delim, pos):
    """The record number of every position: the count of D[j] < p, NO_RECORD for p >= size -> (a list, how many were inside)."""
    D = delimiters(data, delim)
    out = [int(np.searchsorted(D, p, side="left")) if p < len(data) else NO_RECORD for p in pos]
    return out, sum(1 for p in pos if p < len(data))


def record_range(data, delim, first, cnt):
    """Records first .. first + cnt - 1 as one range -> (off, len), or None when first + cnt > N."""
    N, _ = count(data, delim)
    if first + cnt > N:
        return None
    start, length = spans(data, delim)
    s = int(start[first]) if first < N else len(data)
    if cnt == 0:
        return s, 0
    return s, int(start[first + cnt - 1] + length[first + cnt - 1]) - s


def read(data, delim, idx):
    """What read_records writes -> (the packed bytes, the n + 1 starts)."""
    start, length = spans(data, delim)
    parts = [bytes(data[int(start[r]):int(start[r] + length[r])]) for r in idx]
    return b"".join(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64).tolist()
