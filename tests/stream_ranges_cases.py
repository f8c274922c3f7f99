"""Range sets and the brute-force model for the device-resident ReadSeeker's tests (tests/test_stream_ranges_host.py on the host,
tests/test_gpu_stream_ranges.py on the GPU).  A range set is (name, ranges, dst_cap): ranges an (k, 3) uint64 array of (off, len, dst_off).
Deterministic: every choice comes from a seeded generator."""
import numpy as np

from minlz_amd import stream as S
from tests import corrupt as CM

FILL = 0xA5
GROUP = 64 << 20


def chunk_grid(stream):
    """The data chunks of a stream with valid framing, in order -> [(decoded length, type)] (tests/corrupt.py's chunk list)."""
    out = []
    for c in CM.chunks(stream):
        if c.type == 0x01:
            out.append((c.clen - 4, 0x01))
        elif c.type in (0x02, 0x03):
            out.append((S.uvarint(stream, c.off + 8)[0], c.type))
    return out


def _layout(pairs, rng, shuffled):
    """(off, len) pairs -> ranges with destinations: packed in the order given, or in shuffled order with gaps of 0 - 40 bytes."""
    k = len(pairs)
    r = np.zeros((k, 3), dtype=np.uint64)
    if k:
        r[:, :2] = np.asarray(pairs, dtype=np.uint64).reshape(k, 2)
    order = rng.permutation(k) if shuffled else np.arange(k)
    pos = int(rng.integers(0, 30)) if shuffled else 0
    for i in order:
        r[i, 2] = pos
        pos += int(r[i, 1]) + (int(rng.integers(0, 41)) if shuffled else 0)
    return r, pos + (7 if shuffled else 0)


def range_sets(grid, seed=1):
    """The sets every stream is read with (the issue's list).  grid: [(n, type)]."""
    rng = np.random.default_rng(seed)
    size = sum(n for n, _ in grid)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])]).astype(np.int64) if grid else np.zeros(1, np.int64)
    sets = []

    def add(name, pairs, shuffled=True):
        pairs = [(int(o), int(l)) for o, l in pairs if 0 <= o and o + l <= size and l >= 0]
        r, cap = _layout(pairs, rng, shuffled)
        sets.append((name, r, cap))

    add("empty_ranges_only", [(0, 0), (size, 0), (size // 2, 0)])
    if size == 0:
        add("whole", [(0, 0)], shuffled=False)
        return sets
    add("first_and_last_byte", [(0, 1), (size - 1, 1)])
    add("whole", [(0, size)], shuffled=False)
    add("whole_shifted", [(0, size)])
    if size >= 3:
        add("all_but_the_ends", [(1, size - 2)], shuffled=False)
    # chunk borders: ranges that end and start exactly on them, one byte before and after
    inner = [int(b) for b in starts[1:-1]]
    picks = sorted(set(inner[:2] + inner[-2:] + ([inner[len(inner) // 2]] if inner else [])))
    pairs = []
    for b in picks:
        pairs += [(b - 5, 5), (b, 5), (b - 6, 5), (b + 1, 5), (b - 3, 6), (b - 1, 1), (b, 1)]
    if pairs:
        add("borders", pairs)
        b = picks[len(picks) // 2]
        nxt = int(starts[np.searchsorted(starts, b) + 1])
        add("one_chunk_exactly_and_neighbours", [(b, nxt - b), (b - 1, 1), (nxt, 1)] if nxt < size else [(b, nxt - b), (b - 1, 1)])
    q = size // 3
    add("same_range_five_times", [(q, min(700, size - q))] * 5)
    add("nested_and_overlapping", [(q, min(5000, size - q)), (q + 10, min(100, size - q - 10)), (q + 50, min(4950, size - q - 50)), (max(q - 40, 0), 100), (0, size), (q, 1)])
    offs = rng.integers(0, size, 10_000)
    lens = np.minimum(rng.integers(1, 601, 10_000), size - offs)
    add("ten_thousand_short", list(zip(offs, lens)), shuffled=False)
    add("ten_thousand_short_shuffled", list(zip(offs[:3000], lens[:3000])))
    add("mixed_with_empty", [(q, 0), (q, 300 if size - q >= 300 else size - q), (size, 0), (0, 0), (size - 1, 1), (q + 1, 0)])
    return sets


def expected_image(data, ranges, dst_cap):
    img = np.full(dst_cap, FILL, dtype=np.uint8)
    d = np.frombuffer(data, dtype=np.uint8)
    for off, ln, dst in ranges.tolist():
        img[dst:dst + ln] = d[off:off + ln]
    return img


def model(grid, ranges):
    """Brute force over the chunk grid -> (touched chunk indices, scratch bytes): a chunk is touched when it shares a byte with a range; a touched
    compressed chunk stays out of the scratch only when exactly one range touches it and that range covers it wholly."""
    offs, lens = ranges[:, 0].astype(np.int64), ranges[:, 1].astype(np.int64)
    ends = offs + lens
    touched, scratch, start = set(), 0, 0
    for j, (n, ty) in enumerate(grid):
        hit = (lens > 0) & (offs < start + n) & (ends > start)
        if n and hit.any():
            touched.add(j)
            if ty != 0x01 and not (hit.sum() == 1 and (offs[hit] <= start).all() and (ends[hit] >= start + n).all()):
                scratch += n
        start += n
    return touched, scratch
