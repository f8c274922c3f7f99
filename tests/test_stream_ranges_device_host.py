"""The device plan of mlz_dev_reader_read_device without a GPU: tools/stream_ranges_dev_check.cpp runs the kernels' own rules
(minlz_amd/csrc/mlz_stream_ranges_dev.h: the per-range pass, the difference arrays, the scans, the classification, the gather's piece search
and intersection arithmetic) as plain loops and executes the outcome with memcpy.  For every stream of stream_device_cases.valid_streams_cpu()
under every range set of stream_ranges_cases.range_sets (the (off, len) columns, destinations packed in the order given) and under generated
sets, the destination image must be the concatenation of the slices, touched chunks and scratch bytes the brute-force model's, and the plan
(touched list, each chunk's class, each place, the groups) what plan_ranges gives for the same ranges: the tool compares the two itself."""
import struct
import zlib

import numpy as np
import pytest

from minlz_amd import _lib
from tests import stream_device_cases as SC
from tests import stream_ranges_cases as RC
from tests.search_host import build_checker

ERR_DST_TOO_SMALL, ERR_ARG = 6, 8


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    program = build_checker(tmp_path_factory, "stream_ranges_dev_check.cpp")

    def run(cases):
        """cases: (grid or None = the case before's, pairs, dst_cap, data or None = plan only) -> a tuple of ints per case."""
        records = []
        for grid, pairs, cap, data in cases:
            flags = (1 if data is None else 0) | (2 if grid is None else 0)
            records.append(struct.pack("<4Q", len(grid or ()), len(pairs), cap, flags))
            if grid is not None:
                records.append(np.asarray(grid, dtype=np.uint64).reshape(-1, 2).tobytes())
            records.append(np.ascontiguousarray(pairs, dtype=np.uint64).tobytes())
            if grid is not None and data is not None:
                records.append(data)
        return [tuple(int(v) for v in line.split()) for line in program(records)[0]]
    return run


def packed(pairs):
    """(off, len) pairs -> (k, 3) ranges with destinations packed in the order given, and their total."""
    p = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    r = np.zeros((len(p), 3), dtype=np.uint64)
    r[:, :2] = p
    r[:, 2] = np.cumsum(p[:, 1]) - p[:, 1]
    return r, int(p[:, 1].sum())


def extra_sets(grid, seed=21):
    """Generated (name, pairs) the range sets of stream_ranges_cases do not have.  grid: [(n, type)] of a non-empty stream."""
    rng = np.random.default_rng(seed)
    size = sum(n for n, _ in grid)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])]).astype(np.int64)
    out = []
    offs = rng.integers(0, size, 1000)
    lens = np.minimum(rng.integers(1, 400, 1000), size - offs)
    out.append(("everything_and_1000_short", [(0, size)] + list(zip(offs.tolist(), lens.tolist()))))
    j = max(range(len(grid)), key=lambda k: grid[k][0])
    n = grid[j][0]
    offs = starts[j] + rng.integers(0, n, 100_000)
    lens = np.minimum(rng.integers(0, 70, 100_000), starts[j] + n - offs)
    out.append(("100000_in_one_chunk", list(zip(offs.tolist(), lens.tolist()))))   # (the index sum passes 2^32)
    # the same, and one more range at the highest index that covers ANOTHER chunk wholly and alone: its index must come out of the sum
    k = next((k for k in range(len(grid)) if k != j and grid[k][0]), None)
    if k is not None:
        out.append(("sole_toucher_at_a_high_index", list(zip(offs.tolist(), lens.tolist())) + [(int(starts[k]), grid[k][0])]))
    return out


def border_sets(grid):
    """Ranges that begin exactly on and one byte off EVERY chunk border."""
    size = sum(n for n, _ in grid)
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])]).astype(np.int64)
    pairs = []
    for b in sorted(set(starts.tolist())):
        for o, l in ((b, 1), (b, 40), (b - 1, 2), (b + 1, 3), (b - 1, 1), (b - 7, 7), (b, 0)):
            if 0 <= o and o + l <= size:
                pairs.append((o, l))
    return pairs


def _run_and_compare(checker, jobs):
    """jobs: (name, grid, pairs, data) with consecutive equal grids sharing one upload."""
    cases, want, last = [], [], None
    for name, grid, pairs, d in jobs:
        r, total = packed(pairs)
        cap = total + 5
        cases.append((grid if grid is not last else None, r[:, :2], cap, d))
        last = grid
        touched, scratch = RC.model(grid, r)
        want.append((name, len(touched), scratch, zlib.crc32(RC.expected_image(d, r, cap).tobytes()), total))
    got = checker(cases)
    assert len(got) == len(want)
    bad = []
    for (name, n_touched, scratch, crc, total), g in zip(want, got):
        rc, g_touched, g_scratch, g_extent, _, _, g_crc, g_total, diff = g
        if rc != 0 or diff or g_touched != n_touched or g_scratch != scratch or g_crc != crc or g_total != total or g_extent > g_scratch:
            bad.append("%s: tool %s, model touched %d scratch %d crc %d total %d" % (name, g, n_touched, scratch, crc, total))
    assert not bad, "\n".join(bad[:20])


def test_exported():
    assert _lib.lib().mlz_dev_reader_read_device and "mlz_dev_reader_read_device" in _lib.SYMBOLS


def test_valid_streams_every_range_set(checker):
    jobs = []
    for name, s, d in SC.valid_streams_cpu():
        grid = RC.chunk_grid(s)
        assert sum(n for n, _ in grid) == len(d), name
        for rname, ranges, _ in RC.range_sets(grid):
            jobs.append(("%s/%s" % (name, rname), grid, ranges[:, :2], d))
    _run_and_compare(checker, jobs)
    kinds = {t for _, s, _ in SC.valid_streams_cpu() for _, t in RC.chunk_grid(s)}
    assert kinds == {0x01, 0x02, 0x03}


def test_generated_sets(checker):
    jobs = []
    for name, s, d in SC.valid_streams_cpu():
        grid = RC.chunk_grid(s)
        if name.split("_idx")[0] not in ("oracle_L1_bs4096", "oracle_L1_bs65536", "oracle_L1_bs8388608", "oracle_L2_bs1048576", "skippables", "compcrc", "two_streams"):
            continue
        for rname, pairs in extra_sets(grid):
            jobs.append(("%s/%s" % (name, rname), grid, pairs, d))
    assert len(jobs) >= 18
    _run_and_compare(checker, jobs)


def test_tiny_chunks_with_empty_chunks_every_border(checker):
    s, d = SC.tiny_chunks()
    grid = RC.chunk_grid(s)
    assert len(grid) == 200
    # stored chunks of no bytes: in front, alone and in runs between the data chunks, at the very end
    holed = [(0, 0x01)]
    for k, c in enumerate(grid):
        holed.append(c)
        holed += [(0, 0x01)] * (k % 4 if k % 3 == 0 else 0)
    holed += [(0, 0x01)] * 2
    assert sum(1 for n, _ in holed if not n) > 60
    jobs = []
    for g, tag in ((grid, "tiny"), (holed, "tiny_holed")):
        jobs.append((tag + "/every_border", g, border_sets(g), d))
        for rname, ranges, _ in RC.range_sets(g):
            jobs.append(("%s/%s" % (tag, rname), g, ranges[:, :2], d))
        for rname, pairs in extra_sets(g):
            jobs.append(("%s/%s" % (tag, rname), g, pairs, d))
    _run_and_compare(checker, jobs)


def test_long_ranges_over_many_chunks_and_groups(checker):
    """Overlapping long ranges put every chunk through the scratch and are copied in 64 KiB pieces that cross chunks and group borders."""
    rng = np.random.default_rng(9)
    MiB = 1 << 20
    grid = [(8 * MiB, 0x02)] * 9 + [(3 * MiB, 0x01), (0, 0x01)] + [(8 * MiB - 77, 0x03)] * 9
    size = sum(n for n, _ in grid)
    d = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])]).astype(np.int64)
    short = [(int(o), int(l)) for o, l in zip(rng.integers(0, size - 2000, 3000), rng.integers(1, 2000, 3000))]
    sets = {
        "two_over_everything": [(0, size), (1, size - 1)],
        "everything_and_short": short[:1500] + [(0, size)] + short[1500:],
        "straddling_group_borders": [(int(starts[8]) - 3, 9), (int(starts[8]) - 70_000, 140_001), (int(starts[16]) - 1, 2), (int(starts[16]) - 1025, 2050), (5, 0)],
        "short_alone": short,
        "one_direct_middle": [(int(starts[3]), 8 * MiB), (int(starts[12]) + 1, 8 * MiB - 77)],
    }
    jobs = [(k, grid, v, d) for k, v in sets.items()]
    cases = [(grid, packed(sets["two_over_everything"])[0][:, :2], 2 * size - 1, d)]
    (rc, touched, scratch, extent, groups, pieces, _, total, diff), = checker(cases)
    assert rc == 0 and diff == 0 and touched == 19 and groups == 3 and scratch == 18 * 8 * MiB - 9 * 77 and extent <= 72 * MiB and pieces == 2 * ((size + 65535) >> 16) and total == 2 * size - 1
    _run_and_compare(checker, jobs)


def test_argument_rules(checker):
    grid = [(1000, 0x02), (500, 0x01), (1000, 0x03)]
    d = bytes(range(250)) * 10
    ok = [(10 * i % 2400, 7) for i in range(3000)]
    P = lambda *rows: np.array(rows, dtype=np.uint64).reshape(-1, 2)
    cases = [
        (grid, P((0, 2500)), 2500, d),                               # 0: fits exactly
        (None, P((0, 2500)), 2499, d),                               # 1: the total is dst_cap + 1
        (None, P(*ok), 21000, d),                                    # 2: many ranges, the total is dst_cap
        (None, P(*ok), 20999, d),                                    # 3: and dst_cap + 1
        (None, P((0, 2501), *ok), 1 << 40, d),                       # 4: beyond the end at index 0
        (None, P(*ok[:1500], (2500, 1), *ok[1500:]), 1 << 40, d),    # 5: in the middle (off == size, len == 1)
        (None, P(*ok, (2400, 101)), 1 << 40, d),                     # 6: at the last index
        (None, P((2501, 0)), 4000, d),                               # 7: an empty range beyond the end
        (None, P(((1 << 64) - 1, 1)), 4000, d),                      # 8: an int64 -1 as the offset
        (None, P((1, (1 << 64) - 1)), 4000, d),                      # 9: as the length
        (None, P((1 << 63, 1 << 63)), 4000, d),                      # 10: off + len wraps
        (None, P((0, 2501)), 100, d),                                # 11: beyond the end AND too much for dst_cap: the range rule comes first
        (None, P((2500, 0), (0, 0)), 0, d),                          # 12: empty ranges at the very end and the start ask for nothing
        (None, P(), 0, d),                                           # 13: no range at all
    ]
    got = checker(cases)
    assert [g[0] for g in got] == [0, -ERR_DST_TOO_SMALL, 0, -ERR_DST_TOO_SMALL, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, 0, 0]
    assert all(g[8] == 0 for g in got), got   # plan_ranges decides every case the same way
    assert got[2][7] == 21000 and got[2][6] == zlib.crc32(RC.expected_image(d, packed(ok)[0], 21000).tobytes())
