"""The plan of the device-resident ReadSeeker's range read without a GPU: tools/stream_ranges_check.cpp runs the library's own planner
(minlz_amd/csrc/mlz_stream_ranges.h) and executes the plan with memcpy; the destination image, the touched chunks and the scratch bytes
must be the brute-force model's (tests/stream_ranges_cases.py) for every stream of stream_device_cases.valid_streams_cpu() under every
range set, the scratch must stay within a group plus one block, and the argument rules that need no device are the planner's."""
import struct
import zlib

import numpy as np
import pytest

from minlz_amd import _lib
from tests import stream_device_cases as SC
from tests import stream_ranges_cases as RC
from tests.search_host import build_checker

ERR_DST_TOO_SMALL, ERR_ARG = 6, 8
MiB = 1 << 20


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    program = build_checker(tmp_path_factory, "stream_ranges_check.cpp")

    def run(cases):
        """cases: (grid or None = the case before's, ranges, dst_cap, data or None = plan only) -> a tuple of ints per case."""
        records = []
        for grid, ranges, cap, data in cases:
            flags = (1 if data is None else 0) | (2 if grid is None else 0)
            records.append(struct.pack("<4Q", len(grid or ()), len(ranges), cap, flags))
            if grid is not None:
                records.append(np.asarray(grid, dtype=np.uint64).reshape(-1, 2).tobytes())
            records.append(np.ascontiguousarray(ranges, dtype=np.uint64).tobytes())
            if grid is not None and data is not None:
                records.append(data)
        return [tuple(int(v) for v in line.split()) for line in program(records)[0]]
    return run


def test_exported():
    L = _lib.lib()
    assert L.mlz_stream_open_device and L.mlz_dev_reader_size and L.mlz_dev_reader_read and L.mlz_dev_reader_close


def test_valid_streams_every_range_set(checker):
    cases, want = [], []
    for name, s, d in SC.valid_streams_cpu():
        grid = RC.chunk_grid(s)
        assert sum(n for n, _ in grid) == len(d), name
        for k, (rname, ranges, cap) in enumerate(RC.range_sets(grid)):
            cases.append((grid if k == 0 else None, ranges, cap, d))
            touched, scratch = RC.model(grid, ranges)
            want.append(("%s/%s" % (name, rname), len(touched), scratch, zlib.crc32(RC.expected_image(d, ranges, cap).tobytes()), int(ranges[:, 1].sum())))
    got = checker(cases)
    assert len(got) == len(want)
    bad = []
    for (name, n_touched, scratch, crc, _), g in zip(want, got):
        rc, g_touched, g_scratch, g_extent, _, _, g_crc = g
        if rc != 0 or g_touched != n_touched or g_scratch != scratch or g_crc != crc or g_extent > g_scratch:
            bad.append("%s: tool %s, model touched %d scratch %d crc %d" % (name, g, n_touched, scratch, crc))
    assert not bad, "\n".join(bad[:20])
    kinds = {t for _, s, _ in SC.valid_streams_cpu() for _, t in RC.chunk_grid(s)}
    assert kinds == {0x01, 0x02, 0x03}   # stored, compressed and 0x03 chunks were all there


def test_scratch_is_bounded_by_a_group_plus_a_block(checker):
    """4 GiB in 8 MiB chunks, every chunk touched partly; then uneven chunks, where a group is closed by a chunk that takes it beyond 64 MiB."""
    even = [(8 * MiB, 0x02)] * 512
    uneven = [((5 * MiB + 12345) if i % 2 else 8 * MiB, 0x02) for i in range(600)]
    cases = []
    for grid in (even, uneven):
        starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])[:-1]])
        r = np.zeros((len(grid), 3), dtype=np.uint64)
        r[:, 0] = starts + 100
        r[:, 1] = 1000
        r[:, 2] = np.arange(len(grid)) * 1000
        cases.append((grid, r, 1000 * len(grid), None))
    got = checker(cases)
    for grid, g in zip((even, uneven), got):
        rc, touched, scratch, extent, groups, segs, _ = g
        assert rc == 0 and touched == len(grid) == segs
        assert scratch == sum(n for n, _ in grid)
        assert extent <= 64 * MiB + 8 * MiB, g
        assert groups >= scratch // (72 * MiB)
    assert got[0][3] == 64 * MiB and got[0][4] == 64


def test_groups_reuse_the_scratch(checker):
    """Bytes through three groups: the tool overwrites the scratch between two groups, so a segment that read another group's bytes shows."""
    rng = np.random.default_rng(5)
    grid = [(8 * MiB, 0x02)] * 9 + [(3 * MiB, 0x01)] + [(8 * MiB, 0x02)] * 9
    size = sum(n for n, _ in grid)
    d = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    starts = np.concatenate([[0], np.cumsum([n for n, _ in grid])[:-1]])
    pairs = [(int(s) + 3, 5000) for s in starts] + [(int(starts[4]), 8 * MiB), (int(starts[9]) - 10, 3 * MiB + 20)]
    r = np.zeros((len(pairs), 3), dtype=np.uint64)
    r[:, :2] = pairs
    r[:, 2] = np.cumsum(r[:, 1]) - r[:, 1] + 11
    cap = int(r[:, 1].sum()) + 30
    touched, scratch = RC.model(grid, r)
    (rc, g_touched, g_scratch, extent, groups, _, crc), = checker([(grid, r, cap, d)])
    assert rc == 0 and g_touched == len(touched) == 19 and g_scratch == scratch == 18 * 8 * MiB and groups == 3
    assert extent <= 72 * MiB
    assert crc == zlib.crc32(RC.expected_image(d, r, cap).tobytes())


def test_argument_rules(checker):
    grid = [(1000, 0x02), (500, 0x01), (1000, 0x03)]
    d = bytes(range(250)) * 10
    R = lambda *rows: np.array(rows, dtype=np.uint64).reshape(-1, 3)
    cases = [
        (grid, R((0, 2500, 0)), 2500, d),                            # 0: fits exactly
        (None, R((0, 2501, 0)), 4000, d),                            # 1: beyond the end
        (None, R((2500, 1, 0)), 4000, d),                            # 2: beyond the end
        (None, R((2501, 0, 0)), 4000, d),                            # 3: an empty range beyond the end
        (None, R((1 << 63, 1 << 63, 0)), 4000, d),                   # 4: off + len wraps
        (None, R((0, 100, 0), (200, 100, 99)), 4000, d),             # 5: destinations overlap by one byte
        (None, R((200, 100, 99), (0, 100, 0)), 4000, d),             # 6: the same, given the other way round
        (None, R((0, 100, 0), (200, 100, 100)), 4000, d),            # 7: destinations touch
        (None, R((0, 100, 0), (200, 0, 50), (300, 5, 100)), 4000, d),  # 8: an empty range inside another one's destination overlaps nothing
        (None, R((0, 100, 3901)), 4000, d),                          # 9: one byte too many for dst_cap
        (None, R((0, 100, 3900)), 4000, d),                          # 10: fits
        (None, R((0, 1, (1 << 64) - 1)), 4000, d),                   # 11: dst_off + len wraps
        (None, R((10, 5, 0), (10, 5, 5), (10, 5, 2)), 4000, d),      # 12: the same source three times, the third destination inside the others
        (None, R(), 0, d),                                           # 13: no range at all
    ]
    got = [g[0] for g in checker(cases)]
    assert got == [0, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, -ERR_ARG, 0, 0, -ERR_DST_TOO_SMALL, 0, -ERR_DST_TOO_SMALL, -ERR_ARG, 0]
