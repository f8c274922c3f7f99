"""What the tests of the stored record index share (tests/test_record_index_store_host.py, tests/test_gpu_record_index_store.py): the shapes — the
smallest at which a kernel can go wrong — as (name, size, D), and the corruptions of a model blob with the error each must end in."""
import struct

import numpy as np

from tests import record_index_store_model as M

DELIM = 10
T = M.TILE


def _d(*pos):
    return np.array(sorted(pos), dtype=np.uint64)


def _every(lo, hi, step=1):
    return np.arange(lo, hi, step, dtype=np.uint64)


def shapes():
    """[(name, size, D)]: every delimiter position of a stream of `size` bytes."""
    rng = np.random.default_rng(7)
    text = np.sort(rng.choice(T + 1, 1500, replace=False)).astype(np.uint64)
    return [
        ("size 0", 0, _d()),
        ("one byte, the delimiter", 1, _d(0)),
        ("no delimiter", 1000, _d()),
        ("size 65536", T, text[text < T]),
        ("size 65537", T + 1, np.unique(np.append(text, np.uint64(T)))),
        ("delimiters at 65535 and 65536", 70000, _d(T - 1, T)),
        ("a tile of 4096 and one of 4097", 3 * T - 11, np.concatenate([_every(0, T, 16), _every(T, T + 4097 * 15, 15), _d(2 * T + 5)])),
        ("a tile that is all delimiters", 3 * T, np.concatenate([_d(3, 77), _every(T, 2 * T), _d(3 * T - 1)])),
        ("a dense last tile cut by the size", T + 30001, np.concatenate([_d(9), _every(T, T + 30001)])),
        ("an odd sparse count", 5000, _d(1, 2, 4999)),
        ("70000 empty records", 70000, _every(0, 70000)),
    ]


TWO_SECTIONS_SIZE = (64 << 20) + T + 1


def two_sections():
    """64 MiB + 65537 bytes: delimiters at 67 108 863 and 67 108 864 (the sections' border) and a dense tile in the second section."""
    b = 64 << 20
    return "two sections", TWO_SECTIONS_SIZE, np.concatenate([_d(5, b - 1), _every(b, b + 5000 * 13, 13), _d(TWO_SECTIONS_SIZE - 1)])


def data_of(size, D, fill=97):
    d = np.full(size, fill, np.uint8)
    d[D.astype(np.int64)] = DELIM
    return d


# ---- corruptions ----

BASE_SIZE = 3 * T + 30000     # tile 0 sparse with an odd count, tile 1 empty, tile 2 all delimiters, tile 3 dense and cut by the size
BASE_D = np.concatenate([_d(7, 300, 301, 40000, T - 1), _every(2 * T, 3 * T), _every(3 * T, 3 * T + 29990, 2)])
SMALL_SIZE = T + 100          # tile 1 sparse and cut by the size
SMALL_D = _d(5, T + 3, T + 50)


def _u16(sec, off, v):
    sec[off:off + 2] = struct.pack("<H", v)


def corruptions(base, small):
    """base, small: the model's blobs of (BASE_D, BASE_SIZE) with a binding and a longest record, and of (SMALL_D, SMALL_SIZE).
    -> [(name, which ("base" / "small"), blob, ignore_crc, the code the load must return)]"""
    C, U, A, X = M.ERR_CORRUPT, M.ERR_UNSUPPORTED, M.ERR_ARG, M.ERR_CRC
    h = M.parse(base)[0]
    head0 = 16 + 4 * 5          # section 0's head: 4 tiles
    p0 = head0                  # tile 0's payload: 5 entries and a pad
    p2 = p0 + 12                # tile 2's bitmap (tile 1 is empty)
    p3 = p2 + M.BITMAP          # tile 3's bitmap
    out = [
        ("magic", "base", M.reheader(base, magic=b"MLZRIDX2"), False, U),
        ("flags: an unknown bit", "base", M.reheader(base, flags=h["flags"] | 4), False, C),
        ("flags: unbound with a tag", "base", M.reheader(base, flags=h["flags"] & ~1), False, C),
        ("flags: longest unknown with a value", "base", M.reheader(base, flags=h["flags"] & ~2), False, C),
        ("delimiter: the padding", "base", M.reheader(base, pad=b"\0\1\0"), False, C),
        ("size", "base", M.reheader(base, size=h["size"] + 1), False, A),
        ("k", "base", M.reheader(base, k=h["k"] + 1, N=h["N"]), False, C),
        ("N", "base", M.reheader(base, N=h["N"] - 1), False, C),
        ("longest", "base", M.reheader(base, longest=h["size"] + 1), False, C),
        ("stream tag", "base", M.reheader(base, tag=h["tag"] ^ 1), False, A),
        ("data chunks", "base", M.reheader(base, data_chunks=h["data_chunks"] + 1), False, A),
        ("nsections", "base", M.reheader(base, nsections=2), False, C),
        ("the trailing u16", "base", M.reheader(base, zero=1), False, C),
    ]

    def directory(secs, _):
        return [len(secs[0]) + 4]
    out.append(("the directory", "base", M.refit(base, directory), False, C))

    def descend(secs, _):
        secs[0][16 + 8:16 + 12] = struct.pack("<I", 3)      # counts 0 5 3 ...
    out.append(("counts that descend", "base", M.refit(base, descend), False, C))

    def section_number(secs, _):
        secs[0][0:4] = struct.pack("<I", 1)
    out.append(("the section's number", "base", M.refit(base, section_number), False, C))

    def first_rank(secs, _):
        secs[0][8:16] = struct.pack("<Q", 1)
    out.append(("the section's first rank", "base", M.refit(base, first_rank), False, C))

    def disorder(secs, _):
        _u16(secs[0], p0 + 2, 301)
        _u16(secs[0], p0 + 4, 300)
    out.append(("a sparse list out of order", "base", M.refit(base, disorder), False, C))

    def repeat(secs, _):
        _u16(secs[0], p0 + 4, 300)
    out.append(("a sparse entry twice", "base", M.refit(base, repeat), False, C))

    def pad(secs, _):
        _u16(secs[0], p0 + 10, 1)
    out.append(("a sparse pad that is not zero", "base", M.refit(base, pad), False, C))

    def beyond(secs, _):
        _u16(secs[0], 16 + 4 * 3 + 4 + 2, 100)             # tile 1 of `small`: entries 3, 50 -> 3, 100 = the size
    out.append(("a sparse entry at the size", "small", M.refit(small, beyond), False, C))

    def popcount(secs, _):
        secs[0][p2 + 100] &= 0xFE
    out.append(("a dense popcount off by one", "base", M.refit(base, popcount), False, C))

    def dense_beyond(secs, _):
        secs[0][p3] &= 0xFE                                 # position 0 of tile 3 leaves, position 30000 = the size comes
        secs[0][p3 + 30000 // 8] |= 1 << (30000 % 8)
    out.append(("a dense bit at the size", "base", M.refit(base, dense_beyond), False, C))

    sec0 = M.parse(base)[1][0][0]
    flipped = bytearray(base)
    flipped[sec0 + p0 + 1] ^= 0xFF                          # the first entry's high byte: 7 -> 0xff07, above its neighbour
    out.append(("a flipped payload byte", "base", bytes(flipped), False, X))
    out.append(("a flipped payload byte, CRCs ignored", "base", bytes(flipped), True, C))
    stale = bytearray(base)
    stale[M.FIXED_AT + 40] ^= 1                             # the longest record, within the size: only the header's CRC knows
    out.append(("a flipped header byte", "base", bytes(stale), False, X))
    frame = bytearray(base)
    frame[sec0 - 8] = 0x92
    out.append(("a section chunk of another type", "base", bytes(frame), False, C))
    eof = bytearray(base)
    eof[-1] = 1
    out.append(("an EOF chunk with a size", "base", bytes(eof), False, C))
    out += [
        ("truncated by a byte", "base", base[:-1], False, C),
        ("truncated inside the header", "base", base[:40], False, C),
        ("truncated inside the first section", "base", base[:sec0 + 10], False, C),
        ("trailing bytes", "base", base + b"\0\0\0\0", False, C),
    ]
    return out
