"""The pre-fold rule of the batch Writer's search tables in plain Python, beside tests/search_model.py, and its check against that model.

A table's size comes from the call's block size (B = the bits of block_size - 1), not from the block; in a batch every stream's last block is
short.  A fold ORs the upper half of a table into the lower half, so a table folded r times is the bitmap of h & (2^(B - r) - 1).  The
Writer's rule (search_model.build_table) accepts fold r -> r + 1 while the folded table keeps 32 bytes (B - (r + 1) >= 8) and its set bits
are at most `limit` per cent of its 2^(B - r - 1) bits.  The set bits never exceed `marks`, the distinct window positions the block can
index, which follows from the block's length alone.  So with

    prefold(marks, B, limit) = the largest r with B - r >= 8 and marks * 100 <= 2^(B - r) * limit, 0 when no r >= 1 qualifies

the first r folds are certain to be accepted whatever the data, and the 70 % rule cannot fire (marks is at most a quarter of 2^(B - 1)).  A
builder may set bit h & (2^(B - r) - 1) in a table of 2^(B - r) bits and run the fold rule from R = r: build_prefolded below.  grid() is
the set of cases on which build_prefolded was held against build_table; tests/test_stream_encode_batch_tables_host.py runs it."""
import numpy as np

from minlz_amd import synth
from tests import search_model as SMod


def marks(cfg, n, follow):
    """The window positions a block of n bytes can index.  follow: the bytes that follow it in its stream (any number, b"" included), None
    for the stream's last block."""
    T, M, field = cfg
    nxt = follow is not None
    if T == 1:
        return n if nxt else max(n - M + 1, 0)
    if T in (2, 3):
        return n if nxt else max(n - M, 0)
    K, E, _ = SMod.parts_of(field)
    hi = n - 1 if nxt else n - K - M - E
    return hi + 1 + E if hi >= 0 else 0


def prefold(marks_, B, limit):
    for r in range(B - 8, 0, -1):
        if marks_ * 100 <= (1 << (B - r)) * limit:
            return r
    return 0


def build_prefolded(cfg, block, follow, B):
    """search_model.build_table by way of the pre-folded table -> (table bytes, R, r0)."""
    limit = SMod.fold_limit(cfg[0])
    r0 = prefold(marks(cfg, len(block), follow), B, limit)
    if r0 == 0:
        return SMod.build_table(cfg, block, follow, B) + (0,)
    bits = np.zeros(1 << (B - r0), dtype=bool)
    bits[SMod.indexed_hashes(cfg, block, follow, B) & np.uint32((1 << (B - r0)) - 1)] = True
    R = r0
    while len(bits) // 8 >= 64:
        half = len(bits) // 2
        m = bits[:half] | bits[half:]
        if int(m.sum()) * 100 > half * limit:
            break
        bits, R = m, R + 1
    return np.packbits(bits, bitorder="little").tobytes(), R, r0


BITS = (12, 16, 20, 22)
LENGTHS = (1, 5, 7, 8, 31, 100, 1000, 4095, 4096, 4097, 16384, 16385, 65536)
KINDS = ("json_like", "text_like", "random_bytes")
CONFIGS = [SMod.config(1, 6), SMod.config(1, 1), SMod.config(1, 2), SMod.config(1, 8), SMod.config(2, 6, b'":, '), SMod.config(2, 1, b'"'),
           SMod.config(3, 6, SMod.NON_ALNUM), SMod.config(4, 4, b'"user":"', 3), SMod.config(4, 1, b'"', 15)]


def follows():
    """None (the stream's last block), a following block of no bytes, of 2 bytes, of 300."""
    tail = synth.json_like(300, 7).tobytes()
    return [None, b"", tail[:2], tail]


def grid():
    """(cfg, B, block, follow) over every table size, length, kind of data, configuration and following bytes above."""
    data = {k: getattr(synth, k)(max(LENGTHS), 11).tobytes() for k in KINDS}
    for B in BITS:
        for n in LENGTHS:
            if n > 1 << B:
                continue
            for k in KINDS:
                for cfg in CONFIGS:
                    for f in follows():
                        yield cfg, B, data[k][:n], f
