"""Inputs shared by the host and the GPU tests of the block search tables and mlz_dev_reader_search."""
import numpy as np

from minlz_amd import synth

KINDS = ("text_like", "json_like", "enwik_like")


def needle(L, seed):
    return np.random.default_rng(seed).integers(0, 256, L, dtype=np.uint8)


def planted(kind, block_size, n_blocks, L, seed=1, tail=0):
    """n_blocks * block_size + tail bytes of a synth kind with a random needle of L bytes planted inside block 3, inside the middle block and
    across the border between the last two whole blocks -> (data bytes, needle bytes, the planted positions)."""
    d = getattr(synth, kind)(block_size * n_blocks + tail, seed).copy()
    nd = needle(L, seed)
    at = [3 * block_size + block_size // 3, (n_blocks // 2) * block_size + block_size // 3, (n_blocks - 1) * block_size - L // 2]
    for o in at:
        d[o:o + L] = nd
    return d.tobytes(), nd.tobytes(), at


def patterns(data, M, block_size):
    """(name, pattern) for one stream: lengths 1, M - 1, M, M + 1, 16 and 256 taken from the data (inside a block and across a border), an
    overlapping run and an absent one."""
    out = []
    o = 5 * block_size // 3
    for L in sorted({1, max(1, M - 1), M, M + 1, 16, 256}):
        out.append(("inside_L%d" % L, data[o:o + L]))
        b = block_size - L // 2 if L > 1 else block_size
        out.append(("border_L%d" % L, data[b:b + L]))
    out.append(("absent", bytes(needle(16, 99))))
    return out
