"""Inputs shared by the host and the GPU tests of the long-prefix search tables (type 4): configurations, and data with the designed
patterns planted — the smallest patterns at which the searcher's group rule can go wrong."""
import numpy as np

from minlz_amd import synth
from tests import search_cases as SC

USER = b'"user":"'           # the natural prefix of synth.json_like
ID = b'"id":"'
ABSENT_USER = b'xy,"user":"qzjxkvwpqzj'


def letters(n, seed):
    """n lower-case letters: no byte of the prefixes used here."""
    return np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes()


def designed(kind, bs, nblk, tail, M, E, pfx, seed=2):
    """bs * nblk + tail bytes of a synth kind (nblk >= 4) with the designed patterns planted -> (data, [(name, pattern)]).  With
    K = len(pfx) >= 2 and W = M + E, the bytes one group needs behind its prefix:
      p0            the prefix at P[0] and W + 3 letters: one group, t_min = 1
      inside        4 letters, the prefix, W + 2 letters: one group, t_min = 0
      late          5 letters, the prefix, W - 1 letters: no whole group, the tables cannot serve it
      prefix_only   the prefix alone: out of scope, decodes everything
      two_groups    prefix, W letters, prefix, W letters, planted so that the second prefix starts on a block's first byte: one group per table
      straddle      3 letters, the prefix, W + 2 letters, planted so that a border cuts the prefix in two: the group lies in the first block's table
      ends_on_last  2 letters, the prefix, W + 1 letters, planted so that the prefix's last byte is a block's last byte
      natural       bytes of the data behind an occurrence of the prefix, where the data has one
      absent_keyed  an absent pattern with a group; absent: 16 random bytes (no group)"""
    K, W = len(pfx), M + E
    assert K >= 2 and nblk >= 4 and bs >= 4096
    d = bytearray(getattr(synth, kind)(bs * nblk + tail, seed).tobytes())
    p0 = pfx + letters(W + 3, seed + 10)
    inside = letters(4, seed + 11) + pfx + letters(W + 2, seed + 12)
    late = letters(5, seed + 13) + pfx + letters(W - 1, seed + 14)
    two = pfx + letters(W, seed + 15) + pfx + letters(W, seed + 16)
    straddle = letters(3, seed + 17) + pfx + letters(W + 2, seed + 18)
    ends = letters(2, seed + 19) + pfx + letters(W + 1, seed + 20)
    plants = ((bs // 3, p0), (bs // 2, inside), (bs // 2 + 1000, late), (bs - (K + W), two), (2 * bs - 3 - K // 2, straddle),
              (3 * bs - 2 - K, ends))
    for o, p in plants:
        d[o:o + len(p)] = p
    d = bytes(d)
    pats = [("p0", p0), ("inside", inside), ("late", late), ("prefix_only", pfx), ("two_groups", two), ("straddle", straddle), ("ends_on_last", ends),
            ("absent_keyed", b"xy," + pfx + letters(W + 3, seed + 21)), ("absent", bytes(SC.needle(16, 99)))]
    at = d.find(pfx, bs + bs // 4)
    if 0 <= at < len(d) - K - W - 8:
        pats.append(("natural", d[at:at + K + W + 4]))
        pats.append(("natural_inside", d[at - 3:at + K + W + 1]))
    return d, pats

