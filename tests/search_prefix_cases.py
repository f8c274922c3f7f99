"""Inputs shared by the host and the GPU tests of the prefix search tables (types 2 and 3): the two prefix sets, and data with the designed
patterns planted — the smallest patterns at which the searcher's window rule can go wrong."""
import numpy as np

from minlz_amd import synth
from tests import search_cases as SC
from tests import search_model as SMod

SETS = {"json4": b'":, ', "nonalnum": SMod.NON_ALNUM}      # 4 values: table type 2; 194 values: type 3
PFX = ord(":")                                          # a prefix byte of both sets


def letters(n, seed):
    """n lower-case letters: in neither set."""
    return np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes()


def designed(kind, bs, nblk, tail, M, pset, seed=2, L=16):
    """bs * nblk + tail bytes of a synth kind (nblk >= 2, tail >= L) with the designed patterns planted -> (data, [(name, pattern)]):
      one_window   the only prefix byte at P[L - M - 1]: exactly one checkable window, the last one
      unusable     the only prefix byte at P[L - M]: no checkable window, the tables cannot serve it
      late_prefix  the only prefix byte is the last byte (L - M < L - 1 for M > 1): unusable as well
      border_last  an occurrence across a border whose prefix byte is the block's last byte: its window is position n of that block
      border_short one byte of the occurrence in the first block and P[0] no prefix byte: no window in the first block's table (t_min = 0)
      p0_in, p0_out  16 bytes of the data that start with / without a prefix byte
      absent       16 random bytes
      absent_keyed an absent pattern that starts like a JSON key: windows to check, none of them in the data"""
    d = bytearray(getattr(synth, kind)(bs * nblk + tail, seed).tobytes())
    mask = SMod.mask_of(*SMod.field_of(pset))
    one = letters(L - M - 1, seed + 10) + bytes([PFX]) + letters(M, seed + 11)
    unusable = letters(L - M, seed + 12) + bytes([PFX]) + letters(M - 1, seed + 13)
    late = letters(L - 1, seed + 14) + bytes([PFX])
    border = letters(3, seed + 15) + bytes([PFX]) + letters(L - 4, seed + 16)
    short = letters(2, seed + 17) + bytes([PFX]) + letters(L - 3, seed + 18)
    for o, p in ((bs // 3, one), (bs // 2, unusable), (bs // 2 + 100, late), (nblk * bs - 4, border), (bs * (nblk - 1) - 1, short)):
        d[o:o + len(p)] = p
    d = bytes(d)
    a = np.frombuffer(d, np.uint8)
    lo = bs // 4
    o_in = lo + int(np.flatnonzero(mask[a[lo:lo + 4096]])[0])
    o_out = lo + int(np.flatnonzero(~mask[a[lo:lo + 4096]])[0])
    pats = [("one_window", one), ("unusable", unusable), ("late_prefix", late), ("border_last", border), ("border_short", short),
            ("p0_in", d[o_in:o_in + L]), ("p0_out", d[o_out:o_out + L]), ("absent", bytes(SC.needle(16, 99))),
            ("absent_keyed", b'"zq":"' + letters(L - 6, seed + 19))]
    return d, pats


def planted_id(kind, bs, nblk, seed):
    """SC.planted's input with the needle b'"id":"' + SC.needle(10, seed) at the same three places."""
    d = getattr(synth, kind)(bs * nblk, seed).copy()
    nd = np.concatenate([np.frombuffer(b'"id":"', np.uint8), SC.needle(10, seed)])
    L = len(nd)
    at = [3 * bs + bs // 3, (nblk // 2) * bs + bs // 3, (nblk - 1) * bs - L // 2]
    for o in at:
        d[o:o + L] = nd
    return d.tobytes(), nd.tobytes(), at
