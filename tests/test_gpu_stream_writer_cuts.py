"""Where the device-resident Writer's input is cut into ranges does not change the stream.  A range's last block indexes windows and prefixes
that run into the bytes behind it; the Writer hands those bytes over from the next non-empty range (StreamTables::overlap() of them, all four
table types by the same path).  For each table type: 4 KiB blocks, five whole blocks of text and a tail of t bytes, with an indexed
occurrence planted across every cut; every set of cuts must give the uncut stream, and the uncut stream is the model's splice
(tests/search_model.py).

Not vacuous: for every cut used, the model's table of the block in front of it changes when the bytes behind the cut are zeros (so a tail
that is lost, short or misplaced shows), and every whole block has a table (none is stored, none has its table dropped; the tail of a few
bytes behind them is too short to compress and is stored, as in every stream).

The type 4 prefix of 200 bytes starts 150 bytes before the end of block 4 where the stream is long enough to hold it (t = 100).  With
t = 3 and 9 the stream would end inside it and the rule indexes no such start, so there the occurrence ends on the stream's last byte: it
starts in block 4 and takes its last t bytes from the tail."""
import ctypes as C

import pytest

from minlz_amd import _lib, synth
from minlz_amd.api import search_long_prefix_config, search_tables_config
from tests import search_model as SMod
from tests import search_prefix_cases as PC
from tests.search_gpu import first_difference, gather_into

pytestmark = pytest.mark.gpu

BS, NBLK, M, E = 4 << 10, 5, 6, 3
B = SMod.table_bits(BS)
TAILS = (3, 9, 100)
CUT_SETS = ([2 * BS], [2 * BS, 2 * BS], [5 * BS], [BS, BS, 2 * BS, 2 * BS, 5 * BS])
CUTS = sorted({c for cs in CUT_SETS for c in cs})


def long_prefix(K):
    """K bytes that the text does not hold, and that do not overlap themselves."""
    return (b"<" + b"~" * (K - 2) + b">")[:K]


# name -> (keywords of HipCtx.stream_encode_gather_device, the prefix length K of type 4 or None)
CONFIGS = {
    "type1": (dict(search_match_len=M), None),
    "type2": (dict(search_match_len=M, search_prefix=PC.SETS["json4"]), None),
    "type3": (dict(search_match_len=M, search_prefix=PC.SETS["nonalnum"]), None),
    "type4_K12": (dict(search_match_len=M, search_long_prefix=long_prefix(12), search_extras=E), 12),
    "type4_K200": (dict(search_match_len=M, search_long_prefix=long_prefix(200), search_extras=E), 200),
}


def data_for_cuts(name, t):
    """Five blocks of text and t bytes, with what the table type indexes planted across every cut: prefix bytes as the last three bytes in front
    of the cut (types 2, 3: the last one's window lies wholly behind the cut; type 1 indexes every position anyway), the long prefix with its second half
    behind the cut (type 4), or, where the stream ends before that prefix and its windows would, ending on the stream's last byte."""
    kw, K = CONFIGS[name]
    n = NBLK * BS + t
    d = bytearray(synth.text_like(n, 11).tobytes())
    d[NBLK * BS:] = bytes(range(0x41, 0x41 + t))[:t] if t <= 26 else d[NBLK * BS:]   # a tail of letters: no zero byte in it
    for c in CUTS:
        if K is None:
            d[c - 3:c] = bytes([PC.PFX]) * 3
        else:
            g = c - 150 if (K, c) == (200, NBLK * BS) else c - K // 2
            if g + K + M + E > n:
                g = n - K
            d[g:g + K] = kw["search_long_prefix"]
    return bytes(d)


def model_config(name):
    kw, K = CONFIGS[name]
    if K is not None:
        return SMod.config(4, M, kw["search_long_prefix"], E)
    if "search_prefix" in kw:
        T, field = SMod.field_of(kw["search_prefix"])
        return T, M, field
    return SMod.config(1, M)


def model(name, off, d):
    """-> (the model's splice of the table-less stream `off`, its tables)"""
    return SMod.splice(off, d, model_config(name), B)


def block_table(name, block, follow):
    return SMod.build_table(model_config(name), block, follow, B)


def tail_matters(name, d):
    """For every cut: the table of the block in front of it, with the stream's bytes behind it and with zeros there, differ."""
    return all(block_table(name, d[c - BS:c], d[c:c + BS]) != block_table(name, d[c - BS:c], bytes(len(d[c:c + BS]))) for c in CUTS)


def bound(n, kw):
    L = _lib.lib()
    if "search_long_prefix" in kw:
        return L.mlz_stream_bound_long_prefix(n, BS, 0, C.byref(search_long_prefix_config(M, kw["search_long_prefix"], E)))
    if "search_prefix" in kw:
        return L.mlz_stream_bound_tables(n, BS, 0, C.byref(search_tables_config(M, kw["search_prefix"])))
    return L.mlz_stream_bound(n, BS, (4 | M << 8) if kw else 0)


def write(ctx, d, cuts, kw):
    at = [0] + list(cuts) + [len(d)]
    return gather_into(ctx, [d[at[i]:at[i + 1]] for i in range(len(at) - 1)], bound(len(d), kw), 1, BS, False, **kw)


@pytest.mark.parametrize("t", TAILS)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cuts_do_not_change_the_stream(ctx, name, t):
    kw, _ = CONFIGS[name]
    d = data_for_cuts(name, t)
    assert tail_matters(name, d), "the bytes behind a cut do not reach the table in front of it: the test would pass without them"
    off = write(ctx, d, [], {})
    one = write(ctx, d, [], kw)
    want, tables = model(name, off, d)
    assert len(tables) == NBLK + 1 and all(tb is not None for tb in tables[:NBLK]), "a block without a table"
    assert all(typ == 0x02 for _, typ in SMod.data_grid(off)[:NBLK]), "a stored block"
    assert one == want, "uncut: lengths %d / %d, first difference at %d" % (len(one), len(want), first_difference(one, want))
    for cuts in CUT_SETS:
        got = write(ctx, d, cuts, kw)
        assert got == one, "cuts %s: lengths %d / %d, first difference at %d" % (cuts, len(got), len(one), first_difference(got, one))
