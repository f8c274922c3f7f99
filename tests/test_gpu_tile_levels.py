"""The decoder's tile-level classification on hand-built blocks (tests/tile_levels.py): blocks next to the rule — legal by one byte,
illegal by one byte, legal for one pattern only, illegal only through a carried repeat — decoded 8 to a batch into sentinel-filled
buffers, under the option settings that change the schedule.  The bytes must be the oracle's, and the counters of general blocks
(mlz_get_counter 2) and of the team size (6) must be what the restatement predicts.  Each case's intended verdict is pinned to
tile_levels.verdict() by tests/test_tile_levels.py; blocks of real encoders are checked against verdict() directly here.

A wrong schedule shows up in the bytes: a source tile is slow to decode (1-byte literals and short copies), the tile reading it fast
(a few long copies), and every tile's bytes are its own."""
import numpy as np
import pytest

import minlz_amd as mz
import oracle as O
from minlz_amd import synth
from minlz_amd._lib import BlockDesc
from tests import tile_levels as TL
from tests.tile_levels_gpu import check_single as _check_single

pytestmark = pytest.mark.gpu

OPT_DECODE_ALGO, OPT_GENERAL_ALGO, OPT_HOST_GROUP_DEC, OPT_DEVICE_GROUP, OPT_L2_GAP, OPT_LEVEL0_BY_E = 1, 8, 11, 17, 19, 23
COPIES = 8


def _decode_batch(ctx, blocks, sizes):
    """decode_batch_device into a sentinel-filled buffer; bytes outside the blocks' ranges must stay untouched."""
    import torch
    dev = torch.device("cuda", 0)
    offs, cur = [], 0
    for b in blocks:
        offs.append(cur)
        cur += len(b) + 16
    host = np.zeros(cur + 64, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    src = torch.from_numpy(host).to(dev)
    doffs, dcur = [], 0
    for n in sizes:
        doffs.append(dcur)
        dcur += n + 48
    dst = torch.full((dcur + 64,), 0xA5, dtype=torch.uint8, device=dev)
    dlen = torch.zeros(len(blocks), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx.decode_batch_device(st, src.data_ptr(), dst.data_ptr(), [BlockDesc(o, len(b), do, n) for o, b, do, n in zip(offs, blocks, doffs, sizes)], dlen.data_ptr())
    torch.cuda.synchronize()
    dh = dst.cpu().numpy()
    guard = np.ones(dh.size, dtype=bool)
    for do, n in zip(doffs, sizes):
        guard[do:do + n] = False
    assert (dh[guard] == 0xA5).all(), "bytes outside the blocks' output ranges were written"
    return dlen.cpu().tolist(), [dh[do:do + n].tobytes() for do, n in zip(doffs, sizes)]


def _small_case():
    b = TL.Block(2, 77, dlen=40_000)
    return b.case("small_conformant")


def _batches():
    """(name, [cases]) in decode order; no batch follows one of the same bytes."""
    named = {c.name: c for c in TL.cases("named")}
    out = [(c.name, [c] * COPIES) for c in TL.cases("named")]
    out += [(c.name, [c] * COPIES) for c in TL.cases("big")]
    sweep = TL.cases("sweep")
    out += [("sweep_%d" % i, sweep[i:i + 8]) for i in range(0, len(sweep), 8)]
    gen, con, small = named["team_nearest_2_back"], named["fits_fast_only"], _small_case()
    out.append(("mixed_general_first", [gen, con] * (COPIES // 2)))
    out.append(("mixed_conformant_first", [con, gen] * (COPIES // 2)))
    out.append(("mixed_small_after_general", [gen, small, gen, small, con, small]))
    return out


def _expected_team(cases, how):
    teams = [c.intended.team for c in cases if c.intended.general]
    if not teams:
        return 0
    if how == "groups":     # one block per internal group: the largest over the groups
        return max(teams)
    return min(teams)       # one group: the smallest of the batch (fewer than 16 general blocks: no cap by the settling workgroups)


LEGS = [
    ("default", {}, "batch"),
    ("level0_by_exec", {OPT_LEVEL0_BY_E: 0}, None),
    ("general_on_tile_chain", {OPT_GENERAL_ALGO: 1}, None),
    ("serial", {OPT_DECODE_ALGO: 1}, None),
    ("all_on_tile_path", {OPT_DECODE_ALGO: 3}, None),
    ("device_groups_1mib", {OPT_DEVICE_GROUP: 1}, "groups"),
]


@pytest.mark.parametrize("leg,opts,counts", LEGS, ids=[l[0] for l in LEGS])
def test_hand_built_blocks(leg, opts, counts):
    ctx = mz.Context(0)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        bad = []
        for name, cs in _batches():
            assert sum(c.intended.general for c in cs) <= 16
            lens, outs = _decode_batch(ctx, [TL.encode_block(c.body, c.dlen) for c in cs], [c.dlen for c in cs])
            for i, (c, l, o) in enumerate(zip(cs, lens, outs)):
                if l != c.dlen or o != c.expected:
                    first = next((j for j in range(min(len(o), len(c.expected))) if o[j] != c.expected[j]), None)
                    bad.append("%s[%d] %s: len %d, first wrong byte %s (tile %s)" % (name, i, c.name, l, first, None if first is None else first // TL.TILE))
            if counts:
                got = (ctx.general_blocks(), ctx.general_team())
                want = (sum(c.intended.general for c in cs), _expected_team(cs, counts))
                if got != want:
                    bad.append("%s: (general blocks, team) %s, restated %s" % (name, got, want))
        assert not bad, "\n".join(bad)
    finally:
        ctx.close()


def test_oracle_blocks_against_the_restatement(ctx):
    seen = set()
    for size in ((32 << 10) + 1, 64 << 10, 96 << 10, 1 << 20, 3 << 20):
        for kind, gen in (("text", synth.text_like), ("json", synth.json_like)):
            src = np.ascontiguousarray(gen(size, seed=size & 0xFFFF)).tobytes()
            for level in (1, 2, 3):
                v = _check_single(ctx, O.encode(src, level), src, (kind, size, level))
                seen.add(v.general)
    assert seen == {False, True}


def test_own_blocks_against_the_restatement(ctx):
    for size in ((32 << 10) + 1, 1 << 20, 3 << 20):
        for kind, gen in (("text", synth.text_like), ("json", synth.json_like)):
            src = np.ascontiguousarray(gen(size, seed=7 + size % 1000))
            for level in (mz.LevelSuperFast, mz.LevelFastest, mz.LevelBalanced):
                _check_single(ctx, mz.Encode(src, level, ctx), src.tobytes(), (kind, size, level))


@pytest.mark.parametrize("gap", [1, 2, 4, 8])
def test_level_balanced_gaps_against_the_restatement(gap):
    ctx = mz.Context(0)
    try:
        ctx.set_option(OPT_L2_GAP, gap)
        src = np.ascontiguousarray(synth.text_like((2 << 20) + 12345, seed=60 + gap))
        v = _check_single(ctx, mz.Encode(src, mz.LevelBalanced, ctx), src.tobytes(), gap)
        assert v.general
    finally:
        ctx.close()


# ---- counter regressions: counters 2 and 6 describe the whole last decode call ----
def _named(name):
    return next(c for c in TL.cases("named") if c.name == name)


def test_counters_after_a_call_of_empty_blocks(ctx):
    g = _named("fits_none")
    enc = TL.encode_block(g.body, g.dlen)
    assert mz.decode_batch([enc, enc], ctx) == [g.expected] * 2
    assert (ctx.general_blocks(), ctx.general_team()) == (2, 1)
    assert mz.decode_batch([b"\x00"] * 3, ctx) == [b""] * 3        # no tile to decode: no schedule kernel ran
    assert (ctx.general_blocks(), ctx.general_team()) == (0, 0)


@pytest.mark.parametrize("general_first", [True, False])
def test_counters_over_host_groups(general_first):
    g, c = _named("team_nearest_4_back"), _named("fits_three_and_all")
    blocks = [g] * 8 + [c] * 8 if general_first else [c] * 8 + [g] * 8
    ctx = mz.Context(0)
    try:
        ctx.set_option(OPT_HOST_GROUP_DEC, 1)      # host groups of 1 MiB: one block per group
        assert mz.decode_batch([TL.encode_block(b.body, b.dlen) for b in blocks], ctx) == [b.expected for b in blocks]
        assert (ctx.general_blocks(), ctx.general_team()) == (8, 4)
    finally:
        ctx.close()


def _stream(cases):
    """A .mz stream of one compressed chunk per case (block size 1 MiB)."""
    out = bytearray(b"\xff\x06\x00\x00MinLz") + bytes([(1 << 20).bit_length() - 1 - 10])
    for c in cases:
        enc = TL.encode_block(c.body, c.dlen)
        payload = int(O.crc(c.expected)).to_bytes(4, "little") + enc[1:]     # (the chunk holds uvarint(n) + body: no leading 0)
        out += bytes([0x02]) + len(payload).to_bytes(3, "little") + payload
    n = sum(c.dlen for c in cases)
    v = bytearray()
    while n >= 0x80:
        v.append((n & 0x7F) | 0x80)
        n >>= 7
    v.append(n)
    out += bytes([0x20, len(v), 0, 0]) + v
    return bytes(out)


def test_counters_over_stream_groups(ctx):
    g, c = _named("team_nearest_2_back"), _named("fits_dense_only")
    cases = [g] * 8 + [c] * 64                      # 72 MiB: two decode groups of the stream, general blocks in the first only
    s = _stream(cases)
    assert O.stream_decode(s, 72 << 20) == b"".join(x.expected for x in cases)
    assert mz.stream_decode(s, ctx=ctx) == b"".join(x.expected for x in cases)
    assert (ctx.general_blocks(), ctx.general_team()) == (8, 2)
