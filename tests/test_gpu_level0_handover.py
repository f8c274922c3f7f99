"""The hand-over from the decoder's index pass to its exec pass: dec_level0_kernel decodes the level-0 CANDIDATES (tile 16 j of every block) from
the token list alone while one more workgroup of the same launch gives the blocks' verdicts and makes the tile schedule; the exec pass skips
every tile whose done flag is up.  A candidate the kernel cannot finish (it reads an earlier tile, or holds a bad token) is left untouched.

Every case here compares bytes, per-block lengths / error codes and the general-block counters between the default path, a context with
OPT_LEVEL0_KERNEL = 0 (verdict and schedule kernels of their own, every tile by the exec pass) and the oracle's decoder, at the smallest
shapes at which the wiring can go wrong.  Bytes of a block that fails are not compared (which of its tiles were written before the
failure was seen is not part of any contract); nothing outside a block's destination is ever written (0xA5 canary)."""
import numpy as np
import pytest

import minlz_amd as mz
import oracle as O
from minlz_amd import synth
from minlz_amd._lib import BlockDesc
from tests import corrupt as CR
from tests import decode_shapes as DS
from tests import tile_levels as TL

pytestmark = pytest.mark.gpu

T = TL.TILE
OPT_DEBUG_STATUS = 3
OPT_LEVEL0_GRID_CAP = 25       # debug option and counter without names in the header or the module: candidates the level-0 launch takes at most,
COUNTER_LEVEL0_LAUNCHES = 13   # groups of the last decode call that took it


@pytest.fixture(scope="module")
def other():
    """Option 23 off: dec_viol_kernel, dec_schedule_kernel, every tile by the exec pass."""
    c = mz.Context(0)
    c.set_option(mz.OPT_LEVEL0_KERNEL, 0)
    yield c
    c.close()


def oracle_results(blocks):
    """[(length or -code, bytes or None)] per block."""
    out = []
    for b in blocks:
        try:
            d = O.decode(b)
            out.append((len(d), d))
        except O.OracleError as e:
            out.append((-e.code, None))
    return out


def device_results(c, blocks):
    """The blocks through decode_batch_device, destinations at odd offsets with a 0xA5 canary between and behind them ->
    ([(length or -code, the destination's bytes)], general_blocks, general_team, level-0 launches)."""
    import torch
    dev = torch.device("cuda", 0)
    caps = [O.decoded_len(b) for b in blocks]
    soffs, doffs, s, d = [], [], 0, 0
    for b, n in zip(blocks, caps):
        soffs.append(s)
        s += len(b) + 3
        d += 5
        doffs.append(d)
        d += n
    host = np.zeros(s + 64, dtype=np.uint8)
    for o, b in zip(soffs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    src = torch.from_numpy(host).to(dev)
    dst = torch.full((d + 64,), 0xA5, dtype=torch.uint8, device=dev)
    dlen = torch.full((len(blocks),), -77, dtype=torch.int64, device=dev)
    c.decode_batch_device(torch.cuda.current_stream(dev).cuda_stream, src.data_ptr(), dst.data_ptr(),
                          [BlockDesc(so, len(b), do, n) for so, b, do, n in zip(soffs, blocks, doffs, caps)], dlen.data_ptr())
    torch.cuda.synchronize()
    dh = dst.cpu().numpy()
    canary = np.ones(dh.size, dtype=bool)
    for do, n in zip(doffs, caps):
        canary[do:do + n] = False
    assert (dh[canary] == 0xA5).all(), "bytes between or behind the destinations were written"
    lens = dlen.cpu().tolist()
    return ([(l, dh[do:do + n].tobytes()) for l, do, n in zip(lens, doffs, caps)], c.general_blocks(), c.general_team(),
            c.counter(COUNTER_LEVEL0_LAUNCHES))


def check_three_ways(ctx, other, blocks, fused=1):
    """Default path == option 23 off == oracle; returns the default path's results.  fused: groups that must have taken the one launch."""
    want = oracle_results(blocks)
    got, g_n, g_team, g_l0 = device_results(ctx, blocks)
    ref, r_n, r_team, r_l0 = device_results(other, blocks)
    for i, ((wl, wd), (gl, gd), (rl, rd)) in enumerate(zip(want, got, ref)):
        assert gl == rl == wl, (i, gl, rl, wl)
        if wl >= 0:
            assert gd == wd, "block %d: default path" % i
            assert rd == wd, "block %d: option 23 off" % i
    assert (g_n, g_team) == (r_n, r_team)
    assert g_l0 == fused and r_l0 == 0
    return got, g_n, g_team


@pytest.fixture(scope="module")
def conformant(ctx):
    """A LevelFastest block of 17 tiles + 5 bytes: candidates 0 and 16, a ragged last tile."""
    d = synth.enwik_like(17 * T + 5, seed=601)
    return mz.Encode(d, mz.LevelFastest, ctx), d.tobytes()


def test_two_candidates_and_a_ragged_end(ctx, other, conformant):
    for blocks in ([conformant[0]],
                   [mz.Encode(synth.text_like(T, seed=602), mz.LevelFastest, ctx)],          # one tile
                   [mz.Encode(synth.json_like(T - 1, seed=603), mz.LevelFastest, ctx)],      # ... not quite
                   [mz.Encode(synth.enwik_like(16 * T, seed=604), mz.LevelFastest, ctx)],    # 16 tiles exactly: one candidate
                   [mz.Encode(synth.enwik_like(16 * T + 1, seed=605), mz.LevelFastest, ctx)]):   # a second candidate of one byte
        _, n_gen, _ = check_three_ways(ctx, other, blocks)
        assert n_gen == 0


def test_mixed_batch(ctx, other, conformant):
    rng = np.random.default_rng(606)
    stored = mz.Encode(rng.integers(0, 256, 2 * T + 17, dtype=np.uint8), mz.LevelFastest, ctx)
    assert TL.block_body(stored)[0] is None
    balanced = mz.Encode(synth.enwik_like(20 * T + 100, seed=607), mz.LevelBalanced, ctx)     # no levels: tile 16 reads earlier tiles
    blocks = [conformant[0], stored, mz.Encode(b"", mz.LevelFastest, ctx), mz.Encode(b"x", mz.LevelFastest, ctx), balanced,
              DS.block("tiles_65"), DS.block("tiles_129")]     # tiles 16, 32, ... of the two shapes have external entries
    got, n_gen, team = check_three_ways(ctx, other, blocks)
    assert n_gen == 3     # the LevelBalanced block and the two shapes


def test_other_patterns(ctx, other):
    # dense: LevelBalanced with tile levels
    enc = mz.Context(0)
    try:
        enc.set_option(mz.OPT_L2_FREE, 0)
        dense = mz.Encode(synth.enwik_like(33 * T + 9, seed=608), mz.LevelBalanced, enc)
    finally:
        enc.close()
    # fast: a hand-built block with one read that only the fast pattern allows; its tiles 4, 8, 12 (mod 16) are level 0 and no candidates
    kd = TL._only("fast", 17, 32)
    b = TL.Block(32, 609)
    b.reader(kd, (kd - 1) * T + 100, 5000, [kd - 1])
    case = b.case("level0_handover_fast")
    assert case.intended.pattern == "fast" and not case.intended.general
    assert TL.level("fast", 4) == 0 and TL.level("three", 4) != 0
    fast = TL.encode_block(case.body, case.dlen)
    got, n_gen, _ = check_three_ways(ctx, other, [dense, fast])
    assert n_gen == 0
    assert got[1][1] == case.expected


def _damaged(block, tile, seed):
    """Six damaged copies of `block`: a changed header byte in tokens that start inside `tile` — three anywhere in a header, three in the
    last header byte of a copy2 / copy3 without a length field (offset bits only: the block keeps its length)."""
    s = CR.Source("level0_handover", block)
    head = len(s.block) - len(s.body)
    inside = [t for t in s.toks if tile * T + 64 <= t.dpos < (tile + 1) * T - 64]
    offset_only = [t for t in inside if (t.form, t.hlen) in (("copy2", 3), ("copy3", 4))]
    assert len(inside) > 100 and len(offset_only) > 10
    rng = np.random.default_rng(seed)
    picks = [(inside[i], int(rng.integers(0, inside[i].hlen))) for i in rng.integers(0, len(inside), 3).tolist()]
    picks += [(offset_only[i], offset_only[i].hlen - 1) for i in rng.integers(0, len(offset_only), 3).tolist()]
    out = []
    for t, k in picks:
        bad = bytearray(block)
        bad[head + t.spos + k] ^= int(rng.integers(1, 256))
        out.append(bytes(bad))
    return out


@pytest.mark.parametrize("tile", [0, 16])
def test_damaged_candidates(ctx, other, conformant, tile):
    muts = _damaged(conformant[0], tile, 610 + tile)
    check_three_ways(ctx, other, muts)
    # the failure site is the later passes': dec_level0_kernel stores no status, so the default path reports what option 23 off reports
    for c in (ctx, other):
        c.set_option(OPT_DEBUG_STATUS, 1)
    try:
        a, b = device_results(ctx, muts), device_results(other, muts)
        assert [l for l, _ in a[0]] == [l for l, _ in b[0]]
    finally:
        for c in (ctx, other):
            c.set_option(OPT_DEBUG_STATUS, 0)


def test_repeated_calls_on_one_context(conformant):
    c = mz.Context(0)
    try:
        general = [DS.block("team2"), conformant[0], DS.block("chains")]
        want = oracle_results(general)
        got, n_gen, team, l0 = device_results(c, general)
        assert [l for l, _ in got] == [l for l, _ in want] and [d for _, d in got] == [d for _, d in want]
        assert n_gen == 2 and team >= 1 and l0 == 1
        empty = [mz.Encode(b"", mz.LevelFastest, c)] * 3
        got, n_gen, team, l0 = device_results(c, empty)
        assert [l for l, _ in got] == [0, 0, 0]
        assert (n_gen, team, l0) == (0, 0, 0)          # counters 2 and 6 describe THIS call: no tile, no general block
        got, n_gen, team, l0 = device_results(c, [conformant[0]])
        assert got[0] == (len(conformant[1]), conformant[1])
        assert (n_gen, team, l0) == (0, 0, 1)
    finally:
        c.close()


def test_more_candidates_than_the_grid_cap(other):
    # 33 tiles: three candidates; with the grid capped at one the group must take the separate kernels, with the same result
    d = synth.enwik_like(32 * T + 1234, seed=611)
    c = mz.Context(0)
    try:
        block = mz.Encode(d, mz.LevelFastest, c)
        c.set_option(OPT_LEVEL0_GRID_CAP, 1)
        check_three_ways(c, other, [block], fused=0)
        one = mz.Encode(d[:16 * T], mz.LevelFastest, c)      # one candidate fits the cap
        check_three_ways(c, other, [one], fused=1)
        c.set_option(OPT_LEVEL0_GRID_CAP, 0)
        got, _, _ = check_three_ways(c, other, [block], fused=1)
        assert got[0] == (d.size, d.tobytes())
    finally:
        c.close()
