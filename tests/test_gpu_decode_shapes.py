"""The designed decoder inputs of tests/decode_shapes.py on the GPU: exact bytes and exact verdicts against the oracle's decoder, no
tolerances.  What each input reaches (entry counts around the prefetched entries and the slot pool, sources in the ring and below it,
the deepest chains, token forms over tile and segment borders, segments without token starts, 65 and 129 tiles, teams of 2 and 4) is
proved on the CPU by tests/test_decode_shapes.py; here every shape is decoded alone, all of them as one batch under every cross-check
leg of the decoder, interleaved with own-encoder blocks at every alignment through the device entry point, and with damaged token headers."""
import numpy as np
import pytest

import minlz_amd as mz
import oracle as O
from minlz_amd import synth
from minlz_amd._lib import BlockDesc
from tests import decode_shapes as DS

pytestmark = pytest.mark.gpu

OPT_DECODE_ALGO, OPT_GENERAL_ALGO, OPT_GEN_PACKED, OPT_GEN_SETTLE_CAP, OPT_LEVEL0_KERNEL = 1, 8, 13, 20, 23


def _want(name):
    code, data = DS.expected(name)
    assert code == 0
    return data


@pytest.mark.parametrize("name", DS.NAMES)
def test_each_shape_alone(ctx, name):
    s = DS.shape(name)
    code, got = mz.decode_block(s.body, s.dlen, ctx)
    assert code == 0
    want = _want(name)
    if got != want:
        first = next(j for j in range(s.dlen) if got[j] != want[j])
        pytest.fail("%s: first wrong byte %d (tile %d, offset %d in it)" % (name, first, first // DS.TILE, first % DS.TILE))
    assert ctx.general_blocks() == 1
    assert ctx.general_team() == DS.census_of(name).verdict.team


# (name, options, on a context of its own, the general pass runs: its counter must see every block)
LEGS = [
    ("default", {}, False, True),
    ("general_on_tile_chain", {OPT_GENERAL_ALGO: 1}, False, False),
    ("all_on_tile_path", {OPT_DECODE_ALGO: 3}, False, False),
    ("serial", {OPT_DECODE_ALGO: 1}, False, False),
    ("packed_pool", {OPT_GEN_PACKED: 1}, False, True),
    ("level0_by_exec", {OPT_LEVEL0_KERNEL: 0}, True, True),
    ("settle_cap_4", {OPT_GEN_SETTLE_CAP: 4}, False, True),      # four settling workgroups for all the blocks: they take turns
]


@pytest.mark.parametrize("leg,opts,own,counts", LEGS, ids=[l[0] for l in LEGS])
def test_all_shapes_as_one_batch(ctx, leg, opts, own, counts):
    c = mz.Context(0) if own else ctx
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        got = mz.decode_batch([DS.block(n) for n in DS.NAMES], c)
        bad = [n for n, g in zip(DS.NAMES, got) if g != _want(n)]
        assert not bad, (leg, bad)
        if counts:
            assert (c.general_blocks(), c.general_team()) == (len(DS.NAMES), 1)
    finally:
        if own:
            c.close()
        else:
            for k in opts:
                c.set_option(k, 0)


def _place(sizes, first_residue, step, gap):
    """Offsets for back-to-back ranges with at least `gap` bytes between them: range i starts at residue (first_residue + i * step) mod 16."""
    offs, cur = [], 0
    for i, n in enumerate(sizes):
        cur += gap
        cur += ((first_residue + i * step) - cur) % 16
        offs.append(cur)
        cur += n
    return offs, cur


def test_device_batch_at_every_alignment(ctx):
    import torch
    dev = torch.device("cuda", 0)
    data = [synth.text_like(300_001, seed=41), synth.json_like(200_003, seed=42), synth.enwik_like(400_007, seed=43), synth.text_like(70_001, seed=44)]
    own = [(mz.Encode(d, lv, ctx), np.ascontiguousarray(d).tobytes()) for d, lv in zip(data, (-1, 1, 2, 2))]
    items = [(DS.block(n), _want(n)) for n in DS.NAMES]
    for i, o in enumerate(own):                      # interleaved: an own block after every fifth shape
        items.insert(5 * (i + 1) + i, o)
    blocks, wants = [b for b, _ in items], [w for _, w in items]
    soffs, stotal = _place([len(b) for b in blocks], 1, 3, 0)       # step 3 and 7 are odd: 16 blocks in a row cover every residue
    doffs, dtotal = _place([len(w) for w in wants], 5, 7, 1)
    assert len(blocks) >= 16 and {o % 16 for o in soffs} == set(range(16)) == {o % 16 for o in doffs}
    host = np.zeros(stotal + 64, dtype=np.uint8)
    for o, b in zip(soffs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    src = torch.from_numpy(host).to(dev)
    dst = torch.full((dtotal + 64,), 0xA5, dtype=torch.uint8, device=dev)
    dlen = torch.full((len(blocks),), -77, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx.decode_batch_device(st, src.data_ptr(), dst.data_ptr(), [BlockDesc(so, len(b), do, len(w)) for so, b, do, w in zip(soffs, blocks, doffs, wants)],
                            dlen.data_ptr())
    torch.cuda.synchronize()
    dh = dst.cpu().numpy()
    assert dlen.cpu().tolist() == [len(w) for w in wants]
    canary = np.ones(dh.size, dtype=bool)
    for do, w in zip(doffs, wants):
        canary[do:do + len(w)] = False
    assert (dh[canary] == 0xA5).all(), "bytes between or behind the destinations were written"
    bad = [i for i, (do, w) in enumerate(zip(doffs, wants)) if dh[do:do + len(w)].tobytes() != w]
    assert not bad, bad


def _mutants(name):
    """(what, body, dlen): six single-byte changes of token header bytes, one truncation, dlen - 1 and dlen + 1; seeded by the shape's name.
    Three of the six hit any header byte of any token (nearly always the lengths no longer add up: corrupt by the total); three hit the
    last header byte of a copy2 or copy3 without a length field, which holds offset bits only: the block keeps its length and stays valid
    with other bytes, or reaches before its start."""
    s = DS.shape(name)
    tk = DS.census_of(name).tok
    rng = np.random.default_rng(DS._seed("mutants/" + name))
    offset_only = [i for i, (k, h) in enumerate(zip(tk["kind"], tk["hlen"])) if (k, h) in (("copy2", 3), ("copy3", 4))]
    picks = [(i, int(rng.integers(0, int(tk["hlen"][i])))) for i in rng.integers(0, len(tk["spos"]), 3).tolist()]
    picks += [(offset_only[j], int(tk["hlen"][offset_only[j]]) - 1) for j in rng.integers(0, len(offset_only), 3).tolist()]
    out = []
    for i, k in picks:
        at = int(tk["spos"][i]) + k
        b = bytearray(s.body)
        b[at] ^= int(rng.integers(1, 256))
        out.append(("header byte %d of token %d" % (at, i), bytes(b), s.dlen))
    out.append(("truncated", s.body[:int(rng.integers(1, len(s.body)))], s.dlen))
    out.append(("dlen - 1", s.body, s.dlen - 1))
    out.append(("dlen + 1", s.body, s.dlen + 1))
    return out


@pytest.mark.parametrize("name", DS.NAMES)
def test_damaged_headers_get_the_oracles_verdict(ctx, name):
    muts = _mutants(name)
    want = [O.decode_body(b, n) for _, b, n in muts]
    for algo in (0, 1):
        ctx.set_option(OPT_GENERAL_ALGO, algo)
        try:
            for (what, b, n), (ocode, odata) in zip(muts, want):
                gcode, gdata = mz.decode_block(b, n, ctx)
                assert gcode == ocode, (name, what, algo)
                if ocode == 0:
                    assert gdata == odata, (name, what, algo)
        finally:
            ctx.set_option(OPT_GENERAL_ALGO, 0)
