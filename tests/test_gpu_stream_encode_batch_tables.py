"""mlz_stream_encode_batch_device_tables (Context.stream_encode_batch_device and HipTensorCodec.encode_streams with the search_* keywords) on
the GPU: a batch of inputs in HBM written as streams that carry block search tables.  Every stream is compared byte for byte with the
device Writer's stream of that input alone (tests.search_gpu.gather); the sources lie in one buffer between sentinel bands, the destinations
in another with sentinel gaps between them (tests/test_gpu_stream_batch.py's Batch), and after every call the bands are intact."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
from minlz_amd import _lib, api, shard, synth
from tests import search_batch_model as BM
from tests import search_model as SMod
from tests import search_prefold_model as PF
from tests import stream_batch_cases as BC
from tests.search_gpu import first_difference, gather
from tests.test_gpu_stream_batch import Batch
from tests.test_gpu_stream_search_batch import Batch as SearchBatch, check
from tests.test_gpu_stream_search_batch_prune import Pruned, against_the_model

pytestmark = pytest.mark.gpu

MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 6, 8
SEARCH_TABLES, COMPRESS = 4, 64
KIB = 1 << 10
TABLE_SLOT_BYTES = 17                                                                   # mlz_get_counter 17

CONFIGS = {
    "type1_m6": dict(search_match_len=6),
    "type1_m1": dict(search_match_len=1),
    "type2": dict(search_match_len=6, search_prefix=b'":, '),
    "type3": dict(search_match_len=6, search_prefix=b'":,{}[] \n-_'),                   # more than 8 values: the mask
    "type4": dict(search_match_len=6, search_long_prefix=b'"user":"', search_extras=3),
}


def model_cfg(kw):
    """The keywords -> search_model's (T, M, field)."""
    M = kw["search_match_len"] or 6
    if "search_long_prefix" in kw:
        return SMod.config(4, M, kw["search_long_prefix"], kw.get("search_extras", 0))
    if "search_prefix" in kw:
        T, field = SMod.field_of(kw["search_prefix"])
        return T, M, field
    return SMod.config(1, M)


_DATA = {}


def inputs_for(bs, M):
    """The lengths at which a batch can go wrong: nothing, one byte, around a window, around 4 KiB, around a block; two blocks and a last
    one shorter than any overlap; three blocks whose middle one is random (stored: no table); two blocks of zero bytes."""
    if (bs, M) not in _DATA:
        text = synth.json_like(3 * bs + 70_000, 21).tobytes()
        assert text[:50_000].count(b'"user":"') > 100
        out, at = [], 0
        for n in (0, 1, M - 1, M, 100, 4095, 4096, 4097, bs - 1, bs, bs + 1, 2 * bs + 5):
            out.append(text[at:at + n])
            at += 1013
        mid = bytearray(text[5000:5000 + 3 * bs])
        mid[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
        out += [bytes(mid), bytes(2 * bs)]
        _DATA[(bs, M)] = out
    return _DATA[(bs, M)]


_SINGLE = {}


def single(ctx, d, bs, index, level, kw):
    """The device Writer's stream of the one range d: the reference, made once per (input, settings)."""
    key = (d, bs, index, level, tuple(sorted(kw.items())))
    if key not in _SINGLE:
        _SINGLE[key] = gather(ctx, [d], bs, index, level=level, **kw)
    return _SINGLE[key]


def encode(ctx, datas, bs, index, level, kw, caps=None, what="encode"):
    """The batch call into guarded destinations of the bound's size (or caps) -> (batch, results, the destinations' bytes)."""
    caps = caps or [api.stream_bound(len(d), bs, index, **kw) for d in datas]
    b = Batch(datas, caps)
    res = ctx.stream_encode_batch_device(level, bs, index, b.src, b.dst, b.descs(), **kw)
    return b, res, b.check(what)


def same_as_single(ctx, datas, res, outs, bs, index, level, kw, what):
    for i, (d, r, o) in enumerate(zip(datas, res, outs)):
        want = single(ctx, d, bs, index, level, kw)
        got = o[:max(r, 0)].tobytes()
        assert r == len(want) and got == want, "%s: stream %d of %d bytes: %d bytes, the single Writer gives %d; first difference at %d" % (
            what, i, len(d), r, len(want), first_difference(got, want))
        assert (o[r:] == 0).all(), "%s: stream %d: bytes written behind the stream" % (what, i)


# ---- 1. bytes against the single Writer ----

@pytest.mark.parametrize("index", [False, True], ids=["plain", "index"])
@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4k", "64k"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_bytes_are_the_single_writers(ctx, name, bs, index):
    kw = CONFIGS[name]
    datas = inputs_for(bs, kw["search_match_len"])
    for level in ((1, 2) if name == "type1_m6" else (1,)):
        what = "%s bs %d index %d level %d" % (name, bs, index, level)
        b, res, outs = encode(ctx, datas, bs, index, level, kw, what=what)
        same_as_single(ctx, datas, res, outs, bs, index, level, kw, what)
    # what the streams hold: an info chunk behind the identifier, a table in front of every compressed block and none in front of a stored one
    cfg = model_cfg(kw)
    stored = tables = 0
    for d, r, o in zip(datas, res, outs):
        s = o[:r].tobytes()
        got_cfg, B, tabs = SMod.read_tables(s)
        kinds = [t for _, t in SMod.data_grid(s)]
        if not d:
            assert got_cfg is None and not kinds and s[:1] != b"\xff"                     # an empty stream has no head
            continue
        assert got_cfg == cfg and B == SMod.table_bits(bs) and s[10] == SMod.CHUNK_INFO
        for k, (t, tab) in enumerate(zip(kinds, tabs)):
            assert (tab is None) == (t == 0x01), (len(d), k)
            stored += t == 0x01
            tables += tab is not None
    assert stored >= 1 and tables >= 8


def test_a_sliced_block_beside_prefolded_ones(ctx):
    """Blocks of 4 MiB (B = 22: a full block's bitmap takes four slices) with a stream of one full block and 5000 bytes, and one of 5000
    bytes: a sliced table and pre-folded one-slice tables in one launch."""
    bs, kw = 4 << 20, CONFIGS["type1_m6"]
    text = synth.json_like(bs + 5000, 23).tobytes()
    datas = [text, text[7:5007]]
    b, res, outs = encode(ctx, datas, bs, True, 1, kw, what="4 MiB blocks")
    same_as_single(ctx, datas, res, outs, bs, True, 1, kw, "4 MiB blocks")
    cfg = model_cfg(kw)
    slots = [PF.prefold(PF.marks(cfg, n, f), 22, 25) for n, f in ((bs, b"x"), (5000, None), (5000, None))]
    assert slots == [0, 7, 7] and ctx.counter(TABLE_SLOT_BYTES) == ctx.table_slot_bytes == sum(1 << (22 - r - 3) for r in slots)


# ---- 2. pre-fold ----

@pytest.mark.parametrize("name", ["type1_m6", "type2"])
def test_short_blocks_are_built_folded(ctx, name):
    """64 inputs of 4 KiB at blocks of 1 MiB: the single Writer's bytes out of slots of 2 KiB (type 1; type 2: 8 KiB), not of 128 KiB."""
    bs, kw, n = 1 << 20, CONFIGS[name], 64
    text = synth.json_like(n * 4096 + 100, 25).tobytes()
    datas = [text[i * 4096 + i:i * 4096 + i + 4096] for i in range(n)]
    b, res, outs = encode(ctx, datas, bs, False, 1, kw, what="4 KiB in 1 MiB blocks")
    same_as_single(ctx, datas, res, outs, bs, False, 1, kw, "4 KiB in 1 MiB blocks")
    cfg = model_cfg(kw)
    r0 = PF.prefold(PF.marks(cfg, 4096, None), 20, SMod.fold_limit(cfg[0]))
    assert r0 == (6 if name == "type1_m6" else 4)
    assert ctx.table_slot_bytes == n * (1 << (20 - r0 - 3)) and ctx.table_slot_bytes != n * (128 * KIB)
    if name == "type1_m6":
        assert ctx.table_slot_bytes == n * 2 * KIB


# ---- 3. round trip ----

def test_round_trip_through_the_pruned_search(ctx):
    bs, kw = 64 * KIB, CONFIGS["type1_m6"]
    rng = np.random.default_rng(31)
    pats = [bytes(rng.integers(128, 256, 16, dtype=np.uint8)) for _ in range(3)]         # (the last one: absent everywhere)
    datas = []
    for k in range(6):
        d = bytearray(synth.json_like(5 * bs + 100 * k, 92 + k).tobytes())
        if k < 4:
            d[2 * bs - 8:2 * bs + 8] = pats[0]                                             # across a block border
            d[4 * bs + 1000 + k:4 * bs + 1016 + k] = pats[1]
        datas.append(bytes(d))
    datas += [b"", datas[0][:3000], bytes(datas[1][:bs + 10])]
    codec = shard.HipTensorCodec(ctx)
    buf, spans = BC.back_to_back(datas)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    enc, espans = codec.encode_streams(t, spans, mz.LevelFastest, bs, True, **kw)
    host = enc.cpu().numpy()
    streams = [host[o:o + n].tobytes() for o, n in espans]
    for d, s in zip(datas, streams):
        assert s == single(ctx, d, bs, True, 1, kw)
    # decode_streams gives the inputs back
    dec, starts = codec.decode_streams(enc, espans)
    assert dec.cpu().numpy().tobytes() == b"".join(datas) and starts[-1] == len(buf)
    # the pruned search over what the batch Writer wrote: the model's results and the model's plan, fewer chunks decoded than present
    want = BM.result(datas, pats)
    counts, present, hs, pos, which, pc, total = codec.search_streams(enc, espans, pats, max_results=want["total"] + 3, prune=True)
    assert total == want["total"] and counts.cpu().tolist() == want["counts"] and pc.cpu().tolist() == want["pattern_counts"] == [4, 4, 0]
    assert list(zip(hs.cpu().tolist(), pos.cpu().tolist(), which.cpu().tolist())) == want["triples"]
    sb = SearchBatch(streams)
    got, _ = check(Pruned(ctx), sb, datas, pats, "round trip, pruned", singles=[], model=want)
    m = against_the_model(got, streams, pats, "round trip")
    assert got["stats"][1] == m["decoded"] < got["stats"][0] and got["stats"][4] == m["tabbed"] > 0 and got["stats"][7] == 0
    print("round trip: decoded", got["stats"][1], "of", got["stats"][0], "chunks")


# ---- 4. isolation ----

def test_one_short_destination_and_empty_streams(ctx):
    bs, kw = 64 * KIB, CONFIGS["type2"]
    datas = inputs_for(bs, 6)
    bounds = [api.stream_bound(len(d), bs, True, **kw) for d in datas]
    assert bounds[0] == int(_lib.lib().mlz_stream_bound_config(0, bs, 1, C.byref(api.batch_tables_config(**kw))))
    caps = list(bounds)
    caps[11] -= 1
    b, res, outs = encode(ctx, datas, bs, True, 1, kw, caps=caps, what="one short destination")
    assert res[11] == -MLZ_ERR_DST_TOO_SMALL and (outs[11] == 0).all()
    keep = [i for i in range(len(datas)) if i != 11]
    same_as_single(ctx, [datas[i] for i in keep], [res[i] for i in keep], [outs[i] for i in keep], bs, True, 1, kw, "beside a short destination")
    # a batch of empty streams only
    for index in (False, True):
        b, res, outs = encode(ctx, [b"", b"", b""], bs, index, 1, kw, what="empty streams")
        same_as_single(ctx, [b""] * 3, res, outs, bs, index, 1, kw, "empty streams")
        assert ctx.table_slot_bytes == 0


# ---- 5. refusals ----

def _config(T, M, prefix=b"", extras=0, reserved=0, reserved2=0):
    c = _lib.SearchConfig()
    c.table_type, c.match_len, c.extras, c.reserved, c.prefix_len = T, M, extras, reserved, len(prefix)
    c.reserved2[0] = reserved2
    for i, v in enumerate(bytes(prefix)):
        c.prefix[i] = v
    return c


def test_refusals(ctx):
    bs = 64 * KIB
    datas = inputs_for(bs, 6)[3:9]
    kw = CONFIGS["type1_m6"]
    b = Batch(datas, [api.stream_bound(len(d), bs, False, **kw) for d in datas])
    arr = (_lib.BlockDesc * len(datas))(*[_lib.BlockDesc(*d) for d in b.descs()])
    out_len = (C.c_int64 * len(datas))()
    L = _lib.lib()

    def call(cfg, flags=0, level=1, block=bs):
        return L.mlz_stream_encode_batch_device_tables(ctx.handle, None, level, block, flags, None if cfg is None else C.byref(cfg), b.src, b.dst, arr, len(datas), out_len)

    good = _config(1, 6)
    for what, cfg, flags in (("the compress flag", good, COMPRESS), ("the tables flag beside a cfg", good, SEARCH_TABLES), ("match-length bits beside a cfg", good, 6 << 8),
                             ("type 2 without a value", _config(2, 6), 0), ("type 2 with 9 values", _config(2, 6, b"123456789"), 0), ("M = 9", _config(1, 9), 0),
                             ("M + E > 16", _config(4, 8, b'"user":"', 9), 0), ("a reserved byte", _config(1, 6, reserved=1), 0),
                             ("a second reserved byte", _config(3, 6, reserved2=1), 0), ("type 5", _config(5, 6), 0), ("extras with type 1", _config(1, 6, extras=1), 0)):
        assert call(cfg, flags) == -MLZ_ERR_ARG, what
    assert call(good, block=1000) == -MLZ_ERR_ARG and call(good, level=3) == -4
    # the plain call keeps its refusal, by either name
    assert call(None, SEARCH_TABLES) == -MLZ_ERR_ARG and call(None, 6 << 8) == -MLZ_ERR_ARG
    assert L.mlz_stream_encode_batch_device(ctx.handle, None, 1, bs, SEARCH_TABLES, b.src, b.dst, arr, len(datas), out_len) == -MLZ_ERR_ARG
    b.untouched("refused calls")
    # cfg == NULL is the plain call
    assert call(None) == 0
    outs = b.check("cfg NULL")
    for d, r, o in zip(datas, list(out_len), outs):
        assert o[:r].tobytes() == mz.stream_encode(d, 1, bs, False, ctx) and (o[r:] == 0).all()
    # and the good configuration is accepted, through the C entry point itself
    b.reset()
    assert call(good) == 0
    same_as_single(ctx, datas, list(out_len), b.check("cfg"), bs, False, 1, kw, "the C call")
