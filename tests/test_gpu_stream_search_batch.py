"""mlz_stream_search_batch_device (Context.stream_search_batch_device, HipTensorCodec.search_streams) on the GPU: a batch of streams in HBM
searched for many patterns in one call.  Every result is compared with the model (tests/search_batch_model.py: brute force over each
stream's own decoded bytes) and, for healthy streams, with open_stream + search_many(no_tables=True) on that stream alone.  The source
buffer lies between sentinel bands and is unchanged after every call; the outputs lie in over-allocated sentinel-filled tensors and are
untouched beyond what the contract writes."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, stream as S, synth
from tests import corrupt as CM
from tests import fold_model as FM
from tests import search_batch_model as BM
from tests import stream_batch_cases as BC
from tests import stream_device_cases as SC
from tests.search_gpu import gather

pytestmark = pytest.mark.gpu

SENT8, SENT32, SENT64 = 0xA5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
FRONT, GAP, BACK, GUARD = 37, 3, 64, 8
MLZ_ERR_CORRUPT, MLZ_ERR_CRC, MLZ_ERR_ARG = 1, 5, 8
IGNORE_CRC, SEARCH_TABLES, NO_TABLES, IGNORE_CASE = 2, 4, 8, 32
LENGTHS = [1, 2, 3, 7, 16, 40, 256]


def _i64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


class Batch:
    """The sources back to back (GAP sentinel bytes between two) in one device buffer between its bands.  spans may be replaced (aliases)."""

    def __init__(self, sources):
        buf, self.spans = BC.back_to_back(sources, GAP)
        self.image = np.concatenate([np.full(FRONT, SENT8, np.uint8), np.frombuffer(buf, np.uint8), np.full(BACK, SENT8, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()

    @property
    def src(self):
        return self.t.data_ptr() + FRONT

    def search(self, ctx, pats, cap, flags=0, present=True, stream_counts=True, pattern_counts=True, hits=True):
        """The call with guarded outputs -> dict(total, res, stats, stream_counts, pattern_counts, present: rows of words, triples)."""
        n, npat = len(self.spans), len(pats)
        words = (npat + 31) // 32
        sc = torch.full((n + GUARD,), _i64(SENT64), dtype=torch.int64, device="cuda")
        pc = torch.full((npat + GUARD,), _i64(SENT64), dtype=torch.int64, device="cuda")
        pr = torch.full((n * words + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        hs = torch.full((cap + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        hp = torch.full((cap + GUARD,), _i64(SENT64), dtype=torch.int64, device="cuda")
        hw = torch.full((cap + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        total, res, stats = ctx.stream_search_batch_device(
            self.src, self.spans, pats, sc.data_ptr() if stream_counts else None, pc.data_ptr() if pattern_counts else None, pr.data_ptr() if present else None,
            hs.data_ptr() if hits else None, hp.data_ptr() if hits else None, hw.data_ptr() if hits else None, cap if hits else 0, flags=flags)
        torch.cuda.synchronize()
        assert np.array_equal(self.t.cpu().numpy(), self.image), "the input was modified"
        sc, pc, pr, hs, hp, hw = (x.cpu().numpy() for x in (sc, pc, pr, hs, hp, hw))
        k = min(total, cap) if hits else 0
        clean = (hs[cap:] == SENT32).all() and (hp[cap:] == _i64(SENT64)).all() and (hw[cap:] == SENT32).all()
        assert clean and (sc[n:] == _i64(SENT64)).all() and (pc[npat:] == _i64(SENT64)).all() and (pr[n * words:] == SENT32).all(), "written beyond an output's size"
        if stats[3] < 2:   # (after a second pass the positions and patterns between the healthy triples and the first pass's are zero)
            assert (hs[k:] == SENT32).all() and (hp[k:] == _i64(SENT64)).all() and (hw[k:] == SENT32).all(), "written beyond the triples"
        else:
            assert (hs[k:] == SENT32).all() and np.isin(hp[k:cap], (0, _i64(SENT64))).all() and np.isin(hw[k:cap], (0, SENT32)).all()
        if not stream_counts:
            assert (sc == _i64(SENT64)).all()
        if not pattern_counts:
            assert (pc == _i64(SENT64)).all()
        if not present:
            assert (pr == SENT32).all()
        return dict(total=total, res=res, stats=stats, stream_counts=sc[:n].tolist(), pattern_counts=pc[:npat].tolist(),
                    present=(pr[:n * words].astype(np.int64) & 0xFFFFFFFF).reshape(n, words).tolist(), triples=list(zip(hs[:k].tolist(), hp[:k].tolist(), hw[:k].tolist())))

    def single(self, ctx, i, pats, **kw):
        """open_stream on stream i alone + search_many(no_tables=True) -> (total, the pairs)."""
        off, n = self.spans[i]
        rd = ctx.stream_open_device(self.src + off if n else None, n)
        try:
            total, _ = rd.search_many(pats, None, None, None, 0, no_tables=True, **kw)
            pos = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
            which = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
            total2, _ = rd.search_many(pats, None, pos.data_ptr() if total else None, which.data_ptr() if total else None, total, no_tables=True, **kw)
            torch.cuda.synchronize()
            assert total2 == total
            return total, list(zip(pos.cpu().numpy()[:total].tolist(), which.cpu().numpy()[:total].tolist()))
        finally:
            rd.close()


def check(ctx, b, datas, pats, what, cap=None, codes=None, flags=0, singles=None, model=None, fold=False, **kw):
    """datas[i]: stream i's decoded bytes, or None where codes[i] is the error it must return.  -> the call's results."""
    want = model or BM.result([None if d is None else (FM.fold(d) if fold else d) for d in datas], [FM.fold(p) if fold else p for p in pats])
    cap = want["total"] + 3 if cap is None else cap
    got = b.search(ctx, pats, cap, flags=flags, **kw)
    print(what, "streams", len(datas), "total", want["total"], "cap", cap, "stats", got["stats"])
    assert got["total"] == want["total"], what
    assert got["res"] == [c if d is not None else -codes[i] for i, (c, d) in enumerate(zip(want["counts"], datas))], what
    if kw.get("stream_counts", True):
        assert got["stream_counts"] == want["counts"], what
    if kw.get("pattern_counts", True):
        assert got["pattern_counts"] == want["pattern_counts"], what
    if kw.get("present", True):
        assert got["present"] == BM.present_words(want["present"], len(pats)), what
    if kw.get("hits", True):
        assert got["triples"] == want["triples"][:cap], what
    for i in (range(len(datas)) if singles is None else singles):
        if datas[i] is None:
            continue
        total, pairs = b.single(ctx, i, pats, ignore_case=fold)
        assert total == want["counts"][i], "%s: stream %d alone" % (what, i)
        assert [(i, q, p) for q, p in pairs] == [t for t in want["triples"] if t[0] == i], "%s: stream %d alone" % (what, i)
    return got, want


def needles(seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, L, dtype=np.uint8)) for L in lengths]


def plant(d, pats, bs, k0=0):
    """Every pattern once inside a chunk and, where no other plant lies there, across a chunk border of a stream written with blocks of bs
    bytes (a one-byte pattern: the last byte in front of the border).  Which pattern gets which border turns with k0."""
    d = bytearray(d)
    taken = []

    def put(o, p):
        if o < 0 or o + len(p) > len(d) or any(o < e and a < o + len(p) for a, e in taken):
            return
        d[o:o + len(p)] = p
        taken.append((o, o + len(p)))
    for k, p in enumerate(pats):
        put(1000 + 3000 * k + 7 * k0, p)
    nb = max(1, (len(d) - 1) // bs)
    for k, p in enumerate(pats):
        put(bs * (1 + (k + k0) % nb) - (len(p) + 1) // 2, p)
    return bytes(d)


# ---- 1. a mixed batch ----

def _mixed(ctx):
    """(name, stream, data): oracle-made and library-made at several levels and 4 KiB / 64 KiB / 1 MiB blocks, stored chunks, skippables,
    compcrc, empty, no bytes, one byte, a concatenated pair; every pattern planted across chunk borders, and two stream borders that hold
    the halves of a pattern."""
    pats = needles(7) + [bytes(np.random.default_rng(8).integers(0, 256, 16, dtype=np.uint8))]   # (the last one: absent everywhere)
    plants = pats[:-1]
    d = BC.small_data()
    d300 = d[:300_000 + 77]
    p40, p2 = pats[5], pats[1]
    cases = []
    for k, (level, bs, data) in enumerate(((1, 4 << 10, d300), (1, 64 << 10, d300), (1, 1 << 20, d300), (2, 64 << 10, d300), (2, 4 << 10, d[100_000:350_000]), (3, 64 << 10, d300))):
        x = plant(data, plants, bs, k)
        cases.append(("oracle_L%d_bs%d" % (level, bs), O.stream_encode(x, level, bs, k % 2 == 1), x))
    for k, (level, bs, data) in enumerate(((mz.LevelSuperFast, 64 << 10, d300), (0, 4 << 10, d300), (mz.LevelFastest, 1 << 20, d300), (mz.LevelBalanced, 64 << 10, d300),
                                           (mz.LevelFastest, 4 << 10, d[200_000:480_000]), (mz.LevelBalanced, 1 << 20, d300))):
        x = plant(data, plants, bs, k + 3)
        cases.append(("gpu_L%d_bs%d" % (level, bs), mz.stream_encode(x, level, bs, k % 2 == 0, ctx), x))
    # a stream border with the halves of the 40-byte pattern on its two sides: long neighbours
    a, c = d300[:70_000] + p40[:17], p40[17:] + d300[70_000:130_000]
    cases.append(("border_left", O.stream_encode(a, 1, 64 << 10), a))
    cases.append(("border_right", mz.stream_encode(c, mz.LevelFastest, 4 << 10, False, ctx), c))
    s, sd = SC.with_skippables()
    sd2 = plant(sd[:300_000], plants, 64 << 10, 5)
    out = [SC.stream_id(64 << 10), SC.frame(0x80, b"user chunk in front")]
    for i in range(0, len(sd2), 64 << 10):
        out += [SC.data_chunk(sd2[i:i + (64 << 10)]), SC.frame(0xfe, bytes((i >> 16) % 700)), SC.frame(0x99, b"\x02\x00\x00\x01" * 50)]
    cases.append(("skippables", b"".join(out + [SC.eof(len(sd2)), SC.frame(0x81, b"behind the end")]), sd2))
    x = plant(d300, plants, 64 << 10, 6)
    cases.append(("compcrc", SC.to_compcrc(O.stream_encode(x, 1, 64 << 10)), x))
    # the first half of the two-byte pattern at a stream's end; an empty stream, one without bytes and the one-byte stream that is its second half
    x = d300[:50_000] + p2[:1]
    cases.append(("border2_left", O.stream_encode(x, 2, 4 << 10), x))
    cases.append(("empty", O.stream_encode(b"", 1, 1 << 20), b""))
    cases.append(("no_bytes", b"", b""))
    cases.append(("one_byte", O.stream_encode(p2[1:], 1, 1 << 20), p2[1:]))
    # two concatenated streams are ONE decoded sequence: the pattern across the joint is found
    x = d300[:150_001 - 20] + p40 + d300[150_001 + 20:]
    cases.append(("two_streams", O.stream_encode(x[:150_001], 1, 64 << 10) + O.stream_encode(x[150_001:], 2, 4 << 10, True), x))
    r = plant(synth.random_bytes(200_003, seed=31).tobytes(), plants, 64 << 10, 2)
    cases.append(("stored", O.stream_encode(r, 1, 64 << 10), r))
    cases.append(("one_byte_again", O.stream_encode(p2[1:], 1, 1 << 20), p2[1:]))
    cases.append(("no_bytes_last", b"", b""))
    return cases, pats


def test_mixed_batch(ctx):
    cases, pats = _mixed(ctx)
    assert len(cases) >= 24 and all(len(d) <= 300_100 for _, _, d in cases)
    for _, s, d in cases:
        assert O.stream_decode(s, len(d) + 1) == d
    b = Batch([s for _, s, _ in cases])
    datas = [d for _, _, d in cases]
    got, want = check(ctx, b, datas, pats, "mixed")
    assert got["stats"][2] == 0 and got["stats"][3] == 1 and ctx.batch_long_streams() == 0
    assert want["pattern_counts"][-1] == 0 and all(c > 0 for c in want["pattern_counts"][:-1])       # every planted length is found; one pattern is absent
    names = [n for n, _, _ in cases]
    joint = names.index("two_streams")
    assert (joint, 150_001 - 20, 5) in want["triples"]                                              # across the joint of two concatenated streams
    # the halves on the two sides of a stream border are not an occurrence: nothing at the end of the left stream
    left, left2 = names.index("border_left"), names.index("border2_left")
    assert not [t for t in got["triples"] if t[0] == left and t[2] == 5 and t[1] > 70_000 - 40]
    assert not [t for t in got["triples"] if t[0] == left2 and t[2] == 1 and t[1] >= 50_000 - 1]
    assert got["res"][names.index("one_byte")] == BM.result([pats[1][1:]], pats)["total"]
    # under MLZ_STREAM_IGNORE_CRC and with the implied flag spelled out: the same answers
    check(ctx, b, datas, pats, "mixed ignore_crc", flags=IGNORE_CRC | NO_TABLES, singles=[], model=want)


# ---- 2. cap ----

def test_caps_and_null_outputs(ctx):
    cases, pats = _mixed(ctx)
    pats = pats + [pats[3][:2], pats[4][:5]]                                                         # prefixes of planted patterns: two triples at one position
    cases = [cases[i] for i in (1, 17, 0, 18, 6, 12)]
    b = Batch([s for _, s, _ in cases])
    datas = [d for _, _, d in cases]
    want = BM.result(datas, pats)
    counts, tr = want["counts"], want["triples"]
    assert counts[0] > 10 and counts[1] == 0 and counts[2] > 10
    got, _ = check(ctx, b, datas, pats, "cap 0", cap=0, singles=[], model=want)
    assert got["triples"] == []
    inside = next(k for k in range(counts[0] + counts[1] + 3, len(tr)) if tr[k - 1][:2] == tr[k][:2] and tr[k][0] == 2)   # inside stream 2, between two triples of one position: inside a tile
    border = counts[0] + counts[1] + counts[2]                                                      # exactly on a stream border
    assert tr[border - 1][0] == 2 and tr[border][0] > 2
    for cap in (1, inside, border, border + 1, want["total"]):
        check(ctx, b, datas, pats, "cap %d" % cap, cap=cap, singles=[], model=want)
    # every optional output NULL: the count per stream and the total alone
    check(ctx, b, datas, pats, "null outputs", cap=0, singles=[], model=want, present=False, stream_counts=False, pattern_counts=False, hits=False)
    # a cap with the presence matrix alone, and the matrix is exact below the total
    got, _ = check(ctx, b, datas, pats, "cap 5, presence", cap=5, singles=[], model=want, stream_counts=False, pattern_counts=False)
    assert sum(bin(w).count("1") for row in got["present"] for w in row) > 5


# ---- 3. errors ----

def _framed(blocks, crc_flip=None, short_tokens=None):
    """A hand-framed stream of 64 KiB blocks.  crc_flip: that chunk's stored CRC is stale; short_tokens: that chunk's tokens decode to five
    bytes less than its header says (a corrupt block whatever the CRC mode)."""
    out = [SC.stream_id(64 << 10)]
    for k, blk in enumerate(blocks):
        ck = bytearray(SC.data_chunk(blk))
        if k == crc_flip:
            ck[5] ^= 0x20
        if k == short_tokens:
            assert ck[0] == 0x02
            ck = bytearray(SC.frame(0x02, bytes(ck[4:8]) + S.put_uvarint(len(blk)) + O.encode_block(blk[:-5], 1)))
        out.append(bytes(ck))
    return b"".join(out + [SC.eof(sum(len(x) for x in blocks))])


def test_errors_in_one_batch(ctx):
    bs = 64 << 10
    needle, other = needles(11, [16, 3])
    text = synth.text_like(6 * bs, 51).tobytes()

    def data(seed):
        x = bytearray(text[seed * 1000:seed * 1000 + 4 * bs + 123])
        for o in (100 + seed, bs - 8, 2 * bs + 77, 3 * bs + 5000):                                  # (the first: in front of every fault)
            x[o:o + 16] = needle
        return bytes(x)
    blocks = lambda x: [x[i:i + bs] for i in range(0, len(x), bs)]
    healthy = [data(s) for s in range(5)]
    bad = [data(s) for s in (5, 6, 7)]
    good_streams = [_framed(blocks(x)) for x in healthy]
    whole = _framed(blocks(bad[0]))
    cut = whole[:CM.chunks(whole)[-3].off + 4 + 300]                                                 # a framing error: cut inside the last full data chunk's body
    stale = _framed(blocks(bad[1]), crc_flip=2)
    corrupt = _framed(blocks(bad[2]), short_tokens=1)
    codes = [CM.stream_verdict(s, 5 * bs)[0] for s in (cut, stale, corrupt)]
    assert codes[0] != 0 and codes[1:] == [MLZ_ERR_CRC, MLZ_ERR_CORRUPT]
    order = [good_streams[0], cut, good_streams[1], good_streams[2], stale, good_streams[3], corrupt, good_streams[4]]
    datas = [healthy[0], None, healthy[1], healthy[2], None, healthy[3], None, healthy[4]]
    want_codes = {1: codes[0], 4: codes[1], 6: codes[2]}
    pats = [needle, other, b"e"]
    b = Batch(order)
    got, want = check(ctx, b, datas, pats, "errors", codes=want_codes)
    assert got["stats"][2] == 2 and got["stats"][3] == 2
    assert all(got["present"][i] == [0] for i in (1, 4, 6)) and not [t for t in got["triples"] if t[0] in (1, 4, 6)]
    assert all(want["counts"][i] >= 4 for i in (0, 2, 3, 5, 7))
    # the healthy streams' results are those of the batch without the failing streams
    alone = Batch(good_streams)
    got2, _ = check(ctx, alone, healthy, pats, "healthy alone", singles=[])
    assert got2["stats"][3] == 1 and got2["stats"][2] == 0
    remap = {0: 0, 1: 2, 2: 3, 3: 5, 4: 7}
    assert [(remap[s], q, p) for s, q, p in got2["triples"]] == got["triples"] and got2["pattern_counts"] == got["pattern_counts"]
    # with a small cap: the second pass leaves nothing of the first pass's triples
    check(ctx, b, datas, pats, "errors, cap 7", codes=want_codes, cap=7, singles=[], model=want)
    # the needle alone, with room for the first pass's triples (the failing streams hold it in front of their faults): nothing of them is left
    few = BM.result(datas, [needle])
    got4, _ = check(ctx, b, datas, [needle], "errors, the needle alone", codes=want_codes, cap=few["total"] + 2, singles=[], model=few)
    assert got4["total"] == few["total"] == sum(few["counts"][i] for i in (0, 2, 3, 5, 7))
    # MLZ_STREAM_IGNORE_CRC: the stale-CRC stream counts
    datas[4] = bad[1]
    got3, _ = check(ctx, b, datas, pats, "errors, ignore_crc", codes=want_codes, flags=IGNORE_CRC, singles=[])
    assert got3["stats"][2] == 1 and got3["stats"][3] == 2 and got3["res"][4] >= 4


# ---- 4. a group border ----

def test_group_border_and_aliases(ctx):
    mib = 1 << 20
    text = synth.text_like(4 * mib, 61).tobytes()
    one, three = bytearray(text[:mib]), bytearray(text[mib:4 * mib])
    across, inside, frequent = needles(13, [40, 16]) + [b"th"]
    three[mib - 17:mib - 17 + 40] = across                                                          # across the stream's first chunk border: the 64 MiB group border
    one[500_000:500_016] = inside
    one, three = bytes(one), bytes(three)
    s1, s3 = O.stream_encode(one, 1, mib), mz.stream_encode(three, mz.LevelFastest, mib, False, ctx)
    assert len([c for c in CM.chunks(s1) if c.type in (1, 2, 3)]) == 1 and len([c for c in CM.chunks(s3) if c.type in (1, 2, 3)]) == 3
    b = Batch([s1, s3])
    b.spans = [b.spans[0]] * 63 + [b.spans[1]] + [b.spans[0]] * 3
    pats = [across, inside, frequent]
    p1, p3 = BM.stream_pairs(one, pats), BM.stream_pairs(three, pats)
    assert sum(1 for _, p in p1 if p == 1) == 1 and (mib - 17, 0) in p3 and len(p1) > 1000
    counts = [len(p1)] * 63 + [len(p3)] + [len(p1)] * 3
    cap = 2 * len(p1) + 11                                                                          # the frequent pattern with a small cap
    got = b.search(ctx, pats, cap)
    print("group border: total", got["total"], "stats", got["stats"])
    assert got["total"] == sum(counts) and got["res"] == counts and got["stream_counts"] == counts
    assert got["stats"] == (66 + 3, 66 + 3, 0, 1)
    per = [sum(1 for _, p in p1 if p == k) * 66 + sum(1 for _, p in p3 if p == k) for k in range(3)]
    assert got["pattern_counts"] == per and per[0] == 1 and per[1] == 66
    assert got["triples"] == ([(0, q, p) for q, p in p1] + [(1, q, p) for q, p in p1] + [(2, q, p) for q, p in p1])[:cap]
    row1, row3 = sum(1 << k for k in {p for _, p in p1}), sum(1 << k for k in {p for _, p in p3})
    assert got["present"] == [[row1]] * 63 + [[row3]] + [[row1]] * 3 and row3 & 1 and not row1 & 1
    # the stream at the group border and an alias, each alone
    assert b.single(ctx, 63, pats) == (len(p3), p3) and b.single(ctx, 65, pats) == (len(p1), p1)
    # the triples around the border stream: a cap that ends just behind it
    cap = 63 * len(p1) + len(p3) + 2
    got = b.search(ctx, pats, cap, present=False, stream_counts=False, pattern_counts=False)
    assert got["triples"][63 * len(p1):] == [(63, q, p) for q, p in p3] + [(64, q, p) for q, p in p1[:2]]


# ---- 5. a long stream ----

def test_long_stream_between_short_ones(ctx):
    tiny, td = SC.tiny_chunks()
    assert len(CM.chunks(tiny)) > 4096
    last = [c for c in CM.chunks(tiny) if c.type in (1, 2, 3)][-1]
    short = synth.text_like(3000, 71).tobytes()
    tail = td[-16:]
    pats = [tail, td[-40:-33], short[100:103]]
    cases = [(O.stream_encode(short, 1, 4 << 10), short), (tiny, td), (O.stream_encode(short[:100] + tail, 1, 4 << 10), short[:100] + tail)]
    b = Batch([s for s, _ in cases])
    got, want = check(ctx, b, [d for _, d in cases], pats, "long")
    assert ctx.counter(12) > 0 and ctx.batch_long_streams() == 1
    assert (1, len(td) - 16, 0) in got["triples"] and (2, 100, 0) in got["triples"] and last.clen > 16


# ---- 6. 4096 patterns and ignore_case ----

def test_4096_patterns_and_ignore_case(ctx):
    bs = 64 << 10
    rng = np.random.default_rng(81)
    text = bytearray(synth.text_like(16 * bs, 82).tobytes())
    for o in range(0, len(text), 3000):                                                             # stretches of capitals
        text[o:o + 700] = bytes(text[o:o + 700]).upper()
    text = bytes(text)
    datas = [text[i * bs:(i + 1) * bs] for i in range(16)]
    streams = [O.stream_encode(d, 1, bs) if i % 2 else mz.stream_encode(d, mz.LevelFastest, bs, False, ctx) for i, d in enumerate(datas)]
    pats = []
    while len(pats) < 3600:
        o, L = int(rng.integers(0, len(text) - 64)), int(rng.choice([6, 7, 16, 40]))
        p = text[o:o + L]
        pats.append(p.swapcase() if len(pats) % 3 == 0 else p)
    pats += [p[:max(4, len(p) // 2)] for p in pats[:300]]                                            # prefixes of others
    pats += pats[:4096 - len(pats)]                                                                  # duplicates
    assert len(pats) == 4096
    b = Batch(streams)
    got, want = check(ctx, b, datas, pats, "4096", cap=5000, singles=[3])
    gotf, wantf = check(ctx, b, datas, pats, "4096 ignore_case", cap=5000, flags=IGNORE_CASE, singles=[5], fold=True)
    assert wantf["total"] > want["total"] > 4096 and gotf["stats"][3] == 1


# ---- 7. streams with search tables ----

def test_streams_with_search_tables(ctx):
    bs = 64 << 10
    pats = needles(91, [16, 7, 2])
    d = [plant(synth.json_like(5 * bs + 100 * k, 92 + k).tobytes(), pats, bs, k) for k in range(4)]
    streams = [gather(ctx, [d[0]], bs, True, search_match_len=6), O.stream_encode(d[1], 1, bs), gather(ctx, [d[2]], bs, False, search_match_len=0), gather(ctx, [d[3]], bs)]
    assert any(c.type == 0x45 for c in CM.chunks(streams[0])) and not any(c.type == 0x45 for c in CM.chunks(streams[3]))
    b = Batch(streams)
    got, want = check(ctx, b, d, pats, "tables")
    plain = Batch([O.stream_encode(x, 1, bs) for x in d])
    got2, _ = check(ctx, plain, d, pats, "without tables", singles=[], model=want)
    assert got2["triples"] == got["triples"] and got["stats"][1] == got2["stats"][1] == sum((len(x) + bs - 1) // bs for x in d)


# ---- 8. arguments ----

def test_arguments(ctx):
    cases, pats = _mixed(ctx)
    b = Batch([cases[1][1], cases[6][1]])
    L = _lib.lib()
    n, cap = 2, 16
    blob, lens = b"".join(pats), (C.c_uint32 * len(pats))(*[len(p) for p in pats])
    out_count = (C.c_int64 * n)(*([123] * n))
    stats = (C.c_uint64 * 4)(*([77] * 4))
    outs = {k: torch.full((64,), v, dtype=t, device="cuda") for k, v, t in (("sc", 1, torch.int64), ("pc", 2, torch.int64), ("pr", 3, torch.int32), ("hs", 4, torch.int32),
                                                                          ("hp", 5, torch.int64), ("hw", 6, torch.int32))}
    arr = lambda spans: (_lib.BlockDesc * len(spans))(*[_lib.BlockDesc(o, ln, 0, 0) for o, ln in spans])

    def call(flags=0, src=None, spans=None, count=None, blob=blob, lens=lens, npat=len(pats), cap=cap, **ptr):
        p = {k: t.data_ptr() for k, t in outs.items()}
        p.update(ptr)
        spans = b.spans if spans is None else spans
        return L.mlz_stream_search_batch_device(ctx.handle, None, flags, b.src if src is None else src, arr(spans), len(spans) if count is None else count, blob, lens, npat,
                                                out_count, p["sc"], p["pc"], p["pr"], p["hs"], p["hp"], p["hw"], cap, stats)
    host = np.zeros(4096, np.uint8)
    many = (C.c_uint32 * 4097)(*([1] * 4097))
    refused = [
        call(npat=0), call(blob=b"x" * 4097, lens=many, npat=4097),
        call(blob=b"ab", lens=(C.c_uint32 * 2)(0, 2), npat=2), call(blob=b"x" * 258, lens=(C.c_uint32 * 2)(257, 1), npat=2),
        call(hs=None), call(hp=None), call(hw=None),
        call(sc=host.ctypes.data), call(pc=host.ctypes.data), call(pr=host.ctypes.data), call(hp=host.ctypes.data),
        call(src=b.image.ctypes.data + FRONT),
        call(spans=[b.spans[0], (b.spans[1][0], 1 << 35)]),
        call(flags=SEARCH_TABLES), call(flags=16), call(flags=1 << 8), call(flags=1),
        call(count=(1 << 20) + 1), call(count=-1),
    ]
    assert refused == [-MLZ_ERR_ARG] * len(refused), refused
    torch.cuda.synchronize()
    assert list(out_count) == [123] * n and list(stats) == [77] * 4
    for k, v in (("sc", 1), ("pc", 2), ("pr", 3), ("hs", 4), ("hp", 5), ("hw", 6)):
        assert (outs[k].cpu().numpy() == v).all(), k + " was written by a refused call"
    assert np.array_equal(b.t.cpu().numpy(), b.image)
    assert call(count=0) == 0 and list(out_count) == [123] * n
    assert (outs["pr"].cpu().numpy() == 3).all() and (outs["hp"].cpu().numpy() == 5).all()
    assert ctx.stream_search_batch_device(b.src, [], pats)[:2] == (0, [])
    # and the same arguments, accepted
    assert call() == BM.result([cases[1][2], cases[6][2]], pats)["total"] and list(stats)[2:] == [0, 1]


# ---- 9. the Python layers ----

def test_search_streams(ctx):
    codec = shard.HipTensorCodec(ctx)
    bs = 64 << 10
    needle = needles(95, [16])[0]
    text = synth.text_like(3 * bs, 96).tobytes()
    datas = [text[:bs + 50], plant(text[bs:3 * bs], [needle], bs), b"", needle, text[5000:9000] + needle + needle[:3]]
    streams = [O.stream_encode(x, 1, bs) for x in datas]
    buf, spans = BC.back_to_back(streams, 3)
    t = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    pats = [needle, b"the ", needle[:3]]
    want = BM.result(datas, pats)
    counts, present, hs, hp, hw, pc, total = codec.search_streams(t, spans, pats, max_results=want["total"] + 5)
    assert all(x.device == t.device for x in (counts, present, hs, hp, hw, pc))
    assert counts.dtype == torch.int64 and present.dtype == torch.bool and present.shape == (5, 3)
    assert total == want["total"] and counts.tolist() == want["counts"] and pc.tolist() == want["pattern_counts"]
    assert list(zip(hs.tolist(), hp.tolist(), hw.tolist())) == want["triples"]
    assert [set(np.flatnonzero(r).tolist()) for r in present.cpu().numpy()] == want["present"]
    # single-pattern calls: the row sums are counts > 0
    for p in pats:
        c1, p1, _, _, _, _, tot = codec.search_streams(t, spans, [p])
        assert p1.shape == (5, 1) and p1.sum(1).tolist() == (c1 > 0).long().tolist() and tot == int(c1.sum())
    assert codec.search_streams(t, spans, pats, present=False)[1] is None
    # a failing stream: raise names the first one; keep returns the codes
    bad = bytearray(buf)
    off, n = spans[1]
    bad[off + n - 8] ^= 0x04                                                                         # stream 1: a byte of its last chunk's body
    off, n = spans[3]
    cut = [(o, ln) for o, ln in spans]
    cut[3] = (off, n - 2)                                                                            # stream 3: its EOF chunk cut
    tb = torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda()
    with pytest.raises(mz.MinLZError) as e:
        codec.search_streams(tb, cut, pats)
    assert e.value.index == 1 and "stream 1" in str(e.value) and e.value.code in (MLZ_ERR_CORRUPT, MLZ_ERR_CRC)
    counts, present, hs, hp, hw, pc, total = codec.search_streams(tb, cut, pats, max_results=1000, on_error="keep")
    keep = BM.result([datas[0], None, datas[2], None, datas[4]], pats)
    assert counts.tolist()[1] in (-MLZ_ERR_CORRUPT, -MLZ_ERR_CRC) and counts.tolist()[3] == -CM.stream_verdict(streams[3][:-2], 100)[0] < 0
    assert [c for i, c in enumerate(counts.tolist()) if i not in (1, 3)] == [keep["counts"][i] for i in (0, 2, 4)]
    assert total == keep["total"] and list(zip(hs.tolist(), hp.tolist(), hw.tolist())) == keep["triples"] and not present[1].any() and not present[3].any()
    with pytest.raises(ValueError):
        codec.search_streams(t, spans, pats, on_error="ignore")
