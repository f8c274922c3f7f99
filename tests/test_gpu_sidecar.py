"""Sidecar search indexes on the device (mlz_dev_reader_build_sidecar, mlz_dev_reader_attach_sidecar; DeviceReader, DeviceStream) against
tests/sidecar_model.py, the specification in plain Python: a built sidecar is the model's byte for byte, a search through an attached
sidecar returns what a brute-force search of the decoded bytes returns and decodes exactly the chunks the model's plan names, and a
sidecar that lies about the main stream is refused without touching the handle."""

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, shard, synth
from minlz_amd.api import search_config
from tests import search_cases as SC
from tests import search_model as SMod
from tests import sidecar_model as SM
from tests.search_gpu import SENT, Opened, data_for, dev_u8, first_difference, gather_into

pytestmark = pytest.mark.gpu

MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG = 6, 8
BS = 64 << 10
NON_ALNUM = bytes(v for v in range(256) if not chr(v).isalnum())
USER = b'"user":"'


def cfg(T, M=6, prefix=b"", extras=0):
    """(the library's configuration, the model's)"""
    return search_config(T, M, prefix, extras), SMod.config(T, M, prefix, extras)


T1 = {M: cfg(1, M) for M in (1, 4, 6, 8)}
T2, T3, T4 = cfg(2, 6, b'":, '), cfg(3, 6, NON_ALNUM), cfg(4, 6, USER, 3)
ALL_SETS = [[T1[1]], [T1[4]], [T1[6]], [T1[8]], [T2], [T3], [T4], [T1[6], T2, T3, T4]]


class Handle(Opened):
    """A stream on the device, opened; builds go into a guarded destination."""

    def __init__(self, ctx, stream):
        super().__init__(ctx, stream)
        self.stream = stream
        self.keep = None

    def build(self, cfgs, cap=None, **kw):
        lib_cfgs = [c[0] for c in cfgs]
        bound = self.rd.sidecar_bound(lib_cfgs)
        cap = bound if cap is None else cap
        dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        got = self.rd.build_sidecar(lib_cfgs, dst.data_ptr(), cap, **kw)
        o = dst.cpu().numpy()
        assert got <= cap
        assert (o[cap:] == 0x5A).all(), "written behind the room"
        return o[:got].tobytes()

    def attach(self, side, **kw):
        t = dev_u8(side)
        self.rd.attach_sidecar(t.data_ptr(), len(side), **kw)
        self.keep = t

    def search(self, pattern, cap=1 << 17, **kw):
        out = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search(pattern, out.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        k = min(total, cap)
        assert (o[k:] == SENT).all(), "written beyond the results"
        assert self.ctx.search_plan() == stats[1:]
        return total, o[:k].tolist(), stats

    def many(self, pats, cap=1 << 16):
        pos = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        which = torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((len(pats) + 8,), SENT, dtype=torch.int64, device="cuda")
        total, stats = self.rd.search_many(pats, counts.data_ptr(), pos.data_ptr(), which.data_ptr(), cap)
        torch.cuda.synchronize()
        k = min(total, cap)
        assert (pos.cpu().numpy()[k:] == SENT).all() and (counts.cpu().numpy()[len(pats):] == SENT).all()
        return total, list(zip(pos.cpu().numpy()[:k].tolist(), which.cpu().numpy()[:k].tolist())), counts.cpu().numpy()[:len(pats)].tolist(), stats


def check_sidecar_is_a_stream(ctx, side):
    assert O.stream_decode(side, 0) == b""
    t = dev_u8(side)
    assert ctx.stream_decoded_len_device(t.data_ptr(), len(side)) == (0, 0)


def check_builds(ctx, stream, data, sets=ALL_SETS):
    """Every configuration set: the device's sidecar is the model's, and it is a valid stream of no bytes."""
    assert O.stream_decode(stream, len(data)) == data
    h = Handle(ctx, stream)
    cache, sides = {}, []
    try:
        for cfgs in sets:
            want = SM.build(stream, data, [c[1] for c in cfgs], cache=cache)
            got = h.build(cfgs)
            assert len(got) == len(want) and got == want, "%s: first difference at %d" % ([c[1][:2] for c in cfgs], first_difference(got, want))
            check_sidecar_is_a_stream(ctx, got)
            sides.append(got)
    finally:
        h.close()
    return sides


def own_stream(ctx, d, bs, **kw):
    return gather_into(ctx, [d], 2 * len(d) + (1 << 20), 1, bs, kw.pop("add_index", False), **kw)


# ---- build equals the model, byte for byte ----

@pytest.mark.parametrize("kind,bs,nblk", [(k, 4 << 10, 50) for k in SC.KINDS] + [(k, BS, 9) for k in SC.KINDS] + [(k, 1 << 20, 4) for k in SC.KINDS] + [(k, 8 << 20, 2) for k in SC.KINDS])
def test_build_over_own_writer_stream(ctx, kind, bs, nblk):
    """(a) The device Writer's stream without tables, its random block stored: that block gets a table exactly when its population allows."""
    d = data_for(kind, bs, nblk, 1234)
    stream = own_stream(ctx, d, bs)
    grid = SMod.data_grid(stream)
    assert grid[1][1] == 0x01 and grid[-1][0] == 1234
    sides = check_builds(ctx, stream, d)
    B = SMod.table_bits(bs)
    blk = np.frombuffer(d[bs:2 * bs + 5], np.uint8)          # the stored block and its overlap, type 1 at M = 6
    pop = len(np.unique(SMod.hash_windows(blk, B, 6)))
    _, _, tables = SM.parse(sides[2], stream)
    assert (tables[0][1] is not None) == (pop * 100 // (1 << B) <= 70), (pop, B)
    if bs == 4 << 10:
        assert tables[0][1] is not None   # (4096 random windows fill about 63 % of 4096 bits: the stored block has a table)


@pytest.mark.parametrize("level", [1, 2])
def test_build_over_reference_algorithm_stream(ctx, level):
    """(b)"""
    d = data_for("json_like", BS, 9, 777, random_block=None)
    check_builds(ctx, O.stream_encode(d, level, BS), d)


UNEVEN = [5000, 2, 7000, 1, 3, 65536, 9]


def uneven_stream():
    """(c) Chunks of uneven sizes under a 64 KiB header: next chunks shorter than the overlap, a chunk shorter than M, the long prefix
    across three chunks and type 4 windows that run into zeros."""
    n = sum(UNEVEN)
    d = bytearray(synth.json_like(n, 11).tobytes())
    at = 5002 + 7000 - 3
    d[at:at + 8] = USER                                       # 3 bytes in the chunk of 7000, 1, 3, and 1 in the chunk of 65536
    d[n - 9 - 4:n - 9 + 4] = USER                             # across the last border: its windows run into zeros
    d = bytes(d)
    stream = SM.framed(d, UNEVEN)
    assert O.stream_decode(stream, n) == d and [s for s, _ in SMod.data_grid(stream)] == UNEVEN
    return stream, d


def test_build_over_uneven_chunks(ctx):
    stream, d = uneven_stream()
    check_builds(ctx, stream, d)


def test_build_over_a_stream_with_inline_tables_and_index(ctx):
    """(d) Table and index chunks of the main stream are stepped over; the references still name the data chunks' headers."""
    d = data_for("enwik_like", BS, 9, 1234)
    stream = own_stream(ctx, d, BS, add_index=True, search_match_len=6)
    assert any(t == 0x45 for _, t, _ in SMod.chunks_of(stream)) and any(t == 0x40 for _, t, _ in SMod.chunks_of(stream))
    sides = check_builds(ctx, stream, d, [[T1[6]], [T2, T4]])
    refs = [SM.parse_refs(sides[0][p + 4:p + 4 + n], BS)[0][0] for p, t, n in SMod.chunks_of(sides[0]) if t == SM.CHUNK_REF]
    assert refs == [p for p, _ in SM.main_chunks(stream)] and all(stream[p] in (1, 2) for p in refs)


def test_build_over_two_groups(ctx):
    """(e) 9 blocks of 8 MiB: the decode runs in two groups, and the eighth block's overlap is the ninth's first bytes."""
    bs = 8 << 20
    d = data_for("text_like", bs, 9, 0, random_block=None)
    check_builds(ctx, O.stream_encode(d, 1, bs), d, [[T1[6]]])


def test_build_over_two_groups_with_stored_chunks_at_the_border(ctx):
    """(f) 9 blocks of 8 MiB, blocks 7 and 8 random bytes, hence stored: the ninth is copied into the scratch twice, as the overlap behind
    group 0's last chunk and as group 1's first chunk."""
    bs = 8 << 20
    d = data_for("text_like", bs, 9, 0, random_block=None)
    d = d[:7 * bs] + synth.random_bytes(2 * bs, seed=8).tobytes()
    stream = own_stream(ctx, d, bs)
    grid = SMod.data_grid(stream)
    assert [n for n, _ in grid] == [bs] * 9 and grid[7][1] == grid[8][1] == 0x01 and all(t != 0x01 for _, t in grid[:7])
    check_builds(ctx, stream, d, [[T1[6]]])


# ---- search by sidecar ----

def expect(data, sizes, plan, pattern):
    """What a search that decodes `plan` finds: the occurrences whose chunks are all decoded."""
    pos = np.asarray(SMod.brute(data, pattern), np.int64)
    if not len(pos):
        return []
    got = set(plan)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    k0 = np.searchsorted(starts, pos, side="right") - 1
    k1 = np.searchsorted(starts, pos + len(pattern) - 1, side="right") - 1
    left_out = np.concatenate([[0], np.cumsum([1 if sizes[k] and k not in got else 0 for k in range(len(sizes))])])
    return pos[left_out[k1 + 1] == left_out[k0]].tolist()


def search_cases_of(which):
    if which == "uneven":
        stream, d = uneven_stream()
        pats = [d[1000:1016], d[20000:20030], d[-20:], b"\x00absent\x00", d[5000 - 8:5000 + 30], USER + d[5002 + 7000 + 5:5002 + 7000 + 21],
                d[4998:4998 + 12], d[5002 + 7000 - 3:5002 + 7000 + 9]]   # (the last two start in front of chunks shorter than the overlap)
        return stream, d, pats, None
    if which == "planted":
        d, nd, at = SC.planted("text_like", BS, 128, 16, 1)
        return O.stream_encode(d, 1, BS), d, [nd, d[5 * BS // 3:5 * BS // 3 + 16], bytes(SC.needle(16, 99))], nd
    d = data_for("json_like", BS, 12, 100, random_block=None)
    return O.stream_encode(d, 1, BS), d, [p for _, p in SC.patterns(d, 6, BS)] + [USER + b"abc"], None


@pytest.mark.parametrize("which", ["reference", "uneven", "planted"])
def test_search_through_a_sidecar(ctx, which):
    stream, d, pats, planted = search_cases_of(which)
    sizes = [n for _, n in SM.main_chunks(stream)]
    h = Handle(ctx, stream)
    try:
        for p in pats[:2]:
            total, pos, stats = h.search(p)
            assert stats[1] == stats[0] == len(sizes) and stats[2] == 0 and pos == SMod.brute(d, p)   # no sidecar: everything
        plans = {}
        for name, cfgs in (("one", [T1[6]]), ("other", [T2]), ("both", [T1[6], T2])):
            model = [c[1] for c in cfgs]
            side = h.build(cfgs)
            mcfgs, Bs, tables = SM.parse(side, stream)
            assert mcfgs == model
            for src in (side, SM.build(stream, d, model)):       # the device's sidecar, and one the model built
                h.attach(src)
                for p in pats:
                    total, pos, stats = h.search(p)
                    plan = SM.plan(tables, sizes, p, mcfgs, Bs)
                    assert stats == (len(sizes), len(plan), SM.usable(tables, [p], mcfgs, Bs)), (which, name, p)
                    assert pos == expect(d, sizes, plan, p) and total == len(pos), (which, name, p)
                    assert pos == SMod.brute(d, p), (which, name, p)
                    plans[name, p] = set(plan)
            if planted is not None and name == "one":
                assert len(plans[name, planted]) <= 12 and h.search(planted)[1] == SMod.brute(d, planted)
        for p in pats:
            assert plans["both", p] <= plans["one", p] and plans["both", p] <= plans["other", p]
        # many patterns in one call are the loop of single searches
        rng = np.random.default_rng(5)
        pool = pats + [d[o:o + int(L)] for o, L in zip(rng.integers(0, len(d) - 300, 300).tolist(), rng.integers(12, 40, 300).tolist())]
        for n in (1, 16, 300):
            use = pool[:n]
            singles = [h.search(p, cap=1 << 15) for p in use]
            total, pairs, counts, stats = h.many(use)
            assert counts == [s[0] for s in singles] and total == sum(counts)
            if total <= 1 << 16 and all(s[0] <= 1 << 15 for s in singles):
                assert pairs == sorted((q, i) for i, s in enumerate(singles) for q in s[1])
        h.rd.detach_sidecar()
        total, pos, stats = h.search(pats[0])
        assert stats[1] == len(sizes) and stats[2] == 0 and pos == SMod.brute(d, pats[0])
    finally:
        h.close()


def test_device_stream_front_end(ctx):
    d, nd, at = SC.planted("json_like", BS, 16, 16, 3)
    codec_stream = shard.DeviceStream(ctx, dev_u8(O.stream_encode(d, 1, BS)))
    try:
        side = codec_stream.build_sidecar([T1[6][0], T4[0]])
        assert side.is_cuda and side.dtype == torch.uint8
        assert side.cpu().numpy().tobytes() == SM.build(O.stream_encode(d, 1, BS), d, [T1[6][1], T4[1]])
        codec_stream.attach_sidecar(side)
        pos, total = codec_stream.search(nd, 100)
        assert pos.cpu().tolist() == SMod.brute(d, nd) and ctx.search_plan()[0] < 16
        codec_stream.attach_sidecar(None)
        codec_stream.search(nd, 100)
        assert ctx.search_plan() == (16, 0)
    finally:
        codec_stream.close()


# ---- lying and broken sidecars ----

@pytest.fixture(scope="module")
def lying():
    d = data_for("json_like", BS, 12, 100, random_block=None)
    stream = O.stream_encode(d, 1, BS)
    model = [T1[6][1], T2[1]]
    side = SM.build(stream, d, model)
    return d, stream, model, side


def test_broken_tables_are_passed_over(ctx, lying):
    d, stream, model, side = lying
    sizes = [n for _, n in SM.main_chunks(stream)]
    tabs = [(p, n) for p, t, n in SMod.chunks_of(side) if t == SMod.CHUNK_TABLE]
    p0 = tabs[4][0]
    flipped = side[:p0 + 40] + bytes([side[p0 + 40] ^ 0x10]) + side[p0 + 41:]
    as46 = side[:p0] + b"\x46" + side[p0 + 1:]
    pats = [d[5 * BS // 3:5 * BS // 3 + 16], d[BS - 8:BS + 8], bytes(SC.needle(16, 99))]
    h = Handle(ctx, stream)
    try:
        for src, kw in ((side, {}), (flipped, {}), (flipped, {"ignore_crc": True}), (as46, {})):
            mcfgs, Bs, tables = SM.parse(src, stream, ignore_crc=bool(kw))
            h.attach(src, **kw)
            for p in pats:
                total, pos, stats = h.search(p)
                plan = SM.plan(tables, sizes, p, mcfgs, Bs)
                assert stats == (len(sizes), len(plan), SM.usable(tables, [p], mcfgs, Bs))
                assert pos == expect(d, sizes, plan, p)
                if not kw:
                    assert pos == SMod.brute(d, p)
        good = SM.parse(side, stream)[2]
        for src in (flipped, as46):
            t = SM.parse(src, stream)[2]
            gone = [(c, k) for c in range(2) for k in range(len(sizes)) if (t[c][k] is None) != (good[c][k] is None)]
            assert len(gone) == 1 and t[1 - gone[0][0]][gone[0][1]] is not None   # that (chunk, configuration) alone; the other configuration still prunes
        assert SM.parse(flipped, stream, ignore_crc=True)[2] != good and all(x is not None for x in SM.parse(flipped, stream, ignore_crc=True)[2][0])
    finally:
        h.close()


def test_refused_sidecars_leave_the_handle_alone(ctx, lying):
    d, stream, model, side = lying
    sizes = [n for _, n in SM.main_chunks(stream)]
    dcs = SM.main_chunks(stream)
    refs = [(p, n) for p, t, n in SMod.chunks_of(side) if t == SM.CHUNK_REF]

    def with_ref(i, payload):
        p, n = refs[i]
        return side[:p] + SMod.frame(SM.CHUNK_REF, payload) + side[p + 4 + n:]

    u = SM.uvarint
    p3, n3 = refs[3]
    p4, n4 = refs[4]
    bad = {
        "offset off by one": (with_ref(3, u(dcs[3][0] + 1) + u(0)), mz.ErrCorrupt),
        "size off by one": (with_ref(3, u(dcs[3][0]) + u(1)), mz.ErrCorrupt),
        "swapped": (side[:p3] + side[p4:p4 + 4 + n4] + side[p3 + 4 + n3:p4] + side[p3:p3 + 4 + n3] + side[p4 + 4 + n4:], mz.ErrCorrupt),
        "empty reference": (with_ref(3, b""), mz.ErrCorrupt),
        "cut varint": (with_ref(3, u(dcs[3][0])[:-1] if len(u(dcs[3][0])) > 1 else b"\x80"), mz.ErrCorrupt),
        "truncated": (side[:len(side) // 2], mz.ErrCorrupt),
        "no EOF chunk": (side[:-5], mz.ErrCorrupt),
        "data chunk inside": (side[:-5] + stream[dcs[0][0]:dcs[1][0]] + side[-5:], mz.ErrCorrupt),
        "second identifier": (side + side, mz.ErrUnsupported),
    }
    for name, (b, _) in bad.items():
        if name not in ("truncated", "no EOF chunk", "data chunk inside", "second identifier"):
            with pytest.raises(SM.SidecarError):
                SM.parse(b, stream)
    pat = d[5 * BS // 3:5 * BS // 3 + 16]
    h = Handle(ctx, stream)
    try:
        plain = h.search(pat)
        for first in (None, side):
            if first is not None:
                h.attach(first)
            before = h.search(pat)
            assert before[1] == SMod.brute(d, pat) and (before[2][1] < len(sizes)) == (first is not None)
            for name, (b, err) in bad.items():
                with pytest.raises(err):
                    h.attach(b)
                assert h.search(pat) == before, name
            host = np.frombuffer(side, np.uint8).copy()
            with pytest.raises(mz.MinLZError) as e:
                h.rd.attach_sidecar(host.ctypes.data, len(side))
            assert int(str(e.value).split()[2]) == MLZ_ERR_ARG and h.search(pat) == before
        h.rd.detach_sidecar()
        assert h.search(pat) == plain
        # a sidecar without a usable info chunk attaches: the search decodes everything
        h.attach(side[:10] + b"\x44\x03\x00\x00\x09\x06\x10" + b"\x44\x03\x00\x00\x01\x09\x10" + side[10 + 7 + 15:])
        assert h.search(pat)[2] == (len(sizes), len(sizes), 0)
    finally:
        h.close()


# ---- arguments ----

def test_build_arguments(ctx):
    L = _lib.lib()
    d = data_for("text_like", 4 << 10, 6, 77)
    stream = O.stream_encode(d, 1, 4 << 10)
    h = Handle(ctx, stream)
    try:
        good = h.build([T1[6], T4])
        assert good == SM.build(stream, d, [T1[6][1], T4[1]])
        assert len(h.build([T1[6], T4], cap=len(good))) == len(good)                     # room for exactly the result

        def raw(cfgs, n, cap, dst=None):
            arr = (_lib.SearchConfig * max(len(cfgs), 1))(*cfgs)
            room = torch.full((max(cap, 0) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            r = L.mlz_dev_reader_build_sidecar(h.rd.handle, None, 0, arr if cfgs else None, n, room.data_ptr() if dst is None else dst, cap)
            assert (room.cpu().numpy() == 0x5A).all(), "written by a refused call"
            return r

        ok = [T1[6][0], T4[0]]
        for cap in (len(good) - 1, len(good) // 2, 20, 0):
            assert raw(ok, 2, cap) == -MLZ_ERR_DST_TOO_SMALL, cap
        assert raw(ok, 0, 1 << 20) == -MLZ_ERR_ARG and raw(ok * 3, 5, 1 << 20) == -MLZ_ERR_ARG and raw([], 1, 1 << 20) == -MLZ_ERR_ARG

        def broken(**kw):
            c = search_config(kw.pop("T", 1), 6, kw.pop("prefix", b""), 0)
            for k, v in kw.items():
                setattr(c, k, v)
            return c

        r2 = broken()
        r2.reserved2[1] = 1
        for c in (broken(table_type=0), broken(table_type=5), broken(match_len=9), broken(reserved=1), r2, broken(extras=1), broken(T=2, prefix=b"ab", prefix_len=0),
                  broken(T=2, prefix=b"ab", prefix_len=9), broken(T=4, prefix=b"ab", prefix_len=0), broken(T=4, prefix=b"ab", prefix_len=257),
                  broken(T=4, prefix=b"ab", extras=11), broken(T=4, prefix=b"ab", extras=16)):
            assert raw([c], 1, 1 << 20) == -MLZ_ERR_ARG
            assert raw([ok[0], c], 2, 1 << 20) == -MLZ_ERR_ARG
            assert L.mlz_dev_reader_sidecar_bound(h.rd.handle, (_lib.SearchConfig * 1)(c), 1) == -MLZ_ERR_ARG
        host = np.empty(1 << 20, np.uint8)
        assert raw(ok, 2, 1 << 20, dst=host.ctypes.data) == -MLZ_ERR_ARG
        assert L.mlz_dev_reader_sidecar_bound(None, (_lib.SearchConfig * 1)(ok[0]), 1) == -MLZ_ERR_ARG
    finally:
        h.close()
    # a stream without a data chunk with bytes: identifier, info chunks, EOF
    empty = bytes([0xFF, 6, 0, 0]) + b"MinLz" + bytes([6]) + b"\x20\x01\x00\x00\x00"
    h = Handle(ctx, empty)
    try:
        got = h.build([T1[6], T2])
        assert got == empty[:10] + SMod.info_chunk(T1[6][1], 16) + SMod.info_chunk(T2[1], 16) + SM.EOF_CHUNK == SM.build(empty, b"", [T1[6][1], T2[1]])
        h.attach(got)
        assert h.search(b"abc")[0] == 0
    finally:
        h.close()
    # concatenated streams
    two = stream + stream
    h = Handle(ctx, two)
    try:
        with pytest.raises(mz.ErrUnsupported):
            h.build([T1[6]])
    finally:
        h.close()
