"""A batch of streams in HBM opened as ONE handle (include/minlz_hip_stream_set.h; Context.stream_open_batch_device,
HipTensorCodec.open_streams) on the GPU.  The contract is tests/stream_set_model.py; the existing handle calls are held to the same calls
on ONE stream that holds the concatenation, opened with mlz_stream_open_device and searched under MLZ_SEARCH_NO_TABLES.  The source buffer
lies between sentinel bands and is unchanged after every test's calls; every output array is over-allocated, sentinel-filled and untouched
beyond what the contract writes."""
import ctypes as C

import numpy as np
import pytest
import torch

import minlz_amd as mz
import oracle as O
from minlz_amd import _lib, synth
from minlz_amd.device import DeviceStream, HipTensorCodec
from tests import corrupt as CM
from tests import stream_batch_cases as BC
from tests import stream_device_cases as SC
from tests import stream_set_model as M
from tests.search_gpu import dev_u8, dev_u64, gather

pytestmark = pytest.mark.gpu

SENT8, SENT32, SENT64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
FRONT, GAP, BACK, GUARD = 37, 3, 64, 8
MLZ_ERR_UNSUPPORTED, MLZ_ERR_CRC, MLZ_ERR_ARG = 3, 5, 8
U64 = 2 ** 64 - 1
NL = 10


def lines(n, seed, terminated=True):
    """n bytes of JSON lines; terminated: the last byte is the newline, else it is none."""
    d = bytearray(synth.json_like(n, seed).tobytes())
    if n:
        d[-1] = NL if terminated else ord("}")
    return bytes(d)


def guarded(n, dtype=torch.int64):
    sent = {torch.int64: SENT64, torch.int32: SENT32, torch.uint8: SENT8}[dtype]
    return torch.full((n + GUARD,), sent, dtype=dtype, device="cuda")


def clean_behind(t, n):
    """The first n values of a guarded tensor as numpy; nothing behind them was written."""
    a = t.cpu().numpy()
    sent = {np.dtype(np.int64): SENT64, np.dtype(np.int32): SENT32, np.dtype(np.uint8): SENT8}[a.dtype]
    assert (a[n:] == sent).all(), "written beyond an output's size"
    return a[:n]


def dev_u32(values):
    a = np.asarray(values, dtype=np.uint32).view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def token(d, at, n=12):
    """n bytes of d from `at` on or behind it that hold no newline."""
    while NL in d[at:at + n]:
        at += 1
    return d[at:at + n]


def raw(name, *args):
    """The ABI function as it returns: negative codes are results here."""
    return int(getattr(_lib.lib(), name)(*args))


def read_streams(rd, ranges, flags=0, cap=None):
    """mlz_dev_reader_read_streams_device with guarded outputs -> (result, the bytes written, the starts); a refused call has written nothing."""
    n = len(ranges)
    total = sum(r[2] for r in ranges if r[2] < 1 << 40)
    cap = total if cap is None else cap
    which, off, ln = dev_u32([r[0] for r in ranges]), dev_u64([r[1] for r in ranges]), dev_u64([r[2] for r in ranges])
    dst, st = guarded(cap, torch.uint8), guarded(n + 1)
    r = raw("mlz_dev_reader_read_streams_device", rd.handle, None, flags, which.data_ptr(), off.data_ptr(), ln.data_ptr(), n, dst.data_ptr(), cap, st.data_ptr())
    torch.cuda.synchronize()
    if r < 0:   # (a refusal is decided in front of every decode and copy; a chunk's error is known behind them)
        assert r != -MLZ_ERR_ARG or ((dst.cpu().numpy() == SENT8).all() and (st.cpu().numpy() == SENT64).all()), "a refused call wrote"
        clean_behind(dst, cap), clean_behind(st, n + 1)
        return r, None, None
    return r, clean_behind(dst, r).tobytes(), clean_behind(st, n + 1).tolist()


def locate(rd, name, values):
    """mlz_dev_reader_locate or _locate_records with guarded outputs -> (result, which, local)."""
    n = len(values)
    which, local = guarded(n, torch.int32), guarded(n)
    items = dev_u64(values)
    r = raw(name, rd.handle, None, items.data_ptr(), n, which.data_ptr(), local.data_ptr())
    torch.cuda.synchronize()
    return r, (clean_behind(which, n).astype(np.int64) & 0xFFFFFFFF).tolist(), clean_behind(local, n).tolist()


class Set:
    """Sources laid back to back (GAP sentinel bytes between two) into one device buffer between its bands, `order`: the descriptor list
    as indices into the sources (repeats allowed), opened as one handle.  datas[i]: descriptor i's decoded bytes, None for a framing error."""

    def __init__(self, ctx, sources, datas, order=None):
        buf, spans = BC.back_to_back(sources, GAP)
        order = list(range(len(sources))) if order is None else order
        self.ctx, self.spans = ctx, [spans[k] for k in order]
        self.datas = [datas[k] for k in order]
        self.failed = {i for i, d in enumerate(self.datas) if d is None}
        self.clean = [b"" if d is None else d for d in self.datas]
        self.image = np.concatenate([np.full(FRONT, 0xA5, np.uint8), np.frombuffer(buf, np.uint8), np.full(BACK, 0xA5, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()
        self.rd, self.res = ctx.stream_open_batch_device(self.src, self.spans)
        self.size = M.sizes(self.clean)
        self.base = M.bases(self.size)
        self.all = M.concat(self.clean)

    @property
    def src(self):
        return self.t.data_ptr() + FRONT

    def single(self, i):
        """mlz_stream_open_device on descriptor i alone -> what it returns."""
        off, n = self.spans[i]
        h = C.c_void_p()
        r = raw("mlz_stream_open_device", self.ctx.handle, None, self.src + off if n else None, n, C.byref(h))
        if h:
            _lib.lib().mlz_dev_reader_close(h)
        return r

    def unchanged(self):
        torch.cuda.synchronize()
        assert np.array_equal(self.t.cpu().numpy(), self.image), "the input was modified"

    def read_streams(self, ranges, flags=0, cap=None):
        return read_streams(self.rd, ranges, flags, cap)

    def locate(self, name, values):
        return locate(self.rd, name, values)

    def close(self):
        self.rd.close()


# ---- 1. open ----

def _mixed_sources(ctx):
    """(stream, data or None) in the order they lie in the buffer."""
    rng = np.random.default_rng(5)
    big = lines(30_000 + 11, 31)
    whole = O.stream_encode(lines(20_000, 32), 1, 4 << 10)
    cut = whole[:CM.chunks(whole)[4].off + 4 + 50]                               # a framing error in the middle: cut inside a chunk's body
    out = [
        (O.stream_encode(b"", 1, 1 << 20), b""),                                 # the empty stream
        (SC.stream_id(64 << 10), None),                                          # an identifier alone: no EOF chunk, a framing error
        (b"", b""),                                                              # no bytes
        (O.stream_encode(b"x", 1, 1 << 20), b"x"),
        (O.stream_encode(b"\n", 2, 4 << 10), b"\n"),
        (O.stream_encode(big, 1, 4 << 10), big),                                 # 8 chunks of 4 KiB
        (cut, None),
        (b"\x00\x01\x02 not a stream at all", None),                             # a framing error at position 0
        (O.stream_encode(synth.random_bytes(9_000, seed=33).tobytes(), 1, 4 << 10), synth.random_bytes(9_000, seed=33).tobytes()),   # stored chunks
        (O.stream_encode(b"y", 1, 1 << 20), b"y"),
    ]
    for k in range(28):
        n = int(rng.choice([1, 2, 77, 900, 4096, 4097, 12_345]))
        d = lines(n, 40 + k, terminated=k % 3 != 0)
        s = mz.stream_encode(d, mz.LevelFastest, 4 << 10, k % 2 == 0, ctx) if k % 4 == 0 else O.stream_encode(d, 1 + k % 2, (4 << 10) << (k % 3), k % 5 == 0)
        out.append((s, d))
    for s, d in out:
        if d is not None:
            assert O.stream_decode(s, len(d) + 1) == d
    return out


@pytest.fixture(scope="module")
def mixed(ctx):
    src = _mixed_sources(ctx)
    n = len(src)
    order = list(range(n - 1, -1, -1)) + [5, 5, 0]                               # descending source order, then a span three times in all
    s = Set(ctx, [a for a, _ in src], [d for _, d in src], order)
    yield s
    s.unchanged()
    s.close()


def test_open(ctx, mixed):
    s = mixed
    n = len(s.spans)
    assert n >= 40 and len(s.failed) == 3 and s.spans[0][0] > s.spans[1][0] > s.spans[2][0]
    singles = [s.single(i) for i in range(n)]
    assert s.res == singles
    assert [r for i, r in enumerate(s.res) if i not in s.failed] == [len(d) for i, d in enumerate(s.clean) if i not in s.failed]
    assert all(s.res[i] < 0 for i in s.failed)
    assert s.rd.size == sum(s.size) == len(s.all) and s.rd.stream_count() == n and s.rd.stream_bases() == s.base
    # the tensor layer: a framing error raises with the stream's index, or the stream is skipped
    codec = HipTensorCodec(ctx)
    with pytest.raises(mz.api.MinLZError) as e:
        codec.open_streams(s.t[FRONT:], s.spans)
    assert e.value.index == min(s.failed) and e.value.code == -s.res[min(s.failed)]
    with codec.open_streams(s.t[FRONT:], s.spans, on_error="skip") as st:
        assert st.errors == {i: s.res[i] for i in s.failed} and st.sizes == s.size and st.bases == s.base and st.size == len(s.all)
        assert st.read_ranges([0, s.base[7]], [st.size, 9]).cpu().numpy().tobytes() == s.all + s.all[s.base[7]:s.base[7] + 9]
    with codec.open_streams(s.t, []) as st:
        assert st.size == 0 and st.sizes == [] and st.bases == [0] and st.locate(torch.zeros(2, dtype=torch.int64, device="cuda"))[0].tolist() == [-1, -1]
    # n_streams == 0 opens and closes
    rd, res = ctx.stream_open_batch_device(None, [])
    assert rd.size == 0 and res == [] and rd.stream_count() == 0 and rd.stream_bases() == [0]
    assert rd.index_records()[0] == 0 and rd.stream_records() == ([0], 0)
    rd.close()


# ---- 2. read ----

def test_read_whole_and_across_borders(mixed):
    s = mixed
    total = len(s.all)
    dst = guarded(total, torch.uint8)
    assert s.rd.read([(0, total, 0)], dst.data_ptr(), total) == total
    assert clean_behind(dst, total).tobytes() == s.all
    dst = guarded(total, torch.uint8)
    off, ln = dev_u64([0]), dev_u64([total])
    assert s.rd.read_device(off.data_ptr(), ln.data_ptr(), 1, dst.data_ptr(), total) == total
    assert clean_behind(dst, total).tobytes() == s.all
    # ranges that span a stream border (and runs of empty streams), in descending order
    borders = [b for b in sorted(set(s.base)) if 5 <= b <= total - 7]
    ranges = [(b - 5, 12) for b in reversed(borders)] + [(s.base[3], s.base[-4] - s.base[3])]
    want = b"".join(s.all[o:o + n] for o, n in ranges)
    dst, st = guarded(len(want), torch.uint8), guarded(len(ranges) + 1)
    off, ln = dev_u64([o for o, _ in ranges]), dev_u64([n for _, n in ranges])
    got = s.rd.read_device(off.data_ptr(), ln.data_ptr(), len(ranges), dst.data_ptr(), len(want), d_starts=st.data_ptr())
    assert got == len(want) and clean_behind(dst, got).tobytes() == want and len(borders) > 20
    assert clean_behind(st, len(ranges) + 1).tolist() == np.concatenate([[0], np.cumsum([n for _, n in ranges])]).tolist()


def test_read_streams(mixed):
    s = mixed
    rng = np.random.default_rng(6)
    ranges = []
    for i, d in enumerate(s.clean):
        n = len(d)
        ranges += [(i, 0, n), (i, n, 0), (i, 0, 0), (i, n // 2, n - n // 2), (i, n - min(n, 3), min(n, 3))]   # whole, empty at the end, empty, to the end exactly
    ranges += [(int(i), int(o), int(rng.integers(0, len(s.clean[i]) - o + 1))) for i in rng.integers(0, len(s.clean), 200) for o in [rng.integers(0, len(s.clean[i]) + 1)]]
    r, got, st = s.read_streams(ranges)
    want = [s.clean[i][o:o + n] for i, o, n in ranges]
    assert r == sum(map(len, want)) and got == b"".join(want) and st == np.concatenate([[0], np.cumsum(list(map(len, want)))]).tolist()
    # every bad range alone among good ones: refused, and nothing is written
    i = next(i for i, d in enumerate(s.clean) if len(d) > 1000)
    f = min(s.failed)
    n = len(s.clean[i])
    good = [(i, 0, 10), (i + 1, 0, 0)]
    for bad in [(i, n, 1), (i, 0, n + 1), (i, n - 4, 5), (i, n + 1, 0), (i, U64, 0), (i, U64, 1), (i, 1, U64), (i, U64, U64), (len(s.clean), 0, 0), (0xFFFFFFFF, 0, 0), (f, 0, 1), (f, 1, 0)]:
        assert s.read_streams(good + [bad] + good, cap=64)[0] == -MLZ_ERR_ARG, bad
    assert s.read_streams(good + [(f, 0, 0), (i, n, 0)] + good)[0] == 20


def test_many_tiny_ranges_over_300_streams(ctx):
    """70 000 ranges of 0 .. 8 bytes over 300 streams: more than one workgroup in the range check and in the locate kernels."""
    rng = np.random.default_rng(9)
    datas = [lines(int(n), 100 + k, terminated=k % 7 != 0) for k, n in enumerate(rng.choice([0, 1, 30, 200, 700], 300))]
    s = Set(ctx, [O.stream_encode(d, 1, 4 << 10) for d in datas], datas)
    try:
        assert s.res == s.size and s.rd.stream_bases() == s.base
        which = rng.integers(0, 300, 70_000)
        size = np.asarray(s.size)[which]
        off = (rng.random(70_000) * (size + 1)).astype(np.int64)
        ln = np.minimum(size - off, rng.integers(0, 9, 70_000))
        r, got, st = s.read_streams(list(zip(which.tolist(), off.tolist(), ln.tolist())))
        want = b"".join(datas[w][o:o + n] for w, o, n in zip(which.tolist(), off.tolist(), ln.tolist()))
        assert r == len(want) and got == want and st[-1] == r
        # locate: 70 000 positions, the designed ones among them
        pos = rng.integers(0, len(s.all) + 50, 70_000).tolist() + [b for b in s.base] + [b - 1 for b in s.base if b] + [len(s.all) - 1, len(s.all), U64]
        r, w, l = s.locate("mlz_dev_reader_locate", pos)
        want = [M.locate(s.base, p) for p in pos]
        assert (w, l) == ([a for a, _ in want], [b for _, b in want]) and r == sum(1 for p in pos if p < len(s.all))
        # the records of every stream, and 70 000 record numbers
        N = s.rd.index_records()[0]
        first, joined = s.rd.stream_records()
        assert first == M.first(s.base, s.all, NL) and first[-1] == N and joined == M.joined(s.base, s.all, NL) > 10
        recs = rng.integers(0, N + 20, 70_000).tolist() + first + [N - 1, N, U64]
        starts = M.record_starts(s.all, NL)
        r, w, l = s.locate("mlz_dev_reader_locate_records", recs)
        want = [M.locate_record(s.base, s.all, NL, q) for q in recs[:3000] + recs[70_000:]]   # (the model is slow: a sample and the designed ones)
        assert (w[:3000] + w[70_000:], l[:3000] + l[70_000:]) == ([a for a, _ in want], [b for _, b in want]) and r == sum(1 for q in recs if q < N)
        fast = np.searchsorted(np.asarray(s.base), np.asarray(starts)[np.minimum(recs[:70_000], N - 1)], side="right") - 1
        inside = np.asarray(recs[:70_000]) < N
        assert (np.asarray(w[:70_000])[inside] == fast[inside]).all() and (np.asarray(w[:70_000])[~inside] == M.NO_STREAM).all()
        s.unchanged()
    finally:
        s.close()


# ---- 3. the existing calls: the set against ONE stream that holds the concatenation ----

def _eq(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return a.shape == b.shape and bool((a == b).all())
    return a == b


def _equivalence(ctx, sources, datas, planted, spans_of=None):
    """Every existing call on the set and on the single stream of the same bytes -> the set (open) and the single handle's stats of one search."""
    codec = HipTensorCodec(ctx)
    buf, spans = BC.back_to_back(sources, GAP)
    t = dev_u8(buf)
    st = codec.open_streams(t, spans)
    whole = b"".join(datas)
    one = DeviceStream(ctx, dev_u8(O.stream_encode(whole, 1, 64 << 10)))
    try:
        assert st.size == one.size == len(whole) and st.sizes == [len(d) for d in datas] and st.bases == M.bases(st.sizes) and not st.errors
        pats = [planted, b"user_", b"\":\"", whole[1000:1007], b"absent-everywhere", b"T"]
        for kw in (dict(), dict(ignore_case=True)):
            assert _eq(st.search(planted, 50, **kw), one.search(planted, 50, no_tables=True, **kw))
            assert _eq(st.search_many(pats, 5000, **kw), one.search_many(pats, 5000, no_tables=True, **kw))
            assert _eq(st.search_many(pats, 0, **kw), one.search_many(pats, 0, no_tables=True, **kw))
        assert _eq(st.search_records(planted, max_records=64), one.search_records(planted, no_tables=True, max_records=64))
        assert _eq(st.search_records(b"tag15", max_records=7, max_bytes=900), one.search_records(b"tag15", no_tables=True, max_records=7, max_bytes=900))
        N = st.index_records()
        assert N == one.index_records() == len(M.records(whole, NL)) and st.reader.record_count() == N
        idx = torch.from_numpy(np.random.default_rng(3).integers(0, N, 500)).cuda()
        sp = [torch.zeros(1000, dtype=torch.int64, device="cuda") for _ in range(2)]
        tot = [h.reader.record_spans(idx.data_ptr(), 500, x.data_ptr(), x[500:].data_ptr()) for h, x in zip((st, one), sp)]
        assert tot[0] == tot[1] and _eq(sp[0], sp[1])
        assert _eq(st.read_records(idx), one.read_records(idx))
        pos = torch.from_numpy(np.random.default_rng(4).integers(0, len(whole) + 9, 800)).cuda()
        assert _eq(st.line_numbers(pos), one.line_numbers(pos))
        assert st.reader.record_range(3, N - 5) == one.reader.record_range(3, N - 5)
        for kw in (dict(), dict(invert=True), dict(before=2, after=2), dict(count_only=True), dict(ignore_case=True, after=1), dict(max_records=9)):
            assert _eq(st.grep([planted, b"Tom", b"zq"], **kw), one.grep([planted, b"Tom", b"zq"], no_tables=True, **kw)), kw
        return st, one
    except BaseException:
        st.close(); one.close()
        raise


def test_equivalence_with_one_stream(ctx):
    planted = b"PLANTED-ACROSS-A-BORDER"
    datas = [lines(70_000, 61), lines(3, 62, False), b"", lines(150_000 + 5, 63, False), lines(9_000, 64), lines(1, 65), lines(40_000, 66, False)]
    h = len(planted) // 2
    datas[3] = datas[3][:-h] + planted[:h]
    datas[4] = planted[h:] + datas[4][len(planted) - h:]
    datas[0] = datas[0][:5000] + planted + datas[0][5000 + len(planted):]
    sources = [O.stream_encode(d, 1 + k % 2, (4 << 10) << k % 3) for k, d in enumerate(datas)]
    st, one = _equivalence(ctx, sources, datas, planted)
    try:
        # the planted pattern across the stream border is found, and locate shows that it crosses
        pos, total = st.search(planted, 10)
        assert total == 2 and pos.tolist() == [5000, st.bases[4] - h]
        which, local = st.locate(pos)
        assert which.tolist() == [0, 3] and local.tolist() == [5000, len(datas[3]) - h]
        assert local[1] + len(planted) > st.sizes[3] and local[0] + len(planted) <= st.sizes[0]
        w, l = st.locate(torch.tensor([st.size, st.size - 1, -1], dtype=torch.int64, device="cuda"))
        assert w.tolist() == [-1, 6, -1] and l.tolist() == [0, len(datas[6]) - 1, 0]
        # no sidecar on a set
        for f in (lambda: st.build_sidecar([]), lambda: st.attach_sidecar(st.t)):
            with pytest.raises(mz.api.ErrUnsupported):
                f()
    finally:
        st.close(); one.close()


def test_streams_with_search_tables(ctx):
    """Streams that carry type 1 tables: the set returns what the stream without tables returns, decodes every chunk and reports no usable table."""
    datas = [lines(200_000, 71), lines(70_000, 72), lines(130_000, 73)]
    needle = b"QZ-needle-7531"
    datas[1] = datas[1][:30_000] + needle + datas[1][30_000 + len(needle):]
    at = len(datas[0]) + 30_000
    assert b"".join(datas).count(needle) == 1
    sources = [gather(ctx, [d], 64 << 10, k == 0, search_match_len=6) for k, d in enumerate(datas)]
    assert all(any(c.type == 0x45 for c in CM.chunks(s)) for s in sources)
    st, one = _equivalence(ctx, sources, datas, needle)
    try:
        out = guarded(16)
        total, stats = st.reader.search(needle, out.data_ptr(), 16)
        nck = sum((len(d) + (64 << 10) - 1) // (64 << 10) for d in datas)
        assert stats == (nck, nck, 0) and clean_behind(out, total).tolist() == [at]
        total, stats = st.reader.search_many([needle, b"id"], None, None, None, 0)
        assert stats[:3] == (nck, nck, 0)
        # the middle stream alone prunes by its tables: the set does not
        t1 = dev_u8(sources[1])
        with ctx.stream_open_device(t1.data_ptr(), t1.numel()) as alone:
            assert alone.search(needle, None, 0)[1][2] > 0
    finally:
        st.close(); one.close()


# ---- 4. records per stream ----

def test_records_per_stream(ctx):
    codec = HipTensorCodec(ctx)
    datas = [lines(5_000, 81), b"", lines(1, 82), lines(12_000, 83), b"\n\n\n", lines(300, 84), b""]
    needle = token(datas[3], 6000, 5)
    buf, spans = BC.back_to_back([O.stream_encode(d, 1, 4 << 10) for d in datas], GAP)
    with codec.open_streams(dev_u8(buf), spans) as st:
        N = st.index_records()
        first, joined = st.stream_records()
        base, whole = M.bases(st.sizes), b"".join(datas)
        assert joined == 0 and first == M.first(base, whole, NL) and first[-1] == N
        for i, d in enumerate(datas):                                            # stream i owns [first[i], first[i + 1]): its own split
            got, starts = st.read_records(torch.arange(first[i], first[i + 1], dtype=torch.int64, device="cuda"))
            starts, got = starts.tolist(), got.cpu().numpy().tobytes()
            assert [got[a:b] for a, b in zip(starts, starts[1:])] == M.records(d, NL), i
        which, line, kind = st.grep_streams([needle, b"tag15"], before=1)
        R, numbers, kinds, data, starts = st.grep([needle, b"tag15"], before=1)
        want = M.grep_n(datas, (), NL, lambda r: needle in r or b"tag15" in r)
        sel = [(w, l) for w, l, k in zip(which.tolist(), line.tolist(), kind.tolist()) if k]
        assert sel == [(i, k) for i, k, _ in want] and len(sel) > 3 and R == which.numel() and _eq(kind, kinds)
        assert [(w, l) for w, l in zip(which.tolist(), line.tolist())] == [M.locate_record(base, whole, NL, r) for r in numbers.tolist()]
        with pytest.raises(ValueError):                                          # a number tensor of the wrong kind
            st.locate_records(torch.zeros(3, dtype=torch.int32, device="cuda"))
    # two unterminated streams followed by others
    datas = [lines(5_000, 85, False), b"", lines(1, 87, False), lines(700, 86), lines(900, 88, False), b"", b""]
    buf, spans = BC.back_to_back([O.stream_encode(d, 2, 4 << 10) for d in datas], GAP)
    with codec.open_streams(dev_u8(buf), spans) as st:
        with pytest.raises(mz.api.MinLZError):                                   # no index yet: as the other record calls
            st.stream_records()
        N = st.index_records()
        base, whole = M.bases(st.sizes), b"".join(datas)
        first, joined = st.stream_records()
        assert joined == 2 == M.joined(base, whole, NL) and first == M.first(base, whole, NL)
        recs = list(range(N)) + [N, N + 1]
        which, local = st.locate_records(torch.tensor(recs, dtype=torch.int64, device="cuda"))
        want = [M.locate_record(base, whole, NL, r) for r in recs]
        assert which.tolist() == [w if w != M.NO_STREAM else -1 for w, _ in want] and local.tolist() == [l for _, l in want]
        assert 2 not in which.tolist() and 0 in which.tolist()                   # the one-byte unterminated stream starts no record


# ---- 5. errors ----

def test_errors_and_a_set_of_one(ctx):
    bs = 4 << 10
    datas = [lines(20_000, 91), lines(20_000, 92), lines(20_000, 93)]
    sources = [O.stream_encode(d, 1, bs) for d in datas]
    broken = bytearray(sources[1])
    ck = [c for c in CM.chunks(sources[1]) if c.type in (1, 2, 3)][2]
    broken[ck.off + 5] ^= 0x20                                                   # the third chunk's stored CRC
    sources[1] = bytes(broken)
    s = Set(ctx, sources, datas)
    try:
        assert s.res == s.size
        n = 20_000
        assert s.read_streams([(0, 0, n), (2, 5, n - 5), (1, 0, 2 * bs), (1, 3 * bs, n - 3 * bs)])[0] == 3 * n - 5 - bs   # every chunk but the broken one
        assert s.read_streams([(0, 0, n), (1, 2 * bs + 7, 1)])[0] == -MLZ_ERR_CRC
        r, got, _ = s.read_streams([(1, 0, n)], flags=2)
        assert r == n and got == datas[1]
        dst = guarded(100, torch.uint8)
        assert raw("mlz_dev_reader_read", s.rd.handle, None, 0, (C.c_uint64 * 3)(n + 2 * bs - 10, 20, 0), 1, dst.data_ptr(), 100) == -MLZ_ERR_CRC
        # a grep touches every chunk: it fails, and works with the flag; the index is not kept from the failed build
        assert raw("mlz_dev_reader_index_records", s.rd.handle, None, 0, NL, None) == -MLZ_ERR_CRC
        assert raw("mlz_dev_reader_record_count", s.rd.handle) == -MLZ_ERR_ARG
        N = s.rd.index_records(ignore_crc=True)[0]
        assert N == len(M.records(s.all, NL))
        assert raw("mlz_dev_reader_grep_records", s.rd.handle, None, 0, b"id", (C.c_uint32 * 1)(2), 1, 0, 0, None, None, 0, (C.c_uint64 * 4)(), (C.c_uint64 * 4)()) == -MLZ_ERR_CRC
        assert s.rd.grep_records([b"id"], None, None, 0, ignore_crc=True)[0] == sum(1 for r in M.records(s.all, NL) if b"id" in r)
        # records that do not touch the broken chunk are read
        first, _ = s.rd.stream_records()
        idx = dev_u64([0, first[1] - 1, first[2], N - 1])
        dst = guarded(4000, torch.uint8)
        want = b"".join(M.records(s.all, NL)[k] for k in (0, first[1] - 1, first[2], N - 1))
        assert s.rd.read_records(idx.data_ptr(), 4, dst.data_ptr(), 4000) == len(want) and clean_behind(dst, len(want)).tobytes() == want
        # no sidecar
        cfg = (_lib.SearchConfig * 1)(mz.api.search_config(1, 6))
        room = guarded(1 << 16, torch.uint8)
        assert raw("mlz_dev_reader_build_sidecar", s.rd.handle, None, 0, cfg, 1, room.data_ptr(), 1 << 16) == -MLZ_ERR_UNSUPPORTED
        assert raw("mlz_dev_reader_attach_sidecar", s.rd.handle, None, 0, room.data_ptr(), 100) == -MLZ_ERR_UNSUPPORTED
        assert (room.cpu().numpy() == SENT8).all()
        s.unchanged()
    finally:
        s.close()
    # a handle from mlz_stream_open_device answers as a set of one
    d = datas[0][:-1] + b"}"
    t = dev_u8(O.stream_encode(d, 1, bs))
    with ctx.stream_open_device(t.data_ptr(), t.numel()) as rd:
        assert rd.stream_count() == 1 and rd.stream_bases() == [0, len(d)]
        assert locate(rd, "mlz_dev_reader_locate", [0, 7, len(d) - 1, len(d), U64]) == (3, [0, 0, 0, M.NO_STREAM, M.NO_STREAM], [0, 7, len(d) - 1, 0, 0])
        assert read_streams(rd, [(0, 5, 10), (0, len(d), 0)])[:2] == (10, d[5:15])
        assert read_streams(rd, [(1, 0, 0)], cap=8)[0] == read_streams(rd, [(0, len(d), 1)], cap=8)[0] == -MLZ_ERR_ARG
        assert raw("mlz_dev_reader_stream_records", rd.handle, None, (C.c_uint64 * 2)(), None) == -MLZ_ERR_ARG   # no index yet
        N = rd.index_records()[0]
        assert rd.stream_records() == ([0, N], 0)
        assert locate(rd, "mlz_dev_reader_locate_records", [0, N - 1, N]) == (2, [0, 0, M.NO_STREAM], [0, N - 1, 0])


# ---- 6. two decode groups ----

def test_two_decode_groups(ctx):
    """Seven streams of about 12 MiB of compressible lines in 8 MiB blocks: the healthy bytes pass one 64 MiB decode group inside the sixth
    stream (its first chunk ends group 0, its second starts group 1).  Indexed and grepped against the model."""
    unit = lines((1 << 20) + 37, 21)
    needle = b"NEEDLE-IN-TWO-GROUPS"
    datas = []
    for k in range(7):
        n = (12 << 20) + 1001 * k
        d = bytearray((unit * (n // len(unit) + 1))[:n])
        d[-1] = NL
        for o in (4321 + k, (8 << 20) - 7, n - 300):                             # inside a chunk, across the stream's chunk border, in its last line
            d[o:o + len(needle)] = needle
        datas.append(bytes(d))
    sources = [gather(ctx, [d], 8 << 20) for d in datas]
    assert sum(map(len, sources)) < 40 << 20
    buf, spans = BC.back_to_back(sources, GAP)
    codec = HipTensorCodec(ctx)
    with codec.open_streams(dev_u8(buf), spans) as st:
        assert st.sizes == [len(d) for d in datas] and st.bases[5] < 64 << 20 < st.bases[5] + (8 << 20)
        N = st.index_records()
        first, joined = st.stream_records()
        per = [M.records(d, NL) for d in datas]
        assert joined == 0 and first == list(np.concatenate([[0], np.cumsum([len(p) for p in per])])) and N == first[-1]
        which, line, kind = st.grep_streams(needle)
        want = [(i, k) for i, p in enumerate(per) for k, r in enumerate(p) if needle in r]
        assert list(zip(which.tolist(), line.tolist())) == want and len(want) == 21 and bool((kind == 1).all())
        # a range over the group border, inside stream 5
        got = st.read_stream_ranges(torch.tensor([5, 6], device="cuda"), torch.tensor([(8 << 20) - 50, 0], device="cuda"), torch.tensor([100, 10], device="cuda"))
        assert got.cpu().numpy().tobytes() == datas[5][(8 << 20) - 50:(8 << 20) + 50] + datas[6][:10]
