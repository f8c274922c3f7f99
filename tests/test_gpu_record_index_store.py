"""The stored record index on the device (include/minlz_hip_record_index_store.h; DeviceReader.save_record_index / load_record_index,
Context.record_index_build_device, DeviceStream's and HipTensorCodec's forms) against tests/record_index_store_model.py: save and build are the
model's bytes, load on a fresh handle restores the index that index_records builds on a twin handle without decoding a chunk, and every
corruption of a model blob ends in its error code with the handle unchanged.  Every output sits between sentinel bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
from minlz_amd import _lib, api, shard
from tests import record_index_store_cases as K
from tests import record_index_store_model as M
from tests.search_gpu import SENT, Opened, dev_u64, dev_u8, gather

pytestmark = pytest.mark.gpu

BAND = 64
BS = 64 << 10
NL = b"\n"
IGNORE_CRC = 2
COUNTER_RANGE_CHUNKS = 7


def banded(n, shift):
    """Room for n bytes that lies `shift` bytes off a 256-byte boundary, between two sentinel bands -> (the tensor, the room's address)."""
    t = torch.full((BAND + shift + n + BAND,), 0x5A, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + BAND + shift


def bands_of(t, n, shift):
    """-> (the room's bytes, whether both bands and nothing else are untouched)"""
    a = t.cpu().numpy()
    lo = BAND + shift
    return a[lo:lo + n].tobytes(), bool((a[:lo] == 0x5A).all() and (a[lo + n:] == 0x5A).all())


def placed(blob, shift):
    """The blob on the device, `shift` bytes off a 256-byte boundary, with nothing of its own behind it but a band -> (tensor, address)"""
    t, p = banded(len(blob), shift)
    t[BAND + shift:BAND + shift + len(blob)] = dev_u8(blob)
    return t, p


class Handle(Opened):
    def __init__(self, ctx, stream, data):
        super().__init__(ctx, stream)
        self.stream, self.data = bytes(stream), data

    def save(self, shift=0, cap=None):
        """-> (the call's value, the room's bytes up to the bound, info); the bands are checked."""
        bound = self.rd.record_index_bound()
        cap = bound if cap is None else cap
        t, p = banded(bound, shift)
        info = (C.c_uint64 * 4)()
        r = _lib.lib().mlz_dev_reader_save_record_index(self.rd.handle, None, p, cap, info)
        torch.cuda.synchronize()
        room, clean = bands_of(t, bound, shift)
        assert clean, "save wrote outside its room"
        if r < 0:
            assert room == b"\x5a" * bound, "a refused save wrote"
            return r, None, [int(v) for v in info]
        assert room[r:] == b"\x5a" * (bound - r), "save wrote behind the blob"
        return r, room[:r], [int(v) for v in info]

    def load(self, blob, shift=0, flags=0):
        """-> (the call's value, info)"""
        t, p = placed(blob, shift)
        info = (C.c_uint64 * 4)()
        r = _lib.lib().mlz_dev_reader_load_record_index(self.rd.handle, None, flags, p, len(blob), info)
        torch.cuda.synchronize()
        assert bands_of(t, len(blob), shift) == (bytes(blob), True), "load wrote to the blob"
        return r, [int(v) for v in info]

    def spans(self, idx):
        n = len(idx)
        d_idx = dev_u64(idx)
        off = torch.full((n + 8,), SENT, dtype=torch.int64, device="cuda")
        ln = torch.full((n + 8,), SENT, dtype=torch.int64, device="cuda")
        r = _lib.lib().mlz_dev_reader_record_spans(self.rd.handle, None, d_idx.data_ptr() if n else None, n, off.data_ptr(), ln.data_ptr())
        torch.cuda.synchronize()
        off, ln = off.cpu().numpy(), ln.cpu().numpy()
        assert (off[n:] == SENT).all() and (ln[n:] == SENT).all()
        return r, off[:n], ln[:n]

    def records(self, idx):
        n = len(idx)
        total, _, ln = self.spans(idx)
        d_idx = dev_u64(idx)
        dst = torch.full((total + BAND,), 0x5A, dtype=torch.uint8, device="cuda")
        got = self.rd.read_records(d_idx.data_ptr() if n else None, n, dst.data_ptr(), total)
        torch.cuda.synchronize()
        a = dst.cpu().numpy()
        assert got == total and (a[total:] == 0x5A).all()
        return a[:total].tobytes()

    def grep(self, patterns, **kw):
        cap = max(self.rd.record_count(), 1)
        no = torch.full((cap + 8,), SENT, dtype=torch.int64, device="cuda")
        kind = torch.full((cap + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        R, totals, _ = self.rd.grep_records(patterns, no.data_ptr(), kind.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        return R, totals, no.cpu().numpy()[:R].tolist(), kind.cpu().numpy()[:R].tolist()


def expected_spans(D, size):
    """(start, length) of every record, from D"""
    D = D.astype(np.int64)
    N = M.records(len(D), size, len(D) > 0 and int(D[-1]) == size - 1)
    start = np.concatenate([[0], D + 1])[:N]
    end = np.concatenate([D, [size]])[:N]
    return start, end - start


def check_loaded(loaded, twin, D, size):
    """The handle `loaded` (its index came from a blob) answers as `twin` (index_records on the same stream) and as D says."""
    N = twin.rd.record_count()
    assert loaded.rd.record_count() == N
    start, length = expected_spans(D, size)
    assert len(start) == N
    r, off, ln = loaded.spans(np.arange(N))
    assert r == int(length.sum()) and (off == start).all() and (ln == length).all(), "the loaded index is not D"
    r2, off2, ln2 = twin.spans(np.arange(N))
    assert r2 == r and (off2 == off).all() and (ln2 == ln).all()
    if N:
        rng = np.random.default_rng(3)
        idx = np.unique(np.concatenate([[0, N - 1, N // 2], rng.integers(0, N, 40)]))[::-1].copy()
        assert loaded.records(idx) == twin.records(idx)
        for kw in (dict(), dict(invert=True, after=1)):
            assert loaded.grep([b"aaaa", b"a\x0b"], **kw) == twin.grep([b"aaaa", b"a\x0b"], **kw)


def stream_of(data, bs=BS):
    return O.stream_encode(data.tobytes(), 1, bs)


def build_raw(ctx, data, shift, delim=K.DELIM, cap=None):
    """mlz_record_index_build_device over data placed `shift` bytes off a 256-byte boundary -> (value, blob, info)"""
    n = len(data)
    src, sp = banded(n, shift)
    if n:
        src[BAND + shift:BAND + shift + n] = torch.from_numpy(data.copy()).cuda()
    bound = api.record_index_bound(n)
    cap = bound if cap is None else cap
    t, p = banded(bound, (shift + 1) & 3)
    info = (C.c_uint64 * 4)()
    r = _lib.lib().mlz_record_index_build_device(ctx.handle, None, sp if n else None, n, delim, p, cap, info)
    torch.cuda.synchronize()
    room, clean = bands_of(t, bound, (shift + 1) & 3)
    assert clean and bands_of(src, n, shift) == (data.tobytes(), True)
    if r < 0:
        assert room == b"\x5a" * bound
        return r, None, [int(v) for v in info]
    assert room[r:] == b"\x5a" * (bound - r)
    return r, room[:r], [int(v) for v in info]


def tile_kinds(D, size):
    counts = np.diff(np.searchsorted(D, np.arange(M.ntiles(size) + 1, dtype=np.uint64) * np.uint64(M.TILE)))
    return int((counts <= M.SPARSE_MAX).sum()), int((counts > M.SPARSE_MAX).sum())


def round_trip(ctx, stream, data, D, size, shift, streams=None, open_=None):
    """save = the model's bound blob; load on a fresh handle = the twin's index, nothing decoded; build over the raw bytes = the model's
    unbound blob, which loads too."""
    open_ = open_ or (lambda: Handle(ctx, stream, data))
    twin, fresh, third = open_(), open_(), open_()
    try:
        N, info = twin.rd.index_records(NL)
        k = len(D)
        assert (N, info[1]) == (M.records(k, size, k > 0 and int(D[-1]) == size - 1), k)
        want = M.pack(D, size, K.DELIM, bound=M.binding_of(*(streams or [stream])))
        assert twin.rd.record_index_bound() >= len(want)
        r, blob, sinfo = twin.save(shift)
        assert r == len(want) and blob == want, "save is not the model's blob"
        assert sinfo == [len(want), M.nsections(size)] + list(tile_kinds(D, size))
        # load: a fresh handle, no chunk decoded
        r, linfo = fresh.load(blob, shift)
        assert (r, linfo) == (N, [N, k, 8 * k, 0]) and ctx.counter(COUNTER_RANGE_CHUNKS) == 0
        check_loaded(fresh, twin, D, size)
        assert fresh.save((shift + 2) & 3)[1] == want, "a loaded index saves to other bytes"
        # build from the raw bytes: the unbound blob
        r, raw_blob, binfo = build_raw(ctx, data, shift)
        want_raw = M.pack(D, size, K.DELIM)
        assert r == len(want_raw) and raw_blob == want_raw and binfo == [len(want_raw)] + sinfo[1:], "build is not the model's blob"
        r, linfo = third.load(raw_blob, (shift + 3) & 3)
        assert (r, linfo) == (N, [N, k, 8 * k, 0])
        check_loaded(third, twin, D, size)
    finally:
        for h in (twin, fresh, third):
            h.close()


SHAPES = K.shapes()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes(ctx, case, shift):
    """Every shape at a 4-aligned blob (the dword path) and at an odd address (the bytewise path)."""
    name, size, D = case
    data = K.data_of(size, D)
    round_trip(ctx, stream_of(data), data, D, size, shift)


def test_set_handle_of_three_streams(ctx):
    """A handle over three streams saves and loads like any handle: its chunk table binds the blob; records cross from stream to stream."""
    sizes = [70000, 65536 + 9, 40000]
    size = sum(sizes)
    rng = np.random.default_rng(5)
    D = np.unique(np.concatenate([rng.integers(0, size, 900).astype(np.uint64), np.arange(71000, 71000 + 5000, dtype=np.uint64), np.array([69999, 70000], np.uint64)]))
    data = K.data_of(size, D)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    streams = [O.stream_encode(data[cuts[i]:cuts[i + 1]].tobytes(), 1, 16 << 10) for i in range(3)]
    buf, spans = b"", []
    for s in streams:
        buf += b"\xee" * 5
        spans.append((len(buf), len(s)))
        buf += s
    t = dev_u8(buf)

    class SetHandle(Handle):
        def __init__(self):
            self.ctx, self.t, self.stream, self.data = ctx, t, None, data
            self.rd, results = ctx.stream_open_batch_device(t.data_ptr(), spans)
            assert results == sizes

    round_trip(ctx, None, data, D, size, 2, streams=streams, open_=SetHandle)
    # a blob of the set does not load into a handle of the first stream alone, nor into a set in another order
    one = Handle(ctx, streams[0], None)
    whole = SetHandle()
    try:
        whole.rd.index_records(NL)
        blob = whole.save()[1]
        assert one.load(blob)[0] == -M.ERR_ARG
    finally:
        one.close()
        whole.close()


def test_two_sections(ctx):
    """64 MiB + 65537 bytes: the second section starts at position 67 108 864; delimiters on both sides of the border and a dense tile behind it."""
    name, size, D = K.two_sections()
    data = K.data_of(size, D)
    stream = gather(ctx, [data.tobytes()], 4 << 20)
    assert M.nsections(size) == 2
    round_trip(ctx, stream, data, D, size, 0)


def test_refusals_of_save_and_build(ctx):
    """A room that is too small is refused with the size it needs and nothing written; no index, NULL and foreign flags are argument errors."""
    size, D = K.BASE_SIZE, K.BASE_D
    data = K.data_of(size, D)
    h = Handle(ctx, stream_of(data), data)
    try:
        L = _lib.lib()
        room = torch.zeros(64, dtype=torch.uint8, device="cuda")
        info = (C.c_uint64 * 4)()
        assert L.mlz_dev_reader_record_index_bound(h.rd.handle) == -M.ERR_ARG
        assert L.mlz_dev_reader_save_record_index(h.rd.handle, None, room.data_ptr(), 64, info) == -M.ERR_ARG    # (no index)
        with pytest.raises(api.MinLZError):
            h.rd.record_index_bound()
        h.rd.index_records(NL)
        want = M.pack(D, size, K.DELIM, bound=M.binding_of(h.stream))
        r, _, sinfo = h.save(cap=len(want) - 1)
        assert r == -M.ERR_DST_TOO_SMALL and sinfo[0] == len(want)
        assert h.save(cap=len(want))[1] == want
        assert L.mlz_dev_reader_save_record_index(h.rd.handle, None, None, 1 << 20, info) == -M.ERR_ARG
        assert L.mlz_dev_reader_load_record_index(h.rd.handle, None, 4, room.data_ptr(), 64, info) == -M.ERR_ARG
        assert L.mlz_dev_reader_load_record_index(h.rd.handle, None, 0, None, 64, info) == -M.ERR_ARG
        host = np.zeros(128, np.uint8)
        assert L.mlz_dev_reader_load_record_index(h.rd.handle, None, 0, host.ctypes.data, 128, info) == -M.ERR_ARG   # (host memory)
        r, _, binfo = build_raw(ctx, data, 0, cap=len(want) - 60)
        assert r == -M.ERR_DST_TOO_SMALL and binfo[0] == len(M.pack(D, size, K.DELIM))
        assert L.mlz_record_index_build_device(ctx.handle, None, None, 5, 10, room.data_ptr(), 64, info) == -M.ERR_ARG
    finally:
        h.close()


# ---- corruptions: the stated code, and a handle that keeps what it had ----

def longest_of(D, size):
    start, length = expected_spans(D, size)
    return int(length.max())


@pytest.fixture(scope="module")
def corrupt_setup(ctx):
    base_data, small_data = K.data_of(K.BASE_SIZE, K.BASE_D), K.data_of(K.SMALL_SIZE, K.SMALL_D)
    base_stream, small_stream = stream_of(base_data), stream_of(small_data)
    binding = M.binding_of(base_stream)
    base = M.pack(K.BASE_D, K.BASE_SIZE, K.DELIM, bound=binding, longest=longest_of(K.BASE_D, K.BASE_SIZE))
    small = M.pack(K.SMALL_D, K.SMALL_SIZE, K.DELIM)
    hs = {"base": Handle(ctx, base_stream, base_data), "small": Handle(ctx, small_stream, small_data)}
    yield hs, {"base": (K.BASE_SIZE,) + binding, "small": (K.SMALL_SIZE,) + M.binding_of(small_stream)}, base, small
    for h in hs.values():
        h.close()


def test_corruptions(ctx, corrupt_setup):
    """Each corruption of a model blob: the model's unpack names the code, the load returns it — on a handle without an index, which then
    still has none, and on a handle with an index of another delimiter, which still answers as before."""
    hs, expect, base, small = corrupt_setup
    cases = K.corruptions(base, small)
    for name, which, blob, ignore_crc, code in cases:
        with pytest.raises(M.StoreError) as e:
            M.unpack(blob, ignore_crc, expect=expect[which])
        assert e.value.code == code, name
    flags = lambda ignore_crc: IGNORE_CRC if ignore_crc else 0   # noqa: E731
    # no index: the handle still has none
    for i, (name, which, blob, ignore_crc, code) in enumerate(cases):
        h = hs[which]
        assert h.load(blob, i & 3, flags(ignore_crc))[0] == -code, name
        assert _lib.lib().mlz_dev_reader_record_count(h.rd.handle) == -M.ERR_ARG, name
    # an index of another delimiter: it still answers
    before = {}
    for which, h in hs.items():
        N, _ = h.rd.index_records(b"a")
        idx = np.unique(np.linspace(0, N - 1, 50).astype(np.int64))
        before[which] = (N, idx, h.spans(idx), h.records(idx[:5]))
    for i, (name, which, blob, ignore_crc, code) in enumerate(cases):
        h = hs[which]
        N, idx, spans, recs = before[which]
        assert h.load(blob, (i + 1) & 3, flags(ignore_crc))[0] == -code, name
        assert h.rd.record_count() == N, name
        got = h.spans(idx)
        assert got[0] == spans[0] and (got[1] == spans[1]).all() and (got[2] == spans[2]).all(), name
        assert h.rd.index_records(b"a")[1][3] == 0, name       # (the index is still the one for b"a": nothing is decoded)
    assert hs["base"].records(before["base"][1][:5]) == before["base"][3]
    # and the blobs themselves load: the delimiter and the longest record are the header's
    for which, blob in (("base", base), ("small", small)):
        h = hs[which]
        D, size = (K.BASE_D, K.BASE_SIZE) if which == "base" else (K.SMALL_D, K.SMALL_SIZE)
        assert h.load(blob, 1)[0] == M.records(len(D), size, False)
        assert h.rd.index_records(NL)[1][3] == 0
    saved = hs["base"].save()[1]
    assert saved == base, "the longest record of the blob did not come back"
    other = M.reheader(base, delimiter=0x3B)
    assert hs["base"].load(other)[0] == len(K.BASE_D) + 1 and hs["base"].rd.index_records(b";")[1][3] == 0


def test_a_bound_blob_of_another_stream_of_the_same_size(ctx):
    """Two streams of the same size and the same delimiters' count: the blob of one is refused by the other; an unbound blob of the first
    one's raw bytes loads into both (its header says it is checked by the size alone)."""
    size = 2 * M.TILE + 77
    Da, Db = np.array([5, 70000, size - 1], np.uint64), np.array([6, 70001, size - 1], np.uint64)
    da, db = K.data_of(size, Da), K.data_of(size, Db)
    a, b = Handle(ctx, stream_of(da), da), Handle(ctx, stream_of(db), db)
    try:
        a.rd.index_records(NL)
        blob = a.save()[1]
        assert api.record_index_parse(blob)["bound"]
        assert b.load(blob)[0] == -M.ERR_ARG and _lib.lib().mlz_dev_reader_record_count(b.rd.handle) == -M.ERR_ARG
        raw = build_raw(ctx, da, 3)[1]
        assert not api.record_index_parse(raw)["bound"]
        assert b.load(raw)[0] == 3 and a.load(raw)[0] == 3
    finally:
        a.close()
        b.close()


def test_tensor_layer(ctx):
    """DeviceStream.save_record_index / load_record_index and HipTensorCodec.build_record_index."""
    size, D = K.BASE_SIZE, K.BASE_D
    data = K.data_of(size, D)
    stream = stream_of(data)
    codec = shard.HipTensorCodec(ctx)
    t = dev_u8(stream)
    with codec.open_stream(t) as s1, codec.open_stream(t) as s2, codec.open_stream(t) as s3:
        N = s1.index_records()
        blob = s1.save_record_index()
        assert bytes(blob.cpu().numpy()) == M.pack(D, size, K.DELIM, bound=M.binding_of(stream))
        assert s2.load_record_index(blob) == N
        idx = torch.tensor([0, 3, N - 1], dtype=torch.int64, device="cuda")
        want, want_starts = s1.read_records(idx)
        got, starts = s2.read_records(idx)
        assert torch.equal(got, want) and torch.equal(starts, want_starts)
        raw = codec.build_record_index(torch.from_numpy(data.copy()).cuda())
        assert bytes(raw.cpu().numpy()) == M.pack(D, size, K.DELIM)
        assert s3.load_record_index(raw) == N
        assert torch.equal(s3.line_numbers(torch.tensor([0, 7, 8, size - 1], dtype=torch.int64, device="cuda")), s1.line_numbers(torch.tensor([0, 7, 8, size - 1], dtype=torch.int64, device="cuda")))
        with pytest.raises(api.ErrCorrupt):
            s3.load_record_index(raw[:-1].clone())
        raw_semicolon = codec.build_record_index(torch.from_numpy(data.copy()).cuda(), delimiter=b";")
        assert api.record_index_parse(bytes(raw_semicolon.cpu().numpy()))["k"] == 0
