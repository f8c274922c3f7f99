"""Decoder verdicts on mutated blocks and streams (tests/corrupt.py) against the oracle: the code, and the bytes when valid.

Blocks: decode_batch_device batches that mix mutants with untouched blocks under every option leg of test_gpu_tile_levels (sentinel
bytes around every output range, the cut-off bytes of a truncated mutant right after its src_len), the failure sites on the default leg
(option 3), dst_cap one byte short and one byte long, the host entry points (pageable and pinned batches, mlz_decode from several threads,
mlz_decode_block, a two-context batch).  Streams: every code must be exactly the oracle's Reader's, first error in stream order."""
import ctypes as C
import threading
from collections import Counter, defaultdict

import numpy as np
import pytest

import minlz_amd as mz
import oracle as O
from minlz_amd import stream as S, synth
from minlz_amd._lib import BlockDesc
from tests import corrupt as CM
from tests import tile_levels as TL
from tests.test_gpu_tile_levels import LEGS

pytestmark = pytest.mark.gpu

OPT_DEBUG_STATUS = 3
SITE_TOTAL, SITE_OVERRUN = 2, 1
BATCH = 12
_CACHE = {}


def _own_sources(ctx):
    out = []
    for size, per in ((64 << 10, 3), (1 << 20, 3), (8 << 20, 1)):
        src = np.ascontiguousarray(synth.text_like(size, seed=size % 9973))
        for level in (mz.LevelSuperFast, mz.LevelFastest, mz.LevelBalanced):
            out.append(("own_%d_L%d" % (size, level), mz.Encode(src, level, ctx), per))
    return out


def _setup(ctx):
    """(sources by name, mutants, oracle verdict per block): made once per session, the oracle asked once per block."""
    if "m" not in _CACHE:
        srcs = [(n, b, 3) for n, b in CM.cpu_sources()] + _own_sources(ctx)
        muts = []
        for n, b, per in srcs:
            muts += CM.block_mutants(n, b, CM._seed(n), per)
        by_name = {n: b for n, b, _ in srcs}
        verdict = {}
        for b in list(by_name.values()) + [m.block for m in muts]:
            if b not in verdict:
                try:
                    verdict[b] = (0, O.decode(b))
                except O.OracleError as e:
                    verdict[b] = (e.code, None)
        _CACHE["m"] = (by_name, muts, verdict)
    return _CACHE["m"]


def _source_of(by_name, m):
    return by_name[m.name.split("/")[0]]


def _cap(block, verdict):
    code, out = verdict[block]
    if code == 0:
        return len(out)
    try:
        return O.decoded_len(block)
    except O.OracleError:
        return 16


def _batches(by_name, muts):
    """Batches of BATCH entries (block, tail, dst_cap, untouched): mutants and, every few, an untouched source block."""
    rng = np.random.default_rng(11)
    order = rng.permutation(len(muts)).tolist()
    names = sorted(by_name)
    out, cur = [], []
    for k, i in enumerate(order):
        m = muts[i]
        src = _source_of(by_name, m)
        tail = src[len(m.block):len(m.block) + 64] if src.startswith(m.block) and len(m.block) < len(src) else b""
        cur.append((m, tail))
        if k % 5 == 4:
            cur.append((names[k % len(names)], b""))
        if len(cur) >= BATCH - 1:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def _device_batch(ctx, entries, caps, debug=False):
    """decode_batch_device: blocks back to back from offset 0 (a truncated mutant followed by its cut-off bytes), outputs back to back
    with 0xA5 gaps; nothing outside [dst_off, dst_off + dst_cap) may change.  -> (out_len list, outputs)."""
    import torch
    dev = torch.device("cuda", 0)
    blocks = [b for b, _ in entries]
    offs, cur = [], 0
    for b, tail in entries:
        offs.append(cur)
        cur += len(b) + len(tail)
    host = np.zeros(cur + 64, dtype=np.uint8)
    for o, (b, tail) in zip(offs, entries):
        host[o:o + len(b) + len(tail)] = np.frombuffer(b + tail, dtype=np.uint8)
    src = torch.from_numpy(host).to(dev)
    doffs, dcur = [], 0
    for n in caps:
        doffs.append(dcur)
        dcur += n + 40
    dst = torch.full((dcur + 64,), 0xA5, dtype=torch.uint8, device=dev)
    dlen = torch.zeros(len(blocks), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx.decode_batch_device(st, src.data_ptr(), dst.data_ptr(), [BlockDesc(o, len(b), do, n) for o, b, do, n in zip(offs, blocks, doffs, caps)],
                            dlen.data_ptr())
    torch.cuda.synchronize()
    dh = dst.cpu().numpy()
    guard = np.ones(dh.size, dtype=bool)
    for do, n in zip(doffs, caps):
        guard[do:do + n] = False
    assert (dh[guard] == 0xA5).all(), "bytes outside the blocks' output ranges were written"
    return dlen.cpu().tolist(), [dh[do:do + n].tobytes() for do, n in zip(doffs, caps)]


def _run_all(ctx, debug=False):
    """Every mutant through device batches; -> list of (mutant or source name, oracle code, got out_len) and the mismatches."""
    by_name, muts, verdict = _setup(ctx)
    res, bad = [], []
    for batch in _batches(by_name, muts):
        entries, caps, want = [], [], []
        for m, tail in batch:
            blk = by_name[m] if isinstance(m, str) else m.block
            entries.append((blk, tail))
            caps.append(_cap(blk, verdict))
            want.append(verdict[blk])
        lens, outs = _device_batch(ctx, entries, caps)
        for (m, _), (code, data), l, o in zip(batch, want, lens, outs):
            name = m if isinstance(m, str) else m.name
            got = -((-l) & 0xFF) if l < 0 and debug else l
            res.append((m, code, l))
            if code == 0 and (got != len(data) or o[:len(data)] != data):
                bad.append("%s: valid, decoder %d%s" % (name, got, "" if got < 0 else " (bytes differ)"))
            elif code and got != -code:
                bad.append("%s: oracle %d, decoder %d" % (name, code, got))
    return res, bad


@pytest.mark.parametrize("leg,opts,counts", LEGS, ids=[l[0] for l in LEGS])
def test_mutants_in_device_batches(ctx, leg, opts, counts):
    _setup(ctx)
    c = mz.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        res, bad = _run_all(c)
        assert not bad, "\n".join(bad[:40])
        assert len(res) > 300
    finally:
        c.close()


def test_failure_sites_on_the_default_leg(ctx):
    c = mz.Context(0)
    try:
        c.set_option(OPT_DEBUG_STATUS, 1)
        res, bad = _run_all(c, debug=True)
    finally:
        c.close()
    assert not bad, "\n".join(bad[:40])
    hist = defaultdict(Counter)
    shallow = []
    for m, code, l in res:
        if isinstance(m, str) or code == 0:
            continue
        status = -l
        assert status & 0xFF != 7, "%s: a wait gave up (code 7) on a corrupt block" % m.name
        site = status >> 8
        hist[m.family][site] += 1
        if m.keeps_len and site in (SITE_TOTAL, SITE_OVERRUN):
            shallow.append("%s: site %d" % (m.name, site))
    print("\nfailure sites by family (site: count):")
    for f in sorted(hist):
        print("  %-12s %s" % (f, dict(sorted(hist[f].items()))))
    assert not shallow, "length-preserving corrupt mutants caught by the total / overrun check:\n" + "\n".join(shallow)
    assert sum(hist["retarget"].values()) and sum(hist["repeat"].values())


def test_valid_mutants_alone_get_the_restated_verdict(ctx):
    by_name, muts, verdict = _setup(ctx)
    report = Counter()
    bad = []
    for m in muts:
        if m.claim or m.family not in ("retarget", "shift_len", "repeat") or len(m.block) > (1 << 20):
            continue
        v = m.expected_verdict()
        assert mz.decode_batch([m.block], ctx) == [verdict[m.block][1]], m.name
        got = (ctx.general_blocks(), ctx.general_team())
        if got != (int(v.general), v.team):
            bad.append("%s: (general, team) %s, restated %s" % (m.name, got, v))
        if v.general and not m.base_verdict.general:
            report[m.family] += 1
    print("\nvalid mutants that went general (source conformant):", dict(report))
    assert not bad, "\n".join(bad[:40])
    assert report["retarget"]


# ---- dst_cap and src_len on the host and device entry points ----
def _some(ctx, family=None, valid=True, n=6):
    _, muts, verdict = _setup(ctx)
    out = [m for m in muts if (verdict[m.block][0] == 0) == valid and (not valid or verdict[m.block][1]) and (family is None or m.family == family) and len(m.block) < (2 << 20)]
    return out[::max(1, len(out) // n)][:n]


def test_dst_cap_one_short_and_one_long(ctx):
    _, _, verdict = _setup(ctx)
    ms = _some(ctx)
    blocks = [m.block for m in ms]
    want = [verdict[b][1] for b in blocks]
    lens, outs = _device_batch(ctx, [(b, b"") for b in blocks], [len(w) - 1 for w in want])
    assert lens == [-6] * len(blocks)                                   # -MLZ_ERR_DST_TOO_SMALL; the guard checked nothing past the cap
    lens, outs = _device_batch(ctx, [(b, b"") for b in blocks], [len(w) + 100 for w in want])
    assert lens == [len(w) for w in want] and [o[:len(w)] for o, w in zip(outs, want)] == want
    # host batch
    from minlz_amd import _lib
    L = _lib.lib()
    n = len(blocks)
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in blocks]
    outs = [np.full(len(w) + 64, 0xA5, dtype=np.uint8) for w in want]
    vp, sz = C.c_void_p, C.c_size_t
    ol = (C.c_int64 * n)()
    r = L.mlz_decode_batch(ctx.handle, n, (vp * n)(*[a.ctypes.data for a in arrs]), (sz * n)(*[a.size for a in arrs]),
                           (vp * n)(*[o.ctypes.data for o in outs]), (sz * n)(*[len(w) - 1 for w in want]), ol)
    assert r == 0 and list(ol) == [-6] * n
    assert all((o[len(w) - 1:] == 0xA5).all() for o, w in zip(outs, want))


def _host_batch(ctx, blocks, caps, pinned=False):
    from minlz_amd import _lib
    import torch
    L = _lib.lib()
    n = len(blocks)
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in blocks]
    if pinned:
        bufs = [torch.full((c + 64,), 0xA5, dtype=torch.uint8, pin_memory=True) for c in caps]
        ptrs, views = [t.data_ptr() for t in bufs], [t.numpy() for t in bufs]
    else:
        views = [np.full(c + 64, 0xA5, dtype=np.uint8) for c in caps]
        ptrs = [v.ctypes.data for v in views]
    vp, sz = C.c_void_p, C.c_size_t
    ol = (C.c_int64 * n)()
    r = L.mlz_decode_batch(ctx.handle, n, (vp * n)(*[a.ctypes.data for a in arrs]), (sz * n)(*[a.size for a in arrs]),
                           (vp * n)(*ptrs), (sz * n)(*caps), ol)
    assert r == 0
    for v, c in zip(views, caps):
        assert (v[c:] == 0xA5).all(), "written past dst_cap"
    return list(ol), [v[:max(0, l)].tobytes() for v, l in zip(views, ol)]


@pytest.mark.parametrize("pinned", [False, True])
def test_host_batch_mixed_verdicts(ctx, pinned):
    _, _, verdict = _setup(ctx)
    ms = _some(ctx, n=8) + _some(ctx, valid=False, n=8)
    ms = [ms[i] for i in np.random.default_rng(3).permutation(len(ms))]
    lens, outs = _host_batch(ctx, [m.block for m in ms], [_cap(m.block, verdict) for m in ms], pinned)
    for m, l, o in zip(ms, lens, outs):
        code, data = verdict[m.block]
        assert (l, o) == ((len(data), data) if code == 0 else (-code, b"")), m.name


def test_src_len_respected_after_a_stale_tail(ctx):
    by_name, muts, verdict = _setup(ctx)
    cuts = [m for m in muts if m.family == "cut_append" and "cut_" in m.name and len(m.block) < (2 << 20)][:8]
    assert cuts
    for m in cuts:
        full = _source_of(by_name, m)
        assert mz.decode_batch([full], ctx) == [verdict[full][1]]       # the staging buffer now holds the full block
        lens, outs = _host_batch(ctx, [m.block], [_cap(m.block, verdict)])
        code, data = verdict[m.block]
        assert lens[0] == (len(data) if code == 0 else -code), m.name


def test_single_block_entry_points(ctx):
    _, _, verdict = _setup(ctx)
    for m in _some(ctx, n=6) + _some(ctx, valid=False, n=10):
        code, data = verdict[m.block]
        try:
            got = mz.Decode(m.block, ctx, guard=16)
            assert code == 0 and got == data, m.name
        except mz.MinLZError as e:
            assert e.code == code, (m.name, e.code, code)
        body, dlen = TL.block_body(m.block) if m.block[:1] == b"\x00" and code != O.ERR_TOO_LARGE else (None, 0)
        if body is not None and 0 < dlen <= O.MAX_BLOCK_SIZE:
            e, want = O.decode_body(body, dlen)
            r, got = mz.decode_block(body, dlen, ctx)                         # minLZDecode: 0 / 1
            assert r == e and (e or got == want), m.name


def test_threads_each_get_their_own_verdict(ctx):
    _, _, verdict = _setup(ctx)
    ms = _some(ctx, n=8) + _some(ctx, valid=False, n=8)
    errors = []

    def run(k):
        for j in range(3):
            m = ms[(k + j) % len(ms)]
            code, data = verdict[m.block]
            try:
                got = mz.Decode(m.block, ctx)
                if code != 0 or got != data:
                    errors.append((m.name, 0, code))
            except mz.MinLZError as e:
                if e.code != code:
                    errors.append((m.name, e.code, code))

    th = [threading.Thread(target=run, args=(k,)) for k in range(len(ms))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_two_contexts_on_one_device(ctx):
    _, _, verdict = _setup(ctx)
    ms = _some(ctx, n=6) + _some(ctx, valid=False, n=6)
    c2 = mz.Context(devices=[0, 0])
    try:
        lens, outs = _host_batch(c2, [m.block for m in ms], [_cap(m.block, verdict) for m in ms])
        for m, l, o in zip(ms, lens, outs):
            code, data = verdict[m.block]
            assert (l, o) == ((len(data), data) if code == 0 else (-code, b"")), m.name
    finally:
        c2.close()


# ---- streams ----
def _stream(ctx):
    if "s" not in _CACHE:
        d = synth.text_like(2 << 20, 3).tobytes() + synth.random_bytes((1 << 20) + 300_000, seed=4).tobytes() + synth.json_like(700_000, 5).tobytes()
        _CACHE["s"] = d, mz.stream_encode(d, mz.LevelFastest, 1 << 20, ctx=ctx)
    return _CACHE["s"]


def _code(f):
    try:
        f()
        return 0
    except mz.MinLZError as e:
        return e.code


def test_stream_mutants_exact_code(ctx):
    import io
    d, s = _stream(ctx)
    c2 = mz.Context(devices=[0, 0])
    bad = []
    try:
        for name, b in CM.stream_mutants(s):
            want, data = CM.stream_verdict(b, len(d) + 16)
            got = (_code(lambda: mz.stream_decode(b, ctx=ctx)),
                   _code(lambda: S.Reader(io.BytesIO(b), backend=S.HipBackend(ctx)).WriteTo(io.BytesIO())),
                   _code(lambda: mz.stream_decode(b, ctx=c2)))
            if got != (want,) * 3:
                bad.append("%s: (stream_decode, Reader, two contexts) %s, oracle %d" % (name, got, want))
            elif want == 0:
                assert mz.stream_decode(b, ctx=ctx) == data, name
    finally:
        c2.close()
    assert not bad, "\n".join(bad)


def test_stream_first_error_in_stream_order(ctx):
    # a bad CRC in the first chunk and a cut inside the last: the Reader (and the oracle) report the CRC error
    d, s = _stream(ctx)
    cs = [c for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    b = bytearray(s[:cs[-1].off + 4 + cs[-1].clen // 2])
    b[cs[0].off + 5] ^= 1
    assert CM.stream_verdict(bytes(b), len(d))[0] == O.ERR_CRC
    with pytest.raises(mz.ErrCRC):
        mz.stream_decode(bytes(b), ctx=ctx)
