"""The block mutator (tests/corrupt.py) pinned on the CPU: every mutant's claim holds against the oracle, the length-preserving families
really preserve the decoded total, every family has valid and corrupt members, and the walker with offsets agrees with TL.walk."""
import io
from collections import Counter

import pytest

import oracle as O
from minlz_amd import api, stream as S, synth
from tests import corrupt as CM
from tests import tile_levels as TL

MIN_PER_FAMILY = 3


def _oracle(block):
    try:
        return 0, O.decode(block)
    except O.OracleError as e:
        return e.code, None


def test_every_claim_holds_against_the_oracle():
    bad = []
    for m in CM.cpu_mutants():
        code, got = _oracle(m.block)
        if code != m.claim:
            bad.append("%s: oracle %d, claimed %d" % (m.name, code, m.claim))
        elif code == 0:
            if got != m.expected_bytes():
                bad.append("%s: bytes differ from the claim" % m.name)
            body, dlen = TL.block_body(m.block)
            if body is not None and TL.verdict(TL.walk(body, dlen), dlen) != m.expected_verdict():
                bad.append("%s: verdict differs from the claim" % m.name)
    assert not bad, "\n".join(bad[:40])


def test_length_preserving_mutants_keep_the_total():
    n = Counter()
    for m in CM.cpu_mutants():
        if not m.keeps_len:
            continue
        body, dlen = TL.block_body(m.block)
        if body is None:
            continue
        total = 0
        for t in TL.walk_tokens(body):           # framing intact: only offsets (or nothing) are wrong
            total = t.dpos + len(t.lit) + t.cp
        assert total == dlen, m.name
        n[m.claim != 0] += 1
    assert n[True] >= 10 and n[False] >= 10      # corrupt ones only a check deeper than the total can catch


def test_every_family_has_valid_and_corrupt_members():
    per = Counter((m.family, m.claim == 0) for m in CM.cpu_mutants())
    for f in CM.FAMILIES:
        assert per[(f, True)] >= MIN_PER_FAMILY and per[(f, False)] >= MIN_PER_FAMILY, (f, per[(f, True)], per[(f, False)])


def test_retargets_cover_the_sources_asked_for():
    tags = {m.name.split("/")[-1].split("@")[0] for m in CM.cpu_mutants() if m.family == "retarget"}
    assert {"same_tile", "prev_tile", "straddle", "forbidden_tile", "byte0", "before_start_1", "before_start_large"} <= tags
    went_general = [m for m in CM.cpu_mutants() if m.family == "retarget" and m.claim == 0 and not m.base_verdict.general
                    and m.expected_verdict().general]
    assert went_general                          # a retarget that breaks conformance: the block must go general


def test_mutants_are_deterministic():
    a = CM.mutants_of(CM.cpu_sources()[:3])
    b = CM.mutants_of(CM.cpu_sources()[:3])
    assert [(m.name, m.block) for m in a] == [(m.name, m.block) for m in b]


@pytest.mark.parametrize("level", [1, 2, 3])
def test_walker_with_offsets_agrees_with_walk(level):
    src = synth.text_like(200_000, seed=level).tobytes()
    body, dlen = TL.block_body(O.encode(src, level))
    toks = list(TL.walk_tokens(body))
    assert [(t.dpos, t.lit, t.off, t.cp) for t in toks] == list(TL.walk(body, dlen))
    # each token's bytes re-emitted from its fields are the stream's own bytes, and the tokens tile the stream
    ends = [t.spos for t in toks[1:]] + [len(body)]
    forms = Counter()
    for t, e in zip(toks, ends):
        forms[t.form] += 1
        assert t.spos + t.hlen + len(t.lit) == e
        if t.form == "literal":
            assert body[t.spos:e] == O.emit_literal(t.lit)
        elif t.form == "repeat":
            assert body[t.spos:e] == O.emit_repeat(t.cp)
        elif t.form == "copy2_lits":
            assert body[t.spos:e] == O.emit_copy_lits2(t.lit, t.off, t.cp)
        elif t.form == "copy3" and t.lit:
            assert body[t.spos:e] == O.emit_copy_lits3(t.lit, t.off, t.cp)
    assert forms["literal"] and forms["copy2"] and (forms["copy1"] or level == 1)


# ---- streams: the Reader mirror over an oracle backend must give the oracle's exact code ----
class _OracleBackend:
    def decode_bodies(self, bodies):
        res = []
        for b in bodies:
            try:
                res.append(O.decode(b"\x00" + b))
            except O.OracleError as e:
                raise api._ERRS[e.code]()
        return res

    def crcs(self, blocks):
        return [O.crc(b) for b in blocks]


def _reader_code(s):
    try:
        S.Reader(io.BytesIO(s), backend=_OracleBackend()).WriteTo(io.BytesIO())
        return 0
    except api.MinLZError as e:
        return e.code


def _test_stream():
    d = synth.text_like(2 << 20, 3).tobytes() + synth.random_bytes((1 << 20) + 300_000, seed=4).tobytes() + synth.json_like(700_000, 5).tobytes()
    return d, O.stream_encode(d, 1, 1 << 20)


def test_stream_mutants_reader_mirror_gives_the_oracles_code():
    d, s = _test_stream()
    codes = Counter()
    bad = []
    for name, b in CM.stream_mutants(s):
        want, _ = CM.stream_verdict(b, len(d) + 16)
        got = _reader_code(b)
        codes[want] += 1
        if got != want:
            bad.append("%s: reader %d, oracle %d" % (name, got, want))
    assert not bad, "\n".join(bad)
    assert codes[O.ERR_CRC] and codes[O.ERR_CORRUPT] and codes[O.ERR_TOO_LARGE] and codes[O.ERR_UNSUPPORTED] and codes[0]


def test_stream_order_first_error_wins():
    # an early chunk with a bad CRC and a cut inside the last chunk: the Reader reports the CRC error, the first in stream order
    d, s = _test_stream()
    cs = [c for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    b = bytearray(s[:cs[-1].off + 4 + cs[-1].clen // 2])
    b[cs[0].off + 5] ^= 1
    assert CM.stream_verdict(bytes(b), len(d))[0] == O.ERR_CRC
    assert _reader_code(bytes(b)) == api.ErrCRC.code


def test_stream_prefix_len_is_host_only():
    # mlz_stream_decoded_prefix_len: the decoded bytes of the chunks in front of the first framing error (all of them when none)
    import numpy as np
    from minlz_amd import _lib
    L = _lib.lib()
    d, s = _test_stream()
    cs = [c for c in CM.chunks(s) if c.type in (0x01, 0x02, 0x03)]
    n = [O.decoded_len(b"\x00" + s[c.off + 8:c.off + 4 + c.clen]) if c.type == 0x02 else c.clen - 4 for c in cs]

    def host_lens(b):
        a = np.frombuffer(b, dtype=np.uint8)
        return L.mlz_stream_decoded_len(a.ctypes.data, a.size), L.mlz_stream_decoded_prefix_len(a.ctypes.data, a.size)

    assert host_lens(s) == (len(d), len(d))
    assert host_lens(s[:cs[-1].off + 7]) == (-O.ERR_CORRUPT, sum(n[:-1]))
    assert host_lens(s[:cs[2].off]) == (-O.ERR_CORRUPT, sum(n[:2]))
    b = bytearray(s); b[cs[1].off] = 0x00
    assert host_lens(bytes(b)) == (-O.ERR_UNSUPPORTED, n[0])
    assert host_lens(s[:5]) == (-O.ERR_CORRUPT, 0)
    # a stored chunk over the block size in a cut stream: ErrTooLarge, as the oracle says (the size is checked before the bytes are read)
    name, b = next(x for x in CM.stream_mutants(s) if x[0] == "uncompressed_too_large_cut")
    assert CM.stream_verdict(b, len(d))[0] == O.ERR_TOO_LARGE
    assert host_lens(b)[0] == -O.ERR_TOO_LARGE
