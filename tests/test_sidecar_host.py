"""Sidecar search indexes without a GPU: tools/sidecar_check.cpp runs the sidecar rules of the shared header
minlz_amd/csrc/mlz_stream_search.h on the host (the 0x47 writer and parser, the attach validation, the rule over several table sets), and
tests/sidecar_model.py is the same specification in Python, written separately.  The two must agree, and a plan through a sidecar must
hold every chunk with a byte of a true occurrence."""
import ctypes as C
import shutil
import struct

import numpy as np
import pytest

import oracle as O
from minlz_amd import _lib, synth
from minlz_amd.api import search_config
from tests import search_cases as SC
from tests import search_host as H
from tests.search_host import both
from tests import search_model as SMod
from tests import sidecar_model as SM

SRC = "sidecar_check.cpp"
BS = 64 << 10

CFG1 = SMod.config(1, 6)
CFG2 = SMod.config(2, 6, b'":, ')
CFG3 = SMod.config(3, 5, bytes(v for v in range(256) if not chr(v).isalnum()))
CFG4 = SMod.config(4, 6, b'"user":"', 3)


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def test_sanitized_build_links(checkers):
    if checkers[1] is None:
        pytest.skip("this g++ does not link the sanitizer runtimes: " + H.LINK_ERROR[SRC][-300:])
    assert shutil.which("g++")


def test_exported():
    L = _lib.lib()
    names = {"mlz_dev_reader_sidecar_bound", "mlz_dev_reader_build_sidecar", "mlz_dev_reader_attach_sidecar"}
    assert names <= set(_lib.SYMBOLS)
    for n in names:
        assert getattr(L, n)
    assert C.sizeof(_lib.SearchConfig) == 264


def test_python_configuration():
    c = search_config(4, None, b'"user":"', 3)
    assert (c.table_type, c.match_len, c.extras, c.prefix_len, bytes(c.prefix[:8]), c.reserved, bytes(c.reserved2)) == (4, 0, 3, 8, b'"user":"', 0, bytes(2))
    c = search_config(2, 4, b'":, ')
    assert (c.table_type, c.match_len, c.prefix_len, bytes(c.prefix[:4])) == (2, 4, 4, b'":, ')
    c = search_config(3, 6, b"\x00\xff")
    assert c.prefix[0] == 1 and c.prefix[31] == 0x80 and c.prefix_len == 0
    assert search_config(1).table_type == 1
    for args in ((0,), (5,), (1, 9), (1, 6, b"", 1), (2, 6, b""), (2, 6, b"123456789"), (4, 6, b""), (4, 6, b"x" * 257), (4, 6, b"x", 11), (4, 8, b"x", 9)):
        with pytest.raises(ValueError):
            search_config(*args)


# ---- the rule over several table sets ----

def rec_rule(sets, sizes, L):
    out = struct.pack("<IIII", 1, len(sizes), len(sets), L)
    for nw, t_min, ov, a, s in sets:
        out += struct.pack("<III", nw, t_min, ov) + np.asarray(a, np.uint32).tobytes() + np.asarray(s, np.uint32).tobytes()
    return out + np.asarray(sizes, np.uint64).tobytes()


def test_rule_over_several_sets_against_the_model(checkers):
    """400 random (a, s) vectors per number of sets 1 .. 4, sets that cannot vote (nw = 0) among them, and overlaps longer than some chunks."""
    rng = np.random.default_rng(47)
    recs, want = [], []
    for n_sets in (1, 2, 3, 4):
        for _ in range(400):
            nck = int(rng.integers(1, 24))
            L = int(rng.integers(1, 40))
            sizes = [int(v) for v in rng.choice([0, 1, 2, 5, 17, 64, 300], nck)]
            sets, votes = [], []
            for _ in range(n_sets):
                nw = 0 if rng.random() < 0.2 else int(rng.integers(1, 9))
                t_min = int(rng.integers(0, 2))
                hi = max(nw, 1)
                a = [int(v) for v in rng.integers(0, hi + 1, nck)]
                s = [nw if a[k] == nw else int(rng.integers(0, hi)) for k in range(nck)]   # (a probe that finds all says so both ways)
                ov = int(rng.choice([0, 1, 3, 5, 7, 18, 271]))
                sets.append((nw, t_min, ov, a, s))
                if nw:
                    votes.append(SMod.admits(a, s, sizes, nw, L, t_min, ov))
            recs.append(rec_rule(sets, sizes, L))
            want.append(SMod.decoded_set(votes, sizes, L))
    got = both(checkers, recs)
    assert len(got) == len(want)
    for i, line in enumerate(got):
        assert [int(v) for v in line.split()] == want[i], i


# ---- the remote block reference ----

def test_reference_chunk_and_varint_edges(checkers):
    mb = 8 << 20
    pairs = [(0, 0), (127, 0), (128, mb - 1), (1 << 35, 0), (1 << 35, mb - 1), (16383, 16384), ((1 << 36) - 1, 1), (10, 127), (10, 128)]
    lines = both(checkers, [struct.pack("<IQQ", 2, o, m) for o, m in pairs])
    for (o, m), line in zip(pairs, lines):
        assert bytes.fromhex(line) == SM.ref_chunk(o, m), (o, m)
    u = SM.uvarint
    payloads = [
        (u(0) + u(0), mb), (u(127) + u(0), mb), (u(128) + u(mb - 1), mb), (u(1 << 35) + u(0), mb),
        (u(5) + u(1) + u(7) + u(2) + u(1) + u(0), 1 << 16),                    # three references, the later ones relative
        (u(5) + u(1) + u(0) + u(2), 1 << 16),                                  # a relative offset of 0
        (u(5) + u(1 << 16), 1 << 16),                                          # max - actual = max: no bytes
        (u(5) + u((1 << 16) - 1), 1 << 16),                                    # one byte
        (u(1 << 35)[:-1] + b"", mb),                                           # a varint cut short
        (u(1 << 35), mb),                                                      # the size is missing
        (u(5) + b"\x80", mb),                                                  # the size's varint cut short
        (b"", mb),                                                             # an empty payload
        (b"\xff" * 10 + b"\x01" + u(0), mb),                                   # an overflowing varint
        (b"\xff" * 9 + b"\x01" + u(0), mb),                                    # 2^64 - 1: beyond 2^63
        (b"\x80\x00" + u(3), mb),                                              # a padded varint is a varint
    ]
    lines = both(checkers, [struct.pack("<IIQ", 3, len(p), m) + p for p, m in payloads])
    for (p, m), line in zip(payloads, lines):
        want = SM.parse_refs(p, m)
        got = None if line.strip() == "-1" else [tuple(int(x) for x in r.split(":")) for r in line.split()]
        assert got == want, (p.hex(), line)
    assert SM.parse_refs(payloads[4][0], 1 << 16) == [(5, 65535), (12, 65534), (13, 65536)]
    assert [SM.parse_refs(p, m) for p, m in payloads[8:12]] == [None] * 4


# ---- build, attach and plan over whole streams ----

def rec_attach(side, stream, pattern, flags=0):
    return struct.pack("<IQQII", 4, len(side), len(stream), len(pattern), flags) + side + stream + pattern


def parse_line(line):
    if line.strip() == "error":
        return None
    head, _, rest = line.partition(":")
    return tuple(int(v) for v in head.split()), [int(v) for v in rest.split()]


@pytest.fixture(scope="module")
def streams():
    out = {}
    for kind in SC.KINDS:
        data = getattr(synth, kind)(BS * 12, 5).tobytes()
        out[kind] = (data, O.stream_encode(data, 1, BS))
    return out


@pytest.mark.parametrize("kind", SC.KINDS)
def test_spliced_streams_against_the_model(checkers, streams, kind):
    """A sidecar built by the model over a reference-algorithm stream of 12 blocks of 64 KiB, attached and planned by the shared header:
    the same sets as the model's, nothing a true occurrence touches is left out, and two configurations never decode more than one."""
    data, stream = streams[kind]
    sizes = [n for _, n in SM.main_chunks(stream)]
    combos = [[CFG1], [CFG2], [CFG4], [CFG1, CFG2], [CFG1, CFG2, CFG3, CFG4]]
    sides = [SM.build(stream, data, cf) for cf in combos]
    pats = SC.patterns(data, 6, BS) + [("user", b'"user":"abcdefghij'), ("short", b"ab")]
    recs = [rec_attach(side, stream, p) for side in sides for _, p in pats]
    lines = both(checkers, recs)
    plans = {}
    for ci, (cf, side) in enumerate(zip(combos, sides)):
        cfgs, Bs, tables = SM.parse(side, stream)
        assert cfgs == cf and Bs == [16] * len(cf)
        for pi, (name, p) in enumerate(pats):
            got = parse_line(lines[ci * len(pats) + pi])
            want = SM.plan(tables, sizes, p, cfgs, Bs)
            assert got == ((len(cf), SM.usable(tables, [p], cfgs, Bs)), want), (kind, ci, name)
            assert SMod.chunks_touched(sizes, SMod.brute(data, p), len(p)) <= set(want), (kind, ci, name)
            plans[ci, pi] = set(want)
    for pi in range(len(pats)):
        assert plans[3, pi] <= plans[0, pi] and plans[3, pi] <= plans[1, pi]
        assert plans[4, pi] <= plans[3, pi] and plans[4, pi] <= plans[2, pi]
    assert any(len(plans[0, pi]) < len(sizes) for pi in range(len(pats)))   # (the tables do prune)


UNEVEN = [5000, 2, 7000, 1, 3, 9000, 9, 300, 12, 4000]


def test_chunks_shorter_than_the_overlap_hide_nothing(checkers):
    """Chunks of uneven sizes, some shorter than a configuration's overlap: a table in front of such a chunk was built over zeros where its
    windows reach beyond the chunk, so its set abstains there.  Every pattern cut from around every chunk border is found in full by the
    plan of every configuration, alone and together, and the shared header plans what the model plans."""
    user = b'"user":"'
    n = sum(UNEVEN)
    d = bytearray(synth.json_like(n, 11).tobytes())
    ends = np.cumsum(UNEVEN).tolist()
    for at in (5002 + 7000 - 3, ends[5] - 4, ends[7] - 5, 4990):
        d[at:at + 8] = user                                   # the long prefix across borders, once across three chunks
    d = bytes(d)
    stream = SM.framed(d, UNEVEN)
    assert O.stream_decode(stream, n) == d and [m for _, m in SM.main_chunks(stream)] == UNEVEN
    combos = [[CFG1], [CFG2], [CFG3], [CFG4], [CFG1, CFG2, CFG3, CFG4]]
    pats = [d[s:s + L] for e in ends[:-1] for s in range(e - 24, e + 3) for L in (8, 13, 30)] + [d[100:116], user + b"zzzzzzzzzz", b"\x00absent\x00abc"]
    recs, want = [], []
    for cf in combos:
        side = SM.build(stream, d, cf)
        cfgs, Bs, tables = SM.parse(side, stream)
        assert cfgs == cf
        pruned = 0
        for i, p in enumerate(pats):
            plan = SM.plan(tables, UNEVEN, p, cfgs, Bs)
            assert SMod.chunks_touched(UNEVEN, SMod.brute(d, p), len(p)) <= set(plan), (cf, i)
            pruned += len(plan) < len(UNEVEN)
            if i % 7 == 0 or i >= len(pats) - 3:
                recs.append(rec_attach(side, stream, p))
                want.append(((len(cf), SM.usable(tables, [p], cfgs, Bs)), plan))
        assert pruned or len(cf) == 1 and cf[0] != CFG1, cf   # (the tables still prune)
    assert [parse_line(line) for line in both(checkers, recs)] == want


def test_attach_validation_against_the_model(checkers, streams):
    """Lying and broken sidecars: the shared header refuses exactly what the model refuses, and passes over what the model passes over."""
    data, stream = streams["json_like"]
    side, _ = SM.build(stream, data, [CFG1, CFG2], with_tables=True)
    cks = SMod.chunks_of(side)
    refs = [(p, n) for p, t, n in cks if t == SM.CHUNK_REF]
    tabs = [(p, n) for p, t, n in cks if t == SMod.CHUNK_TABLE]
    mb = BS

    def with_ref(i, payload):
        p, n = refs[i]
        return side[:p] + SMod.frame(SM.CHUNK_REF, payload) + side[p + 4 + n:]

    dcs = SM.main_chunks(stream)
    cases = {
        "good": side,
        "offset off by one": with_ref(3, SM.uvarint(dcs[3][0] + 1) + SM.uvarint(0)),
        "size off by one": with_ref(3, SM.uvarint(dcs[3][0]) + SM.uvarint(1)),
        "swapped": with_ref(3, SM.uvarint(dcs[4][0]) + SM.uvarint(0)),
        "empty 0x47": with_ref(3, b""),
        "cut varint": with_ref(3, SM.uvarint(dcs[3][0])[:-1]),
        "two in one": with_ref(3, SM.uvarint(dcs[3][0]) + SM.uvarint(0) + SM.uvarint(dcs[4][0] - dcs[3][0]) + SM.uvarint(0)),   # (then 4 comes again)
        "0x46 for 0x45": side[:tabs[2][0]] + b"\x46" + side[tabs[2][0] + 1:],
        "flipped table bit": side[:tabs[2][0] + 30] + bytes([side[tabs[2][0] + 30] ^ 4]) + side[tabs[2][0] + 31:],
        "first info invalid": side[:10] + b"\x44\x03\x00\x00\x09\x06\x10" + side[17:],
    }
    # a reference chunk with two references, followed by the rest minus the block it swallowed: valid
    p3, n3 = refs[3]
    p4, n4 = refs[4]
    merged = side[:p3] + SMod.frame(SM.CHUNK_REF, SM.uvarint(dcs[3][0]) + SM.uvarint(0) + SM.uvarint(dcs[4][0] - dcs[3][0]) + SM.uvarint(0)) + side[p3 + 4 + n3:p4] + side[p4 + 4 + n4:]
    cases["merged references"] = merged
    pat = data[5 * BS // 3:5 * BS // 3 + 16]
    names = list(cases)
    for flags in (0, 2):
        lines = both(checkers, [rec_attach(cases[k], stream, pat, flags) for k in names])
        for k, line in zip(names, lines):
            try:
                cfgs, Bs, tables = SM.parse(cases[k], stream, ignore_crc=bool(flags))
                want = ((len(cfgs), SM.usable(tables, [pat], cfgs, Bs)), SM.plan(tables, [n for _, n in dcs], pat, cfgs, Bs))
            except SM.SidecarError as e:
                assert e.kind == "corrupt"
                want = None
            assert parse_line(line) == want, (k, flags)
    refused = {k for k in names if _refused(cases[k], stream)}
    assert refused == {"offset off by one", "size off by one", "swapped", "empty 0x47", "cut varint", "two in one"}
    assert mb == SM.max_block_of(SM.identifier(stream))


def _refused(side, stream):
    try:
        SM.parse(side, stream)
        return False
    except SM.SidecarError:
        return True


def test_model_walk_errors():
    """What the walk decides: a truncated sidecar, a missing EOF chunk, a data chunk inside, a second identifier."""
    data = synth.text_like(3 * 4096, 3).tobytes()
    stream = O.stream_encode(data, 1, 4096)
    side = SM.build(stream, data, [CFG1])
    assert O.stream_decode(side, 0) == b""
    for bad, kind in ((side[:-3], "corrupt"), (side[:-5], "corrupt"), (side[:-5] + stream[10:], "corrupt"), (side + side, "unsupported")):
        with pytest.raises(SM.SidecarError) as e:
            SM.parse(bad, stream)
        assert e.value.kind == kind
