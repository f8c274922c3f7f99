"""MLZ_SEARCH_IGNORE_CASE without a GPU: tools/stream_search_fold_check.cpp runs the host code the flagged searches share with their kernels
(minlz_amd/csrc/mlz_stream_search.h: the two folds, search_windows_fold, search_pattern_hashes_fold, search_probe_fold with the decoded-set
rule, and the index and the tile rule of the search for many over folded patterns), plain and under the sanitizers, and tests/fold_model.py
says what must come out."""
import re
import struct

import numpy as np
import pytest

import oracle as O
from minlz_amd import api
from tests import fold_model as FM
from tests import search_host as H
from tests import search_model as SMod

SRC = "stream_search_fold_check.cpp"
NO_TABLE = 0xFFFFFFFF
BS, M = 4096, 6
B = SMod.table_bits(BS)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    both = H.checkers(tmp_path_factory, SRC)
    return lambda records: H.both(both, records)


def test_the_flag_is_the_headers_and_the_bindings():
    import os
    text = open(os.path.join(H.ROOT, "include", "minlz_hip.h")).read()
    (value,) = re.findall(r"^#define MLZ_SEARCH_IGNORE_CASE ([^/\n]+)", text, flags=re.M)
    assert eval(re.sub(r"(\d)u\b", r"\1", value)) == 32 == api.IGNORE_CASE                                      # the header's value is the binding's
    assert api.IGNORE_CASE == 32 and api._flags(ignore_case=True) == 32 and api._flags(no_tables=True, invert=True, ignore_case=True) == 8 | 16 | 32
    assert "C.MLZ_SEARCH_IGNORE_CASE" in open(os.path.join(H.ROOT, "go", "minlz_hip.go")).read()


# ---- the folds ----

def test_dword_fold_is_the_byte_fold(checker):
    """All 256 values in each of the four byte positions, between neighbours of 0x00 and of 0xFF: a carry between the bytes would show."""
    line, = checker([struct.pack("<I", 1)])
    words, _, single = line.partition("|")
    words, single = [int(w, 16) for w in words.split()], [int(b, 16) for b in single.split()]
    want = [FM.fold_byte(v) for v in range(256)]
    assert single == want and [v for v in range(256) if want[v] != v] == list(range(0x41, 0x5B))
    assert all(want[v] == v for v in (0x40, 0x5B, 0x60, 0x7B)) and all(want[v] == v for v in range(0x80, 256))
    assert FM.fold(bytes(range(256))) == bytes(want) and FM.fold(np.arange(256, dtype=np.uint8)).tolist() == want
    assert len(words) == 2048
    it = iter(words)
    for pos in range(4):
        for nb in (0x00, 0xFF):
            for v in range(256):
                x = [nb] * 4
                x[pos] = v
                assert next(it) == int.from_bytes(bytes(want[b] if j == pos else b for j, b in enumerate(x)), "little"), (pos, nb, v)


# ---- windows and hashes ----

def rec_windows(cfg, pattern, budget=FM.MAX_HASHES):
    T, M_, field = cfg
    return struct.pack("<IIIIIII", 2, T, M_, B, len(field), len(pattern), budget) + bytes(field) + bytes(pattern)


def parse_windows(line):
    head, _, rest = line.partition(":")
    starts, _, hashes = rest.partition("|")
    nw, gsize, t_min, served, over = (int(v) for v in head.split())
    hs = [None if w == "-" else [int(h) for h in w.split(",")] for w in hashes.split()]
    return dict(nw=nw, gsize=gsize, t_min=t_min, served=bool(served), over=bool(over), starts=[int(v) for v in starts.split()], hashes=hs)


def model_windows(cfg, pattern):
    groups, t_min = FM.windows(pattern, cfg)
    chk = FM.checks(cfg, pattern, B)
    flat = None if chk is None else [w for g in chk[0] for w in g]
    gsize = SMod.parts_of(cfg[2])[1] + 1 if cfg[0] == 4 else 1
    return dict(nw=len(groups), gsize=gsize, t_min=t_min, served=chk is not None, over=False, starts=[i for g in groups for i in g],
                hashes=flat if flat is not None else [])


T2_a = SMod.config(2, M, b"a;")             # holds a, not A
T3_aA = SMod.config(3, M, b"aA;")           # holds both
T4_plain = SMod.config(4, M, b"#47", 1)
T4_letters = SMod.config(4, M, b"id#", 1)
WINDOW_CASES = [
    # (name, cfg, pattern, served, t_min or None)
    ("no letters, type 1", SMod.config(1, M), b"#4711-;99", True, 1),
    ("no letters, type 2", SMod.config(2, M, b"#;"), b";#4711-;99", True, 1),
    ("no letters, type 3", SMod.config(3, M, SMod.NON_ALNUM), b"4#4711-;99", True, 0),
    ("no letters, type 4", T4_plain, b"#4711-;9901", True, 1),
    ("all letters", SMod.config(1, M), b"ErrorLogged", False, 1),
    ("all letters, type 3", SMod.config(3, M, SMod.NON_ALNUM + b"rR"), b"ErrorLogged", False, 0),
    ("the cap exactly", SMod.config(1, M), b"aB1c23", True, 1),
    ("the cap and one more", SMod.config(1, M), b"aB1cD3", False, 1),
    ("a window above the cap in front of two at the cap", SMod.config(1, M), b"xaB1c23y", True, 1),
    ("few letters", SMod.config(1, M), b"K#4711-a", True, 1),
    ("type 2, a without A in front of a window", T2_a, b"1a123456;123456", True, 0),
    ("type 2, only a in front of windows", T2_a, b"1a1234567", False, 0),
    ("type 2, pattern starts with a", T2_a, b"a1;234567", True, 0),
    ("type 3, a and A in front of a window", T3_aA, b"1a1234567", True, 0),
    ("type 3, pattern starts with A", T3_aA, b"A1234567", True, 1),
    ("type 3, pattern starts with ;", T3_aA, b";123456a7654321", True, 1),
    ("type 4, prefix without letters", T4_plain, b"k#4711-a;99", True, 0),
    ("type 4, pattern starts with the prefix", T4_plain, b"#4711-a;990", True, 1),
    ("type 4, two groups", T4_plain, b"#4711-a;9#4722-b;77", True, 1),
    ("type 4, prefix with letters", T4_letters, b"id#4711-a;99", False, 0),
    ("type 4, prefix with letters in another case", T4_letters, b"ID#4711-a;99", False, 0),
    ("shorter than M", SMod.config(1, M), b"#47-a", False, 1),
]


def test_windows_and_hashes_are_the_models(checker):
    lines = checker([rec_windows(cfg, p) for _, cfg, p, _, _ in WINDOW_CASES])
    for (name, cfg, p, served, t_min), line in zip(WINDOW_CASES, lines):
        got, want = parse_windows(line), model_windows(cfg, p)
        assert got == want, (name, got, want)
        assert got["served"] == served and got["t_min"] == t_min, name
        if name.startswith("no letters"):        # exactly the unfolded functions
            if cfg[0] == 4:
                G, tm = SMod.groups(p, cfg)
                K, E, _ = SMod.parts_of(cfg[2])
                starts = [i + K + j for i in G for j in range(E + 1)]
            else:
                starts, tm = SMod.windows(p, cfg)
            assert got["starts"] == starts and got["t_min"] == tm and got["hashes"] == [[h] for g in SMod.checks(cfg, p, B)[0] for h in g], name
    by = {name: parse_windows(line) for (name, *_), line in zip(WINDOW_CASES, lines)}
    assert [len(h) for h in by["the cap exactly"]["hashes"]] == [8] and by["the cap and one more"]["hashes"] == []
    assert [None if h is None else len(h) for h in by["a window above the cap in front of two at the cap"]["hashes"]] == [None, 8, 8]
    assert by["type 2, a without A in front of a window"]["starts"] == [9] and by["type 3, a and A in front of a window"]["starts"] == [2]
    assert by["type 4, two groups"]["nw"] == 2 and by["type 4, two groups"]["gsize"] == 2


def test_hash_budget(checker):
    """A pattern whose variant hashes do not fit leaves nothing behind and says so."""
    p = b"aB1c23-x#4711"                                            # windows of 8, 4, 4, 4, 2, 2, 2, 2 variants
    want = model_windows(SMod.config(1, M), p)
    n = sum(len(h) for h in want["hashes"])
    assert n == 28
    fits, tight, over = (parse_windows(l) for l in checker([rec_windows(SMod.config(1, M), p, b) for b in (FM.MAX_HASHES, n, n - 1)]))
    assert fits == want and tight == want
    assert over == dict(want, served=False, over=True, hashes=[])


# ---- the probe and the decoded set ----

def unit(k):
    return b";%03d#%03d-" % (7 * k % 1000, 13 * k % 1000)


def stream_case(nblk, cfg, needles, tail=123):
    """nblk blocks of 4 KiB, each a repetition of a short unit of digits and punctuation (few distinct windows: small, sparse tables), with
    each needle planted in other cases inside block 1, across the border of blocks 2 and 3 (each side in a different case) and in the last
    block; tables by the model's writer.  -> (data, sizes, tables)"""
    d = bytearray()
    for k in range(nblk):
        d += (unit(k) * (BS // len(unit(k)) + 1))[:BS]
    d += (unit(nblk) * 20)[:tail]
    for j, nd in enumerate(needles):
        half = len(nd) // 2
        d[BS + 100 + 40 * j:BS + 100 + 40 * j + len(nd)] = nd.upper()
        if j == 0:
            d[3 * BS - half:3 * BS - half + len(nd)] = nd[:half].upper() + nd[half:].lower()
        d[len(d) - 20 - 40 * j - len(nd):len(d) - 20 - 40 * j] = nd.swapcase()
    d = bytes(d)
    sp, tables = SMod.splice(O.stream_encode(d, 1, BS), d, cfg, B, stored_too=True)   # (whichever chunk type the encoder chose)
    sizes = [n for n, _ in SMod.data_grid(sp)]
    assert len(sizes) == nblk + 1 and all(t is not None for t in tables)
    return d, sizes, tables


def rec_plan(cfg, sizes, tables, pats, budget=FM.MAX_HASHES):
    T, M_, field = cfg
    out = [struct.pack("<IIIIIIII", 3, T, M_, B, len(field), len(sizes), len(pats), budget), bytes(field), np.asarray(sizes, np.uint64).tobytes()]
    for t in tables:
        out.append(struct.pack("<II", NO_TABLE, 0) if t is None else struct.pack("<II", t[1], len(t[0])) + t[0])
    return b"".join(out) + np.asarray([len(p) for p in pats], np.uint32).tobytes() + b"".join(pats)


def parse_plan(line):
    head, _, rest = line.partition(":")
    served, unserved = (int(v) for v in head.split())
    return served, unserved, [int(v) for v in rest.split()]


FEW = b"k#4711-a"                                                  # at most one letter per window
PLAN_CONFIGS = [
    ("type 1", SMod.config(1, M), [FEW, b";k#4711-a"]),
    ("type 2", SMod.config(2, M, b"#-;"), [b";k#4711-a", b";#4722-b"]),
    ("type 3", SMod.config(3, M, SMod.NON_ALNUM), [b";k#4711-a", b"#k4711-aB-9"]),
    ("type 4", SMod.config(4, M, b"#47", 1), [b"k#4711-a;99", b"#4711-B;9901"]),
]


@pytest.mark.parametrize("name,cfg,needles", PLAN_CONFIGS, ids=[c[0] for c in PLAN_CONFIGS])
@pytest.mark.parametrize("nblk", [6, 10])
def test_decoded_set_is_the_models_and_truthful(checker, name, cfg, needles, nblk):
    d, sizes, tables = stream_case(nblk, cfg, needles)
    everything = [k for k in range(len(sizes)) if sizes[k]]
    absent = [b";z#9911-q;00", b"#47;q-0001x"]
    unserved = [b"ErrorLogged", b"#47-a"]
    singles = needles + [p.upper() for p in needles] + absent + unserved + [b"Logged" + needles[0]]
    lists = [[p] for p in singles] + [needles, needles + absent, absent + unserved[:1], [needles[0], needles[0].upper(), needles[0].swapcase()]]
    lines = checker([rec_plan(cfg, sizes, tables, lst) for lst in lists])
    pruned = 0
    for lst, line in zip(lists, lines):
        want, n_bad = FM.plan_many([tables], sizes, lst, [cfg], [B])
        served, bad, got = parse_plan(line)
        assert (served, bad, got) == (len(lst) - n_bad, n_bad, want), (name, lst)
        for p in lst:                                                # truthful: every chunk that holds the start of a folded occurrence
            occ = FM.search(d, p)
            assert FM.chunks_with_a_start(sizes, occ) <= set(got), (name, p)
            if p in needles:
                assert len(occ) >= 2, (name, p)
        if n_bad:
            assert got == everything
        if len(lst) == 1 and lst[0] in needles and len(got) < len(everything):
            pruned += 1
    for p in unserved:
        assert FM.plan_many([tables], sizes, [p], [cfg], [B])[1] == 1, (name, p)
    # the cap keeps the test honest: a few-letter needle's set is a real selection, by the model alone
    assert pruned >= 1 and len(FM.plan(tables, sizes, needles[0], cfg, B)) < len(everything), name
    assert FM.plan(tables, sizes, needles[0].upper(), cfg, B) == FM.plan(tables, sizes, needles[0], cfg, B)


def test_no_letters_is_the_unfolded_plan(checker):
    for name, cfg, needles in PLAN_CONFIGS:
        d, sizes, tables = stream_case(8, cfg, needles)
        for p in (b";007#091-;0", b"#4711-;9901", unit(3) + unit(3)[:4]):
            assert FM.plan(tables, sizes, p, cfg, B) == SMod.plan(tables, sizes, p, cfg, B), (name, p)
            served, bad, got = parse_plan(checker([rec_plan(cfg, sizes, tables, [p])])[0])
            assert got == SMod.plan(tables, sizes, p, cfg, B) and bad == (0 if SMod.checks(cfg, p, B) else 1), (name, p)


def test_budget_in_a_list(checker):
    """Patterns are taken in order; the one that does not fit is not served, and everything is decoded."""
    name, cfg, needles = PLAN_CONFIGS[0]
    d, sizes, tables = stream_case(6, cfg, needles)
    lst = [FEW, b"aB1c23", FEW]
    n = [FM.n_hashes(FM.checks(cfg, p, B)) for p in lst]
    assert n == [5, 8, 5]
    for budget, bad in ((18, 0), (17, 1), (12, 1), (5, 2), (4, 3)):
        want = FM.plan_many([tables], sizes, lst, [cfg], [B], budget=budget)
        assert want[1] == bad
        served, unserved, got = parse_plan(checker([rec_plan(cfg, sizes, tables, lst, budget)])[0])
        assert (got, unserved) == want, budget


# ---- the search for many ----

def rec_pairs(pats, data, fold):
    return struct.pack("<IIII", 4, len(pats), 1 if fold else 0, len(data)) + np.asarray([len(p) for p in pats], np.uint32).tobytes() + b"".join(pats) + data


def parse_pairs(line):
    head, _, rest = line.partition(":")
    order, _, pairs = rest.partition("|")
    return [int(v) for v in head.split()], [int(v) for v in order.split()], [tuple(int(x) for x in v.split(":")) for v in pairs.split()]


def test_index_and_tile_pairs_folded(checker):
    """Against a plain loop; Ab and aB fold to the same bytes, share a bucket and each count for themselves."""
    rng = np.random.default_rng(5)
    d = bytes(rng.choice(np.frombuffer(b"aAbB@[`{\xc1\xe1", np.uint8), 6000))
    sets = [[b"Ab", b"aB", b"@[", b"`{"], [b"A"], [b"abAB", b"ABab", b"\xc1a", b"\xe1A", b"b"], [b"aBa" * 20, b"bb", b"Bb", b"BB"]]
    lines = checker([rec_pairs(ps, d, True) for ps in sets] + [rec_pairs(ps, d, False) for ps in sets])
    for i, ps in enumerate(sets):
        (m, hb), order, pairs = parse_pairs(lines[i])
        want, counts = FM.search_many(d, ps)
        assert pairs == want and m == min(4, min(len(p) for p in ps)) and sorted(order) == list(range(len(ps))), ps
        assert parse_pairs(lines[len(sets) + i])[2] == sorted((q, j) for j, p in enumerate(ps) for q in SMod.brute(d, p)), ps
    (m, hb), order, pairs = parse_pairs(lines[0])
    assert order.index(1) == order.index(0) + 1                      # one bucket, pattern order
    want, counts = FM.search_many(d, sets[0])
    assert counts[0] == counts[1] > 0 and counts[2] == len(SMod.brute(d, b"@[")) > 0 and counts[3] == len(SMod.brute(d, b"`{")) > 0
    assert FM.search_many(d, [b"\xc1a"])[1] == [len(SMod.brute(d, b"\xc1a")) + len(SMod.brute(d, b"\xc1A"))]   # 0xC1 / 0xE1 do not fold
