"""mlz_stream_encode_batch_device_tables without a GPU: the pre-fold rule against its model (tests/search_prefold_model.py) and the model
against search_model.build_table, the bound, the header and its binding, and tools/search_prefold_check.cpp, which holds the rule of
minlz_amd/csrc/mlz_stream_search.h against build-then-fold, plain and under the sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import oracle as O
from minlz_amd import _lib, api
from tests import search_host as H
from tests import search_model as SMod
from tests import search_prefold_model as PF

SRC = "search_prefold_check.cpp"
HEADER = "minlz_hip_encode_batch_tables.h"
NAMES = ["mlz_stream_bound_config", "mlz_search_table_prefold", "mlz_stream_encode_batch_device_tables"]
MLZ_ERR_ARG = 8
ADD_INDEX, SEARCH_TABLES, COMPRESS = 1, 4, 64


@pytest.fixture(scope="module")
def cases():
    """The grid, each case with search_model.build_table's (table, R): made once for the tests below."""
    return [(cfg, B, block, follow) + SMod.build_table(cfg, block, follow, B) for cfg, B, block, follow in PF.grid()]


def test_the_library_rule_is_the_models(cases):
    """mlz_search_table_prefold over every (marks, B, type) of the grid, and around every threshold of every table size."""
    f = _lib.lib().mlz_search_table_prefold
    seen = set()
    for cfg, B, block, follow, _, _ in cases:
        seen.add((PF.marks(cfg, len(block), follow), B, cfg[0]))
    for B in range(8, 24):
        for T in (1, 2, 3, 4):
            for r in range(0, B - 7):
                edge = (1 << (B - r)) * SMod.fold_limit(T) // 100
                seen.update((m, B, T) for m in (edge - 1, edge, edge + 1) if m >= 0)
            seen.update(((0, B, T), (1 << B, B, T)))
    assert len(seen) > 1500
    for m, B, T in sorted(seen):
        assert f(m, B, T) == PF.prefold(m, B, SMod.fold_limit(T)), (m, B, T)
    assert f(0, 20, 1) == 12 and f(4096 - 5, 20, 1) == 6 and f(4096, 20, 2) == 4 and f(1 << 20, 20, 1) == 0     # (4 KiB at 1 MiB blocks: 2 KiB, not 128 KiB)
    for bad in ((0, 7, 1), (0, 24, 1), (0, 20, 0), (0, 20, 5), ((1 << 32) + 1, 20, 1)):
        assert f(*bad) == -MLZ_ERR_ARG, bad


def test_the_prefolded_build_is_build_table(cases):
    """The model's identity over the whole grid: the same (table, R), and the grid reaches what it is there for."""
    n = folded = long_marked = 0
    for cfg, B, block, follow, want_tab, want_R in cases:
        tab, R, r0 = PF.build_prefolded(cfg, block, follow, B)
        assert (tab, R) == (want_tab, want_R), (cfg[:2], B, len(block), follow if follow is None else len(follow))
        n += 1
        folded += r0 > 0
        long_marked += cfg[0] == 4 and tab is not None and any(tab)
        assert tab is None or R >= r0
    assert n == 5184 and 4000 < folded < n and long_marked > 0


def _cfg(T, M, prefix=b"", extras=0, reserved=0, reserved2=0, prefix_len=None):
    c = _lib.SearchConfig()
    c.table_type, c.match_len, c.extras, c.reserved = T, M, extras, reserved
    c.reserved2[1] = reserved2
    pfx = bytes(prefix)
    if T == 3:
        for v in pfx:
            c.prefix[v >> 3] |= 1 << (v & 7)
    else:
        for i, v in enumerate(pfx[:256]):
            c.prefix[i] = v
    c.prefix_len = len(pfx) if prefix_len is None else prefix_len
    return c


def test_the_bound_is_the_single_writers():
    L = _lib.lib()
    bound = L.mlz_stream_bound_config
    for n in (0, 1, 4096, 100_000, 5 << 20):
        for bs in (4 << 10, 64 << 10, 1 << 20, 4 << 20):
            for flags in (0, ADD_INDEX):
                assert bound(n, bs, flags, None) == L.mlz_stream_bound(n, bs, flags)
                for M in (0, 1, 6, 8):
                    assert bound(n, bs, flags, C.byref(_cfg(1, M))) == L.mlz_stream_bound(n, bs, flags | SEARCH_TABLES | M << 8)
                    t = api.search_tables_config(M, b'":, ')
                    assert t.table_type == 2 and bound(n, bs, flags, C.byref(_cfg(2, M, b' ",:'))) == L.mlz_stream_bound_tables(n, bs, flags, C.byref(t))
                    t = api.search_tables_config(M, SMod.NON_ALNUM)
                    assert t.table_type == 3 and bound(n, bs, flags, C.byref(_cfg(3, M, SMod.NON_ALNUM))) == L.mlz_stream_bound_tables(n, bs, flags, C.byref(t))
                    lp = api.search_long_prefix_config(M, b'"user":"', 3)
                    assert bound(n, bs, flags, C.byref(_cfg(4, M, b'"user":"', 3))) == L.mlz_stream_bound_long_prefix(n, bs, flags, C.byref(lp))
    n, bs = 100_000, 64 << 10
    assert bound(n, bs, 0, C.byref(_cfg(1, 6))) > L.mlz_stream_bound(n, bs, 0) > 0
    # what the three refuse
    refused = [(_cfg(0, 6), 0), (_cfg(5, 6), 0), (_cfg(1, 9), 0), (_cfg(2, 6, b""), 0), (_cfg(2, 6, b"123456789"), 0), (_cfg(4, 6, b""), 0), (_cfg(4, 6, b"x", prefix_len=257), 0),
               (_cfg(4, 8, b"x", 9), 0), (_cfg(4, 1, b"x", 16), 0), (_cfg(1, 6, extras=1), 0), (_cfg(1, 6, reserved=1), 0), (_cfg(3, 6, b"x", reserved2=1), 0),
               (_cfg(1, 6), SEARCH_TABLES), (_cfg(2, 6, b'"'), 6 << 8)]
    for cfg, flags in refused:
        assert bound(n, bs, flags, C.byref(cfg)) == -MLZ_ERR_ARG, (cfg.table_type, cfg.match_len, flags)
    assert bound(n, 1000, 0, C.byref(_cfg(1, 6))) == -MLZ_ERR_ARG and bound(n, 1000, 0, None) == -MLZ_ERR_ARG
    assert bound(n, bs, 9 << 8 | SEARCH_TABLES, None) == L.mlz_stream_bound(n, bs, 9 << 8 | SEARCH_TABLES) == -MLZ_ERR_ARG


def test_the_keywords_choose_the_gather_writers_configuration():
    """api.batch_tables_config: the table type by the gather Writer's rule, the values sorted, and a bound equal to api.stream_bound's."""
    assert api.batch_tables_config() is None
    for kw in (dict(search_match_len=0), dict(search_match_len=4), dict(search_match_len=6, search_prefix=b',":'), dict(search_match_len=6, search_prefix=SMod.NON_ALNUM),
               dict(search_match_len=6, search_prefix=b""), dict(search_match_len=5, search_long_prefix=b'"user":"', search_extras=3)):
        c = api.batch_tables_config(**kw)
        want = 4 if "search_long_prefix" in kw else 1 if "search_prefix" not in kw else 2 if 1 <= len(set(kw["search_prefix"])) <= 8 else 3
        assert c.table_type == want and c.match_len == kw["search_match_len"]
        if want == 2:
            assert bytes(c.prefix[:c.prefix_len]) == bytes(sorted(set(kw["search_prefix"])))
        for idx in (False, True):
            assert _lib.lib().mlz_stream_bound_config(300_000, 64 << 10, int(idx), C.byref(c)) == api.stream_bound(300_000, 64 << 10, idx, **kw)
    with pytest.raises(ValueError):
        api.batch_tables_config(search_prefix=b'"')
    with pytest.raises(ValueError):
        api.batch_tables_config(search_match_len=6, search_extras=2)


def test_exported(tmp_path):
    """The library exports the three symbols; the header declares them and nothing else, in the order of _lib.ABI_EXT's entry and with as many
    parameters as the entry has argument types; a C99 client compiles against it, and its host-only calls and a refused call answer without a GPU."""
    L = _lib.lib()
    for name in NAMES:
        assert getattr(L, name)
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert len(argtypes) == params.count(",") + 1 and name not in _lib.ABI, name
        assert restype is (_lib.i32 if name == NAMES[2] else _lib.i64)
    assert [len(_lib.ABI_EXT[HEADER][n][1]) for n in NAMES] == [4, 3, 11]
    src = tmp_path / "client.c"
    src.write_text('#include "%s"\n'
                   "int main(void) {\n"
                   "    mlz_search_config c = {1, 6, 0, 0, 0, {0, 0}, {0}};\n"
                   "    if (mlz_stream_bound_config(100000, 65536, 0, &c) <= mlz_stream_bound(100000, 65536, 0)) return 1;\n"
                   "    if (mlz_search_table_prefold(4091, 20, 1) != 6) return 2;\n"
                   "    if (mlz_stream_encode_batch_device_tables(0, 0, 1, 65536, 0, &c, 0, 0, 0, 0, 0) != -MLZ_ERR_ARG) return 3;\n"
                   "    return 0;\n"
                   "}\n" % HEADER)
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0


# ---- tools/search_prefold_check.cpp ----

@pytest.fixture(scope="module")
def records(cases):
    """A part of the grid (every configuration, table size and following form; three or four lengths per table size) as the tool's records,
    and what the model says of each: (r0, R, table bytes, the table's CRC)."""
    recs, want = [], []
    for cfg, B, block, follow, tab, R in cases:
        if len(block) not in (7, 100, 4096 if B == 12 else 4097, 16385):
            continue
        T, M, field = cfg
        recs.append(struct.pack("<IIIIII", T, M, B, len(block), 0xFFFFFFFF if follow is None else len(follow), len(field)) + field + block + (follow or b""))
        r0 = PF.prefold(PF.marks(cfg, len(block), follow), B, SMod.fold_limit(T))
        want.append("%d %d %d %d" % ((r0, 0, 0, 0) if tab is None else (r0, R, len(tab), O.crc(tab))))
    return recs, want


def _check(lines, want):
    head = lines[0].split()
    assert head[0] == "self" and int(head[1]) > 5000          # the program's own designed and pseudo-random blocks
    assert len(want) > 1000 and lines[1:] == want


def test_the_shared_rule_builds_what_the_model_builds(tmp_path_factory, records):
    run = H.build_checker(tmp_path_factory, SRC)
    _check(run(records[0])[0], records[1])


def test_the_shared_rule_under_the_sanitizers(tmp_path_factory, records):
    """The check tool as a stand-alone program under AddressSanitizer and UBSan: no mark leaves a pre-folded table."""
    run = H.build_checker(tmp_path_factory, SRC, sanitized=True, flags=("-static-libasan", "-static-libubsan"))
    assert run is not None, H.LINK_ERROR[SRC]
    lines, err = run(records[0])
    assert "ERROR" not in err and "runtime error" not in err, err[-2000:]
    _check(lines, records[1])
