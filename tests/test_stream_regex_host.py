"""Regular expressions in the grep over the record index without a GPU (include/minlz_hip_regex.h): the compiler (minlz_amd/csrc/mlz_regex_compile.h)
and the rules the call shares with its kernels (minlz_amd/csrc/mlz_stream_regex.h: the walk byte by byte and in 16-byte blocks, the group rule, the
mark layout, the longest record), run as plain loops by tools/stream_regex_check.cpp, plain and under AddressSanitizer and UBSan, and through
ctypes; tests/regex_model.py (Python's own `re` on the bytes) says what must come out."""
import itertools
import os
import re
import struct
import subprocess
import time

import numpy as np
import pytest

from minlz_amd import _lib, api
from tests import grep_model as GM
from tests import regex_model as RM
from tests import search_host as H

SRC = "stream_regex_check.cpp"
HEADER = "minlz_hip_regex.h"
NAMES = ["mlz_regex_compile", "mlz_regex_free", "mlz_regex_info", "mlz_regex_test", "mlz_dev_reader_grep_regex"]
ARG, UNSUPPORTED = api.ERR_ARG, api.ERR_UNSUPPORTED


def test_exported(tmp_path):
    """The library exports the symbols; include/minlz_hip_regex.h declares exactly the entries of _lib.ABI_EXT under its name, each with as many
    parameters as the entry has argument types, and minlz_hip.h declares none of them; the header compiles as C99 on its own (it includes
    minlz_hip.h); a client without a device compiles an expression, reads its info, tests two records and gets -MLZ_ERR_ARG for NULLs."""
    L = _lib.lib()
    inc = os.path.join(H.ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    protos = re.findall(r"\b(mlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)
    assert [name for name, _ in protos] == list(_lib.ABI_EXT[HEADER]) == NAMES
    for name, params in protos:
        restype, argtypes = _lib.ABI_EXT[HEADER][name]
        assert getattr(L, name) and len(argtypes) == params.count(",") + 1 and name not in _lib.ABI
        assert restype is {"mlz_regex_free": None, "mlz_dev_reader_grep_regex": _lib.i64}.get(name, _lib.i32)
    main_h = open(os.path.join(inc, "minlz_hip.h")).read()
    assert HEADER in main_h and not any(re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", main_h, flags=re.S)) for n in NAMES)
    defines = dict(re.findall(r"#define (MLZ_REGEX_[A-Z_]+) (\d+)u", open(os.path.join(inc, HEADER)).read()))
    assert defines == {"MLZ_REGEX_IGNORE_CASE": str(api.REGEX_IGNORE_CASE), "MLZ_REGEX_MAX_RECORD": str(api.REGEX_MAX_RECORD)}
    src = tmp_path / "client.c"
    src.write_text("""#include "%s"
int main(void) {
    mlz_regex* re = 0;
    uint64_t where[2], info[4];
    const uint8_t expr[] = "^a+b$", bad[] = "a**";
    const uint32_t len = 5, bad_len = 3;
    if (mlz_regex_compile(0, 0, 0, 0, 0, 0) != -MLZ_ERR_ARG) return 1;
    if (mlz_regex_compile(0, 0, 0, 0, &re, where) != -MLZ_ERR_ARG || re) return 2;
    if (mlz_regex_compile(bad, &bad_len, 1, 0, &re, where) != -MLZ_ERR_ARG || re || where[0] != 0 || where[1] != 2) return 3;
    if (mlz_regex_compile(expr, &len, 1, 2, &re, 0) != -MLZ_ERR_ARG || re) return 4;
    if (mlz_regex_info(0, info) != -MLZ_ERR_ARG || mlz_regex_test(0, expr, 1) != -MLZ_ERR_ARG) return 5;
    if (mlz_dev_reader_grep_regex(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != -MLZ_ERR_ARG) return 6;
    if (mlz_regex_compile(expr, &len, 1, MLZ_REGEX_IGNORE_CASE, &re, where) != 0 || !re) return 7;
    if (mlz_regex_info(re, 0) != -MLZ_ERR_ARG || mlz_regex_info(re, info) != 0 || info[0] < 3 || info[1] < 2 || info[2] > 65536 || info[3] != 0) return 8;
    if (mlz_regex_test(re, (const uint8_t*)"AAb", 3) != 1 || mlz_regex_test(re, (const uint8_t*)"aabb", 4) != 0 || mlz_regex_test(re, 0, 0) != 0) return 9;
    if (mlz_dev_reader_grep_regex(0, 0, 0, re, 0, 0, 0, 0, 0, 0, 0) != -MLZ_ERR_ARG) return 10;
    mlz_regex_free(re);
    mlz_regex_free(0);
    return 0;
}
""" % HEADER)
    so_dir = os.path.dirname(_lib.SO)
    exe = str(tmp_path / "client")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe, "-L", so_dir, "-lminlz_hip", "-Wl,-rpath," + so_dir])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=300).returncode == 0          # (nothing here touches a device)


# ---- the case file of tools/stream_regex_check.cpp ----

def as_list(exprs):
    return [exprs] if isinstance(exprs, bytes) else list(exprs)


def rec_set(exprs, flags):
    exprs = as_list(exprs)
    return struct.pack("<II", flags, len(exprs)) + b"".join(struct.pack("<I", len(e)) for e in exprs) + b"".join(exprs)


def rec_strings(exprs, flags, alphabet, listed):
    return (struct.pack("<I", 1) + rec_set(exprs, flags) + struct.pack("<I", 1 if alphabet else 0) + (alphabet or bytes(4)) + struct.pack("<I", len(listed)) +
            b"".join(struct.pack("<I", len(s)) + s for s in listed))


def rec_groups(exprs, flags, delim, data, cuts):
    return struct.pack("<I", 2) + rec_set(exprs, flags) + struct.pack("<IQ", delim, len(data)) + data + struct.pack("<I", len(cuts)) + np.asarray(cuts, np.uint64).tobytes()


def over(alphabet):
    """Every string of length 0 .. 6 over the four bytes, in the checker's order: 5461 of them."""
    return [bytes(alphabet[i] for i in t) for n in range(7) for t in itertools.product(range(4), repeat=n)]


# (expression or expressions, an alphabet of four bytes: those the expression's sets begin and end at, and one >= 0x80)
TABLE = [
    (b"abc", b"abc\x80"), (b"a.c", b"ac\n\x80"), (b"", b"ab\n\x80"), (b"a|", b"ab\n\x80"), (b"()", b"ab\n\x80"), (b"(?:)a", b"ab\n\x80"),
    # nested groups, alternation under * and +
    (b"(a|b)*c", b"abc\x80"), (b"((a|b)*c|ca)*b$", b"abc\x80"), (b"(?:(ab|a)(c|bc))+$", b"abc\xff"), (b"^(a(b|c)*)*$", b"abc\x80"), (b"(a*)*b", b"abc\x80"),
    (b"^(a*)+$", b"ab\n\x80"), (b"(a|b|)*c", b"abc\x80"), (b"(|a)+b$", b"abc\x80"), (b"((((a))))b", b"abc\x80"), (b"(a|ab)(c|bc)(c*)$", b"abc\x80"),
    # counted repetition
    (b"a{0}b", b"abc\x80"), (b"^a{0,0}b$", b"abc\x80"), (b"a{1,1}b", b"abc\x80"), (b"^a{2,}$", b"ab\n\x80"), (b"^a{0,255}$", b"ab\n\x80"), (b"a{2}", b"ab\n\x80"),
    (b"^(ab){2,3}$", b"abc\x80"), (b"a{1,3}b{2}c?", b"abc\x80"), (b"x{0,2}y{3,}", b"xyz\x80"), (b"(a{2}){2}b", b"abc\x80"), (b"(^a|b){2}$", b"abc\x80"),
    (b"a+b", b"abc\x80"), (b"a*b", b"abc\x80"), (b"a?b", b"abc\x80"), (b"^a?$", b"ab\n\x80"), (b"^x*$", b"xy\n\x80"),
    # classes: ranges, escapes, negation
    (b"[b-c]d", b"abc\x80"), (b"[b-c]+$", b"abc\x80"), (b"[^b-c]", b"abc\x80"), (b"[^a]b", b"aAb\x80"), (b"[Z-a]", b"Zaz\x80"), (b"[^Z-a]$", b"Zaz\x80"),
    (b"[\\d]x|\\D$", b"09x\x80"), (b"\\d+\\.\\d", b"09.\x80"), (b"\\w+", b"_ z\x80"), (b"^\\W+$", b"_ z\x80"), (b"\\s\\S", b" \tz\x80"), (b"[\\s\\d]{2}", b" 9z\x80"),
    (b"[^\\s\\d]{2}", b" 9z\x80"), (b"[^\\W]\\S", b"a _\x80"), (b"[\\]\\^-]", b"]^-\x80"), (b"[-a]", b"-ab\x80"), (b"[a-]$", b"-ab\x80"), (b"[+-\\-]", b"+,-\x80"),
    (b"[\\x80-\\xff]", b"\x7f\x80\xff\x00"), (b"\\x00\\0", b"\x00\x01a\x80"), (b"[a-c]x", b"AaC\x80"), (b"[.|*]", b".|*\x80"), (b"[\\n-\\r]", b"\t\n\r\x80"),
    # escapes
    (b"\\.\\*", b".*a\x80"), (b"\\(\\)", b"()a\x80"), (b"\\{\\}", b"{}a\x80"), (b"\\^\\$", b"^$a\x80"), (b"\\\\\\/", b"\\/a\x80"), (b'\\"\\-', b'"-a\x80'),
    (b"\\n\\r|\\t\\f\\v", b"\n\r\t\x80"), (b"\\+\\?\\|", b"+?|\x80"), (b"\\[\\]", b"[]a\x80"), (b"\\x41b", b"Aab\x80"), (b"Ab", b"aAb\x80"),
    # ^ and $, also inside alternations and where they can never hold
    (b"^a", b"ab\n\x80"), (b"a$", b"ab\n\x80"), (b"^$", b"ab\n\x80"), (b"(a|^b)c$", b"abc\x80"), (b"^a|b$", b"abc\x80"), (b"(^|a)b", b"abc\x80"), (b"a($|b)", b"abc\x80"),
    (b"a^", b"ab\n\x80"), (b"$a", b"ab\n\x80"), (b"$^", b"ab\n\x80"), (b"^^a$$", b"ab\n\x80"), (b"(^a|b$)+", b"ab\n\x80"), (b"^(a|b)$|^$", b"abc\x80"), (b"(^)*a", b"abc\x80"),
    (b"($)?a", b"abc\x80"), (b"^.$", b"a\n\x80\x00"), (b"a.*z", b"az\n\x80"), (b".{3}$", b"a\n\x80\x00"), (b"(a|^b)c$|d", b"abcd"),
    # several expressions in one compile
    ((b"a", b"^b$"), b"ab\n\x80"), ((b"ab", b""), b"ab\n\x80"), ((b"^a", b"b$", b"c{2}"), b"abc\x80"), ((b"a{3}", b"^[^a]$", b"b\\x80"), b"ab\n\x80"),
]
assert len(TABLE) >= 60 and all(len(a) == 4 for _, a in TABLE)


def random_strings(alphabet, seed):
    """2000 strings of up to 64 bytes, nine bytes in ten from the alphabet."""
    rng = np.random.default_rng(seed)
    out = []
    for n in rng.integers(0, 65, 2000):
        s = np.frombuffer(alphabet, np.uint8)[rng.integers(0, 4, n)].copy()
        other = rng.random(n) < 0.1
        s[other] = rng.integers(0, 256, int(other.sum()))
        out.append(s.tobytes())
    return out


@pytest.fixture(scope="module")
def table_cases():
    """-> (records, notes, wanted verdict strings): every table expression with and without MLZ_REGEX_IGNORE_CASE."""
    recs, notes, want = [], [], []
    for i, (exprs, alphabet) in enumerate(TABLE):
        listed = random_strings(alphabet, 1000 + i)
        strings = over(alphabet) + listed
        assert len(strings) == 5461 + 2000
        for fold in (0, 1):
            p = RM.pattern(exprs, bool(fold))
            recs.append(rec_strings(exprs, fold, alphabet, listed))
            notes.append((exprs, fold))
            want.append("".join("1" if p.search(s) else "0" for s in strings))
    return recs, notes, want


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    return H.checkers(tmp_path_factory, SRC)


def test_table_against_re(checkers, table_cases):
    """The compiler's automaton, walked byte by byte and in 16-byte blocks at four misalignments, equals Python's `re` on every string of length 0 .. 6
    over each expression's alphabet and on 2000 random strings of up to 64 bytes; plain and under AddressSanitizer and UBSan (the stand-alone
    program, nothing preloaded), which must print the same."""
    recs, notes, want = table_cases
    lines = H.both(checkers, recs)
    assert checkers[1] is not None, H.LINK_ERROR.get(SRC)
    assert len(lines) == len(want) == 2 * len(TABLE)
    matched_some = 0
    for line, w, note in zip(lines, want, notes):
        head, _, bits = line.partition(" : ")
        assert head.startswith("ok "), (note, line[:80])
        if bits != w:
            strings = over(TABLE[notes.index(note) // 2][1])
            wrong = [i for i in range(len(w)) if bits[i:i + 1] != w[i]]
            pytest.fail("%r: %d verdicts differ from re, the first on %r" % (note, len(wrong), strings[wrong[0]] if wrong[0] < len(strings) else wrong[0]))
        S, C, image, empty = (int(v) for v in head.split()[1:])
        assert 2 <= S and 1 <= C <= 256 and image <= 64 << 10 and empty == int(w[0])       # (the first string is the empty one)
        matched_some += "1" in w and "0" in w
    assert matched_some > len(want) * 0.8                                                   # the table tells expressions apart


def test_ctypes_equals_the_model(table_cases):
    """api.Regex.test (mlz_regex_test) on a few hundred of the same strings, and info() against the checker's own line."""
    _, notes, want = table_cases
    rng = np.random.default_rng(5)
    checked = 0
    for k in range(0, len(notes), 7):
        exprs, fold = notes[k]
        alphabet = TABLE[k // 2][1]
        strings = over(alphabet) + random_strings(alphabet, 1000 + k // 2)
        with api.Regex(exprs, ignore_case=bool(fold)) as rx:
            S, C, image, empty = rx.info()
            assert empty == (want[k][0] == "1") and image >= 256 + 2 * S * C and image % 16 == 0
            for i in [0, 1, 5] + [int(v) for v in rng.integers(0, len(strings), 12)]:
                assert rx.test(strings[i]) == (want[k][i] == "1"), (exprs, fold, strings[i])
                checked += 1
    assert checked >= 300
    rx = api.Regex(b"a")
    rx.close()
    rx.close()
    with pytest.raises(ValueError, match="^Regex is closed$"):
        rx.test(b"a")


def test_ignore_case_is_re_ignorecase():
    """The three observations of the contract: under re.I, [^a] does not match A, [Z-a] matches z and [^Z-a] does not."""
    for expr, s, plain, folded in [(b"[^a]", b"A", True, False), (b"[Z-a]", b"z", False, True), (b"[^Z-a]", b"z", True, False), (b"\\x41", b"a", False, True),
                                   (b"[^\\W]", b"\xe9", False, False), (b"\\D", b"\xe9", True, True)]:
        for fold, want in ((False, plain), (True, folded)):
            assert bool(RM.pattern(expr, fold).search(s)) == want
            with api.Regex(expr, ignore_case=fold) as rx:
                assert rx.test(s) == want, (expr, s, fold)


# ---- refusals: (expression(s), code, index of the expression, offset) ----

DEEP = b"(" * 257 + b"a" + b")" * 257
REFUSALS = [
    # -MLZ_ERR_ARG
    (b"a**", ARG, 0, 2), (b"a{2}{3}", ARG, 0, 4), (b"a+*", ARG, 0, 2), (b"*a", ARG, 0, 0), (b"^*", ARG, 0, 1), (b"$+", ARG, 0, 1), (b"|+", ARG, 0, 1), (b"(?:*)", ARG, 0, 3),
    (b"a{", ARG, 0, 1), (b"a{,3}", ARG, 0, 1), (b"a{x}", ARG, 0, 1), (b"a{2", ARG, 0, 1), (b"a{2,3", ARG, 0, 1), (b"{2}", ARG, 0, 0), (b"a{256}", ARG, 0, 1), (b"a{3,2}", ARG, 0, 1),
    (b"a{2,256}", ARG, 0, 1), (b"a}", ARG, 0, 1), (b"a]", ARG, 0, 1), (b"a)", ARG, 0, 1), (b"(a", ARG, 0, 2), (b"(a|b", ARG, 0, 4), (b"\\", ARG, 0, 1), (b"\\x4", ARG, 0, 3),
    (b"\\xZ1", ARG, 0, 2), (b"[]", ARG, 0, 1), (b"[^]", ARG, 0, 2), (b"[b-a]", ARG, 0, 1), (b"[a", ARG, 0, 2), (b"[a^]", ARG, 0, 2), (b"[\\d-z]", ARG, 0, 1),
    (b"[a-\\d]", ARG, 0, 1), (b"[a-c-e]", ARG, 0, 4), (b"[a-b-]x[ab-c]*", None, 0, 0), ((b"ok", b"a**"), ARG, 1, 2), ((b"a",) * 3 + (b"[z-a]",), ARG, 3, 1),
    # -MLZ_ERR_UNSUPPORTED
    (b"\\b", UNSUPPORTED, 0, 0), (b"a\\B", UNSUPPORTED, 0, 1), (b"\\A", UNSUPPORTED, 0, 0), (b"a\\Z", UNSUPPORTED, 0, 1), (b"(a)\\1", UNSUPPORTED, 0, 3), (b"\\9", UNSUPPORTED, 0, 0),
    (b"\\e", UNSUPPORTED, 0, 0), (b"\\Q", UNSUPPORTED, 0, 0), (b"\\01", UNSUPPORTED, 0, 0), (b"[\\b]", UNSUPPORTED, 0, 1), (b"(?i)a", UNSUPPORTED, 0, 2), (b"(?=a)", UNSUPPORTED, 0, 2),
    (b"(?!a)", UNSUPPORTED, 0, 2), (b"(?<=a)b", UNSUPPORTED, 0, 2), (b"(?P<n>a)", UNSUPPORTED, 0, 2), (b"(?", UNSUPPORTED, 0, 2), (b"a*?", UNSUPPORTED, 0, 2), (b"a+?", UNSUPPORTED, 0, 2),
    (b"a??", UNSUPPORTED, 0, 2), (b"a{1,2}?", UNSUPPORTED, 0, 6), (b"a*+", UNSUPPORTED, 0, 2), (b"a++", UNSUPPORTED, 0, 2), (b"[[:alpha:]]", UNSUPPORTED, 0, 1), (DEEP, UNSUPPORTED, 0, 256),
    # the limits: positions, states
    (b"(a{255}){17}", UNSUPPORTED, 0, 12), ((b"a{255}",) * 17, UNSUPPORTED, 16, 6), (b"[ab]*a[ab]{16}", UNSUPPORTED, 0, 14), (b"[ab]*a[ab]{200}", UNSUPPORTED, 0, 15),
    ((b"x", b"[ab]*a[ab]{16}"), UNSUPPORTED, 1, 14),
]


def test_refusals(checkers):
    """Every refusal the contract names, with its code, its expression and its offset, from the checker (plain and sanitized) and as the
    exception api.Regex raises; n_exprs 0 and 257 and an expression of 4097 bytes; the two expressions whose DFA blows up are refused within a second each."""
    cases = [c for c in REFUSALS if c[1] is not None] + [((), ARG, 0, 0), ((b"a",) * 257, ARG, 257, 0), ((b"a", b"a" * 4097), ARG, 1, 4096)]
    lines = H.both(checkers, [rec_strings(e, 0, None, []) for e, *_ in cases])
    for line, (exprs, code, index, off) in zip(lines, cases):
        assert line.split() == ["err", str(code), str(index), str(off)], (exprs if len(exprs) < 40 else exprs[:40], line[:60])
    for exprs, code, index, off in cases:
        t = time.monotonic()
        with pytest.raises(api.ErrUnsupported if code == UNSUPPORTED else api.MinLZError) as e:
            api.Regex(exprs)
        assert time.monotonic() - t < 1.0, exprs
        assert type(e.value) is (api.ErrUnsupported if code == UNSUPPORTED else api.MinLZError)
        assert str(e.value) == "Regex: minlz error %d in expression %d at offset %d" % (code, index, off)
    for exprs, code, *_ in REFUSALS:                        # (what the model's own compiler says: an accepted expression is valid there too)
        if code is None:
            RM.pattern(exprs)
            api.Regex(exprs).close()
    api.Regex([b"a"] * 256).close()                         # the limits themselves are accepted
    api.Regex(b"[a]" * 1365 + b"a").close()                 # 4096 bytes
    with api.Regex(b"a{255}" * 16) as rx:                   # 4080 positions, and as many states and two
        assert rx.info()[:2] == (4082, 2) and rx.test(b"a" * 4080) and not rx.test(b"a" * 4079)
    with pytest.raises(api.ErrUnsupported, match="in expression 0 at offset 4096$"):
        api.Regex(b"a" * 4096)                              # 4096 positions are 4098 states
    api.Regex(b"(" * 256 + b"a" + b")" * 256).close()
    assert _lib.lib().mlz_regex_compile(b"a", (_lib.u32 * 1)(1), 1, 0, None, None) == -ARG          # nowhere to put the handle


# ---- the group rule, the mark layout, the longest record ----

NL = 10
LENGTHS = [0, 1, 15, 16, 17, 300]
CUTS = [1, 2, 7, 16, 64, 1000, 0]
COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 129]
GROUP_EXPRS = [b"a.*z", b"^a", b"z$", b"^$", b"zq"]


def group_data(N, closing, rng):
    """N records of the designed lengths over the bytes a z q ., the first two and the last two empty where N allows it (doubled delimiters at the
    start and at the end); closing: the stream ends with the delimiter (else its last record has a byte)."""
    recs = []
    for r in range(N):
        n = LENGTHS[(r * 5 + 2) % len(LENGTHS)] if N >= 6 and 2 <= r < N - 2 else (0 if N >= 6 else LENGTHS[(r + 1) % len(LENGTHS)])
        recs.append(np.frombuffer(b"azq.", np.uint8)[rng.integers(0, 4, n)].tobytes())
    if recs and not closing and not recs[-1]:
        recs[-1] = b"z"
    return b"\n".join(recs) + (b"\n" if closing and recs else b"")


@pytest.fixture(scope="module")
def group_cases():
    rng = np.random.default_rng(40)
    recs, notes, want = [], [], []
    for N in COUNTS:
        for closing in (True, False):
            data = group_data(N, closing, rng)
            records = GM.records(data, b"\n")
            assert len(records) == N and len(data) < 16 << 10
            if N >= 64:
                assert {len(r) for r in records} >= set(LENGTHS) and data.startswith(b"\n\n") and (not closing or data.endswith(b"\n\n\n"))
            for expr in GROUP_EXPRS:
                M = RM.matching(records, expr)
                recs.append(rec_groups(expr, 0, NL, data, CUTS))
                notes.append((N, closing, expr))
                want.append((N, max([len(r) for r in records] + [0]), "".join("1" if r in M else "0" for r in range(N))))
    return recs, notes, want


def test_group_rule_and_mark_layout(checkers, group_cases):
    """Records of length 0, 1, 15, 16, 17 and 300, doubled delimiters at both ends, streams with and without a closing delimiter, N from 0 to 129,
    cut into groups of 1, 2, 7, 16, 64 and 1000 bytes and into one: the bitmap is the model's M at every group size, every record is finished by
    exactly one group, no word has two writers in a launch (the checker ends with status 3 otherwise), and regex_longest is the longest record."""
    recs, notes, want = group_cases
    lines = H.both(checkers, recs)
    assert len(lines) == len(want)
    seen = set()
    for line, (N, longest, bits), note in zip(lines, want, notes):
        parts = [p.strip() for p in line.split("|")]
        assert parts[0].split() == [str(N), str(longest)], note
        assert len(parts) == 1 + len(CUTS)
        for cut, got in zip(CUTS, parts[1:]):
            assert got == bits, (note, cut)
        seen |= set(bits)
    assert seen == {"0", "1"}
