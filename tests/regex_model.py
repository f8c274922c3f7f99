"""The contract of the grep for regular expressions over the record index (include/minlz_hip_regex.h: mlz_dev_reader_grep_regex) in plain Python,
for tests/test_stream_regex_host.py and tests/test_gpu_stream_regex.py.  An accepted expression is Python's own `re` on bytes, compiled with
re.DOTALL (and re.IGNORECASE), with every unescaped $ outside a class rewritten to \\Z and every such ^ to \\A: Python's bare $ also matches in
front of a trailing newline, which matters where the delimiter is another byte.  M = the records in which the pattern is found; everything behind
M is tests/grep_model.py's."""
import re

from tests import grep_model as GM


def anchored(expr):
    """expr with ^ -> \\A and $ -> \\Z outside escapes and classes."""
    out, i, in_class = bytearray(), 0, False
    while i < len(expr):
        c = expr[i:i + 1]
        if c == b"\\":
            out += expr[i:i + 2]
            i += 2
            continue
        if in_class:
            in_class = c != b"]"
        elif c == b"[":
            in_class = True
            if expr[i + 1:i + 2] == b"^":       # (the class's own ^ stays)
                out += b"[^"
                i += 2
                continue
        elif c in (b"^", b"$"):
            c = b"\\A" if c == b"^" else b"\\Z"
        out += c
        i += 1
    return bytes(out)


def pattern(exprs, ignore_case=False):
    """The union of the expressions (a bytes object, or a sequence of them) as one compiled pattern."""
    exprs = [exprs] if isinstance(exprs, (bytes, bytearray)) else list(exprs)
    return re.compile(b"|".join(b"(?:" + anchored(bytes(e)) + b")" for e in exprs), re.DOTALL | (re.IGNORECASE if ignore_case else 0))


def matching(recs, exprs, ignore_case=False):
    """M: the numbers of the records in which some substring is in the language."""
    p = pattern(exprs, ignore_case)
    return {r for r, rec in enumerate(recs) if p.search(rec)}


def result(data, delim, exprs, ignore_case=False, invert=False, before=0, after=0):
    """grep_model.result with M from the expressions: dict(N, M, S, C, R, numbers, kinds, totals) without a cut."""
    recs = GM.records(data, delim)
    N = len(recs)
    M = matching(recs, exprs, ignore_case)
    S = set(range(N)) - M if invert else M
    C = sorted(GM.context(S, N, before, after))
    return dict(N=N, M=sorted(M), S=sorted(S), C=C, R=len(C), numbers=C, kinds=[1 if r in S else 0 for r in C],
                totals=(len(C), len(S), sum(len(recs[r]) for r in C), sum(len(recs[r]) for r in C)), recs=recs)


def cut(m, rec_cap):
    """The model's answer at rec_cap: the first k = min(R, rec_cap) numbers and kinds, the totals with the bytes of the k written records."""
    k = min(m["R"], rec_cap)
    return dict(m, numbers=m["C"][:k], kinds=m["kinds"][:k], totals=(m["R"], len(m["S"]), sum(len(m["recs"][r]) for r in m["C"][:k]), m["totals"][3]))
