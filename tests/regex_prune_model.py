"""The contract of the regex grep that prunes by search tables (include/minlz_hip_regex_prune.h) in plain Python, for
tests/test_regex_prune_host.py and tests/test_gpu_stream_regex_prune.py: the required literals of an expression (a parser of the accepted syntax and
the rule of the header, node by node), the widening of a set of taken chunks to whole records, the runs of the widened set, and which records a
pruned call evaluates.  What the expression matches is tests/regex_model.py's, Python's own `re`."""
import bisect

from tests import grep_model as GM
from tests import regex_model as RM

MAX_LITERALS, MAX_LEN, PRODUCT, SMALL_SET = 64, 256, 16, 4
META = b"\\.[](){}*+?|^$"
DIGIT = frozenset(range(0x30, 0x3a))
WORD = DIGIT | frozenset(range(0x41, 0x5b)) | frozenset(range(0x61, 0x7b)) | {0x5f}
SPACE = frozenset(b" \t\n\r\f\v")
ALL = frozenset(range(256))


def close_case(s):
    return frozenset(s) | {b ^ 0x20 for b in s if 0x41 <= (b & ~0x20) <= 0x5a}


class Parser:
    """The syntax tree of an ACCEPTED expression, node for node the compiler's: ("set", bytes), ("cat", kids), ("alt", kids), ("rep", node, m, n or
    None), ("begin",), ("end",), ("empty",); a concatenation or an alternation of one item is that item."""

    def __init__(self, expr, fold):
        self.e, self.p, self.fold = bytes(expr), 0, fold

    def peek(self):
        return self.e[self.p:self.p + 1]

    def escape(self):
        """At a backslash -> (set, the single byte or None)."""
        c = self.e[self.p + 1]
        self.p += 2
        if c in b"dDwWsS":
            s = {0x64: DIGIT, 0x77: WORD, 0x73: SPACE}[c | 0x20]
            return (ALL - s if c < 0x61 else s), None
        if c == 0x78:
            b = int(self.e[self.p:self.p + 2], 16)
            self.p += 2
        else:
            b = {0x6e: 10, 0x72: 13, 0x74: 9, 0x66: 12, 0x76: 11, 0x30: 0}.get(c, c)
        return frozenset([b]), b

    def klass(self):
        self.p += 1
        negate = self.peek() == b"^"
        self.p += negate
        items, first = set(), True
        while first or self.peek() != b"]":
            first = False
            if self.peek() == b"\\":
                s, lo = self.escape()
            else:
                lo = self.e[self.p]
                s = frozenset([lo])
                self.p += 1
            if self.peek() == b"-" and self.e[self.p + 1:self.p + 2] != b"]" and lo is not None:
                self.p += 1
                if self.peek() == b"\\":
                    _, hi = self.escape()
                else:
                    hi = self.e[self.p]
                    self.p += 1
                s = frozenset(range(lo, hi + 1))
            items |= s
        self.p += 1
        if self.fold:
            items = close_case(items)
        return ("set", frozenset(ALL - items if negate else items))

    def atom(self):
        c = self.peek()
        if c == b"(":
            self.p += 3 if self.e[self.p + 1:self.p + 3] == b"?:" else 1
            r = self.alt()
            assert self.peek() == b")"
            self.p += 1
            return r
        if c == b"[":
            return self.klass()
        self.p += 1
        if c == b".":
            return ("set", ALL)
        if c == b"^":
            return ("begin",)
        if c == b"$":
            return ("end",)
        if c == b"\\":
            self.p -= 1
            s, single = self.escape()
            return ("set", close_case(s) if self.fold and single is not None else s)
        assert c not in META, c
        return ("set", close_case(c) if self.fold else frozenset(c))

    def rep(self):
        a = self.atom()
        c = self.peek()
        if c in (b"*", b"+", b"?"):
            self.p += 1
            return ("rep", a) + {b"*": (0, None), b"+": (1, None), b"?": (0, 1)}[c]
        if c == b"{":
            end = self.e.index(b"}", self.p)
            m, _, n = self.e[self.p + 1:end].partition(b",")
            self.p = end + 1
            return ("rep", a, int(m), (int(n) if n else None) if _ else int(m))
        return a

    def cat(self):
        items = []
        while self.p < len(self.e) and self.peek() not in (b"|", b")"):
            items.append(self.rep())
        return ("empty",) if not items else items[0] if len(items) == 1 else ("cat", items)

    def alt(self):
        items = [self.cat()]
        while self.peek() == b"|":
            self.p += 1
            items.append(self.cat())
        return items[0] if len(items) == 1 else ("alt", items)


def parse(expr, fold=False):
    ps = Parser(expr, fold)
    tree = ps.alt()
    assert ps.p == len(ps.e), (expr, ps.p)
    return tree


# ---- the literal rule: a node -> (E or None, F or None), sets as sorted tuples of bytes ----

def norm(strings):
    return tuple(sorted(set(strings)))


def product(a, b):
    """a x b within the caps, else None."""
    if len(a) * len(b) > PRODUCT or any(len(x) + len(y) > MAX_LEN for x in a for y in b):
        return None
    return norm(x + y for x in a for y in b)


def best(candidates):
    """Of the candidates in the order they arose: none with the empty string; the larger shortest string, then the fewer strings, then the leftmost."""
    top = None
    for c in candidates:
        if not c or min(len(s) for s in c) == 0:
            continue
        if top is None or (min(map(len, c)), -len(c)) > (min(map(len, top)), -len(top)):
            top = c
    return top


def node_sets(node, fold):
    kind = node[0]
    if kind in ("empty", "begin", "end"):
        return (b"",), None
    if kind == "set":
        img = {b + 32 if fold and 0x41 <= b <= 0x5a else b for b in node[1]}
        if len(img) > SMALL_SET:
            return None, None
        E = norm(bytes([b]) for b in img)
        return E, E
    if kind == "cat":
        X, closed, cands = (b"",), False, []
        for kid in node[1]:
            E, F = node_sets(kid, fold)
            p = product(X, E) if E is not None else None
            if p is not None:
                X = p
            else:
                cands.append(X)
                closed = True
                X = E if E is not None else (b"",)
            if F is not None:
                cands.append(F)
        cands.append(X)
        return (None if closed else X), best(cands)
    if kind == "alt":
        E, F = (), ()
        for kid in node[1]:
            e, f = node_sets(kid, fold)
            E = None if E is None or e is None else norm(E + e)
            F = None if F is None or f is None else norm(F + f)
            E = None if E is not None and len(E) > PRODUCT else E
            F = None if F is not None and len(F) > MAX_LITERALS else F
        return E, F
    _, a, m, n = node
    E, F = node_sets(a, fold)
    if m == 0:
        e = norm(E + (b"",)) if n == 1 and E is not None else None
        return (e if e is not None and len(e) <= PRODUCT else None), None
    power = (b"",) if E is not None else None
    for _ in range(m):
        power = product(power, E) if power is not None else None
    return (power if m == n else None), best([F, power])


def literals(exprs, fold=False):
    """L of one compile: the sorted list of required literals, [] for none."""
    exprs = [exprs] if isinstance(exprs, (bytes, bytearray)) else list(exprs)
    F = ()
    for e in exprs:
        f = node_sets(parse(e, fold), fold)[1]
        F = None if F is None or f is None else norm(F + f)
        if F is not None and len(F) > MAX_LITERALS:
            F = None
    return list(F or ())


def sound(lits, fold, string):
    """Does the string (folded under the flag) hold a literal."""
    s = bytes(b + 32 if 0x41 <= b <= 0x5a else b for b in string) if fold else string
    return any(l in s for l in lits)


# ---- widen, runs, the evaluated records ----

def spans(data, delim):
    """[(start, end)] of the records of data, the delimiter excluded, and number(p) for every position."""
    recs = GM.records(data, delim)
    out, at = [], 0
    for r in recs:
        out.append((at, at + len(r)))
        at += len(r) + 1
    number = [0] * len(data)
    for r, (s, e) in enumerate(out):
        for p in range(s, min(e + 1, len(data))):
            number[p] = r
    return out, number


def widen(chunks, take, rec_spans, number):
    """chunks: [(off, n)] in stream order, each with bytes; take: a set of chunk numbers -> the widened set: per taken chunk the span from the start
    of the record that holds its first byte to the end of the record that holds its last, and every chunk that intersects it."""
    offs, ends = [o for o, _ in chunks], [o + n for o, n in chunks]
    out = set(take)
    for c in take:
        off, n = chunks[c]
        lo, hi = rec_spans[number[off]][0], rec_spans[number[off + n - 1]][1]
        out.update(range(bisect.bisect_right(ends, lo), bisect.bisect_left(offs, hi)))
    return out


def runs(chunks, taken):
    """The maximal pieces [first, end) of decoded stream whose chunks are all taken."""
    out = []
    for c in sorted(taken):
        off, n = chunks[c]
        if out and out[-1][1] == off:
            out[-1][1] = off + n
        else:
            out.append([off, off + n])
    return [tuple(r) for r in out]


def evaluated(rec_spans, run_list):
    """The records a run holds whole: run.first <= s < run.end and e <= run.end (an empty record needs its delimiter inside the run)."""
    firsts, out = [a for a, _ in run_list], set()
    for r, (s, e) in enumerate(rec_spans):
        i = bisect.bisect_right(firsts, s) - 1
        if i >= 0 and s < run_list[i][1] and e <= run_list[i][1]:
            out.add(r)
    return out


def marks(rec_spans, number, chunks, take, M):
    """What a pruned call marks when the plan takes `take` and the expression matches the records M: (the widened set, M restricted to the
    records its runs hold whole)."""
    wide = widen(chunks, take, rec_spans, number)
    return wide, set(M) & evaluated(rec_spans, runs(chunks, wide))


def cut_chunks(size, n):
    """[(off, n)] of a stream of `size` bytes in chunks of n bytes."""
    return [(o, min(n, size - o)) for o in range(0, size, n)]
