// mlz_regex_compile.h — the compiler of mlz_regex_compile (include/minlz_hip_regex.h): regular expressions over bytes -> the search automaton
// that mlz_stream_regex.h walks.  Host only, plain C++17, no HIP: tools/stream_regex_check.cpp includes it as mlz_hip.hip does.
//
//   expression(s) -> syntax tree -> Thompson NFA (counted repetitions expanded) -> DFA by subset construction -> Moore's partition refinement
//   -> byte classes merged -> the table, pre-multiplied and numbered as mlz_stream_regex.h says.
//
// Syntax: a subset of Python's `re` on bytes in which every accepted expression means the same there (re.DOTALL; ^ and $ as \A and \Z of a record).
//   alt  := cat ('|' cat)*          cat := rep*  (may be empty)          rep := atom quant?
//   quant: * + ? {m} {m,} {m,n}, 0 <= m <= n <= 255.  A second quantifier, a quantifier with nothing to repeat (also behind ^ or $), a { that opens
//          none of the three forms: -ARG.  A quantifier followed by ? or + (lazy, possessive): -UNSUPPORTED.
//   atom : a byte that is none of \ . [ ] ( ) { } * + ? | ^ $;  .  (any byte);  a class;  ( alt );  (?: alt );  ^;  $;  an escape.
//          (? followed by anything but ':' : -UNSUPPORTED.  Groups nest kRegexMaxDepth deep at the most (-UNSUPPORTED beyond).
//   escape: \ and a metacharacter or one of - / " : that byte;  \n \r \t \f \v \0;  \xHH;  \d \D \w \W \s \S (ASCII);  \0 followed by a digit
//          (an octal escape in Python) and \ followed by anything else: -UNSUPPORTED.
//   class: '[' '^'? items ']';  an item is a byte, lo-hi (bytes, lo <= hi) or an escape;  ] and ^ meant literally are escaped;  - is literal as the
//          first or the last item;  an empty class, an unescaped ^ behind the first place, a range from or to \d \w \s ..., a - behind a range that
//          is not the last item: -ARG;  [: (a POSIX bracket name): -UNSUPPORTED.
// MLZ_REGEX_IGNORE_CASE: every byte set (a literal as a singleton, a class before its ^, \d \w \s) is closed under the ASCII case swap before a
//   negation is applied: what re.IGNORECASE does on bytes.  The fold lives in the class map; the walk folds nothing.
// Limits, checked while the automaton is built (the subset construction stops at the limit, it never builds a blow-up first): kRegexMaxPositions
//   byte positions behind the expansion, kRegexMaxStates states, kRegexLdsMax bytes of class map and table: -UNSUPPORTED.
// Errors come with (index of the expression, byte offset in it): the offset of the byte at which the parser stopped — the quantifier with nothing to
//   repeat, the second quantifier, the ? or + behind a quantifier, the byte behind "(?", the backslash of an escape, the first byte of a bad class
//   item, the expression's length where it ends too early.  A limit of the automaton as a whole reports the last expression and its length; a bad
//   count of expressions reports (n_exprs, 0).
// Required literals (Literals below; the rule and its limits are written out in mlz_stream_regex_prune.h): a set of byte strings of which every
//   matching record holds one, derived from the syntax tree.  Compiling never fails because of them: an expression too rich has none.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "mlz_stream_regex_prune.h"

namespace mlz {

constexpr int kRegexErrUnsupported = 3, kRegexErrArg = 8;   // MLZ_ERR_UNSUPPORTED, MLZ_ERR_ARG (this header compiles without minlz_hip.h)

// The compiled form: plain arrays
struct RegexProgram {
    uint8_t cmap[256];               // byte -> class, below C
    std::vector<uint16_t> next;      // S * C entries: next[state + class] = the next state; states pre-multiplied by C
    uint32_t S = 0, C = 0;
    uint32_t start = 0;              // the state in front of a record's first byte
    uint32_t end_hi = 0;             // the end-accepting states are [2 C, end_hi)
    uint32_t n_end = 0;              // how many
    bool empty_ok = false;           // the start state accepts the empty record
    uint32_t flags = 0;
    std::vector<std::string> literals;   // the required literals (mlz_stream_regex_prune.h), sorted, folded under kRegexIgnoreCase; empty: none
    uint32_t image_bytes() const { return regex_image_bytes(S, C); }
    // The image the kernel loads: cmap | next | zeros up to a multiple of 16
    void image(uint8_t* out) const {
        memset(out, 0, image_bytes());
        memcpy(out, cmap, 256);
        memcpy(out + 256, next.data(), next.size() * 2);
    }
};

namespace regex_detail {

struct ByteSet {
    uint64_t w[4] = {0, 0, 0, 0};
    void add(uint32_t b) { w[b >> 6] |= uint64_t(1) << (b & 63); }
    void add_range(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; b++) add(b); }
    bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
    void unite(const ByteSet& o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
    void invert() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
    void close_case() {
        for (uint32_t b = 'a'; b <= 'z'; b++) {
            if (has(b)) add(b - 32);
            else if (has(b - 32)) add(b);
        }
    }
    bool operator<(const ByteSet& o) const { return memcmp(w, o.w, sizeof w) < 0; }
};

inline ByteSet set_digit() { ByteSet s; s.add_range('0', '9'); return s; }
inline ByteSet set_word() { ByteSet s; s.add_range('0', '9'); s.add_range('A', 'Z'); s.add_range('a', 'z'); s.add('_'); return s; }
inline ByteSet set_space() { ByteSet s; for (uint8_t b : {' ', '\t', '\n', '\r', '\f', '\v'}) s.add(b); return s; }

enum Kind : uint8_t { kEmpty, kSet, kCat, kAlt, kRep, kBegin, kEnd };
struct Node {
    Kind kind;
    int32_t a = -1, b = -1;          // kSet: a = the set; kRep: a = the body; kCat / kAlt: children [a, b) of `kids`
    int32_t min = 0, max = 0;        // kRep; max < 0: no upper bound
};

struct Error { int code = 0; uint64_t off = 0; };

struct Parser {
    const uint8_t* e;
    size_t n, p = 0;
    bool fold;
    std::vector<Node> nodes;
    std::vector<int32_t> kids;
    std::vector<ByteSet> sets;
    Error err;

    static bool meta(uint8_t c) { return c && strchr("\\.[](){}*+?|^$", c) != nullptr; }
    int fail(int code, size_t off) { if (!err.code) { err.code = code; err.off = off; } return -1; }
    int node(Node nd) { nodes.push_back(nd); return int(nodes.size()) - 1; }
    int set_node(ByteSet s) { sets.push_back(s); Node nd{kSet}; nd.a = int32_t(sets.size()) - 1; return node(nd); }
    int list_node(Kind kind, const std::vector<int32_t>& items) {
        Node nd{kind};
        nd.a = int32_t(kids.size());
        kids.insert(kids.end(), items.begin(), items.end());
        nd.b = int32_t(kids.size());
        return node(nd);
    }

    // An escape at e[p] == '\\' -> the set (single: one byte, *byte); -1 after fail()
    int escape(ByteSet* out, bool* single, uint8_t* byte) {
        const size_t at = p;
        if (p + 1 >= n) return fail(kRegexErrArg, n);
        const uint8_t c = e[p + 1];
        p += 2;
        *single = true;
        ByteSet s;
        if (meta(c) || c == '-' || c == '/' || c == '"') *byte = c;
        else if (c == 'n') *byte = '\n';
        else if (c == 'r') *byte = '\r';
        else if (c == 't') *byte = '\t';
        else if (c == 'f') *byte = '\f';
        else if (c == 'v') *byte = '\v';
        else if (c == '0') {
            if (p < n && e[p] >= '0' && e[p] <= '9') return fail(kRegexErrUnsupported, at);
            *byte = 0;
        } else if (c == 'x') {
            uint32_t v = 0;
            for (int i = 0; i < 2; i++, p++) {
                if (p >= n) return fail(kRegexErrArg, n);
                const uint8_t h = e[p];
                if (h >= '0' && h <= '9') v = v * 16 + (h - '0');
                else if (h >= 'a' && h <= 'f') v = v * 16 + (h - 'a' + 10);
                else if (h >= 'A' && h <= 'F') v = v * 16 + (h - 'A' + 10);
                else return fail(kRegexErrArg, p);
            }
            *byte = uint8_t(v);
        } else if (c == 'd' || c == 'D' || c == 'w' || c == 'W' || c == 's' || c == 'S') {
            *single = false;
            s = c == 'd' || c == 'D' ? set_digit() : c == 'w' || c == 'W' ? set_word() : set_space();
            if (c < 'a') s.invert();   // (\d \w \s are closed under the case swap as they stand)
            *out = s;
            return 0;
        } else {
            return fail(kRegexErrUnsupported, at);
        }
        s.add(*byte);
        *out = s;
        return 0;
    }

    int klass() {   // e[p] == '['
        p++;
        bool negate = false;
        if (p < n && e[p] == '^') { negate = true; p++; }
        ByteSet all;
        bool first = true;
        for (;; first = false) {
            if (p >= n) return fail(kRegexErrArg, n);
            const size_t at = p;
            uint8_t c = e[p];
            if (c == ']') {
                if (first) return fail(kRegexErrArg, at);
                p++;
                break;
            }
            ByteSet item;
            bool single = true;
            uint8_t lo = c;
            if (c == '\\') {
                if (escape(&item, &single, &lo) < 0) return -1;
            } else {
                if (c == '^') return fail(kRegexErrArg, at);
                if (c == '[' && p + 1 < n && e[p + 1] == ':') return fail(kRegexErrUnsupported, at);
                if (c == '-' && !first && !(p + 1 < n && e[p + 1] == ']')) return fail(kRegexErrArg, at);   // (a - in the middle that is no range's)
                p++;
                item.add(c);
            }
            if (p + 1 < n && e[p] == '-' && e[p + 1] != ']') {   // a range
                if (!single) return fail(kRegexErrArg, at);
                p++;
                ByteSet hi_set;
                bool hi_single = true;
                uint8_t hi = e[p];
                if (hi == '\\') {
                    if (escape(&hi_set, &hi_single, &hi) < 0) return -1;
                    if (!hi_single) return fail(kRegexErrArg, at);
                } else {
                    if (hi == '[' && p + 1 < n && e[p + 1] == ':') return fail(kRegexErrUnsupported, p);
                    if (hi == '^') return fail(kRegexErrArg, p);
                    p++;
                }
                if (lo > hi) return fail(kRegexErrArg, at);
                item = ByteSet();
                item.add_range(lo, hi);
                if (p + 1 < n && e[p] == '-' && e[p + 1] != ']') return fail(kRegexErrArg, p);   // a - behind a range that is not the last item
            }
            all.unite(item);
        }
        if (fold) all.close_case();
        if (negate) all.invert();
        return set_node(all);
    }

    int atom(uint32_t depth) {
        const uint8_t c = e[p];
        if (c == '(') {
            if (depth >= kRegexMaxDepth) return fail(kRegexErrUnsupported, p);
            p++;
            if (p < n && e[p] == '?') {
                if (!(p + 1 < n && e[p + 1] == ':')) return fail(kRegexErrUnsupported, p + 1 < n ? p + 1 : n);
                p += 2;
            }
            const int r = alt(depth + 1);
            if (r < 0) return -1;
            if (p >= n || e[p] != ')') return fail(kRegexErrArg, p);
            p++;
            return r;
        }
        if (c == '[') return klass();
        if (c == '.') { p++; ByteSet s; s.invert(); return set_node(s); }
        if (c == '^') { p++; return node(Node{kBegin}); }
        if (c == '$') { p++; return node(Node{kEnd}); }
        if (c == '\\') {
            ByteSet s;
            bool single;
            uint8_t byte;
            if (escape(&s, &single, &byte) < 0) return -1;
            if (single && fold) s.close_case();
            return set_node(s);
        }
        if (meta(c)) return fail(kRegexErrArg, p);   // ] } ) and a quantifier with nothing to repeat
        p++;
        ByteSet s;
        s.add(c);
        if (fold) s.close_case();
        return set_node(s);
    }

    // A quantifier at e[p] -> min, max; 0 = none there
    int quant(int32_t* mn, int32_t* mx) {
        if (p >= n) return 0;
        const uint8_t c = e[p];
        if (c == '*') { *mn = 0; *mx = -1; p++; return 1; }
        if (c == '+') { *mn = 1; *mx = -1; p++; return 1; }
        if (c == '?') { *mn = 0; *mx = 1; p++; return 1; }
        if (c != '{') return 0;
        const size_t at = p;
        p++;
        auto number = [&](int32_t* v) {
            size_t digits = 0;
            for (*v = 0; p < n && e[p] >= '0' && e[p] <= '9'; p++, digits++) *v = *v > 1000 ? *v : *v * 10 + (e[p] - '0');
            return digits;
        };
        if (!number(mn)) return fail(kRegexErrArg, at);
        *mx = *mn;
        if (p < n && e[p] == ',') {
            p++;
            if (!number(mx)) *mx = -1;
        }
        if (p >= n || e[p] != '}') return fail(kRegexErrArg, at);
        p++;
        if (*mn > int32_t(kRegexMaxRepeat) || *mx > int32_t(kRegexMaxRepeat) || (*mx >= 0 && *mn > *mx)) return fail(kRegexErrArg, at);
        return 1;
    }

    int rep(uint32_t depth) {
        const bool anchor = e[p] == '^' || e[p] == '$';   // (a group around one may be repeated)
        const int a = atom(depth);
        if (a < 0) return -1;
        int32_t mn = 0, mx = 0;
        const size_t at = p;
        const int q = quant(&mn, &mx);
        if (q < 0) return -1;
        if (!q) return a;
        if (anchor) return fail(kRegexErrArg, at);   // nothing to repeat
        if (p < n && (e[p] == '?' || e[p] == '+')) return fail(kRegexErrUnsupported, p);
        if (p < n && (e[p] == '*' || e[p] == '{')) return fail(kRegexErrArg, p);
        Node nd{kRep};
        nd.a = a; nd.min = mn; nd.max = mx;
        return node(nd);
    }

    int cat(uint32_t depth) {
        std::vector<int32_t> items;
        while (p < n && e[p] != '|' && e[p] != ')') {
            const int r = rep(depth);
            if (r < 0) return -1;
            items.push_back(r);
        }
        if (items.empty()) return node(Node{kEmpty});
        return items.size() == 1 ? items[0] : list_node(kCat, items);
    }

    int alt(uint32_t depth) {
        std::vector<int32_t> items;
        for (;;) {
            const int r = cat(depth);
            if (r < 0) return -1;
            items.push_back(r);
            if (p < n && e[p] == '|') { p++; continue; }
            break;
        }
        return items.size() == 1 ? items[0] : list_node(kAlt, items);
    }

    int parse() {
        const int r = alt(0);
        if (r < 0) return -1;
        if (p < n) return fail(kRegexErrArg, p);   // an unmatched )
        return r;
    }
};

// The required literals of a syntax tree, node by node: E, the finite set of all strings the node matches (or unknown), and F, the best set of
// required factors (or none).  Sets are sorted and hold no string twice.
using LitStrings = std::vector<std::string>;
struct LitNode { bool e_known = false, f_some = false; LitStrings E, F; };

inline void lit_normalize(LitStrings* v) { std::sort(v->begin(), v->end()); v->erase(std::unique(v->begin(), v->end()), v->end()); }
inline LitStrings lit_union(const LitStrings& a, const LitStrings& b) { LitStrings u = a; u.insert(u.end(), b.begin(), b.end()); lit_normalize(&u); return u; }
// a x b within the caps of a product; false beyond them
inline bool lit_product(const LitStrings& a, const LitStrings& b, LitStrings* out) {
    if (!regex_lit_product_fits(a.size(), b.size())) return false;
    LitStrings p;
    for (const std::string& x : a)
        for (const std::string& y : b) {
            if (x.size() + y.size() > kRegexMaxLiteralLen) return false;
            p.push_back(x + y);
        }
    lit_normalize(&p);
    *out = std::move(p);
    return true;
}
inline size_t lit_shortest(const LitStrings& v) {
    size_t m = ~size_t(0);
    for (const std::string& s : v) m = std::min(m, s.size());
    return v.empty() ? 0 : m;
}
// The candidates of a node in the order they arise; best(): regex_lit_better decides, the leftmost wins a tie
struct LitCandidates {
    bool some = false;
    LitStrings best;
    void offer(const LitStrings& v) {
        if (v.empty() || lit_shortest(v) == 0) return;   // (a set that holds the empty string is no candidate)
        if (!some || regex_lit_better(lit_shortest(v), v.size(), lit_shortest(best), best.size())) { best = v; some = true; }
    }
};

struct Literals {
    const Parser& ps;
    bool fold;

    static LitNode empty_string() { LitNode n; n.e_known = true; n.E.assign(1, std::string()); return n; }
    LitNode of(int id) const {
        const Node& nd = ps.nodes[id];
        switch (nd.kind) {
        case kEmpty: case kBegin: case kEnd: return empty_string();
        case kSet: {
            const ByteSet& s = ps.sets[nd.a];
            ByteSet img;
            for (uint32_t b = 0; b < 256; b++) if (s.has(b)) img.add(fold ? regex_lit_fold(uint8_t(b)) : b);
            LitNode n;
            for (uint32_t b = 0; b < 256; b++) if (img.has(b)) n.E.push_back(std::string(1, char(b)));
            if (n.E.size() > kRegexLitSmallSet) { n.E.clear(); return n; }
            n.e_known = n.f_some = true;
            n.F = n.E;
            return n;
        }
        case kCat: {
            LitStrings X(1, std::string());
            bool closed = false;
            LitCandidates c;
            for (int32_t i = nd.a; i < nd.b; i++) {
                const LitNode k = of(ps.kids[i]);
                LitStrings p;
                if (k.e_known && lit_product(X, k.E, &p)) X = std::move(p);
                else {
                    c.offer(X);
                    closed = true;
                    X = k.e_known ? k.E : LitStrings(1, std::string());
                }
                if (k.f_some) c.offer(k.F);
            }
            c.offer(X);
            LitNode n;
            if (!closed) { n.e_known = true; n.E = X; }
            n.f_some = c.some; n.F = c.best;
            return n;
        }
        case kAlt: {
            LitNode n;
            n.e_known = n.f_some = true;
            for (int32_t i = nd.a; i < nd.b; i++) {
                const LitNode k = of(ps.kids[i]);
                if (n.e_known && k.e_known) { n.E = lit_union(n.E, k.E); n.e_known = n.E.size() <= kRegexLitProduct; } else n.e_known = false;
                if (n.f_some && k.f_some) { n.F = lit_union(n.F, k.F); n.f_some = n.F.size() <= kRegexMaxLiterals; } else n.f_some = false;
            }
            if (!n.e_known) n.E.clear();
            if (!n.f_some) n.F.clear();
            return n;
        }
        case kRep: {
            const LitNode a = of(nd.a);
            LitNode n;
            if (nd.min == 0) {
                if (nd.max == 1 && a.e_known) { n.E = lit_union(a.E, LitStrings(1, std::string())); n.e_known = n.E.size() <= kRegexLitProduct; }
                if (!n.e_known) n.E.clear();
                return n;
            }
            LitStrings pw(1, std::string());
            bool known = a.e_known;
            for (int32_t i = 0; i < nd.min && known; i++) { LitStrings p; known = lit_product(pw, a.E, &p); if (known) pw = std::move(p); }
            LitCandidates c;
            if (a.f_some) c.offer(a.F);
            if (known) c.offer(pw);
            n.f_some = c.some; n.F = c.best;
            if (known && nd.min == nd.max) { n.e_known = true; n.E = pw; }
            return n;
        }
        }
        return LitNode();
    }
};

// The NFA: kByte consumes a byte of its set and goes to out1; kSplit goes to out1 and out2 (-1: none) for nothing; kAtBegin / kAtEnd go to out1
// for nothing in front of the first / behind the last byte only; kMatch is the end.
enum NfaKind : uint8_t { kSplit, kByte, kAtBegin, kAtEnd, kMatch };
struct NfaNode { NfaKind kind; int32_t out1 = -1, out2 = -1, set = -1; };

constexpr size_t kRegexMaxNodes = size_t(1) << 18;   // of the NFA, counted repetitions expanded

struct Builder {
    const Parser& ps;
    std::vector<NfaNode>& nfa;
    std::vector<ByteSet>& sets;
    bool full = false;

    int make(NfaKind kind, int32_t set = -1) {
        if (nfa.size() >= kRegexMaxNodes) { full = true; return 0; }
        NfaNode nd{kind};
        nd.set = set;
        nfa.push_back(nd);
        return int(nfa.size()) - 1;
    }
    // byte positions of a node behind the expansion, saturating
    uint64_t positions(int id) const {
        const Node& nd = ps.nodes[id];
        uint64_t v = 0;
        switch (nd.kind) {
        case kSet: return 1;
        case kCat: case kAlt:
            for (int32_t i = nd.a; i < nd.b; i++) v = std::min<uint64_t>(v + positions(ps.kids[i]), uint64_t(1) << 40);
            return v;
        case kRep:
            return std::min<uint64_t>(positions(nd.a) * uint64_t(nd.max >= 0 ? nd.max : std::max(nd.min, 1)), uint64_t(1) << 40);
        default: return 0;
        }
    }
    // Builds node id: entered at the returned node, left through *exit (a kSplit without outs, to be wired by the caller)
    int build(int id, int* exit) {
        const Node& nd = ps.nodes[id];
        switch (nd.kind) {
        case kEmpty: { const int s = make(kSplit); *exit = s; return s; }
        case kSet: { const int s = make(kByte, int32_t(intern(ps.sets[nd.a]))), x = make(kSplit); nfa[s].out1 = x; *exit = x; return s; }
        case kBegin: case kEnd: { const int s = make(nd.kind == kBegin ? kAtBegin : kAtEnd), x = make(kSplit); nfa[s].out1 = x; *exit = x; return s; }
        case kCat: {
            int entry = -1, last = -1;
            for (int32_t i = nd.a; i < nd.b && !full; i++) {
                int x;
                const int s = build(ps.kids[i], &x);
                if (entry < 0) entry = s; else nfa[last].out1 = s;
                last = x;
            }
            *exit = last;
            return entry;
        }
        case kAlt: {
            const int x = make(kSplit);
            int entry = -1;
            for (int32_t i = nd.b - 1; i >= nd.a && !full; i--) {   // a chain of splits, the first alternative in front
                int bx;
                const int s = build(ps.kids[i], &bx);
                nfa[bx].out1 = x;
                const int sp = make(kSplit);
                nfa[sp].out1 = s; nfa[sp].out2 = entry;
                entry = sp;
            }
            *exit = x;
            return entry;
        }
        case kRep: {
            // a body without byte positions matches the empty string at the most: x{m,n} is x for m >= 1 and nothing for m == 0
            if (nd.max == 0 || (positions(nd.a) == 0 && nd.min == 0)) { const int s = make(kSplit); *exit = s; return s; }
            if (positions(nd.a) == 0) return build(nd.a, exit);
            const int entry = make(kSplit), x = make(kSplit);
            int last = entry;
            for (int32_t i = 0; i < nd.min && !full; i++) {
                int bx;
                const int s = build(nd.a, &bx);
                nfa[last].out1 = s;
                last = bx;
                if (nd.max < 0 && i == nd.min - 1) {   // no upper bound: the last mandatory copy may be entered again
                    const int loop = make(kSplit);
                    nfa[bx].out1 = loop; nfa[loop].out1 = s;
                    last = make(kSplit);
                    nfa[loop].out2 = last;
                }
            }
            if (nd.max < 0 && nd.min == 0) {   // a star: entry -> body -> back to a split that re-enters or leaves
                int bx;
                const int sp = make(kSplit), s = build(nd.a, &bx);
                nfa[last].out1 = sp; nfa[sp].out1 = s; nfa[bx].out1 = sp;
                last = make(kSplit);
                nfa[sp].out2 = last;
            }
            for (int32_t i = nd.min; nd.max >= 0 && i < nd.max && !full; i++) {   // optional copies: each may leave for the exit
                int bx;
                const int sp = make(kSplit), s = build(nd.a, &bx);
                nfa[last].out1 = sp; nfa[sp].out1 = s; nfa[sp].out2 = x;
                last = bx;
            }
            nfa[last].out1 = x;
            *exit = x;
            return entry;
        }
        }
        *exit = 0;
        return 0;
    }
    std::map<ByteSet, size_t> seen;
    size_t intern(const ByteSet& s) {
        auto it = seen.find(s);
        if (it != seen.end()) return it->second;
        sets.push_back(s);
        return seen[s] = sets.size() - 1;
    }
};

// The closure of `seeds` under the moves that consume nothing -> the byte nodes reached, ascending; *match: kMatch was reached
struct Closure {
    const std::vector<NfaNode>& nfa;
    std::vector<uint32_t> stamp, stack;
    uint32_t now = 0;
    explicit Closure(const std::vector<NfaNode>& a) : nfa(a), stamp(a.size(), 0) {}
    void run(const std::vector<int32_t>& seeds, bool at_begin, bool at_end, std::vector<int32_t>* bytes, bool* match) {
        now++;
        bytes->clear();
        *match = false;
        stack.clear();
        auto push = [&](int32_t v) { if (v >= 0 && stamp[v] != now) { stamp[v] = now; stack.push_back(uint32_t(v)); } };
        for (int32_t s : seeds) push(s);
        while (!stack.empty()) {
            const NfaNode& nd = nfa[stack.back()];
            const int32_t id = int32_t(stack.back());
            stack.pop_back();
            switch (nd.kind) {
            case kSplit: push(nd.out1); push(nd.out2); break;
            case kByte: bytes->push_back(id); break;
            case kAtBegin: if (at_begin) push(nd.out1); break;
            case kAtEnd: if (at_end) push(nd.out1); break;
            case kMatch: *match = true; break;
            }
        }
        std::sort(bytes->begin(), bytes->end());
    }
};

}  // namespace regex_detail

// n expressions, back to back in `exprs` -> *out.  Returns 0, -kRegexErrArg or -kRegexErrUnsupported; where (may be NULL) receives the index of
// the expression and the byte offset in it.
inline int regex_compile(const uint8_t* exprs, const uint32_t* expr_len, size_t n, uint32_t flags, RegexProgram* out, uint64_t* where) {
    using namespace regex_detail;
    auto refuse = [&](int code, uint64_t i, uint64_t off) { if (where) { where[0] = i; where[1] = off; } return -code; };
    if (where) where[0] = where[1] = 0;
    if (n < 1 || n > kRegexMaxExprs || !expr_len || (flags & ~kRegexIgnoreCase)) return refuse(kRegexErrArg, n, 0);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (expr_len[i] > kRegexMaxExprLen) return refuse(kRegexErrArg, i, kRegexMaxExprLen);
        total += expr_len[i];
    }
    if (total && !exprs) return refuse(kRegexErrArg, 0, 0);
    const bool fold = (flags & kRegexIgnoreCase) != 0;

    // the NFA of the union: one start that splits to every expression, one match
    std::vector<NfaNode> nfa;
    std::vector<ByteSet> sets;
    nfa.push_back(NfaNode{kMatch});
    const int32_t match = 0;
    int32_t start = -1;
    uint64_t positions = 0;
    size_t at = 0;
    LitStrings lits;          // the alternation of the expressions' roots: the union of their F while every one has some
    bool lits_some = true;
    for (size_t i = 0; i < n; at += expr_len[i], i++) {
        static const uint8_t nothing = 0;
        Parser ps{total ? exprs + at : &nothing, expr_len[i], 0, fold, {}, {}, {}, {}};
        const int root = ps.parse();
        if (root < 0) return refuse(ps.err.code, i, ps.err.off);
        if (lits_some) {
            const LitNode ln = Literals{ps, fold}.of(root);
            lits_some = ln.f_some;
            if (lits_some) { lits = lit_union(lits, ln.F); lits_some = lits.size() <= kRegexMaxLiterals; }
        }
        Builder b{ps, nfa, sets, false, {}};
        positions += b.positions(root);
        if (positions > kRegexMaxPositions) return refuse(kRegexErrUnsupported, i, expr_len[i]);
        int x;
        const int s = b.build(root, &x);
        if (b.full) return refuse(kRegexErrUnsupported, i, expr_len[i]);
        nfa[x].out1 = match;
        NfaNode sp{kSplit};
        sp.out1 = s; sp.out2 = start;
        nfa.push_back(sp);
        start = int32_t(nfa.size()) - 1;
    }
    const uint64_t last = n - 1, last_len = expr_len[n - 1];

    // byte classes: two bytes are one class when every set holds both or neither
    uint8_t cls[256];
    uint32_t C0 = 1;
    memset(cls, 0, sizeof cls);
    for (const ByteSet& s : sets) {
        std::map<std::pair<uint32_t, bool>, uint32_t> split;
        uint8_t fresh[256];
        for (uint32_t b = 0; b < 256; b++) {
            auto key = std::make_pair(uint32_t(cls[b]), s.has(b));
            auto it = split.find(key);
            if (it == split.end()) it = split.emplace(key, uint32_t(split.size())).first;
            fresh[b] = uint8_t(it->second);
        }
        memcpy(cls, fresh, sizeof cls);
        C0 = uint32_t(split.size());
    }
    std::vector<uint8_t> rep_byte(C0, 0);
    for (uint32_t b = 256; b-- > 0;) rep_byte[cls[b]] = uint8_t(b);

    // subset construction.  A state is its byte nodes and whether the record matches if it ends here; raw state 0 is "matched".
    Closure cl(nfa);
    std::map<std::vector<int32_t>, uint32_t> ids;
    std::vector<std::vector<int32_t>> members;   // the byte nodes, ascending (raw state 0: none)
    std::vector<uint8_t> ends;
    std::vector<uint32_t> raw;                   // raw[s * C0 + c]
    members.emplace_back(); ends.push_back(1);
    std::vector<int32_t> seeds, bytes, scratch;
    auto state_of = [&](bool at_begin) -> int64_t {   // the state of `seeds`; -1 beyond the limit
        bool m = false, m_end = false;
        cl.run(seeds, at_begin, false, &bytes, &m);
        if (m) return 0;
        cl.run(seeds, at_begin, true, &scratch, &m_end);
        std::vector<int32_t> key = bytes;
        key.push_back(m_end ? -2 : -1);
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        if (members.size() >= kRegexMaxStates) return -1;
        ids.emplace(std::move(key), uint32_t(members.size()));
        members.push_back(bytes); ends.push_back(m_end ? 1 : 0);
        return int64_t(members.size()) - 1;
    };
    seeds.assign(1, start);
    const int64_t raw_start = state_of(true);
    for (size_t s = 0; s < members.size(); s++) {
        raw.resize((s + 1) * C0, 0);
        if (s == 0) continue;   // matched: absorbing
        const std::vector<int32_t> mine = members[s];
        for (uint32_t c = 0; c < C0; c++) {
            seeds.assign(1, start);   // the start set is injected again at every position
            for (int32_t v : mine) if (sets[nfa[v].set].has(rep_byte[c])) seeds.push_back(nfa[v].out1);
            const int64_t t = state_of(false);
            if (t < 0) return refuse(kRegexErrUnsupported, last, last_len);
            raw[s * C0 + c] = uint32_t(t);
        }
    }
    const uint32_t S0 = uint32_t(members.size());

    // Moore: refine {matched} | {end-accepting} | {the rest} until nothing splits
    std::vector<uint32_t> group(S0);
    for (uint32_t s = 0; s < S0; s++) group[s] = s == 0 ? 0 : ends[s] ? 1 : 2;
    for (size_t count = 0;;) {
        std::map<std::vector<uint32_t>, uint32_t> sig;
        std::vector<uint32_t> fresh(S0), key(C0 + 1);
        for (uint32_t s = 0; s < S0; s++) {
            key[0] = group[s];
            for (uint32_t c = 0; c < C0; c++) key[c + 1] = group[raw[s * C0 + c]];
            auto it = sig.find(key);
            if (it == sig.end()) it = sig.emplace(key, uint32_t(sig.size())).first;
            fresh[s] = it->second;
        }
        group.swap(fresh);
        if (sig.size() == count) break;
        count = sig.size();
    }
    // the numbering of mlz_stream_regex.h: dead 0, matched 1, the end-accepting states, the rest.  Dead and matched exist in every table.
    uint32_t G = 0;
    for (uint32_t g : group) G = std::max(G, g + 1);
    std::vector<uint32_t> member_of(G, 0);
    for (uint32_t s = S0; s-- > 0;) member_of[group[s]] = s;
    std::vector<int64_t> number(G, -1);
    number[group[0]] = 1;
    for (uint32_t g = 0; g < G; g++) {   // the dead state: accepts nowhere and never leaves
        const uint32_t s = member_of[g];
        if (s == 0 || ends[s]) continue;
        bool stays = true;
        for (uint32_t c = 0; c < C0 && stays; c++) stays = group[raw[s * C0 + c]] == g;
        if (stays) number[g] = 0;
    }
    uint32_t S = 2, n_end = 0;
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t s = 0; s < S0; s++) {
            const uint32_t g = group[s];
            if (number[g] >= 0 || (ends[s] != 0) != (pass == 0)) continue;
            number[g] = S++;
            n_end += pass == 0 ? 1 : 0;
        }
    // classes whose columns are equal are one
    std::map<std::vector<uint32_t>, uint32_t> cols;
    std::vector<uint32_t> col_of(C0), col(G);
    for (uint32_t c = 0; c < C0; c++) {
        for (uint32_t g = 0; g < G; g++) col[g] = uint32_t(number[group[raw[member_of[g] * C0 + c]]]);
        auto it = cols.find(col);
        if (it == cols.end()) it = cols.emplace(col, uint32_t(cols.size())).first;
        col_of[c] = it->second;
    }
    const uint32_t C = uint32_t(cols.size());
    if (S > kRegexMaxStates || uint64_t(256) + uint64_t(S) * C * 2 > kRegexLdsMax) return refuse(kRegexErrUnsupported, last, last_len);

    RegexProgram& pr = *out;
    pr.S = S; pr.C = C; pr.flags = flags; pr.n_end = n_end;
    pr.end_hi = (2 + n_end) * C;
    for (uint32_t b = 0; b < 256; b++) pr.cmap[b] = uint8_t(col_of[cls[b]]);
    pr.next.assign(size_t(S) * C, 0);
    for (uint32_t c = 0; c < C; c++) pr.next[C + c] = uint16_t(C);   // matched stays; dead's row is 0
    for (uint32_t g = 0; g < G; g++) {
        const uint32_t s = member_of[g], to = uint32_t(number[g]);
        if (to < 2) continue;
        for (uint32_t c = 0; c < C0; c++) pr.next[size_t(to) * C + col_of[c]] = uint16_t(uint32_t(number[group[raw[s * C0 + c]]]) * C);
    }
    pr.start = uint32_t(number[group[size_t(raw_start)]]) * C;
    pr.empty_ok = regex_verdict(pr.start, true, C, pr.end_hi) != 0;
    pr.literals = lits_some ? lits : LitStrings();
    return 0;
}

// 1 when some substring of record[0, len) is in the language, else 0: the rule the kernel runs, byte by byte
inline int regex_test(const RegexProgram& pr, const uint8_t* record, size_t len) {
    const uint32_t state = regex_walk(pr.next.data(), pr.cmap, pr.C, [&](uint64_t p) { return record[p]; }, 0, len, pr.start);
    return int(regex_verdict(state, true, pr.C, pr.end_hi));
}

}  // namespace mlz
