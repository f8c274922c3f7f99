// mlz_stream_regex_prune.h — the rules of the regex grep that prunes by search tables (mlz_dev_reader_grep_regex_pruned,
// mlz_stream_regex_prune.hip.inc), shared with the compiler (mlz_regex_compile.h) and their host check (tools/regex_prune_check.cpp, which
// runs them as plain loops).  Plain C++: compiles for the host alone and for gfx950.
//
//   literals  the compiler derives a set L of byte strings from the syntax tree such that every record the expression matches holds some l of L
//             (under kRegexIgnoreCase: the record with A - Z folded to a - z does, and L is stored folded).  L may be empty: none.  Per node two
//             values: E, the finite set of ALL strings the node matches, or unknown; F, the best set of required factors, or none.  A byte set is
//             first mapped to its lower-case image under the flag (regex_lit_fold).
//               byte set S     E = the one-byte strings if |S| <= kRegexLitSmallSet, else unknown; F = E.
//               ^ $ empty      E = {""}; F = none.
//               concatenation  left to right with a running set X = {""}: while E(child) is known, |X| |E(child)| <= kRegexLitProduct
//                              (regex_lit_product_fits) and no product string exceeds kRegexMaxLiteralLen, X = X x E(child); otherwise X becomes
//                              a candidate and a new X starts from E(child), or from {""} if that is unknown.  Every child's F is a candidate when
//                              the child has been taken, the final X is the last one.  E = X if the run was never closed, else unknown; F = the best.
//               alternation    E = the union of the branches' E if all are known and it holds at most kRegexLitProduct strings; F = the union of
//                              the branches' F if every branch has one and it holds at most kRegexMaxLiterals strings.
//               a{m,n}         m = 0: F = none, E = E(a) + {""} if n = 1 and E(a) is known (and the cap holds).  m >= 1: E(a)^m is built as m
//                              products, each within the caps; F = the better of F(a) and E(a)^m; E = E(a)^m if m = n.
//               n expressions  an alternation of their roots.
//             Best (regex_lit_better): a set that holds the empty string is no candidate; the larger shortest string wins, then the fewer strings,
//             then the leftmost.  Sets hold no string twice; L is sorted bytewise, a prefix in front of its extensions.
//   widen     an occurrence of a literal in a taken chunk proves only that SOME record touching the chunk may match, and the automaton needs that
//             record whole: per taken chunk [first, last] the span from the start of the record that holds `first` to the end of the record that
//             holds `last` (regex_widen: two bisections); every chunk that intersects such a span joins the list (regex_widen_take).  One step
//             suffices: a record that touches an originally taken chunk lies inside it or holds its first or its last byte.
//   runs      the widened list is decoded in groups, a group's chunks side by side in the scratch.  A run is a maximal piece of decoded stream
//             whose chunks are all in the list; it may go on from one group into the next, so a group holds PIECES of runs (RegexRun: decoded
//             [first, end) at scratch offset `at`), of which only the first can continue a run of the group in front (the run then began at
//             head_first) and only the last can go on in the next group (the run then ends at tail_end) (regex_run_table).
//   lanes     the lanes of a group's launch cover the records from that of its first decoded byte to that of its last in the layout of
//             mlz_stream_regex.h.  Record r = [s, e) looks for the piece with the largest first <= s, or the group's first piece (it crossed in).
//             It is evaluated iff one run holds it whole: run.first <= s < run.end and e <= run.end (so an empty record needs its delimiter
//             inside the run), and the piece holds something of [s, e].  It then walks [max(s, first), min(e, end)), takes the carry when
//             s < first and finishes when e < end or the run ends with the piece; else it writes the carry (regex_run_lane_of).  A record that a
//             run cuts is not evaluated: it touches no originally taken chunk, so it cannot match.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mlz_stream_regex.h"

namespace mlz {

constexpr uint32_t kRegexMaxLiterals = 64;        // strings of L, and of a union of F
constexpr uint32_t kRegexMaxLiteralLen = 256;     // bytes of a string: the search's pattern limit (kSearchMaxPattern)
constexpr uint32_t kRegexLitProduct = 16;         // strings of an E, and of a product
constexpr uint32_t kRegexLitSmallSet = 4;         // bytes of a set that is still spelled out
constexpr uint32_t kRegexMaxRuns = 2048;          // pieces of one group's run table: 48 KiB of LDS behind the automaton's image
constexpr uint32_t kRegexWidenThreads = 64;

MLZ_REGEX_HD uint8_t regex_lit_fold(uint8_t b) { return b >= 'A' && b <= 'Z' ? uint8_t(b + 32) : b; }
MLZ_REGEX_HD bool regex_lit_product_fits(uint64_t a, uint64_t b) { return a * b <= kRegexLitProduct; }
// Is candidate a (its shortest string, its strings) better than b, which stands to its left
MLZ_REGEX_HD bool regex_lit_better(uint64_t a_shortest, uint64_t a_count, uint64_t b_shortest, uint64_t b_count) {
    return a_shortest != b_shortest ? a_shortest > b_shortest : a_count < b_count;
}

// ---- widen ----

struct RegexTaken { uint64_t first, last; };      // a taken chunk's first and last decoded position (the chunk has bytes)
struct RegexWiden { uint64_t start, end; };       // the positions its records need: [start, end)
static_assert(sizeof(RegexTaken) == 16 && sizeof(RegexWiden) == 16, "records shared with the kernels");

template <class At>
MLZ_REGEX_HD RegexWiden regex_widen(At at, uint64_t k, uint64_t size, RegexTaken t) {
    const RindexSpan a = rindex_span(at, k, size, rindex_number(at, k, t.first)), b = rindex_span(at, k, size, rindex_number(at, k, t.last));
    return RegexWiden{a.off, b.off + b.len};
}

// take[c] |= chunk c has bytes and intersects a span.  The chunks lie in stream order (off_of(c), n_of(c): where chunk c's decoded bytes lie and
// how many), the spans in the order of their chunks, so both their starts and their ends ascend: one pass.  -> how many chunks are taken now.
template <class Off, class N>
size_t regex_widen_take(size_t n_chunks, Off off_of, N n_of, const RegexWiden* spans, size_t n_spans, std::vector<uint8_t>* take) {
    size_t c = 0, done = 0;   // c: the first chunk that may still intersect a span; done: one past the last chunk the spans in front have looked at
    for (size_t i = 0; i < n_spans; i++) {
        const RegexWiden w = spans[i];
        while (c < n_chunks && uint64_t(off_of(c)) + uint64_t(n_of(c)) <= w.start) c++;
        for (done = done > c ? done : c; done < n_chunks && uint64_t(off_of(done)) < w.end; done++) if (n_of(done)) (*take)[done] = 1;
    }
    size_t n = 0;
    for (size_t j = 0; j < n_chunks; j++) n += (*take)[j] ? 1 : 0;
    return n;
}

// ---- runs ----

struct RegexRun { uint64_t first, end, at; };     // a piece of a run in a group: decoded [first, end), its bytes at scratch + at
static_assert(sizeof(RegexRun) == 24, "a record shared with the kernels");
// Group g's pieces are runs[r0, r1); its bytes are scratch[0, used); its records are those of [runs[r0].first, runs[r1 - 1].end)
struct RegexRunGroup { size_t r0, r1; uint64_t head_first, tail_end, used; };
struct RegexRunTable { std::vector<RegexRun> runs; std::vector<RegexRunGroup> groups; std::vector<uint64_t> at; };

// The run table of a decode list of `count` chunks with bytes, in stream order (off_of(i), n_of(i)), cut into groups at gend; at[i]: chunk i's
// place in the scratch, the chunks of a group side by side from 0 on.
template <class Off, class N>
RegexRunTable regex_run_table(size_t count, const std::vector<size_t>& gend, Off off_of, N n_of) {
    RegexRunTable t;
    t.at.resize(count);
    std::vector<uint64_t> run_first(count), run_end(count);   // of the run that holds chunk i
    for (size_t i = 0; i < count; i++) run_first[i] = i && uint64_t(off_of(i - 1)) + uint64_t(n_of(i - 1)) == uint64_t(off_of(i)) ? run_first[i - 1] : uint64_t(off_of(i));
    for (size_t i = count; i-- > 0;) run_end[i] = i + 1 < count && uint64_t(off_of(i)) + uint64_t(n_of(i)) == uint64_t(off_of(i + 1)) ? run_end[i + 1] : uint64_t(off_of(i)) + uint64_t(n_of(i));
    for (size_t g = 0, i = 0; g < gend.size(); g++) {
        const size_t end = gend[g] < count ? gend[g] : count;
        RegexRunGroup gr{t.runs.size(), t.runs.size(), 0, 0, 0};
        for (; i < end; i++) {
            const uint64_t off = uint64_t(off_of(i)), n = uint64_t(n_of(i));
            t.at[i] = gr.used;
            if (t.runs.size() > gr.r0 && t.runs.back().end == off) t.runs.back().end = off + n;
            else t.runs.push_back(RegexRun{off, off + n, gr.used});
            gr.used += n;
            if (t.runs.size() == gr.r0 + 1 && t.runs.back().first == off) gr.head_first = run_first[i];
            gr.tail_end = run_end[i];
        }
        gr.r1 = t.runs.size();
        t.groups.push_back(gr);
    }
    return t;
}

// ---- lanes ----

// What record [s, e) does in a group whose pieces are run_at(0 .. n_runs): idle, or the RegexLane of mlz_stream_regex.h and its piece
struct RegexRunLane { bool active; uint32_t piece; RegexLane lane; };
template <class RunAt>
MLZ_REGEX_HD RegexRunLane regex_run_lane_of(RunAt run_at, uint32_t n_runs, uint64_t head_first, uint64_t tail_end, uint64_t s, uint64_t e) {
    const RegexRunLane idle{false, 0, RegexLane{0, 0, false, false}};
    if (n_runs == 0) return idle;
    uint32_t lo = 0, hi = n_runs;   // run_at(j).first <= s for j < lo, > s for j >= hi
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (run_at(mid).first <= s) lo = mid + 1; else hi = mid;
    }
    const uint32_t i = lo ? lo - 1 : 0;
    const RegexRun p = run_at(i);
    const uint64_t run_first = i == 0 ? head_first : p.first, run_end = i + 1 == n_runs ? tail_end : p.end;
    if (!(run_first <= s && s < run_end && e <= run_end)) return idle;   // no run holds the record whole
    if (!(s < p.end && e >= p.first)) return idle;                       // the record lies in another group's piece of the run
    return RegexRunLane{true, i, RegexLane{s > p.first ? s : p.first, e < p.end ? e : p.end, s < p.first, e < p.end || run_end == p.end}};
}

}  // namespace mlz
