// mlz_stream_regex.h — the rules of the grep for regular expressions over the record index (mlz_dev_reader_grep_regex, mlz_stream_regex.hip.inc),
// shared with the compiler (mlz_regex_compile.h) and their host check (tools/stream_regex_check.cpp, which runs them as plain loops).
// Plain C++: compiles for the host alone and for gfx950.
//
// The automaton is a SEARCH automaton over bytes: run over a record's bytes from left to right it decides "some substring of the record is in
// the language".  It is a table of S states by C byte classes, 16 bits an entry, and a class map of 256 bytes.
//   states    a state is kept PRE-MULTIPLIED by C, so that a step is one add and one read: next[state + cmap[byte]] (regex_step).  Numbering:
//             0       dead: no continuation can match (reachable for fully anchored expressions only).  Its row is all 0.
//             C       matched: a match has been completed that needs nothing more.  Absorbing: its row is all C.
//             [2 C, end_hi)   accepting at the end: the record matches if it ends here ($, and the empty record at the start state).
//             [end_hi, S C)   everything else.
//             A lane stops at dead or matched: state <= C (regex_stopped).  Both rows exist in every table, reachable or not.
//   verdict   matched, or at the record's end in an end-accepting state (regex_verdict).  The verdict of the empty record is that of the start state.
//   walk      regex_walk steps byte by byte; regex_walk_blocks is the same in 16-byte blocks of memory (coordinates y as in mlz_stream_record_index.h:
//             y % 16 == 0 is a 16-byte boundary, the group's bytes are the region [ylo, yhi)): a block that the region covers wholly is one load,
//             its bytes in front of `from` and at or behind `to` are masked out of the steps; a block at the region's edge is read bytewise;
//             nothing outside the region is read.
//   groups    the stream is decoded in groups that lie contiguous in the scratch; group g holds the decoded positions [first, first + n).  Its
//             records are r_lo = number(first) .. r_hi = number(first + n - 1) (regex_bounds).  Record r = [s, e) walks [max(s, first),
//             min(e, first + n)) (regex_lane).  s < first: the record crossed in, its lane starts from the carried state.  e >= first + n in a
//             group that is not the stream's last: the record goes on — also when only its delimiter lies beyond, it then finishes in the next
//             group without a step — and the lane writes the carry: record number, state, whether it is decided.  The state is the whole
//             summary of a record's prefix.  At most one record crosses a border; a record that crosses several rewrites the carry.  Group g
//             reads slot g % 2 and writes slot (g + 1) % 2, so the lane that reads and the lane that writes never meet in one launch.
//   marks     lane i of a group's launch takes record (r_lo & ~63) + i (regex_lane_record): a wavefront owns two whole words of the N-bit
//             bitmap; records below r_lo or above r_hi are idle lanes.  The two halves of a ballot go out as sel[w] |= bits by lanes 0 and 32.
//             Launches of consecutive groups are ordered on the stream and within a launch a word has one writer: no atomics.
//   longest   the longest record of an index is the maximum of rindex_span(j).len over j = 0 .. k (regex_longest).
// A record is walked by ONE lane, L dependent steps for L bytes: records beyond kRegexMaxRecord are not accepted (a cooperative path for longer
// records is out of scope).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_grep.h"

#if defined(__HIPCC__)
#define MLZ_REGEX_HD __host__ __device__ inline
#else
#define MLZ_REGEX_HD inline
#endif

namespace mlz {

constexpr uint32_t kRegexIgnoreCase = 1;                        // MLZ_REGEX_IGNORE_CASE
constexpr uint32_t kRegexMaxExprs = 256, kRegexMaxExprLen = 4096, kRegexMaxRepeat = 255, kRegexMaxDepth = 256;
constexpr uint32_t kRegexMaxPositions = 4096, kRegexMaxStates = 4096;
constexpr uint32_t kRegexLdsMax = 64u << 10;                    // class map + table: everything the mark kernel keeps in LDS
constexpr uint64_t kRegexMaxRecord = uint64_t(1) << 20;         // MLZ_REGEX_MAX_RECORD
constexpr uint32_t kRegexThreads = 256, kRegexLanes = 64, kRegexBlock = 16;
constexpr uint32_t kRegexMaxGrid = 2048;                        // workgroups of a mark launch; each takes slices of kRegexThreads records in turn
constexpr uint32_t kRegexLongestThreads = 256;

// The bytes of the image the kernel loads into LDS: the class map, then S * C entries; a multiple of 16
MLZ_REGEX_HD uint32_t regex_image_bytes(uint32_t S, uint32_t C) { return (256u + S * C * 2u + 15u) & ~15u; }

MLZ_REGEX_HD uint32_t regex_step(const uint16_t* next, const uint8_t* cmap, uint32_t state, uint8_t byte) { return next[state + cmap[byte]]; }
MLZ_REGEX_HD bool regex_stopped(uint32_t state, uint32_t C) { return state <= C; }
MLZ_REGEX_HD uint32_t regex_verdict(uint32_t state, bool at_end, uint32_t C, uint32_t end_hi) { return state == C || (at_end && state >= 2 * C && state < end_hi) ? 1u : 0u; }

// The state behind the bytes load(from) .. load(to - 1), or the dead / matched state the walk stopped at
template <class Load>
MLZ_REGEX_HD uint32_t regex_walk(const uint16_t* next, const uint8_t* cmap, uint32_t C, Load load, uint64_t from, uint64_t to, uint32_t state) {
    for (uint64_t p = from; p < to && !regex_stopped(state, C); p++) state = regex_step(next, cmap, state, load(p));
    return state;
}

// The same over the bytes y in [from, to) of the region [ylo, yhi), a 16-byte block of memory at a time.  vec(y, out): the four little-endian
// words of a block that lies wholly in the region; byte(y): one byte of the region.  Neither is called for anything else.
template <class Vec, class Byte>
MLZ_REGEX_HD uint32_t regex_walk_blocks(const uint16_t* next, const uint8_t* cmap, uint32_t C, Vec vec, Byte byte, int64_t ylo, int64_t yhi, int64_t from, int64_t to, uint32_t state) {
    for (int64_t y = from; y < to && !regex_stopped(state, C);) {
        const int64_t bs = y & ~int64_t(kRegexBlock - 1), e = bs + kRegexBlock < to ? bs + kRegexBlock : to;
        if (bs >= ylo && bs + int64_t(kRegexBlock) <= yhi) {
            uint32_t v[4];
            vec(bs, v);
            const uint32_t lo = uint32_t(y - bs), cnt = uint32_t(e - y);   // the block's bytes lo .. lo + cnt - 1 are the record's
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t j = 0; j < kRegexBlock; j++) {   // (a stopped state steps to itself: no test inside the block)
                const uint32_t ns = regex_step(next, cmap, state, uint8_t(v[j >> 2] >> (8 * (j & 3))));
                state = j - lo < cnt ? ns : state;
            }
        } else {
            for (int64_t q = y; q < e; q++) state = regex_step(next, cmap, state, byte(q));
        }
        y = bs + kRegexBlock;
    }
    return state;
}

// ---- the group rule ----

struct RegexGroup { uint64_t first, n; };                      // the decoded positions [first, first + n), n > 0
struct RegexBounds { uint64_t r_lo, r_hi; };                   // the group's records
struct RegexCarry { uint64_t rec; uint32_t state, decided; };  // the record that crosses a border
static_assert(sizeof(RegexGroup) == 16 && sizeof(RegexBounds) == 16 && sizeof(RegexCarry) == 16, "records shared with the kernels");

template <class At>
MLZ_REGEX_HD RegexBounds regex_bounds(At at, uint64_t k, RegexGroup g) { return RegexBounds{rindex_number(at, k, g.first), rindex_number(at, k, g.first + g.n - 1)}; }

// What record r does in group g: the positions it walks, whether it crossed in, whether it finishes here
struct RegexLane { uint64_t from, to; bool crossed_in, finishes; };
template <class At>
MLZ_REGEX_HD RegexLane regex_lane(At at, uint64_t k, uint64_t size, RegexGroup g, uint64_t r) {
    const RindexSpan sp = rindex_span(at, k, size, r);
    const uint64_t s = sp.off, e = sp.off + sp.len, gend = g.first + g.n;
    return RegexLane{s > g.first ? s : g.first, e < gend ? e : gend, s < g.first, e < gend || gend == size};
}

// One lane's whole work: walk(from, to, state) -> state is regex_walk or regex_walk_blocks over the decoded positions.  in: the slot this group
// reads.  finished: verdict is the record's; else carry is what the lane writes.
struct RegexLaneOut { bool finished; uint32_t verdict; RegexCarry carry; };
// ... from the positions ln says (regex_lane; the pruned grep's lanes come from regex_run_lane_of, mlz_stream_regex_prune.h)
template <class Walk>
MLZ_REGEX_HD RegexLaneOut regex_lane_result(RegexLane ln, uint64_t r, RegexCarry in, uint32_t start, uint32_t C, uint32_t end_hi, Walk walk) {
    uint32_t state = ln.crossed_in ? (in.rec == r ? in.state : 0u) : start;   // (a carry for another record: the host check's failure; dead here)
    if (ln.from < ln.to) state = walk(ln.from, ln.to, state);
    if (ln.finishes) return RegexLaneOut{true, regex_verdict(state, true, C, end_hi), RegexCarry{r, state, 1}};
    return RegexLaneOut{false, 0, RegexCarry{r, state, regex_stopped(state, C) ? 1u : 0u}};
}
template <class At, class Walk>
MLZ_REGEX_HD RegexLaneOut regex_run_lane(At at, uint64_t k, uint64_t size, RegexGroup g, uint64_t r, RegexCarry in, uint32_t start, uint32_t C, uint32_t end_hi, Walk walk) {
    return regex_lane_result(regex_lane(at, k, size, g, r), r, in, start, C, end_hi, walk);
}

// ---- the mark layout ----

MLZ_REGEX_HD uint64_t regex_launch_base(RegexBounds b) { return b.r_lo & ~uint64_t(kRegexLanes - 1); }
MLZ_REGEX_HD uint64_t regex_lane_record(RegexBounds b, uint64_t lane) { return regex_launch_base(b) + lane; }
// Slices of kRegexThreads lanes that cover the group's records
MLZ_REGEX_HD uint64_t regex_slices(RegexBounds b) { return (b.r_hi - regex_launch_base(b)) / kRegexThreads + 1; }
// The word a wavefront's half (0: lanes 0 .. 31, 1: lanes 32 .. 63) writes, from the record of its lane 0
MLZ_REGEX_HD uint64_t regex_word(uint64_t wave_first_record, uint32_t half) { return wave_first_record / 32 + half; }

// ---- the longest record ----

template <class At>
MLZ_REGEX_HD uint64_t regex_record_len(At at, uint64_t k, uint64_t size, uint64_t j) { return rindex_span(at, k, size, j).len; }   // j <= k; j == k: what follows the last delimiter
template <class At>
MLZ_REGEX_HD uint64_t regex_longest(At at, uint64_t k, uint64_t size) {
    uint64_t m = 0;
    for (uint64_t j = 0; j <= k; j++) { const uint64_t l = regex_record_len(at, k, size, j); m = l > m ? l : m; }
    return m;
}

}  // namespace mlz
