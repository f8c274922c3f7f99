// mlz_stream_grep.h — the rules of the grep over the record index (mlz_dev_reader_grep_records, mlz_stream_grep.hip.inc), shared with their
// host check (tools/stream_grep_check.cpp, which runs them as plain loops).  Plain C++: compiles for the host alone and for gfx950.
//
// N records (N < 2^32) are one bit each, 32 to a word, record r = bit r % 32 of word r / 32; W = grep_words(N).
//   mark      an occurrence at position p sets bit number(p) (rindex_number).  A tile of start positions [p0, p1] finds number(p0) and
//             number(p1) once (grep_narrow) and every hit bisects between the two (grep_number_between): the same value as the full bisection.
//   select    S = the marked words, or their complement with the bits at and beyond N cleared (grep_select_word, grep_valid_bits).
//   context   record r is in C when the nearest selected record at or below it lies at most `after` records away, or the nearest at or above
//             it at most `before`.  Inside a word that is a smear of S's bits (grep_smear_up, grep_smear_down, at most 31 places); from the
//             words below comes the nearest selected record of all lower words and from above the nearest of all higher words — a forward
//             and a backward maximum scan over one value per word (grep_last_key, grep_first_key: 0 = none) —, each of which covers a run
//             of the word's low resp. high bits (grep_context_word).  Nothing depends on the sizes of before and after.
//   compact   the rank of a record of C is the set bits of C in front of it: a word's exclusive prefix of popcounts plus the lower bits.
//             Ranks below rec_cap are written (number, kind = "in S"); every record adds end - start to the bytes of all, the written ones
//             also to the bytes written (grep_emit_word).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_record_index.h"

namespace mlz {

constexpr uint32_t kGrepInvert = 16;                       // MLZ_GREP_INVERT
constexpr uint64_t kGrepMaxRecords = uint64_t(1) << 32;    // N below this: record numbers, ranks and the scans' keys are 32 bits
constexpr uint32_t kGrepScanThreads = 1024, kGrepCompactThreads = 256;

// What comes home, once per call: R, |S|, the bytes of the written records, the bytes of all R records
struct GrepTotals { uint64_t records, selected, written, bytes; };
static_assert(sizeof(GrepTotals) == 32, "a record shared with the kernels");

MLZ_RINDEX_HD uint64_t grep_words(uint64_t N) { return (N + 31) / 32; }
// The words of lane `tid` of the select pass, one workgroup of kGrepScanThreads lanes over W words: slabs in lane order
struct GrepSlab { uint64_t b, e; };
MLZ_RINDEX_HD GrepSlab grep_slab(uint64_t W, uint32_t tid) {
    const uint64_t per = (W + kGrepScanThreads - 1) / kGrepScanThreads;
    const uint64_t b = tid * per < W ? tid * per : W;
    return GrepSlab{b, W - b > per ? b + per : W};
}
// The bits of word w that are records: all 32, fewer in the last word when N % 32 != 0, none beyond
MLZ_RINDEX_HD uint32_t grep_valid_bits(uint64_t w, uint64_t N) {
    const uint64_t lo = w * 32;
    if (lo >= N) return 0;
    return N - lo >= 32 ? ~uint32_t(0) : (uint32_t(1) << uint32_t(N - lo)) - 1;
}
// before / after as the rules use them: values >= N behave like N
MLZ_RINDEX_HD uint64_t grep_clamp(uint64_t reach, uint64_t N) { return reach < N ? reach : N; }

// The record numbers of a tile's first and last start position: every position between them has a number in [lo, hi]
struct GrepNarrow { uint64_t lo, hi; };
template <class At>
MLZ_RINDEX_HD GrepNarrow grep_narrow(At at, uint64_t k, uint64_t p_first, uint64_t p_last) {
    return GrepNarrow{rindex_number(at, k, p_first), rindex_number(at, k, p_last)};
}
// rindex_number(at, k, p) for p_first <= p <= p_last, bisecting between the tile's two values only: D[j] < p_first <= p for j < lo and
// D[j] >= p_last >= p for j >= hi, which is rindex_number's invariant
template <class At>
MLZ_RINDEX_HD uint64_t grep_number_between(At at, GrepNarrow nr, uint64_t p) {
    uint64_t lo = nr.lo, hi = nr.hi;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (at(mid) < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

MLZ_RINDEX_HD uint32_t grep_select_word(uint32_t marked, uint64_t w, uint64_t N, bool invert) { return (invert ? ~marked : marked) & grep_valid_bits(w, N); }

// x with every set bit repeated in the n places above (below) it, n <= 31: OR of x << j (x >> j) for j = 0 .. n, by doubling
MLZ_RINDEX_HD uint32_t grep_smear_up(uint32_t x, uint32_t n) {
    for (uint32_t done = 0; done < n;) {
        const uint32_t step = done + 1 < n - done ? done + 1 : n - done;
        x |= x << step;
        done += step;
    }
    return x;
}
MLZ_RINDEX_HD uint32_t grep_smear_down(uint32_t x, uint32_t n) {
    for (uint32_t done = 0; done < n;) {
        const uint32_t step = done + 1 < n - done ? done + 1 : n - done;
        x |= x >> step;
        done += step;
    }
    return x;
}

MLZ_RINDEX_HD uint32_t grep_high_bit(uint32_t x) {   // x != 0
    uint32_t b = 31;
    while (!(x >> b)) b--;
    return b;
}
MLZ_RINDEX_HD uint32_t grep_low_bit(uint32_t x) {   // x != 0
    uint32_t b = 0;
    while (!((x >> b) & 1u)) b++;
    return b;
}
// The scans' keys of one word of S, 0 = the word selects nothing; both scans take the maximum.
//   forward:  1 + the word's highest selected record   (the larger, the nearer below a later word)
//   backward: N - the word's lowest selected record     (the larger, the nearer above an earlier word); N < 2^32, so both fit 32 bits
MLZ_RINDEX_HD uint32_t grep_last_key(uint32_t s, uint64_t w) { return s ? uint32_t(w * 32 + grep_high_bit(s) + 1) : 0; }
MLZ_RINDEX_HD uint32_t grep_first_key(uint32_t s, uint64_t w, uint64_t N) { return s ? uint32_t(N - (w * 32 + grep_low_bit(s))) : 0; }

// Word w of C.  s: word w of S; below: the maximum of grep_last_key over the words < w; above: the maximum of grep_first_key over the words > w;
// before, after: clamped (grep_clamp).
MLZ_RINDEX_HD uint32_t grep_context_word(uint32_t s, uint64_t w, uint32_t below, uint32_t above, uint64_t before, uint64_t after, uint64_t N) {
    const uint64_t lo = w * 32;
    uint32_t c = grep_smear_up(s, uint32_t(after < 31 ? after : 31)) | grep_smear_down(s, uint32_t(before < 31 ? before : 31));
    if (below) {   // records lo .. p + after behind the selected record p < lo
        const uint64_t top = uint64_t(below) - 1 + after;
        if (top >= lo) c |= top - lo >= 31 ? ~uint32_t(0) : (uint32_t(2) << uint32_t(top - lo)) - 1;
    }
    if (above) {   // records q - before .. lo + 31 in front of the selected record q > lo + 31
        const uint64_t q = N - above, bot = q > before ? q - before : 0;
        if (bot <= lo + 31) c |= bot <= lo ? ~uint32_t(0) : ~uint32_t(0) << uint32_t(bot - lo);
    }
    return c & grep_valid_bits(w, N);
}

// The records of one word of C from `rank` on: put(rank, record, kind) for every rank < rec_cap, ascending; len(record) = end - start.
// Adds every record's length to *bytes and the written ones' to *written.
template <class Len, class Put>
MLZ_RINDEX_HD void grep_emit_word(uint32_t c, uint32_t s, uint64_t w, uint64_t rank, uint64_t rec_cap, Len len, Put put, uint64_t* written, uint64_t* bytes) {
    for (uint32_t b = 0; c; b++, c >>= 1) {
        if (!(c & 1u)) continue;
        const uint64_t r = w * 32 + b, l = len(r);
        *bytes += l;
        if (rank < rec_cap) { put(rank, r, uint8_t((s >> b) & 1u)); *written += l; }
        rank++;
    }
}

}  // namespace mlz
