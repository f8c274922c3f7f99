// mlz_stream_records.h — the rules of the search that returns RECORDS (mlz_dev_reader_search_records, mlz_stream_records.hip.inc), shared with
// their host check (tools/stream_records_check.cpp, which runs them as plain loops).  Plain C++: compiles for the host alone and for gfx950.
//
// A record is a maximal run of decoded bytes without the delimiter.  The call looks at most W bytes (the reach) to either side of an occurrence:
//   window    of an occurrence at p: [lo, hi) = [max(0, p - W), min(size, p + L + W)) (records_window).  Windows of neighbouring occurrences
//             that touch or overlap merge (records_window_opens); merged windows are disjoint and ascending, and the read phase fetches them.
//   bounds    s = behind the last delimiter of [lo, p), or lo (cut left when lo > 0); e = the first delimiter of [p + L, hi), or hi (cut right
//             when hi < size): records_left, records_right.  A wavefront looks for the delimiter 1024 bytes a step, a 16-byte block of the
//             window buffer per lane (records_back_block, records_fwd_block, records_block_mask): blocks are aligned in MEMORY, a block that
//             the region covers wholly is one 16-byte load, a block at the region's edge is read bytewise, and nothing outside is read.
//   opening   occurrence i opens a record when i == 0 or s_i != s_{i-1} (records_opens); a record is [s of its first, e of its last occurrence).
//   caps      the first k records are written: the largest k <= rec_cap whose bytes sum to at most dst_cap (records_fits, per record).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MLZ_RECORDS_HD __host__ __device__ inline
#else
#define MLZ_RECORDS_HD inline
#endif

namespace mlz {

constexpr uint32_t kRecordsMaxReach = 1u << 20, kRecordsDefaultReach = 65536;
constexpr uint8_t kRecordCutLeft = 1, kRecordCutRight = 2;
constexpr uint64_t kRecordsMaxOccurrences = uint64_t(1) << 31;   // one wavefront per occurrence in one launch; a window's index is 32 bits
constexpr uint32_t kRecordsLanes = 64, kRecordsBlock = 16, kRecordsStep = kRecordsLanes * kRecordsBlock;

// What comes back to the host, once per call, behind the bounds: nothing per record or per occurrence does.
struct RecordsHeader { uint64_t records, bytes, flagged, k, written, pieces; };
// ... and in front of the read phase: the merged windows and their bytes (what the window buffer must hold)
struct RecordsWindows { uint64_t n, bytes; };
static_assert(sizeof(RecordsHeader) == 48 && sizeof(RecordsWindows) == 16, "records shared with the kernels");

// The window of an occurrence at p (p + L <= size).
struct RecordsWindow { uint64_t lo, hi; };
MLZ_RECORDS_HD RecordsWindow records_window(uint64_t p, uint32_t L, uint32_t W, uint64_t size) {
    return RecordsWindow{p > W ? p - W : 0, size - (p + L) > W ? p + L + W : size};
}
// The merge rule: the window of occurrence i > 0 starts a new merged window when it lies behind the previous one with a gap; touching windows merge.
MLZ_RECORDS_HD bool records_window_opens(uint64_t lo, uint64_t prev_hi) { return lo > prev_hi; }

// The bounds from what the look-around found.  found: a delimiter at `at`; else the region [lo, p) resp. [p + L, hi) holds none.
MLZ_RECORDS_HD uint64_t records_left(bool found, uint64_t at, uint64_t lo, uint8_t* cut) {
    if (found) return at + 1;
    if (lo > 0) *cut |= kRecordCutLeft;
    return lo;
}
MLZ_RECORDS_HD uint64_t records_right(bool found, uint64_t at, uint64_t hi, uint64_t size, uint8_t* cut) {
    if (found) return at;
    if (hi < size) *cut |= kRecordCutRight;
    return hi;
}

// The wavefront's look-around.  Coordinates y = x + mis, where x is a position of the decoded stream and mis the misalignment of the window
// buffer's byte for x = 0 (so y % 16 == 0 is a 16-byte boundary in memory).  Backwards from ytop = y(p) rounded up: lane 63 of step 0 has the
// block that ends at ytop; forwards from ybot = y(p + L) rounded down: lane 0 of step 0 has the block that starts at ybot.
MLZ_RECORDS_HD int64_t records_back_block(int64_t ytop, uint32_t step, uint32_t lane) { return ytop - (int64_t(step) * kRecordsLanes + (kRecordsLanes - lane)) * kRecordsBlock; }
MLZ_RECORDS_HD int64_t records_fwd_block(int64_t ybot, uint32_t step, uint32_t lane) { return ybot + (int64_t(step) * kRecordsLanes + lane) * kRecordsBlock; }
// Bit j: byte bs + j lies in the region [ylo, yhi) and is the delimiter.  vec(y, out): the 16 bytes of a block that lies wholly in the region;
// byte(y): one byte of the region.  Neither is called for anything else.
template <class Vec, class Byte>
MLZ_RECORDS_HD uint32_t records_block_mask(int64_t bs, int64_t ylo, int64_t yhi, uint8_t delim, Vec vec, Byte byte) {
    const int64_t b = bs > ylo ? bs : ylo, e = bs + kRecordsBlock < yhi ? bs + kRecordsBlock : yhi;
    uint32_t m = 0;
    if (b >= e) return 0;
    if (e - b == kRecordsBlock) {
        uint32_t v[4];
        vec(bs, v);
        const uint32_t d4 = uint32_t(delim) * 0x01010101u;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t x = v[k] ^ d4;   // a zero byte = a delimiter (bytes little-endian in the word)
            for (uint32_t j = 0; j < 4; j++) m |= ((x >> (8 * j)) & 0xffu) ? 0u : 1u << (4 * k + j);
        }
    } else {
        for (int64_t y = b; y < e; y++) m |= byte(y) == delim ? 1u << uint32_t(y - bs) : 0u;
    }
    return m;
}

// The same bounds as plain loops over a byte accessor at(x), x a position of the decoded stream: the contract's own words.
struct RecordsBounds { uint64_t s, e; uint8_t cut; };
template <class At>
MLZ_RECORDS_HD RecordsBounds records_bounds(At at, uint64_t p, uint32_t L, const RecordsWindow& w, uint64_t size, uint8_t delim) {
    RecordsBounds r{0, 0, 0};
    uint64_t x = p;
    while (x > w.lo && at(x - 1) != delim) x--;
    r.s = records_left(x > w.lo, x - 1, w.lo, &r.cut);
    x = p + L;
    while (x < w.hi && at(x) != delim) x++;
    r.e = records_right(x < w.hi, x, w.hi, size, &r.cut);
    return r;
}

// The opening rule.
MLZ_RECORDS_HD bool records_opens(uint64_t i, uint64_t s, uint64_t s_prev) { return i == 0 || s != s_prev; }

// The cut at the caps: record r (r + 1 records with it, `end` bytes with it) is written when both caps hold it.  The ends ascend, so the
// records that fit are the first k.
MLZ_RECORDS_HD bool records_fits(uint64_t r, uint64_t end, uint64_t rec_cap, uint64_t dst_cap) { return r < rec_cap && end <= dst_cap; }

// The copy: a record of more than short_max bytes goes in pieces of `piece` bytes, a workgroup each; others by 16 lanes.
MLZ_RECORDS_HD uint64_t records_pieces(uint64_t len, uint32_t short_max, uint32_t piece) { return len > short_max ? (len + piece - 1) / piece : 0; }

}  // namespace mlz
