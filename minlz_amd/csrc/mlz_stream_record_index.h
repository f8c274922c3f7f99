// mlz_stream_record_index.h — the rules of the record index (mlz_dev_reader_index_records and the calls that read it,
// mlz_stream_record_index.hip.inc), shared with their host check (tools/stream_record_index_check.cpp, which runs them as plain loops).
// Plain C++: compiles for the host alone and for gfx950.
//
// The index is D[0] < D[1] < ... < D[k-1]: the positions of all bytes of the decoded stream that equal the delimiter, 8 bytes each.
//   records   N = k + 1 when size > 0 and the last byte is no delimiter, else k (rindex_records).  Record r is [start(r), end(r)):
//             start(0) = 0, start(r) = D[r-1] + 1; end(r) = D[r] for r < k, end(k) = size (rindex_span).  Empty records count.
//   numbers   the record number of position p < size is the count of D[j] < p (rindex_number): a delimiter has the number of the record it ends.
//   scan      the bytes of a group lie side by side in memory.  Coordinates y = x + mis, where x is an offset into the group's bytes and mis
//             the misalignment of its first byte (so y % 16 == 0 is a 16-byte boundary in memory); the region is [mis, mis + n).  A workgroup
//             of kRindexThreads lanes takes a tile of kRindexTile bytes of y in kRindexSteps steps, a 16-byte block per lane and step
//             (rindex_block_at).  A block that the region covers wholly is one 16-byte load, a block at the region's edge is read bytewise,
//             nothing outside is read (rindex_block_mask).  The delimiter test is exact per byte (rindex_zero_bytes: no carry crosses a byte).
//   ranks     delimiters are numbered in memory order: tile, step, wavefront, lane, bit.  A hit's rank is its tile's base + the hits of the
//             (step, wavefront) slots in front of its own (rindex_slot) + the hits of the lower lanes of its wavefront + the lower bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MLZ_RINDEX_HD __host__ __device__ inline
#else
#define MLZ_RINDEX_HD inline
#endif

namespace mlz {

constexpr uint32_t kRindexBlock = 16, kRindexLanes = 64, kRindexWaves = 4, kRindexThreads = kRindexLanes * kRindexWaves;
constexpr uint32_t kRindexStepBytes = kRindexThreads * kRindexBlock, kRindexSteps = 16, kRindexTile = kRindexStepBytes * kRindexSteps;   // 4 KiB a step, 64 KiB a tile
constexpr uint32_t kRindexSlots = kRindexSteps * kRindexWaves;
constexpr uint64_t kRindexMaxItems = uint64_t(1) << 31;   // record numbers or positions of one call: one launch, a lane each
constexpr uint64_t kRindexNoRecord = ~uint64_t(0);
static_assert(kRindexTile == 65536 && kRindexSlots == kRindexLanes, "one wavefront scans a tile's slots");

// What comes home from the spans and the numbers kernel: the sum of the lengths (resp. the positions inside the stream), "an index is >= N"
struct RindexSums { uint64_t total, bad; };
static_assert(sizeof(RindexSums) == 16, "a record shared with the kernels");

// Bit 7 of every byte of x that is zero, and of no other.  (x & 0x7f) + 0x7f stays below 0x100 in every byte, so no carry crosses into the
// byte above — the shorter (x - 0x01010101) & ~x & 0x80808080 lets a borrow mark the byte above a zero byte when that byte is 0x01.
MLZ_RINDEX_HD uint32_t rindex_zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
// Bit j (j < 4): byte j of the word (little-endian) is the delimiter; d4 = the delimiter in all four bytes.  The product moves bit 8 j to
// bit 24 + j; its other terms land on bits 3, 10, 11, 17, 18, 19 or beyond bit 31, so nothing carries.
MLZ_RINDEX_HD uint32_t rindex_word_mask(uint32_t word, uint32_t d4) { return (((rindex_zero_bytes(word ^ d4) >> 7) * 0x01020408u) >> 24) & 0xfu; }
MLZ_RINDEX_HD uint32_t rindex_splat(uint8_t delim) { return uint32_t(delim) * 0x01010101u; }
// The 16 bytes of a block as four little-endian words -> a 16-bit mask
MLZ_RINDEX_HD uint32_t rindex_vec_mask(const uint32_t* v, uint32_t d4) {
    return rindex_word_mask(v[0], d4) | rindex_word_mask(v[1], d4) << 4 | rindex_word_mask(v[2], d4) << 8 | rindex_word_mask(v[3], d4) << 12;
}

// The block of lane `tid` in step `step` of tile `tile`, in y
MLZ_RINDEX_HD int64_t rindex_block_at(uint64_t tile, uint32_t step, uint32_t tid) { return int64_t(tile) * kRindexTile + int64_t(step) * kRindexStepBytes + int64_t(tid) * kRindexBlock; }
MLZ_RINDEX_HD uint64_t rindex_tiles(uint64_t mis, uint64_t n) { return n ? (mis + n + kRindexTile - 1) / kRindexTile : 0; }

// Bit j: byte bs + j lies in the region [ylo, yhi) and is the delimiter.  vec(y, out): the 16 bytes of a block that lies wholly in the region;
// byte(y): one byte of the region.  Neither is called for anything else.
template <class Vec, class Byte>
MLZ_RINDEX_HD uint32_t rindex_block_mask(int64_t bs, int64_t ylo, int64_t yhi, uint8_t delim, Vec vec, Byte byte) {
    const int64_t b = bs > ylo ? bs : ylo, e = bs + kRindexBlock < yhi ? bs + kRindexBlock : yhi;
    if (b >= e) return 0;
    if (e - b == kRindexBlock) {
        uint32_t v[4];
        vec(bs, v);
        return rindex_vec_mask(v, rindex_splat(delim));
    }
    uint32_t m = 0;
    for (int64_t y = b; y < e; y++) m |= byte(y) == delim ? 1u << uint32_t(y - bs) : 0u;
    return m;
}

MLZ_RINDEX_HD uint32_t rindex_popcount(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint32_t(__popc(m));
#else
    uint32_t c = 0;
    for (; m; m &= m - 1) c++;
    return c;
#endif
}

// The slot of (step, wavefront) in a tile's 64 slot totals: slots are summed up in this order
MLZ_RINDEX_HD uint32_t rindex_slot(uint32_t step, uint32_t wave) { return step * kRindexWaves + wave; }

// The hits of one block, from `rank` on: put(rank, y) for every set bit, ascending; rank < limit is the caller's bound on the table
template <class Put>
MLZ_RINDEX_HD void rindex_emit(uint32_t mask, uint64_t rank, uint64_t limit, int64_t bs, Put put) {
    for (uint32_t j = 0; mask; j++, mask >>= 1)
        if (mask & 1u) { if (rank < limit) put(rank, bs + int64_t(j)); rank++; }
}

// N from k, the size and whether the last byte is a delimiter (D[k-1] == size - 1)
MLZ_RINDEX_HD uint64_t rindex_records(uint64_t k, uint64_t size, bool last_is_delim) { return size > 0 && !last_is_delim ? k + 1 : k; }

// Record r <= N: its first byte and its length.  at(j) = D[j].  r == N (one past the last record): the empty span at the end, which
// mlz_dev_reader_record_range uses for a count of 0.
struct RindexSpan { uint64_t off, len; };
template <class At>
MLZ_RINDEX_HD RindexSpan rindex_span(At at, uint64_t k, uint64_t size, uint64_t r) {
    const uint64_t s = r == 0 ? 0 : r <= k ? at(r - 1) + 1 : size;
    const uint64_t e = r < k ? at(r) : size;
    return RindexSpan{s < e ? s : e, s < e ? e - s : 0};
}

// The record number of position p < size: how many D[j] < p (a lower bound by bisection)
template <class At>
MLZ_RINDEX_HD uint64_t rindex_number(At at, uint64_t k, uint64_t p) {
    uint64_t lo = 0, hi = k;   // D[j] < p for j < lo, D[j] >= p for j >= hi
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (at(mid) < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace mlz
