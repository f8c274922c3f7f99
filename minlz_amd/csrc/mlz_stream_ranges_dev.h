// mlz_stream_ranges_dev.h — the rules of the range read whose ranges lie in DEVICE memory (mlz_dev_reader_read_device,
// mlz_stream_ranges_dev.hip.inc), shared with their host check (tools/stream_ranges_dev_check.cpp, which runs them as plain loops and compares
// the outcome with plan_ranges of mlz_stream_ranges.h).  Plain C++: compiles for the host alone and for gfx950.
//
// The plan has the host planner's outcome (direct / scratch / stored, the touched chunks in stream order, groups of about 64 MiB) but no step
// of it loops over a range's chunks, and nothing per range visits the host:
//   per range   bounds; the first and the last touched chunk (rdev_range_rule); +1 / +index at `first` and -1 / -index behind `last` in two
//               difference arrays over the chunk index (modulo 2^32: where the count is 1 the index sum IS the index); the exclusive prefix
//               of the lengths (the packed destination) and of the numbers of long pieces, per block of kRdevBlock ranges + block sums.
//   per chunk   a running sum of the difference arrays gives "how many ranges touch it" and, where that is one, which (rdev_chunk_rule); the
//               touched chunks are compacted in stream order (RdevTouched, 16 bytes each: what the host reads back).
//   host        groups and scratch offsets of the touched chunks (rdev_host_places): O(touched chunks).  One RdevPlace per touched chunk goes up.
//   gather      per group, straight from the range arrays: a range of up to `short_max` bytes walks from its first chunk; a longer one is cut
//               into pieces of `piece` bytes of the RANGE, each found from the piece prefix (rdev_piece_owner) and located on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_ranges.h"

namespace mlz {

struct RdevHeader { uint64_t total, pieces; uint32_t err, touched; uint64_t pad; };   // the first read-back: sum of the lengths, long pieces, "a range is out of bounds", touched chunks
struct RdevTouched { uint32_t chunk, where; uint64_t at; };            // the second read-back.  direct: offset in the destination; else 0
struct RdevPlace { uint64_t base; uint32_t group, where; };            // the upload, per touched chunk.  scratch: offset in the scratch
static_assert(sizeof(RdevHeader) == 32 && sizeof(RdevTouched) == 16 && sizeof(RdevPlace) == 16, "records shared with the kernels");

constexpr uint32_t kRdevBlock = 1024;                        // ranges per block of the per-range pass: one prefix block
constexpr uint64_t kRdevMaxRanges = uint64_t(1) << 31;       // a range's index is a 32-bit addend
constexpr uint64_t kRdevMaxGrid = (uint64_t(1) << 31) - 1;   // long pieces + ranges / 16 of one call: one launch

MLZ_RANGE_HD uint64_t rdev_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~uint64_t(0) : a + b; }   // (2^31 lengths below 2^63 can pass 2^64)

// One range.  bad: it runs beyond the decoded size.  live: it asks for a byte; then [j0, j1] are its first and last touched chunk (both
// non-empty; empty ones between them are "touched" by the difference arrays and dropped by rdev_chunk_rule).  pieces: its long pieces.
struct RdevRange { uint32_t j0, j1; uint64_t pieces; bool bad, live; };
MLZ_RANGE_HD RdevRange rdev_range_rule(const RdevChunk* ck, uint32_t nck, uint64_t size, uint64_t avg, uint64_t off, uint64_t len, uint32_t short_max, uint32_t piece) {
    RdevRange r{0, 0, 0, false, false};
    r.bad = off > size || len > size - off;
    r.live = !r.bad && len > 0 && nck > 0;
    if (!r.live) return r;
    const uint64_t last = off + len - 1;
    r.j0 = range_locate(ck, nck, avg, off);
    r.j1 = last < ck[r.j0].out_off + ck[r.j0].n ? r.j0 : range_locate(ck, nck, avg, last);
    r.pieces = len > short_max ? (len + piece - 1) / piece : 0;
    return r;
}

// Where range i's bytes start in the packed destination: its block's offset + its offset in the block.
MLZ_RANGE_HD uint64_t rdev_start(const uint64_t* block_off, const uint64_t* local, uint64_t i) { return block_off[i / kRdevBlock] + local[i]; }

// One chunk with the running sums of the difference arrays at its index: false = not touched (or empty).  off / len: the range arrays.
MLZ_RANGE_HD bool rdev_chunk_rule(const RdevChunk& c, uint32_t j, uint32_t cnt, uint32_t who, const uint64_t* off, const uint64_t* len, const uint64_t* block_off,
                                 const uint64_t* local, RdevTouched* t) {
    if (!cnt || !c.n) return false;
    t->chunk = j; t->where = kRangeScratch; t->at = 0;
    if (c.type == 0x01) t->where = kRangeStored;
    else if (cnt == 1 && off[who] <= c.out_off && off[who] + len[who] >= c.out_off + c.n) {
        t->where = kRangeDirect;
        t->at = rdev_start(block_off, local, who) + (c.out_off - off[who]);
    }
    return true;
}

// The range that owns long piece p (p < the number of pieces): the last block, then the last range in it, whose exclusive piece prefix is at
// most p (ranges and blocks without pieces share their successor's prefix and are stepped over).  n: ranges, nb: blocks.  *q: the piece's
// index in its range.
MLZ_RANGE_HD uint64_t rdev_piece_owner(const uint64_t* piece_block_off, const uint32_t* piece_local, uint64_t n, uint64_t nb, uint64_t p, uint64_t* q) {
    uint64_t lo = 0, hi = nb;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (piece_block_off[mid] <= p) lo = mid; else hi = mid;
    }
    const uint64_t b = lo, rel = p - piece_block_off[b];
    lo = b * kRdevBlock;
    hi = lo + kRdevBlock < n ? lo + kRdevBlock : n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (piece_local[mid] <= rel) lo = mid; else hi = mid;
    }
    *q = rel - piece_local[lo];
    return lo;
}

// The part of a range (decoded bytes from `off` on, packed at `start`) inside the window [wb, we) that lies in the non-empty chunk c with
// place pl, for the gather of group `group`: false = nothing to copy here (another group's chunk, a direct one, no common byte).
// *src: offset in the stream (*from_stream) or in the scratch; *dst: offset in the destination.
MLZ_RANGE_HD bool rdev_intersect(const RdevChunk& c, const RdevPlace& pl, uint32_t group, uint64_t off, uint64_t start, uint64_t wb, uint64_t we, uint64_t* src,
                                uint64_t* dst, uint32_t* n, bool* from_stream) {
    if (pl.group != group || pl.where == kRangeDirect) return false;
    const uint64_t b = wb > c.out_off ? wb : c.out_off, e = we < c.out_off + c.n ? we : c.out_off + c.n;
    if (b >= e) return false;
    *from_stream = pl.where == kRangeStored;
    *src = (*from_stream ? c.body_off : pl.base) + (b - c.out_off);
    *dst = start + (b - off);
    *n = uint32_t(e - b);   // (at most a chunk)
    return true;
}

// Host: groups (range_group_ends over the touched chunks, n_of(chunk) = its decoded bytes) and scratch offsets.  places[t].base: a scratch chunk's
// offset in its group's scratch; group_copies[g]: the group has a chunk that is not direct (something to gather).
template <class N>
void rdev_host_places(const RdevTouched* t, size_t nt, N n_of, std::vector<RdevPlace>* places, std::vector<size_t>* gend, std::vector<uint8_t>* group_copies, uint64_t* scratch_total,
                      uint64_t* scratch_max) {
    range_group_ends(nt, [&](size_t k) { return uint64_t(n_of(t[k].chunk)); }, gend);
    places->resize(nt);
    group_copies->assign(gend->size(), 0);
    *scratch_total = *scratch_max = 0;
    for (size_t g = 0, k = 0; g < gend->size(); g++) {
        uint64_t used = 0;
        for (; k < (*gend)[g]; k++) {
            (*places)[k] = RdevPlace{0, uint32_t(g), t[k].where};
            if (t[k].where == kRangeScratch) { (*places)[k].base = used; used += n_of(t[k].chunk); }
            if (t[k].where != kRangeDirect) (*group_copies)[g] = 1;
        }
        *scratch_total += used;
        *scratch_max = std::max(*scratch_max, used);
    }
}

}  // namespace mlz
