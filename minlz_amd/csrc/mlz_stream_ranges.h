// mlz_stream_ranges.h — the plan of a range read on the device-resident ReadSeeker (mlz_stream_ranges.hip.inc), shared with its host check
// (tools/stream_ranges_check.cpp): from the chunk list of an opened stream and a list of byte ranges to "which chunks, decoded where, in
// which groups, and which pieces are then copied where".  Plain C++: compiles for the host alone and for gfx950.
//
// Rules (a touched chunk = one that holds at least one requested byte; it is decoded whole, once, however many ranges touch it):
//   direct   a compressed chunk touched by exactly one range which covers it wholly decodes straight into its place in the destination;
//   scratch  any other touched compressed chunk decodes into the group's scratch, and one segment per (range, chunk) pair moves the wanted
//            part to the destination;
//   stored   a stored chunk (0x01) is never decoded and never visits the scratch: one segment per (range, chunk) pair reads its body where
//            it lies in the stream.
// The touched chunks run in groups, in stream order; a group is closed by the first chunk that takes its decoded bytes to
// kRangeGroupBytes or beyond (as the whole-stream call forms them), and the scratch is reused from group to group: it is bounded by a group
// plus one block, not by the number or the size of the ranges.
// The ranges are not sorted: a range finds its first chunk from its offset (a guess from the mean chunk size, corrected by a few steps; a
// binary search when the chunk sizes are far from even), which costs less than a sort for 100 000 short ranges and needs no search structure.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define MLZ_RANGE_HD __host__ __device__ inline
#else
#define MLZ_RANGE_HD inline
#endif

namespace mlz {

// A data chunk as the planners and the plan kernels see it: decoded bytes [out_off, out_off + n) of the stream's, its body in the stream; type
// 0x01 = stored.  (Named for the kernels of mlz_stream_ranges_dev.hip.inc, whose exported names carry it.)
struct RdevChunk { uint64_t out_off, body_off; uint32_t n, type; };
static_assert(sizeof(RdevChunk) == 24, "a record shared with the kernels");
struct ByteRange { uint64_t off, len, dst_off; };             // decoded bytes [off, off + len) -> destination [dst_off, dst_off + len)   (= mlz_range)

constexpr uint64_t kRangeGroupBytes = uint64_t(64) << 20;
constexpr int kRangeErrDstTooSmall = 6, kRangeErrArg = 8;     // MLZ_ERR_DST_TOO_SMALL, MLZ_ERR_ARG (include/minlz_hip.h), negated on return
constexpr uint8_t kRangeDirect = 0, kRangeScratch = 1, kRangeStored = 2;

struct RangeTouched { uint32_t chunk; uint8_t where; uint64_t at; };        // direct: offset in the destination; scratch: offset in the scratch; stored: 0
struct RangeSeg { uint32_t touched; uint64_t rel, dst_off, len; };          // bytes [rel, rel + len) of that touched chunk -> destination [dst_off, dst_off + len)
struct RangeGroup { size_t t0, t1, s0, s1; uint64_t scratch; };             // touched [t0, t1), segments [s0, s1), bytes of scratch it uses
struct RangePlan {
    std::vector<RangeTouched> touched;   // in stream order
    std::vector<RangeSeg> segs;          // group by group
    std::vector<RangeGroup> groups;
    uint64_t total = 0;                  // sum of the ranges' lengths
    uint64_t scratch_total = 0;          // decoded bytes that go through the scratch (all groups)
    uint64_t scratch_max = 0;            // the largest group's
};

// Groups of a list of `count` chunks with n_of(i) decoded bytes each: ends->at(g) = one past group g's last chunk.
template <class N> void range_group_ends(size_t count, N n_of, std::vector<size_t>* ends) {
    ends->clear();
    for (size_t i = 0; i < count;) {
        uint64_t acc = 0;
        while (i < count && acc < kRangeGroupBytes) acc += n_of(i++);
        ends->push_back(i);
    }
}

// The chunk that holds byte `off` (off < size, nck > 0): a guess from avg = max(1, size / nck), corrected by a few steps, else a binary search.
MLZ_RANGE_HD uint32_t range_locate(const RdevChunk* ck, uint32_t nck, uint64_t avg, uint64_t off) {
    const uint64_t q = off / avg;
    uint32_t g = q < nck - 1 ? uint32_t(q) : nck - 1;
    for (int s = 0; s < 16; s++) {
        if (ck[g].out_off > off) g--;                         // (chunk 0 starts at 0: never below it)
        else if (ck[g].out_off + ck[g].n <= off) g++;         // (the last chunk ends at size: never beyond it)
        else return g;
    }
    uint32_t lo = 0, hi = nck;   // the last chunk that starts at or in front of off (empty chunks share their successor's offset)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ck[mid].out_off <= off) lo = mid; else hi = mid;
    }
    return lo;
}

// ck[0, nck): the stream's data chunks in order (out_off running, the last one ends at `size`).  Returns 0, or -kRangeErrArg (a range runs
// beyond the decoded size; two destinations overlap), -kRangeErrDstTooSmall (a destination runs beyond dst_cap): the argument rules that need
// no device.  Empty ranges ask for nothing and overlap nothing.
inline int plan_ranges(const RdevChunk* ck, size_t nck, uint64_t size, const ByteRange* r, size_t nr, uint64_t dst_cap, RangePlan* p) {
    p->touched.clear(); p->segs.clear(); p->groups.clear();
    p->total = p->scratch_total = p->scratch_max = 0;
    for (size_t i = 0; i < nr; i++)
        if (r[i].off > size || r[i].len > size - r[i].off) return -kRangeErrArg;
    for (size_t i = 0; i < nr; i++)
        if (r[i].dst_off > dst_cap || r[i].len > dst_cap - r[i].dst_off) return -kRangeErrDstTooSmall;
    {   // destinations: in ascending order as given (packed output) one pass decides; else by a sort
        bool ordered = true;
        uint64_t end = 0;
        for (size_t i = 0; i < nr && ordered; i++) {
            if (!r[i].len) continue;
            ordered = r[i].dst_off >= end;
            end = r[i].dst_off + r[i].len;
        }
        if (!ordered) {
            std::vector<std::pair<uint64_t, uint64_t>> d;
            d.reserve(nr);
            for (size_t i = 0; i < nr; i++) if (r[i].len) d.emplace_back(r[i].dst_off, r[i].len);
            std::sort(d.begin(), d.end());
            for (size_t i = 1; i < d.size(); i++) if (d[i].first < d[i - 1].first + d[i - 1].second) return -kRangeErrArg;
        }
    }
    uint64_t total = 0;
    for (size_t i = 0; i < nr; i++) total += r[i].len;
    p->total = total;
    if (!total || !nck) return 0;

    const uint64_t avg = std::max<uint64_t>(1, size / nck);
    // pass 1: how many ranges touch each chunk, and whether one of them covers it wholly
    std::vector<uint32_t> cnt(nck, 0), first(nr, 0);
    std::vector<uint8_t> cov(nck, 0);
    size_t cmin = nck, cmax = 0;
    for (size_t i = 0; i < nr; i++) {
        if (!r[i].len) continue;
        const uint64_t off = r[i].off, end = off + r[i].len;
        size_t j = range_locate(ck, uint32_t(nck), avg, off);
        first[i] = uint32_t(j);
        cmin = std::min(cmin, j);
        for (; j < nck && ck[j].out_off < end; j++) {
            if (!ck[j].n) continue;
            cnt[j]++;
            if (off <= ck[j].out_off && end >= ck[j].out_off + ck[j].n) cov[j] = 1;
            cmax = std::max(cmax, j);
        }
    }

    // the touched chunks in stream order, their groups and places; a chunk's count, once used, gives way to its index in `touched`
    std::vector<uint32_t>& slot = cnt;
    std::vector<size_t> fill;
    {
        RangeGroup g{0, 0, 0, 0, 0};
        uint64_t acc = 0;
        size_t nseg = 0;
        auto close = [&] {
            g.t1 = p->touched.size(); g.s1 = nseg;
            p->groups.push_back(g);
            p->scratch_max = std::max(p->scratch_max, g.scratch);
            g = RangeGroup{g.t1, g.t1, nseg, nseg, 0};
            acc = 0;
        };
        for (size_t j = cmin; j <= cmax; j++) {
            if (!cnt[j]) continue;
            RangeTouched t{uint32_t(j), kRangeScratch, 0};
            if (ck[j].type == 0x01) t.where = kRangeStored;
            else if (cnt[j] == 1 && cov[j]) t.where = kRangeDirect;
            if (t.where == kRangeScratch) { t.at = g.scratch; g.scratch += ck[j].n; p->scratch_total += ck[j].n; }
            if (t.where != kRangeDirect) nseg += cnt[j];
            slot[j] = uint32_t(p->touched.size());
            p->touched.push_back(t);
            acc += ck[j].n;
            if (acc >= kRangeGroupBytes) close();
        }
        if (p->touched.size() > g.t0) close();
        p->segs.resize(nseg);
        fill.resize(p->groups.size());
        for (size_t k = 0; k < p->groups.size(); k++) fill[k] = p->groups[k].s0;
    }
    std::vector<uint32_t> group_of(p->touched.size());
    for (size_t k = 0; k < p->groups.size(); k++)
        for (size_t t = p->groups[k].t0; t < p->groups[k].t1; t++) group_of[t] = uint32_t(k);

    // pass 2: the direct chunks' places and the segments, group by group
    for (size_t i = 0; i < nr; i++) {
        if (!r[i].len) continue;
        const uint64_t off = r[i].off, end = off + r[i].len;
        for (size_t j = first[i]; j < nck && ck[j].out_off < end; j++) {
            if (!ck[j].n) continue;
            const uint32_t t = slot[j];
            RangeTouched& tc = p->touched[t];
            if (tc.where == kRangeDirect) { tc.at = r[i].dst_off + (ck[j].out_off - off); continue; }
            const uint64_t b = std::max(off, ck[j].out_off), e = std::min(end, ck[j].out_off + ck[j].n);
            p->segs[fill[group_of[t]]++] = RangeSeg{t, b - ck[j].out_off, r[i].dst_off + (b - off), e - b};
        }
    }
    return 0;
}

}  // namespace mlz
