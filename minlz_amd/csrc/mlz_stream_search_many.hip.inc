// mlz_stream_search_many.hip.inc — mlz_dev_reader_search_many: where each of up to 4096 byte strings occurs in a .mz stream that lies in HBM,
// in one call (included behind mlz_stream_search.hip.inc, whose per-handle tables, decode helpers and prefix kernel it uses).
//
// Plan (dev_reader_search_plan, mlz_stream_search.hip.inc: the plan of the search for one pattern with more patterns): the host computes every
// pattern's windows and their hashes (search_pattern_hashes: work proportional to the patterns); search_plan_kernel, one lane per (data chunk,
// pattern), probes the chunk's table and the next one's in every table set and applies the decoded-set rule of that pattern to ONE byte array:
// the union of the patterns' sets.  Only those nck bytes come back.  A pattern the tables cannot serve puts every chunk into the set, so the kernel is not run then.
// Scan: the set is decoded once, group by group (search_decode_run), and search_many_kernel<kSearchManyCount> examines each tile of start positions:
// the tile's bytes are staged in LDS, a lane walks 64 neighbouring positions, hashes the first m bytes of each to a bucket of the pattern
// index (heads and order in LDS) and verifies the bucket's patterns as far as the run holds their bytes.  Per-pattern counts gather in LDS and leave
// with one 64-bit atomic per non-zero counter.  Per group, search_prefix_kernel then continues the running sum over the tile counts
// and search_many_kernel<kSearchManyWrite> finds the pairs of the tiles below `cap` again, while the group's bytes are still in the scratch, and
// writes (position, pattern) in ascending order.
// The grep over the record index (mlz_stream_grep.hip.inc) runs the same walk in a third mode, once per group: every verified pair sets the bit
// of its position's record in a bitmap, and nothing is counted or written.
// The search over a batch of streams (mlz_stream_search_batch.hip.inc) runs the count and write modes over the tiles of all its streams and a
// fourth mode once per group: every verified pair sets the bit of its pattern in the row of the tile's stream, the presence matrix.

#include "mlz_stream_grep.h"

namespace mlz {

// What the scan needs of a SearchManyIndex, in device memory
struct SearchManyIx { const uint16_t* heads; const uint16_t* order; const uint32_t* off; const uint8_t* blob; uint32_t n, hb, m, lmax, blob_bytes, in_lds; };

constexpr uint32_t kSearchManyThreads = 256, kSearchManyPer = kSearchManyTile / kSearchManyThreads;
static_assert(kSearchManyPer == 64, "a lane's positions are one skew unit");
// The tile's bytes in LDS: a word of padding behind every 64 bytes, so that the lanes' words (17 apart) fall into different banks
__host__ __device__ constexpr uint32_t search_many_skew(uint32_t b) { return b + ((b >> 6) << 2); }
constexpr uint32_t kSearchManyTileLds = (search_many_skew(kSearchManyTile + kSearchMaxPattern + 8) + 8) & ~3u;
// LDS of one workgroup, in words: heads | order | per-pattern counters | scan | tile bytes | (pattern offsets | pattern bytes, when they fit)
constexpr uint32_t kSearchManyLdsBudget = 64u << 10;
struct SearchManyLds { uint32_t heads, order, counts, scan, tile, off, blob, words; };
__host__ __device__ inline SearchManyLds search_many_lds(uint32_t n, uint32_t hb, uint32_t blob_bytes, bool in_lds) {
    SearchManyLds l;
    uint32_t w = 0;
    l.heads = w; w += ((1u << hb) + 2) / 2;
    l.order = w; w += (n + 1) / 2;
    l.counts = w; w += n;
    l.scan = w; w += kSearchManyThreads;
    l.tile = w; w += kSearchManyTileLds / 4;
    l.off = l.blob = w;
    if (in_lds) { w += n + 1; l.blob = w; w += (blob_bytes + 3) / 4; }
    l.words = w;
    return l;
}

// The marking modes' arguments.  Records: the handle's record index D[0, k) and the bitmap of its records, a bit each.  Streams (the search
// over a batch of streams, mlz_stream_search_batch.hip.inc): every tile's stream and the presence matrix `bits`, a row of `words` words per stream
struct SearchManyMark { const uint64_t* D; uint64_t k; uint32_t* bits; const uint32_t* tile_stream; uint32_t words; };
enum { kSearchManyCount = 0, kSearchManyWrite = 1, kSearchManyMarkRecords = 2, kSearchManyMarkStreams = 3 };

// One workgroup per tile.  kSearchManyCount: counts[tile] = the tile's pairs, pat_counts[p] += pattern p's.  kSearchManyWrite: the pairs of a tile
// whose first pair lies below cap go to out_pos / out_which from prefix[tile] on, as far as they lie below cap.  kSearchManyMarkRecords: bit
// number(position) of mk.bits is set for every pair (mlz_stream_grep.h, mark); the tile's two record numbers lie in the scan words of the LDS
// layout, which this mode does not use otherwise, and every lane reads the same two words (a broadcast).
// kSearchManyMarkStreams: bit p of row mk.tile_stream[tile] of mk.bits is set for every pair of pattern p; the tile's stream is one uniform
// load for the workgroup, and nothing is counted or written.
// kFold (MLZ_SEARCH_IGNORE_CASE): the index and the blob are those of the folded patterns, and the tile's bytes are folded a word at a time
// (search_fold4) on their way from the scratch into LDS, so the key and the verify loop compare folded bytes at no cost per position.
template <int kMode, bool kFold>
__global__ __launch_bounds__(kSearchManyThreads) void search_many_kernel(const uint8_t* __restrict__ scratch, const SearchTile* __restrict__ tiles, uint32_t tile0, SearchManyIx ix,
                                                                         uint32_t* __restrict__ tile_counts, unsigned long long* __restrict__ pat_counts,
                                                                         const uint64_t* __restrict__ prefix, uint64_t cap, uint64_t* __restrict__ out_pos,
                                                                         uint32_t* __restrict__ out_which, SearchManyMark mk) {
    constexpr bool kWrite = kMode == kSearchManyWrite;
    extern __shared__ uint32_t lds[];
    const uint32_t tid = threadIdx.x, tile = tile0 + blockIdx.x;
    uint64_t first = 0;
    if (kWrite) {
        first = prefix[tile];
        if (first >= cap) return;   // (the whole workgroup)
    }
    const SearchManyLds l = search_many_lds(ix.n, ix.hb, ix.blob_bytes, ix.in_lds != 0);
    uint16_t *heads = reinterpret_cast<uint16_t*>(lds + l.heads), *order = reinterpret_cast<uint16_t*>(lds + l.order);
    uint32_t *counts = lds + l.counts, *scan = lds + l.scan, *tw = lds + l.tile;
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(tw);
    const SearchTile t = tiles[tile];
    for (uint32_t i = tid; i < (1u << ix.hb) + 1; i += kSearchManyThreads) heads[i] = ix.heads[i];
    for (uint32_t i = tid; i < ix.n; i += kSearchManyThreads) order[i] = ix.order[i];
    if (kMode == kSearchManyCount) for (uint32_t i = tid; i < ix.n; i += kSearchManyThreads) counts[i] = 0;
    const uint32_t* off = ix.off;
    const uint8_t* blob = ix.blob;
    if (ix.in_lds) {
        uint32_t *lo = lds + l.off, *lb = lds + l.blob;
        for (uint32_t i = tid; i < ix.n + 1; i += kSearchManyThreads) lo[i] = ix.off[i];
        const uint32_t* gb = reinterpret_cast<const uint32_t*>(ix.blob);   // (the blob's room is a whole number of words)
        for (uint32_t i = tid; i < (ix.blob_bytes + 3) / 4; i += kSearchManyThreads) lb[i] = gb[i];
        off = lo;
        blob = reinterpret_cast<const uint8_t*>(lb);
    }
    // the bytes the tile's pairs can touch: count - 1 + lmax from src_off on, as far as the run has them in this group; whole words from
    // the word that holds src_off (the scratch has room behind its last chunk)
    const uint32_t shift = uint32_t(t.src_off) & 3;
    uint32_t avail = t.count - 1 + ix.lmax;
    if (avail > t.hi_end) avail = t.hi_end;
    const uint32_t* gw = reinterpret_cast<const uint32_t*>(scratch + (t.src_off - shift));
    for (uint32_t w = tid; w < (shift + avail + 3) / 4; w += kSearchManyThreads) tw[w + (w >> 4)] = kFold ? search_fold4(gw[w]) : gw[w];
    if (kMode == kSearchManyMarkRecords && tid < 2 && t.count)   // two lanes: the numbers of the tile's first and last start position (below 2^32)
        scan[tid] = uint32_t(rindex_number([&](uint64_t j) { return mk.D[j]; }, mk.k, tid ? t.gpos + t.count - 1 : t.gpos));
    __syncthreads();
    auto byte_at = [&](uint32_t i) { return uint32_t(tb[search_many_skew(shift + i)]); };
    const uint32_t i0 = tid * kSearchManyPer, i1 = i0 + kSearchManyPer < t.count ? i0 + kSearchManyPer : t.count;
    auto walk = [&](auto emit) {
        if (i0 >= i1) return;
        uint32_t w = byte_at(i0) | byte_at(i0 + 1) << 8 | byte_at(i0 + 2) << 16;   // (bytes beyond the tile's: in the LDS array, masked off or unused)
        for (uint32_t i = i0; i < i1; i++) {
            w |= byte_at(i + 3) << 24;
            const uint32_t h = search_many_key(w, ix.m, ix.hb);
            w >>= 8;
            for (uint32_t e = heads[h], e1 = heads[h + 1]; e < e1; e++) {
                const uint32_t p = order[e], po = off[p], L = off[p + 1] - po, end = i + L;
                if (end > t.hi_end) continue;   // (the run ends in this group, in front of the pattern's end)
                uint32_t j = 0;
                while (j < L && byte_at(i + j) == blob[po + j]) j++;
                if (j == L) emit(i, p);
            }
        }
    };
    auto plus = [](uint32_t x, uint32_t y) { return x + y; };
    uint32_t cnt = 0;
    if (kMode == kSearchManyMarkRecords) {
        const GrepNarrow nr{scan[0], scan[1]};
        walk([&](uint32_t i, uint32_t) {
            const uint64_t r = grep_number_between([&](uint64_t j) { return mk.D[j]; }, nr, t.gpos + i);
            uint32_t* word = mk.bits + (r >> 5);
            const uint32_t bit = 1u << (uint32_t(r) & 31);
            // the test in front of the atomic: a record with thousands of occurrences costs a few atomics, not thousands; a stale word only costs another
            if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
        });
    } else if (kMode == kSearchManyMarkStreams) {
        uint32_t* row = mk.bits + size_t(mk.tile_stream[tile]) * mk.words;   // (the same address in every lane: read once)
        walk([&](uint32_t, uint32_t p) {
            uint32_t* word = row + (p >> 5);
            const uint32_t bit = 1u << (p & 31);
            // as for the records: a stream with thousands of occurrences of one key costs a few atomics
            if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
        });
    } else if (kMode == kSearchManyCount) {
        walk([&](uint32_t, uint32_t p) { atomicAdd(&counts[p], 1u); cnt++; });
        uint32_t total;
        wg_scan<kSearchManyThreads>(cnt, scan, tid, plus, &total);   // (its barriers also settle the counters)
        if (tid == 0) tile_counts[tile] = total;
        for (uint32_t i = tid; i < ix.n; i += kSearchManyThreads) {
            const uint32_t v = counts[i];
            if (v) atomicAdd(&pat_counts[i], static_cast<unsigned long long>(v));
        }
    } else {
        walk([&](uint32_t, uint32_t) { cnt++; });
        uint64_t at = first + wg_scan<kSearchManyThreads>(cnt, scan, tid, plus);
        walk([&](uint32_t i, uint32_t p) {
            if (at < cap) { out_pos[at] = t.gpos + i; out_which[at] = p; }
            at++;
        });
    }
}

}  // namespace mlz

namespace {

// The pattern list of a call: at most MLZ_SEARCH_MAX_PATTERNS patterns of 1 .. kSearchMaxPattern bytes, back to back in `patterns`.  Returns
// their bytes together or -MLZ_ERR_ARG; whether n == 0 is an error is the caller's rule.
int64_t search_pattern_list(const uint8_t* patterns, const uint32_t* pattern_len, size_t n) {
    if (n > MLZ_SEARCH_MAX_PATTERNS || (n && (!patterns || !pattern_len))) return -MLZ_ERR_ARG;
    int64_t blob = 0;
    for (size_t i = 0; i < n; i++) {
        if (pattern_len[i] == 0 || pattern_len[i] > mlz::kSearchMaxPattern) return -MLZ_ERR_ARG;
        blob += pattern_len[i];
    }
    return blob;
}

// The many-pattern scan of one call, host side: prepare (fold and index, once), take (from the caller's carves, which the caller then ensures),
// clear and send (behind that ensure), then one launch per method over the tiles [t0, t1) of a group whose bytes are in the scratch (DESIGN.md).
struct SearchManyScan {
    bool fold = false, counting = false;
    size_t n = 0;
    const uint8_t* patterns = nullptr;   // folded under `fold` (then in `folded`), else the caller's
    std::vector<uint8_t> folded;
    mlz::SearchManyIndex index;
    // The counting regions of the workspace (c->d_rplan): per-pattern counts | total | (the index) | tile counts | prefix; taken only when `counting`
    Region<unsigned long long> pat_counts{};
    Region<uint64_t> total{}, prefixes{};
    Region<uint32_t> tile_counts{};
    void prepare(uint32_t flags, const uint8_t* pats, const uint32_t* pattern_len, size_t n_patterns) {
        fold = (flags & MLZ_SEARCH_IGNORE_CASE) != 0; n = n_patterns; patterns = pats;
        if (fold) {
            size_t bytes = 0;
            for (size_t i = 0; i < n; i++) bytes += pattern_len[i];
            folded.resize(bytes);
            for (size_t i = 0; i < bytes; i++) folded[i] = mlz::search_fold(pats[i]);
            patterns = folded.data();
        }
        mlz::search_many_index(patterns, pattern_len, n, &index);
    }
    // nt: the tiles to count, or NULL where nothing is counted (the grep).  The index goes up as one block: heads | order | offsets | pattern bytes
    void take(Carve* cv, Carve* pin, const size_t* nt) {
        counting = nt != nullptr;
        up = Carve{};   // (the batch search takes anew for its second pass)
        if (counting) { pat_counts = cv->take<unsigned long long>(n); total = cv->take<uint64_t>(2); }
        u_heads = up.take<uint16_t>(index.heads.size()); u_order = up.take<uint16_t>(n);
        u_off = up.take<uint32_t>(n + 1); u_blob = up.take<uint8_t>(size_t(index.off[n]) + 4);
        dev = cv->take<uint8_t>(up.bytes); host = pin->take<uint8_t>(up.bytes);
        if (counting) { tile_counts = cv->take<uint32_t>(*nt, 4); prefixes = cv->take<uint64_t>(*nt); }
    }
    int clear(mlz_ctx* c, hipStream_t sm) const {
        if (!counting) return 0;
        HIPCHK(c, hipMemsetAsync(pat_counts.at(c->d_rplan.p), 0, n * sizeof(unsigned long long), sm));
        HIPCHK(c, hipMemsetAsync(total.at(c->d_rplan.p), 0, 16, sm));
        return 0;
    }
    // The upload; d_tiles and sm are those of every launch that follows
    int send(mlz_ctx* ctx, hipStream_t stream, const mlz::SearchTile* tiles) {
        c = ctx; sm = stream; d_tiles = tiles;
        const uint32_t blob_bytes = index.off[n];
        void *d_up = dev.at(c->d_rplan.p), *h_up = host.at(c->pinned2);
        std::memcpy(u_heads.at(h_up), index.heads.data(), index.heads.size() * 2);
        std::memcpy(u_order.at(h_up), index.order.data(), n * 2);
        std::memcpy(u_off.at(h_up), index.off.data(), (n + 1) * 4);
        std::memcpy(u_blob.at(h_up), patterns, blob_bytes);
        const bool in_lds = mlz::search_many_lds(uint32_t(n), index.hb, blob_bytes, true).words * 4 <= mlz::kSearchManyLdsBudget;
        ix = mlz::SearchManyIx{u_heads.at(d_up), u_order.at(d_up), u_off.at(d_up), u_blob.at(d_up), uint32_t(n), index.hb, index.m, index.lmax, blob_bytes, in_lds ? 1u : 0u};
        lds_bytes = mlz::search_many_lds(uint32_t(n), index.hb, blob_bytes, in_lds).words * 4;
        HIPCHK(c, hipMemcpyAsync(d_up, h_up, up.bytes, hipMemcpyHostToDevice, sm));
        return 0;
    }
    void count(size_t t0, size_t t1) const { launch<mlz::kSearchManyCount>(t0, t1, 0, nullptr, nullptr, mlz::SearchManyMark{}); }
    void prefix(size_t t0, size_t t1) const {
        void* ws = c->d_rplan.p;
        hipLaunchKernelGGL(mlz::search_prefix_kernel, dim3(1), dim3(1024), 0, sm, tile_counts.at(ws), uint32_t(t0), uint32_t(t1), prefixes.at(ws), total.at(ws));
    }
    void write(size_t t0, size_t t1, uint64_t cap, uint64_t* out_pos, uint32_t* out_which) const { launch<mlz::kSearchManyWrite>(t0, t1, cap, out_pos, out_which, mlz::SearchManyMark{}); }
    void mark_records(size_t t0, size_t t1, const uint64_t* D, uint64_t k, uint32_t* bits) const { launch<mlz::kSearchManyMarkRecords>(t0, t1, 0, nullptr, nullptr, mlz::SearchManyMark{D, k, bits, nullptr, 0}); }
    void mark_streams(size_t t0, size_t t1, const uint32_t* ts, uint32_t* bits, uint32_t words) const { launch<mlz::kSearchManyMarkStreams>(t0, t1, 0, nullptr, nullptr, mlz::SearchManyMark{nullptr, 0, bits, ts, words}); }
    // What the counting calls run per group: count, the running prefix continued and, while the group's bytes are still in the scratch, the pairs below cap
    void count_prefix_write(size_t t0, size_t t1, uint64_t cap, uint64_t* out_pos, uint32_t* out_which) const {
        count(t0, t1);
        prefix(t0, t1);
        if (cap) write(t0, t1, cap, out_pos, out_which);
    }
private:
    mlz_ctx* c = nullptr;   // (c, sm and d_tiles: send's)
    hipStream_t sm = nullptr;
    const mlz::SearchTile* d_tiles = nullptr;
    Carve up;
    Region<uint16_t> u_heads{}, u_order{};
    Region<uint32_t> u_off{};
    Region<uint8_t> u_blob{}, dev{}, host{};   // the block's layout, and its copies in the workspace and the pinned buffer
    mlz::SearchManyIx ix{};
    uint32_t lds_bytes = 0;
    // Every launch of search_many_kernel.  The counting regions go to every mode of a counting call (NULL otherwise); a mode reads only its own arguments
    template <int kMode>
    void launch(size_t t0, size_t t1, uint64_t cap, uint64_t* out_pos, uint32_t* out_which, const mlz::SearchManyMark& mk) const {
        void* ws = counting ? c->d_rplan.p : nullptr;
        const auto kernel = fold ? mlz::search_many_kernel<kMode, true> : mlz::search_many_kernel<kMode, false>;
        hipLaunchKernelGGL(kernel, dim3(uint32_t(t1 - t0)), dim3(mlz::kSearchManyThreads), lds_bytes, sm, c->d_range.as<uint8_t>(), d_tiles, uint32_t(t0), ix, ws ? tile_counts.at(ws) : nullptr,
                           ws ? pat_counts.at(ws) : nullptr, ws ? static_cast<const uint64_t*>(prefixes.at(ws)) : nullptr, cap, out_pos, out_which, mk);
    }
};

int64_t dev_reader_search_many_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* patterns, const uint32_t* pattern_len, size_t n, uint64_t* d_counts,
                                      uint64_t* d_offsets, uint32_t* d_which, uint64_t cap, uint64_t* stats) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    search_begin(rd, stats);
    HIPCHK(c, hipSetDevice(c->device));
    auto nothing = [&]() -> int64_t {   // no chunk to scan: every count is 0
        if (d_counts) {
            HIPCHK(c, hipMemsetAsync(d_counts, 0, n * 8, sm));
            HIPCHK(c, hipStreamSynchronize(sm));
        }
        return 0;
    };
    if (nck == 0) return nothing();
    SearchManyScan scan;
    scan.prepare(flags, patterns, pattern_len, n);
    std::vector<uint8_t> take(nck, 0);
    size_t n_take = 0;
    const int64_t pr = dev_reader_search_plan(rd, sm, flags, scan.patterns, scan.index.off, n, &take, &n_take, stats, true);
    if (pr) return pr;
    if (n_take == 0) return nothing();
    SearchDecode sd;
    search_decode_plan(rd->chunks, take, n_take, scan.index.lmin, scan.index.lmax, mlz::kSearchManyTile, &sd);
    const size_t nt = sd.lay.tiles.size();
    if (nt > 0x7fffffffu) return -MLZ_ERR_ARG;
    Carve cv, pin;   // workspace: the scan's (per-pattern counts | total | the index | tile counts | prefix) | the decode's; pinned: the index | the decode's
    scan.take(&cv, &pin, &nt);
    int e = search_decode_ready(rd->ctx, rd->chunks, &sd, &cv, &pin);
    if (e) return e;
    { WorkspaceOrder order(c, sm); }
    if ((e = scan.clear(c, sm)) || (e = scan.send(c, sm, sd.tiles.at(c->d_rplan.p)))) return e;
    const int64_t r = search_decode_run(rd->ctx, rd->d_src, rd->chunks, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, &sd, [&](size_t, size_t t0, size_t t1) {
        scan.count_prefix_write(t0, t1, cap, d_offsets, d_which);
        return 0;
    });
    if (r < 0) return r;
    if (d_counts) HIPCHK(c, hipMemcpyAsync(d_counts, scan.pat_counts.at(c->d_rplan.p), n * 8, hipMemcpyDeviceToDevice, sm));
    if ((e = fetch(c, sm, c->pinned2, scan.total.at(c->d_rplan.p), 8))) return e;
    return int64_t(*static_cast<const uint64_t*>(c->pinned2));
}

}  // namespace

extern "C" int64_t mlz_dev_reader_search_many(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns,
                                              uint64_t* d_counts, uint64_t* d_offsets, uint32_t* d_which, size_t cap, uint64_t* stats) {
    if (!rd || search_pattern_list(patterns, pattern_len, n_patterns) < 0 || (cap && (!d_offsets || !d_which))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (n_patterns && ((d_counts && !on_device(c, d_counts)) || (cap && (!on_device(c, d_offsets) || !on_device(c, d_which))))) return -MLZ_ERR_ARG;
    if (n_patterns == 0) {
        search_begin(rd, stats);
        return 0;
    }
    begin_decode_call(c);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_search_many_locked(rd, sm, flags, patterns, pattern_len, n_patterns, d_counts, d_offsets, d_which, uint64_t(cap), stats));
}
