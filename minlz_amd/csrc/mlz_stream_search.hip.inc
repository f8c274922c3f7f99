// mlz_stream_search.hip.inc — mlz_dev_reader_search: where a byte string occurs in a .mz stream that lies in HBM (included at the end of
// mlz_hip.hip, behind the device-resident ReadSeeker whose handle, chunk-list decode and scratch it uses).
//
// The stream's block search tables (SPEC_SEARCH.md: an info chunk 0x44 behind the identifier, a bit table 0x45 in front of a block; table
// types 1 to 4) say which blocks can hold the pattern's windows of M bytes — with a prefix table (types 2 and 3) the windows behind one
// of the stream's prefix bytes, which are the only ones its blocks index; with a long-prefix table (type 4) the groups of E + 1 windows behind
// an occurrence of the stream's prefix in the pattern, probed group by group.  Per handle, once: search_info_kernel reads the info chunk, search_locate_kernel
// (one lane per data chunk) hops over the chunk headers between the previous data chunk's end and its own start to the first table chunk
// that fits, and the existing CRC pass checks the tables.  Per call: the host hashes the pattern's windows (search_pattern_hashes),
// search_plan_kernel looks them up in every table of every table set (one set for a stream's inline tables, up to four for an attached
// sidecar: mlz_stream_sidecar.hip.inc) and applies the rule of mlz_stream_search.h (search_decoded_mark_all); one byte per chunk comes back:
// the set of chunks to decode.  The search for many patterns plans through the same function.  The scratch decode (ScratchDecode,
// mlz_stream_walk.hip.inc) brings exactly those into the scratch, chunks that are neighbours in the stream side by side, and search_scan_kernel marks the occurrences of every
// run in a bitmap (one bit per decoded byte of the set) and counts them per tile.  search_prefix_kernel's scan over the tile counts and search_write_kernel then
// put the smallest `cap` positions out in ascending order.  The call's body ends at the prefix kernel (dev_reader_search_scan_locked); the write and
// the total's way home are steps of their own, so that the search for records (mlz_stream_records.hip.inc) can size its buffer by the total first.
// MLZ_SEARCH_IGNORE_CASE: the pattern is folded once on the host, the plan probes the windows' case variants (search_plan_kernel<true>) and the scan folds
// every data byte in a register (search_scan_kernel<true>); the <false> instantiations are the code without the flag.

namespace mlz {

using SearchInfo = SearchConfig;   // (T, M, B, prefix field) of an info chunk; ok = 0: none that is usable
struct SearchHop { uint64_t from, limit; };                               // where a lane starts to hop and the data chunk's body, which it never reaches

__device__ __forceinline__ bool search_is_data(uint8_t t) { return t >= 1 && t <= 3; }

__global__ __launch_bounds__(64) void search_info_kernel(const uint8_t* __restrict__ src, uint64_t limit /* the first data chunk's body, or the stream's end */,
                                                         SearchInfo* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    out->M = out->B = out->ok = out->T = 0;   // (filled in place: the field is too large for registers)
    for (uint32_t i = 0; i < sizeof(out->field); i++) out->field[i] = 0;
    bool seen_id = false;
    for (uint64_t p = 0; p + 4 <= limit;) {
        uint8_t type;
        const uint32_t clen = walk_header(src, p, &type);
        if (search_is_data(type)) break;
        if (type == 0xff) seen_id = true;
        else if (type == kChunkSearchInfo && seen_id) {
            if (p + 4 + clen <= limit) out->ok = search_info(src + p + 4, clen, &out->T, &out->M, &out->B, out->field) ? 1 : 0;
            break;
        }
        p += 4 + uint64_t(clen);
    }
}

// skip[k]: fitting tables in front of chunk k that an earlier round found broken (a stale CRC; a compressed table that does not parse or
// decode) and that are passed over.  A fitting compressed table (0x46) is taken as a candidate: pad = kSearchTabArena, off and bytes = its body
// (cst_resolve, mlz_stream_search_compressed.hip.inc, expands it or has it skipped).
__global__ __launch_bounds__(64) void search_locate_kernel(const uint8_t* __restrict__ src, const SearchHop* __restrict__ hop, const uint32_t* __restrict__ skip, uint32_t nck,
                                                           const SearchInfo* __restrict__ info, SearchTab* __restrict__ tabs) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nck) return;
    SearchTab t{0, 0, kSearchNoTable, 0, 0};
    struct { uint32_t M, B, ok, T; const uint8_t* field; } in{info->M, info->B, info->ok, info->T, info->field};
    if (in.ok) {
        const uint64_t limit = hop[k].limit;
        uint32_t left = skip[k];
        for (uint64_t p = hop[k].from; p + 4 <= limit;) {
            uint8_t type;
            const uint32_t clen = walk_header(src, p, &type);
            if (search_is_data(type)) break;
            if (type == kChunkSearchTable && p + 4 + clen <= limit) {
                const int R = search_table_reductions(src + p + 4, clen, in.M, in.B, in.T, in.field);
                if (R >= 0 && left-- == 0) {
                    const uint32_t f = search_field_len(in.T, in.field);
                    const uint8_t* q = src + p + 8 + f;
                    t = SearchTab{p + 12 + f, clen - 8 - f, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, 0};
                    break;
                }
            } else if (type == kChunkSearchTableCompressed && p + 4 + clen <= limit) {
                const int R = cst_fixed_fields(src + p + 4, clen, in.M, in.B, in.T, in.field);
                if (R >= 0 && left-- == 0) {
                    const uint8_t* q = src + p + 8 + search_field_len(in.T, in.field);
                    t = SearchTab{p + 4, clen, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, kSearchTabArena};
                    break;
                }
            }
            p += 4 + uint64_t(clen);
        }
    }
    tabs[k] = t;
}

// The plan of both searches.  The table sets of a handle: one for a stream's inline tables, up to kSidecarMaxConfigs for an attached sidecar;
// set c's table of chunk k is tabs[c * nck + k], its bytes lie at base + off (base: the stream, or the sidecar), those of an expanded
// compressed table (pad = kSearchTabArena) at arena + off.  pats[p * sets.n + c] is
// pattern p as set c sees it (nw = 0: the set cannot serve the pattern; L is set in every record).
// ov[c]: search_chunk_candidate's ov, a sidecar set's overlap (0 for inline tables).
struct SearchPlanSets { uint32_t n, B[kSidecarMaxConfigs], ov[kSidecarMaxConfigs]; };
// kFold (MLZ_SEARCH_IGNORE_CASE): a pattern's h_off names its window offsets in voff, which name the windows' variant hashes in `hashes`
// (search_pattern_hashes_fold); a lane loops over a window's variants until one bit is set (search_probe_fold).  Without it voff is not read.
// One lane per (data chunk, pattern): every set's verdict on the chunk (search_chunk_candidate over the probes of its table and the next
// chunk's), their conjunction, and the marking (search_decoded_mark_all) ORed into take[].  A lane loops over the sets: there are four at the
// most, and the conjunction wants all votes of a (chunk, pattern) in one place.
template <bool kFold>
__global__ __launch_bounds__(256) void search_plan_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ arena, const SearchTab* __restrict__ tabs, const uint64_t* __restrict__ n_of, uint32_t nck,
                                                          SearchPlanSets sets, const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ voff,
                                                          const SearchManyPat* __restrict__ pats, uint32_t np, uint8_t* __restrict__ take) {
    const uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= uint64_t(nck) * np) return;
    const uint32_t k = uint32_t(idx % nck);
    const SearchManyPat* mine = pats + (idx / nck) * sets.n;
    auto sizes = [&](size_t j) { return n_of[j]; };
    auto admits = [&](uint32_t c) {
        const SearchManyPat pt = mine[c];
        if (!pt.nw) return true;
        const uint32_t* h = hashes + pt.h_off;
        auto probe = [&](size_t j, bool lead) {
            const SearchTab t = tabs[size_t(c) * nck + j];
            uint32_t a = pt.nw, s = pt.nw;
            if (t.R != kSearchNoTable) {
                const uint8_t* bits = (t.pad ? arena : base) + t.off;
                if (kFold) search_probe_fold(bits, sets.B[c] - t.R, voff + pt.h_off, hashes, pt.nw, &a, &s, pt.gsize);
                else search_probe(bits, sets.B[c] - t.R, h, pt.nw, &a, &s, pt.gsize);
            }
            return lead ? a : s;
        };
        return search_chunk_candidate(k, nck, [&](size_t j) { return probe(j, true); }, [&](size_t j) { return probe(j, false); }, sizes, pt.nw, pt.L, pt.t_min, sets.ov[c]);
    };
    search_decoded_mark_all(k, nck, sets.n, admits, sizes, mine[0].L, take);
}

// One workgroup per tile: bit i of the tile's bitmap = "the pattern starts at the tile's position i"; counts[tile] = the set bits.
// kFold (MLZ_SEARCH_IGNORE_CASE): pat is folded, and every byte of the scratch is folded in a register on its way into a comparison.
template <bool kFold>
__global__ __launch_bounds__(256) void search_scan_kernel(const uint8_t* __restrict__ scratch, const SearchTile* __restrict__ tiles, uint32_t tile0,
                                                          const uint8_t* __restrict__ pat, uint32_t L, uint64_t* __restrict__ masks, uint32_t* __restrict__ counts) {
    __shared__ uint8_t sp[kSearchMaxPattern];
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, tile = tile0 + blockIdx.x;
    if (tid < L) sp[tid] = pat[tid];
    __syncthreads();
    const SearchTile t = tiles[tile];
    const uint8_t* s = scratch + t.src_off;
    uint64_t* m = masks + size_t(tile) * kSearchTileWords;
    const uint8_t p0 = sp[0];
    auto at = [&](uint32_t i) { return kFold ? search_fold(s[i]) : s[i]; };
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < kSearchTile / 256; it++) {
        const uint32_t i = it * 256 + tid;
        bool hit = false;
        if (i < t.count && at(i) == p0) {
            uint32_t j = 1;
            while (j < L && at(i + j) == sp[j]) j++;
            hit = j == L;
        }
        const uint64_t b = __ballot(hit);
        if ((tid & 63) == 0) { m[i >> 6] = b; cnt += uint32_t(__popcll(b)); }
    }
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) counts[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// prefix[i] = *total + the counts of the tiles [t0, i) for t0 <= i < t1, then *total += all of them: run once over all tiles with *total = 0
// (one pattern), or group by group in stream order (many)
__global__ __launch_bounds__(1024) void search_prefix_kernel(const uint32_t* __restrict__ counts, uint32_t t0, uint32_t t1, uint64_t* __restrict__ prefix, uint64_t* __restrict__ total) {
    __shared__ uint64_t lds[1024];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = *total;
    for (uint32_t base = t0; base < t1; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t sum;
        const uint64_t before = wg_scan<1024>(uint64_t(i < t1 ? counts[i] : 0), lds, tid, [](uint64_t x, uint64_t y) { return x + y; }, &sum);
        if (i < t1) prefix[i] = carry + before;
        carry += sum;
    }
    __syncthreads();   // (every lane has read *total)
    if (tid == 0) *total = carry;
}

// One workgroup per tile: the positions of its set bits to out[prefix[tile] ...), as far as they lie below cap
__global__ __launch_bounds__(kSearchTileWords) void search_write_kernel(const SearchTile* __restrict__ tiles, const uint64_t* __restrict__ masks, const uint64_t* __restrict__ prefix,
                                                                        uint64_t cap, uint64_t* __restrict__ out) {
    __shared__ uint32_t lds[kSearchTileWords];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t first = prefix[tile];
    if (first >= cap) return;
    uint64_t w = masks[size_t(tile) * kSearchTileWords + tid];
    const uint32_t c = uint32_t(__popcll(w));
    uint64_t at = first + wg_scan<kSearchTileWords>(c, lds, tid, [](uint32_t x, uint32_t y) { return x + y; });
    const uint64_t g = tiles[tile].gpos + uint64_t(tid) * 64;
    for (; w && at < cap; w &= w - 1, at++) out[at] = g + uint64_t(__builtin_ctzll(w));
}

}  // namespace mlz

namespace {

// Once per handle and CRC mode: (T, M, B, prefix field) of the stream and every data chunk's table.  Caller holds c->mu.
int64_t dev_reader_search_tables(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc) {
    mlz_dev_reader::SearchTables& st = rd->search[ignore_crc ? 1 : 0];
    if (st.ready) return 0;
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    std::vector<mlz::SearchHop> hop(nck);
    for (size_t k = 0; k < nck; k++) hop[k] = mlz::SearchHop{k ? uint64_t(rd->chunks[k - 1].body_off + rd->chunks[k - 1].body_len) : 0, uint64_t(rd->chunks[k].body_off)};
    std::vector<uint32_t> skip(nck, 0);
    Carve cv, pin;   // workspace: hops | skips | info | table CRCs; what comes back: tables | table CRCs | info
    const auto r_hop = cv.take<mlz::SearchHop>(nck);
    const auto r_skip = cv.take<uint32_t>(nck);
    const auto r_info = cv.take<mlz::SearchInfo>(1);
    const auto r_crc = cv.take<uint32_t>(nck);
    const auto r_htabs = pin.take<mlz::SearchTab>(nck);
    const auto r_hcrc = pin.take<uint32_t>(nck, 4);
    const auto r_hinfo = pin.take<mlz::SearchInfo>(1, 4);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    if (!st.d_tabs) HIPCHK(c, hipMalloc(&st.d_tabs, nck * sizeof(mlz::SearchTab)));
    int r = ensure_stream_objects(c, 0, pin.bytes);
    if (r) return r;
    void* ws = c->d_rplan.p;
    mlz::SearchHop* d_hop = r_hop.at(ws);
    mlz::SearchInfo *d_info = r_info.at(ws), *h_info = r_hinfo.at(c->pinned2);
    uint32_t *d_skip = r_skip.at(ws), *d_crc = r_crc.at(ws), *h_crc = r_hcrc.at(c->pinned2);
    mlz::SearchTab *d_tabs = static_cast<mlz::SearchTab*>(st.d_tabs), *h_tabs = r_htabs.at(c->pinned2);
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(d_hop, hop.data(), nck * sizeof(mlz::SearchHop), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_info_kernel, dim3(1), dim3(64), 0, sm, rd->d_src, hop[0].limit, d_info);
    for (;;) {
        HIPCHK(c, hipMemcpyAsync(d_skip, skip.data(), nck * 4, hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(mlz::search_locate_kernel, dim3(uint32_t((nck + 63) / 64)), dim3(64), 0, sm, rd->d_src, d_hop, d_skip, uint32_t(nck), d_info, d_tabs);
        HIPCHK(c, hipMemcpyAsync(h_tabs, d_tabs, nck * sizeof(mlz::SearchTab), hipMemcpyDeviceToHost, sm));
        if ((r = fetch(c, sm, h_info, d_info, sizeof(mlz::SearchInfo)))) return r;
        st.tabs.assign(h_tabs, h_tabs + nck);
        st.ncfg = h_info->ok ? 1 : 0;
        st.cfg[0] = *h_info;
        st.base = rd->d_src;
        if (!st.ncfg) break;
        bool again = false;
        if ((r = cst_resolve(c, sm, rd->d_src, &st, &st.tabs, nck, ignore_crc, &skip, &again, st.d_tabs))) return r;   // the compressed tables: expanded, or skipped
        if (again) continue;
        if (ignore_crc) break;
        std::vector<mlz_block_desc> desc;
        std::vector<size_t> who;
        for (size_t k = 0; k < nck; k++)
            if (st.tabs[k].R != mlz::kSearchNoTable && !st.tabs[k].pad) { desc.push_back(mlz_block_desc{st.tabs[k].off, st.tabs[k].bytes, 0, 0}); who.push_back(k); }
        if (desc.empty()) break;
        r = crc_device_locked(c, sm, rd->d_src, desc.data(), int(desc.size()), d_crc);
        if (r) return r;
        if ((r = fetch(c, sm, h_crc, d_crc, desc.size() * 4))) return r;
        for (size_t i = 0; i < who.size(); i++)
            if (h_crc[i] != st.tabs[who[i]].crc) { skip[who[i]]++; again = true; }   // a broken table: the next one that fits, if there is one
        if (!again) break;
    }
    st.ready = true;
    return 0;
}

// The table sets a search on the handle uses: those of the attached sidecar, else the stream's inline ones (found by the handle's first search)
int64_t dev_reader_search_sets(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const mlz_dev_reader::SearchTables** out) {
    if (rd->side_on) { *out = &rd->side; return 0; }
    *out = &rd->search[ignore_crc ? 1 : 0];
    return dev_reader_search_tables(rd, sm, ignore_crc);
}

// The plan of both searches: the union of the patterns' decoded sets -> take[] and their number, the patterns no table set can serve and the
// context's counter 11 (the chunks with a usable table of at least one set that serves a pattern).  off[i]: pattern i's bytes in `patterns`.
// The host hashes every pattern's windows for every set (search_pattern_hashes); search_plan_kernel marks the set and one byte per chunk
// comes back.  A pattern that is not served puts every chunk with a byte into the set, so the kernel is not run then.
// Under MLZ_SEARCH_IGNORE_CASE `patterns` are the FOLDED patterns, and the hashes are those of the windows' case variants
// (search_pattern_hashes_fold, at most kSearchFoldMaxHashes in a call: a pattern that does not fit is not served).
// A set that keeps its streams' tables (mlz_stream_open_batch_device_tables) plans by the rule of mlz_stream_set_tables.h, which needs to know
// the kind of call it serves.  records: an occurrence lies inside one record of the handle's index (grep and the pruned regex grep); else it
// may lie anywhere (the position searches).
int64_t dev_reader_set_tables_plan(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* patterns, const std::vector<uint32_t>& off, size_t np, bool records,
                                   std::vector<uint8_t>* take, size_t* n_take, uint64_t* unserved, bool* planned);   // mlz_stream_set_tables.hip.inc
int64_t dev_reader_search_plan(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* patterns, const std::vector<uint32_t>& off, size_t n,
                               std::vector<uint8_t>* take, size_t* n_take, uint64_t* stats, bool many, bool records = false) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0, fold = (flags & MLZ_SEARCH_IGNORE_CASE) != 0;
    uint64_t unserved = n;
    auto planned = [&]() {   // what every caller reports: counter 10, stats[1 .. 2] and, for many patterns, stats[3]
        c->search_chunks = *n_take;
        if (stats) { stats[1] = *n_take; stats[2] = c->search_tables; if (many) stats[3] = unserved; }
        return 0;
    };
    if (!(flags & MLZ_SEARCH_NO_TABLES) && rd->tabled.on) {
        bool done = false;
        const int64_t r = dev_reader_set_tables_plan(rd, sm, flags, patterns, off, n, records, take, n_take, &unserved, &done);
        if (r) return r;
        if (done) return planned();
    } else if (!(flags & MLZ_SEARCH_NO_TABLES)) {
        const mlz_dev_reader::SearchTables* stp = nullptr;
        const int64_t r = dev_reader_search_sets(rd, sm, ignore_crc, &stp);
        if (r) return r;
        const mlz_dev_reader::SearchTables& st = *stp;
        auto usable_of = [&](uint32_t serving /* a bit per set */, size_t* compressed = nullptr) {   // *compressed: those with a table that came from a 0x46 chunk
            size_t u = 0, uc = 0;
            for (size_t k = 0; k < nck; k++) {
                bool any = false, anyc = false;
                for (uint32_t s = 0; s < st.ncfg; s++) {
                    const mlz::SearchTab& t = st.tabs[s * nck + k];
                    const bool use = ((serving >> s) & 1) && t.R != mlz::kSearchNoTable;
                    any = any || use;
                    anyc = anyc || (use && t.pad);
                }
                u += any ? 1 : 0;
                uc += anyc ? 1 : 0;
            }
            if (compressed) *compressed = uc;
            return u;
        };
        if (st.ncfg && usable_of((1u << st.ncfg) - 1)) {
            std::vector<uint32_t> win(mlz::kSearchMaxWindows), hs, voff;
            std::vector<mlz::SearchManyPat> pats(n * st.ncfg);
            uint32_t serving = 0;
            size_t served = 0;
            for (size_t i = 0; i < n; i++) {
                bool any = false;
                uint32_t mine = 0;   // the sets that serve pattern i
                const size_t h0 = hs.size(), v0 = voff.size();
                for (uint32_t s = 0; s < st.ncfg; s++) {
                    const mlz::SearchConfig& cf = st.cfg[s];
                    mlz::SearchManyPat& pt = pats[i * st.ncfg + s];
                    pt = mlz::SearchManyPat{0, 0, 1, 1, off[i + 1] - off[i], 0};
                    if (!fold) {
                        if (mlz::search_pattern_hashes(patterns + off[i], off[i + 1] - off[i], cf.T, cf.M, cf.B, cf.field, win.data(), &hs, &pt)) { any = true; mine |= 1u << s; }
                        continue;
                    }
                    // under folding the call's variant hashes have a budget; a pattern that does not fit entirely, over all sets, is not served
                    bool over = false;
                    if (mlz::search_pattern_hashes_fold(patterns + off[i], off[i + 1] - off[i], cf.T, cf.M, cf.B, cf.field, win.data(), &voff, &hs, &pt,
                                                        uint32_t(mlz::kSearchFoldMaxHashes - hs.size()), &over)) { any = true; mine |= 1u << s; }
                    else if (over) {
                        for (uint32_t b = 0; b < st.ncfg; b++) pats[i * st.ncfg + b] = mlz::SearchManyPat{0, 0, 1, 1, off[i + 1] - off[i], 0};   // (L is set in every record)
                        hs.resize(h0); voff.resize(v0);
                        any = false; mine = 0;
                        break;
                    }
                }
                serving |= mine;
                served += any ? 1 : 0;
            }
            size_t usable_compressed = 0;
            const size_t usable = usable_of(serving, &usable_compressed);
            // (a pattern whose serving sets hold no table at all is one the tables cannot serve)
            if (!usable) served = 0;
            unserved = n - served;
            if (served) { c->search_tables = usable; c->search_compressed = usable_compressed; }
            if (unserved == 0) {
                // hashes, pattern records and the chunks' sizes go up as one block, staged in the pinned buffer; one byte per chunk comes back
                Carve up;
                const auto u_hs = up.take<uint32_t>(hs.size());
                const auto u_pats = up.take<mlz::SearchManyPat>(pats.size());
                const auto u_n = up.take<uint64_t>(nck);
                Region<uint32_t> u_voff{};
                if (fold) u_voff = up.take<uint32_t>(voff.size());   // (behind the unflagged call's block, which stays as it is)
                Carve cv;
                const auto r_up = cv.take<uint8_t>(up.bytes);
                const auto r_take = cv.take<uint8_t>(nck);
                HIPCHK(c, c->d_rplan.ensure(cv.bytes));
                int e = ensure_stream_objects(c, 0, up.bytes > nck ? up.bytes : nck);
                if (e) return e;
                void *ws = r_up.at(c->d_rplan.p), *h_up = c->pinned2;
                std::memcpy(u_hs.at(h_up), hs.data(), hs.size() * 4);
                std::memcpy(u_pats.at(h_up), pats.data(), pats.size() * sizeof(mlz::SearchManyPat));
                if (fold) std::memcpy(u_voff.at(h_up), voff.data(), voff.size() * 4);
                uint64_t* h_n = u_n.at(h_up);
                for (size_t k = 0; k < nck; k++) h_n[k] = rd->chunks[k].n;
                uint8_t* d_take = r_take.at(c->d_rplan.p);
                mlz::SearchPlanSets sets{};
                sets.n = st.ncfg;
                for (uint32_t s = 0; s < st.ncfg; s++) {
                    sets.B[s] = st.cfg[s].B;
                    sets.ov[s] = stp == &rd->side ? mlz::search_overlap(st.cfg[s].T, st.cfg[s].M, st.cfg[s].field) : 0;
                }
                { WorkspaceOrder order(c, sm); }
                HIPCHK(c, hipMemcpyAsync(ws, h_up, up.bytes, hipMemcpyHostToDevice, sm));
                HIPCHK(c, hipMemsetAsync(d_take, 0, nck, sm));
                const uint64_t lanes = uint64_t(nck) * n;
                hipLaunchKernelGGL(fold ? mlz::search_plan_kernel<true> : mlz::search_plan_kernel<false>, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, sm, st.base,
                                   static_cast<const uint8_t*>(st.d_arena),
                                   static_cast<const mlz::SearchTab*>(st.d_tabs), u_n.at(ws), uint32_t(nck), sets, u_hs.at(ws), fold ? u_voff.at(ws) : static_cast<const uint32_t*>(nullptr),
                                   u_pats.at(ws), uint32_t(n), d_take);
                if ((e = fetch(c, sm, c->pinned2, d_take, nck))) return e;   // (behind the upload on sm: the staged block has left the pinned buffer)
                std::memcpy(take->data(), c->pinned2, nck);
                *n_take = 0;
                for (size_t k = 0; k < nck; k++) *n_take += (*take)[k];
                return planned();
            }
        }
    }
    *n_take = 0;   // a pattern the tables cannot serve: every chunk that holds a byte
    for (size_t k = 0; k < nck; k++) *n_take += ((*take)[k] = rd->chunks[k].n ? 1 : 0);
    return planned();
}

// The decoded set of both searches on its way through the scratch (ScratchDecode): the decode list in stream order, its groups (range_group_ends), every
// chunk's place and the tiles of start positions (search_layout), and where the carried bytes and the tiles lie in the two workspaces.
struct SearchDecode {
    ScratchDecode dec;
    mlz::SearchLayout lay;
    Region<uint8_t> carry;
    Region<mlz::SearchTile> tiles, htiles;
};

// The groups (range_group_ends), every chunk's place and the tiles (search_layout) of a decode list that stands in sd->dec.jobs; out_off_of(i):
// job i's place in the decoded sequence the layout sees (a stream's own positions; the virtual positions of a batch of streams)
template <class Off>
void search_decode_layout(const std::vector<StreamChunk>& chunks, Off out_off_of, uint32_t lmin, uint32_t lmax, uint32_t tile, SearchDecode* sd) {
    const std::vector<ChunkJob>& jobs = sd->dec.jobs;
    mlz::range_group_ends(jobs.size(), [&](size_t i) { return uint64_t(chunks[jobs[i].ck].n); }, &sd->dec.gend);
    mlz::search_layout(jobs.size(), sd->dec.gend, out_off_of, [&](size_t i) { return uint64_t(chunks[jobs[i].ck].n); }, lmin, lmax, tile, &sd->lay);
    sd->dec.at = sd->lay.at;
}

// The three helpers below take the context, the stream's bytes and its chunk table, not a handle: the handle calls pass rd->ctx, rd->d_src and
// rd->chunks, the search over a batch of streams (mlz_stream_search_batch.hip.inc) its batch's.
// lmin, lmax: the shortest and the longest pattern of the call; tile: the most start positions of a tile (search_layout)
void search_decode_plan(const std::vector<StreamChunk>& chunks, const std::vector<uint8_t>& take, size_t n_take, uint32_t lmin, uint32_t lmax, uint32_t tile, SearchDecode* sd) {
    std::vector<ChunkJob>& jobs = sd->dec.jobs;
    jobs.reserve(n_take);
    for (size_t k = 0; k < chunks.size(); k++) if (take[k]) jobs.push_back(ChunkJob{k, nullptr});
    search_decode_layout(chunks, [&](size_t i) { return uint64_t(chunks[jobs[i].ck].out_off); }, lmin, lmax, tile, sd);
}

// Behind the caller's own regions: carried bytes | tiles in the workspace (c->d_rplan), the decode's | tiles in the pinned buffer; then every
// buffer of the call, once: the workspace and the pinned buffer as they are carved now, the scratch, the copies' descriptors
int search_decode_ready(mlz_ctx* c, const std::vector<StreamChunk>& chunks, SearchDecode* sd, Carve* cv, Carve* pin) {
    const size_t nt = sd->lay.tiles.size();
    sd->carry = cv->take<uint8_t>(mlz::kSearchMaxPattern);
    sd->tiles = cv->take<mlz::SearchTile>(nt);
    if (const int e = sd->dec.take(c, chunks, pin)) return e;
    sd->htiles = pin->take<mlz::SearchTile>(nt, 64);
    HIPCHK(c, c->d_rplan.ensure(cv->bytes));
    return ensure_stream_objects(c, 0, pin->bytes);
}

// Decodes the set group by group into the scratch, calls scan(g, t0, t1) for the tiles [t0, t1) of group g with its bytes in place, and
// carries a run's last bytes in front of the next group.  Returns stream_run_chunk_jobs' verdict (with per_job: every job's own, and 0).
template <class Scan>
int64_t search_decode_run(mlz_ctx* c, const uint8_t* d_src, const std::vector<StreamChunk>& chunks, hipStream_t sm, bool ignore_crc, SearchDecode* sd, Scan scan,
                          std::vector<int64_t>* per_job = nullptr) {
    const mlz::SearchLayout& lay = sd->lay;
    const size_t nt = lay.tiles.size();
    uint8_t *scratch = c->d_range.as<uint8_t>(), *d_carry = sd->carry.at(c->d_rplan.p);
    mlz::SearchTile *d_tiles = sd->tiles.at(c->d_rplan.p), *h_tiles = sd->htiles.at(c->pinned2);
    if (nt) {
        std::memcpy(h_tiles, lay.tiles.data(), nt * sizeof(mlz::SearchTile));
        HIPCHK(c, hipMemcpyAsync(d_tiles, h_tiles, nt * sizeof(mlz::SearchTile), hipMemcpyHostToDevice, sm));
    }
    return sd->dec.run(c, sm, ignore_crc, d_src, chunks, [&](size_t g) -> int {
        const size_t t0 = g ? lay.tile_end[g - 1] : 0, t1 = lay.tile_end[g];
        if (t1 > t0) { const int e = scan(g, t0, t1); if (e) return e; }
        if (lay.carry[g]) {   // the run goes on in the next group: its last bytes in front of that group's first chunk
            HIPCHK(c, hipMemcpyAsync(d_carry, scratch + lay.used[g] - lay.carry[g], lay.carry[g], hipMemcpyDeviceToDevice, sm));
            HIPCHK(c, hipMemcpyAsync(scratch + mlz::kSearchPad - lay.carry[g], d_carry, lay.carry[g], hipMemcpyDeviceToDevice, sm));
        }
        return 0;
    }, per_job);
}

// The opening of both searches: counters 10, 11 and 14 cleared, stats = {data chunks, 0, 0, 0}
void search_begin(mlz_dev_reader* rd, uint64_t* stats) {
    rd->ctx->search_chunks = rd->ctx->search_tables = rd->ctx->search_compressed = 0;
    if (stats) { stats[0] = rd->chunks.size(); stats[1] = stats[2] = stats[3] = 0; }
}

// What a search leaves in the workspace (c->d_rplan) behind its count pass and its prefix scan, until the workspace is carved anew: the tiles,
// their bitmaps and prefixes and the total, still on its way (nt == 0: nothing was scanned and the total is 0).  search_found_write puts the
// smallest `cap` positions out; a caller that sizes its buffer by the total fetches *d_total first.
struct SearchFound {
    size_t nt = 0;
    const mlz::SearchTile* d_tiles = nullptr;
    const uint64_t *d_masks = nullptr, *d_prefix = nullptr, *d_total = nullptr;
};

void search_found_write(hipStream_t sm, const SearchFound& f, uint64_t cap, uint64_t* d_offsets) {
    if (cap && f.nt) hipLaunchKernelGGL(mlz::search_write_kernel, dim3(uint32_t(f.nt)), dim3(mlz::kSearchTileWords), 0, sm, f.d_tiles, f.d_masks, f.d_prefix, cap, d_offsets);
}

// The plan, the decode and the scan of a search for one pattern, up to the prefix kernel: everything but the positions and the total's way home.
int64_t dev_reader_search_scan_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* pattern, uint32_t L, uint64_t* stats, SearchFound* found) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0, fold = (flags & MLZ_SEARCH_IGNORE_CASE) != 0;
    search_begin(rd, stats);
    if (nck == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t folded[mlz::kSearchMaxPattern];
    if (fold) {   // the pattern is folded once, here; the plan and the scan see the folded one
        for (uint32_t i = 0; i < L; i++) folded[i] = mlz::search_fold(pattern[i]);
        pattern = folded;
    }
    std::vector<uint8_t> take(nck, 0);
    size_t n_take = 0;
    const int64_t pr = dev_reader_search_plan(rd, sm, flags, pattern, std::vector<uint32_t>{0, L}, 1, &take, &n_take, stats, false);
    if (pr) return pr;
    if (n_take == 0) return 0;

    // the decode list, its groups, every chunk's place in the scratch and the tiles of start positions (search_layout), the stored chunks' copies
    SearchDecode sd;
    search_decode_plan(rd->chunks, take, n_take, L, L, mlz::kSearchTile, &sd);
    const size_t nt = sd.lay.tiles.size();
    if (nt > 0x7fffffffu) return -MLZ_ERR_ARG;
    Carve cv, pin;   // workspace: pattern | total | counts | prefix | bitmaps | the decode's; pinned: pattern | the decode's
    const auto r_pat = cv.take<uint8_t>(mlz::kSearchMaxPattern);
    const auto r_total = cv.take<uint64_t>(2);
    const auto r_counts = cv.take<uint32_t>(nt, 4);
    const auto r_prefix = cv.take<uint64_t>(nt), r_masks = cv.take<uint64_t>(nt * mlz::kSearchTileWords, 8);
    const auto r_hpat = pin.take<uint8_t>(mlz::kSearchMaxPattern + 16, 8);
    int e = search_decode_ready(rd->ctx, rd->chunks, &sd, &cv, &pin);
    if (e) return e;
    uint8_t *ws = r_pat.at(c->d_rplan.p), *h_pat = r_hpat.at(c->pinned2);
    std::memcpy(h_pat, pattern, L);
    uint32_t* d_counts = r_counts.at(c->d_rplan.p);
    uint64_t *d_prefix = r_prefix.at(c->d_rplan.p), *d_masks = r_masks.at(c->d_rplan.p), *d_total = r_total.at(c->d_rplan.p);
    const mlz::SearchTile* d_tiles = sd.tiles.at(c->d_rplan.p);
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(ws, h_pat, L, hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemsetAsync(d_total, 0, 16, sm));
    const int64_t r = search_decode_run(rd->ctx, rd->d_src, rd->chunks, sm, ignore_crc, &sd, [&](size_t, size_t t0, size_t t1) {
        hipLaunchKernelGGL(fold ? mlz::search_scan_kernel<true> : mlz::search_scan_kernel<false>, dim3(uint32_t(t1 - t0)), dim3(256), 0, sm, c->d_range.as<uint8_t>(), d_tiles, uint32_t(t0), ws, L, d_masks, d_counts);
        return 0;
    });
    if (r < 0) return r;
    if (nt == 0) return 0;
    hipLaunchKernelGGL(mlz::search_prefix_kernel, dim3(1), dim3(1024), 0, sm, d_counts, 0u, uint32_t(nt), d_prefix, d_total);   // (d_total: cleared above)
    *found = SearchFound{nt, d_tiles, d_masks, d_prefix, d_total};
    return 0;
}

// The total of a search whose scan is enqueued (SearchFound), waited for
int64_t search_found_total(mlz_ctx* c, hipStream_t sm, const SearchFound& f) {
    if (f.nt == 0) return 0;
    const int e = fetch(c, sm, c->pinned2, f.d_total, 8);
    if (e) return e;
    return int64_t(*static_cast<const uint64_t*>(c->pinned2));
}

int64_t dev_reader_search_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* pattern, uint32_t L, uint64_t* d_offsets, uint64_t cap, uint64_t* stats) {
    SearchFound found;
    const int64_t r = dev_reader_search_scan_locked(rd, sm, flags, pattern, L, stats, &found);
    if (r < 0) return r;
    search_found_write(sm, found, cap, d_offsets);
    return search_found_total(rd->ctx, sm, found);
}

}  // namespace

extern "C" int64_t mlz_dev_reader_search(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* pattern, size_t pattern_len, uint64_t* d_offsets, size_t cap,
                                         uint64_t* stats) {
    if (!rd || !pattern || pattern_len == 0 || pattern_len > mlz::kSearchMaxPattern || (!d_offsets && cap)) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (cap && !on_device(c, d_offsets)) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_search_locked(rd, sm, flags, pattern, uint32_t(pattern_len), d_offsets, uint64_t(cap), stats));
}
