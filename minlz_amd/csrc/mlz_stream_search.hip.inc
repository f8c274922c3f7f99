// mlz_stream_search.hip.inc — mlz_dev_reader_search: where a byte string occurs in a .mz stream that lies in HBM (included at the end of
// mlz_hip.hip, behind the device-resident ReadSeeker whose handle, chunk-list decode and scratch it uses).
//
// The stream's block search tables (SPEC_SEARCH.md: an info chunk 0x44 behind the identifier, a bit table 0x45 in front of a block) say
// which blocks can hold the pattern's windows of M bytes.  Per handle, once: search_info_kernel reads the info chunk, search_locate_kernel
// (one lane per data chunk) hops over the chunk headers between the previous data chunk's end and its own start to the first table chunk
// that fits, and the existing CRC pass checks the tables.  Per call: search_probe_kernel looks the pattern's windows up in every table
// (8 bytes per chunk come back), the rule of mlz_stream_search.h turns that into the set of chunks to decode, stream_run_chunk_jobs decodes
// exactly those into the scratch, chunks that are neighbours in the stream side by side, and search_scan_kernel marks the occurrences of every
// run in a bitmap (one bit per decoded byte of the set) and counts them per tile.  A scan over the tile counts and search_write_kernel then
// put the smallest `cap` positions out in ascending order.

namespace mlz {

struct SearchInfo { uint32_t M, B, ok, pad; };
struct SearchHop { uint64_t from, limit; };                               // where a lane starts to hop and the data chunk's body, which it never reaches

__device__ __forceinline__ bool search_is_data(uint8_t t) { return t >= 1 && t <= 3; }

__global__ __launch_bounds__(64) void search_info_kernel(const uint8_t* __restrict__ src, uint64_t limit /* the first data chunk's body, or the stream's end */,
                                                         SearchInfo* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    SearchInfo r{0, 0, 0, 0};
    bool seen_id = false;
    for (uint64_t p = 0; p + 4 <= limit;) {
        const uint8_t type = src[p];
        const uint32_t clen = uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
        if (search_is_data(type)) break;
        if (type == 0xff) seen_id = true;
        else if (type == kChunkSearchInfo && seen_id) {
            if (p + 4 + clen <= limit) r.ok = search_info(src + p + 4, clen, &r.M, &r.B) ? 1 : 0;
            break;
        }
        p += 4 + uint64_t(clen);
    }
    *out = r;
}

// skip[k]: fitting tables in front of chunk k that an earlier round found broken (CRC) and that are passed over
__global__ __launch_bounds__(64) void search_locate_kernel(const uint8_t* __restrict__ src, const SearchHop* __restrict__ hop, const uint32_t* __restrict__ skip, uint32_t nck,
                                                           const SearchInfo* __restrict__ info, SearchTab* __restrict__ tabs) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nck) return;
    SearchTab t{0, 0, kSearchNoTable, 0, 0};
    const SearchInfo in = *info;
    if (in.ok) {
        const uint64_t limit = hop[k].limit;
        uint32_t left = skip[k];
        for (uint64_t p = hop[k].from; p + 4 <= limit;) {
            const uint8_t type = src[p];
            const uint32_t clen = uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
            if (search_is_data(type)) break;
            if (type == kChunkSearchTable && p + 4 + clen <= limit) {
                const int R = search_table_reductions(src + p + 4, clen, in.M, in.B);
                if (R >= 0 && left-- == 0) {
                    const uint8_t* q = src + p + 8;
                    t = SearchTab{p + 12, clen - 8, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, 0};
                    break;
                }
            }
            p += 4 + uint64_t(clen);
        }
    }
    tabs[k] = t;
}

__global__ __launch_bounds__(64) void search_probe_kernel(const uint8_t* __restrict__ src, const SearchTab* __restrict__ tabs, uint32_t nck, uint32_t B,
                                                          const uint32_t* __restrict__ hashes, uint32_t nw, uint2* __restrict__ out) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nck) return;
    const SearchTab t = tabs[k];
    uint32_t a = nw, s = nw;
    if (t.R != kSearchNoTable) search_probe(src + t.off, B - t.R, hashes, nw, &a, &s);
    out[k] = make_uint2(a, s);
}

// One workgroup per tile: bit i of the tile's bitmap = "the pattern starts at the tile's position i"; counts[tile] = the set bits.
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
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < kSearchTile / 256; it++) {
        const uint32_t i = it * 256 + tid;
        bool hit = false;
        if (i < t.count && s[i] == p0) {
            uint32_t j = 1;
            while (j < L && s[i + j] == sp[j]) j++;
            hit = j == L;
        }
        const uint64_t b = __ballot(hit);
        if ((tid & 63) == 0) { m[i >> 6] = b; cnt += uint32_t(__popcll(b)); }
    }
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) counts[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// prefix[i] = the occurrences in the tiles in front of tile i; *total = all of them
__global__ __launch_bounds__(1024) void search_prefix_kernel(const uint32_t* __restrict__ counts, uint32_t nt, uint64_t* __restrict__ prefix, uint64_t* __restrict__ total) {
    __shared__ uint64_t lds[1024];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nt; base += 1024) {
        const uint32_t i = base + tid;
        const uint64_t v = i < nt ? counts[i] : 0;
        lds[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t x = tid >= d ? lds[tid - d] : 0;
            __syncthreads();
            lds[tid] += x;
            __syncthreads();
        }
        if (i < nt) prefix[i] = carry + lds[tid] - v;
        carry += lds[1023];
        __syncthreads();
    }
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
    lds[tid] = c;
    __syncthreads();
    for (uint32_t d = 1; d < kSearchTileWords; d <<= 1) {
        const uint32_t x = tid >= d ? lds[tid - d] : 0;
        __syncthreads();
        lds[tid] += x;
        __syncthreads();
    }
    uint64_t at = first + lds[tid] - c;
    const uint64_t g = tiles[tile].gpos + uint64_t(tid) * 64;
    for (; w && at < cap; w &= w - 1, at++) out[at] = g + uint64_t(__builtin_ctzll(w));
}

}  // namespace mlz

namespace {

// Once per handle and CRC mode: (M, B) of the stream and every data chunk's table.  Caller holds c->mu.
int64_t dev_reader_search_tables(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc) {
    mlz_dev_reader::SearchTables& st = rd->search[ignore_crc ? 1 : 0];
    if (st.ready) return 0;
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    std::vector<mlz::SearchHop> hop(nck);
    for (size_t k = 0; k < nck; k++) hop[k] = mlz::SearchHop{k ? uint64_t(rd->chunks[k - 1].body_off + rd->chunks[k - 1].body_len) : 0, uint64_t(rd->chunks[k].body_off)};
    std::vector<uint32_t> skip(nck, 0);
    const size_t o_skip = nck * sizeof(mlz::SearchHop), o_info = (o_skip + nck * 4 + 15) & ~size_t(15), o_crc = o_info + sizeof(mlz::SearchInfo), ws_bytes = o_crc + nck * 4;
    HIPCHK(c, c->d_rplan.ensure(ws_bytes));
    if (!st.d_tabs) HIPCHK(c, hipMalloc(&st.d_tabs, nck * sizeof(mlz::SearchTab)));
    int r = ensure_stream_objects(c, 0, nck * (sizeof(mlz::SearchTab) + 4) + sizeof(mlz::SearchInfo));
    if (r) return r;
    uint8_t* ws = c->d_rplan.as<uint8_t>();
    mlz::SearchHop* d_hop = reinterpret_cast<mlz::SearchHop*>(ws);
    uint32_t* d_skip = reinterpret_cast<uint32_t*>(ws + o_skip);
    mlz::SearchInfo* d_info = reinterpret_cast<mlz::SearchInfo*>(ws + o_info);
    uint32_t* d_crc = reinterpret_cast<uint32_t*>(ws + o_crc);
    mlz::SearchTab* d_tabs = static_cast<mlz::SearchTab*>(st.d_tabs);
    mlz::SearchTab* h_tabs = static_cast<mlz::SearchTab*>(c->pinned2);
    uint32_t* h_crc = reinterpret_cast<uint32_t*>(h_tabs + nck);
    mlz::SearchInfo* h_info = reinterpret_cast<mlz::SearchInfo*>(h_crc + nck);
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(d_hop, hop.data(), nck * sizeof(mlz::SearchHop), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_info_kernel, dim3(1), dim3(64), 0, sm, rd->d_src, hop[0].limit, d_info);
    for (;;) {
        HIPCHK(c, hipMemcpyAsync(d_skip, skip.data(), nck * 4, hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(mlz::search_locate_kernel, dim3(uint32_t((nck + 63) / 64)), dim3(64), 0, sm, rd->d_src, d_hop, d_skip, uint32_t(nck), d_info, d_tabs);
        HIPCHK(c, hipMemcpyAsync(h_tabs, d_tabs, nck * sizeof(mlz::SearchTab), hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipMemcpyAsync(h_info, d_info, sizeof(mlz::SearchInfo), hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
        HIPCHK(c, hipGetLastError());
        st.tabs.assign(h_tabs, h_tabs + nck);
        st.M = h_info->M; st.B = h_info->B; st.info = h_info->ok != 0;
        if (ignore_crc || !st.info) break;
        std::vector<mlz_block_desc> desc;
        std::vector<size_t> who;
        for (size_t k = 0; k < nck; k++)
            if (st.tabs[k].R != mlz::kSearchNoTable) { desc.push_back(mlz_block_desc{st.tabs[k].off, st.tabs[k].bytes, 0, 0}); who.push_back(k); }
        if (desc.empty()) break;
        r = crc_device_locked(c, sm, rd->d_src, desc.data(), int(desc.size()), d_crc);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(h_crc, d_crc, desc.size() * 4, hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
        HIPCHK(c, hipGetLastError());
        bool again = false;
        for (size_t i = 0; i < who.size(); i++)
            if (h_crc[i] != st.tabs[who[i]].crc) { skip[who[i]]++; again = true; }   // a broken table: the next one that fits, if there is one
        if (!again) break;
    }
    st.usable = 0;
    for (size_t k = 0; k < nck; k++) st.usable += st.tabs[k].R != mlz::kSearchNoTable ? 1 : 0;
    st.ready = true;
    return 0;
}

int64_t dev_reader_search_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* pattern, uint32_t L, uint64_t* d_offsets, uint64_t cap, uint64_t* stats) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0;
    c->search_chunks = c->search_tables = 0;
    if (stats) { stats[0] = nck; stats[1] = stats[2] = stats[3] = 0; }
    if (nck == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint8_t> take(nck, 1);
    size_t n_take = 0;
    bool with_tables = (flags & MLZ_SEARCH_NO_TABLES) == 0;
    if (with_tables) {
        const int64_t r = dev_reader_search_tables(rd, sm, ignore_crc);
        if (r) return r;
        const mlz_dev_reader::SearchTables& st = rd->search[ignore_crc ? 1 : 0];
        with_tables = st.info && L >= st.M && st.usable;
        if (with_tables) {
            // the windows' hashes go up, two counts per chunk come back
            const uint32_t nw = L - st.M + 1;
            std::vector<uint32_t> hs(nw);
            for (uint32_t i = 0; i < nw; i++) {
                uint64_t v = 0;
                for (uint32_t j = 0; j < st.M; j++) v |= uint64_t(pattern[i + j]) << (8 * j);
                hs[i] = mlz::search_hash(v, st.B, st.M);
            }
            const size_t o_out = (size_t(nw) * 4 + 15) & ~size_t(15);
            HIPCHK(c, c->d_rplan.ensure(o_out + nck * 8));
            int e = ensure_stream_objects(c, 0, nck * 8);
            if (e) return e;
            uint32_t* d_hs = c->d_rplan.as<uint32_t>();
            uint2* d_out = reinterpret_cast<uint2*>(c->d_rplan.as<uint8_t>() + o_out);
            { WorkspaceOrder order(c, sm); }
            HIPCHK(c, hipMemcpyAsync(d_hs, hs.data(), size_t(nw) * 4, hipMemcpyHostToDevice, sm));
            hipLaunchKernelGGL(mlz::search_probe_kernel, dim3(uint32_t((nck + 63) / 64)), dim3(64), 0, sm, rd->d_src, static_cast<const mlz::SearchTab*>(st.d_tabs), uint32_t(nck), st.B,
                               d_hs, nw, d_out);
            HIPCHK(c, hipMemcpyAsync(c->pinned2, d_out, nck * 8, hipMemcpyDeviceToHost, sm));
            HIPCHK(c, hipStreamSynchronize(sm));
            HIPCHK(c, hipGetLastError());
            const uint32_t* as = static_cast<const uint32_t*>(c->pinned2);
            n_take = mlz::search_decoded_set(nck, [&](size_t k) { return as[2 * k]; }, [&](size_t k) { return as[2 * k + 1]; },
                                             [&](size_t k) { return uint64_t(rd->chunks[k].n); }, nw, L, take.data());
            c->search_tables = st.usable;
        }
    }
    if (!with_tables) {
        n_take = 0;
        for (size_t k = 0; k < nck; k++) n_take += (take[k] = rd->chunks[k].n ? 1 : 0);
    }
    c->search_chunks = n_take;
    if (stats) { stats[1] = n_take; stats[2] = c->search_tables; }
    if (n_take == 0) return 0;

    // the decode list, its groups, every chunk's place in the scratch and the tiles of start positions (search_layout), the stored chunks' copies
    std::vector<ChunkJob> jobs;
    jobs.reserve(n_take);
    for (size_t k = 0; k < nck; k++) if (take[k]) jobs.push_back(ChunkJob{k, nullptr});
    std::vector<size_t> gend;
    mlz::range_group_ends(jobs.size(), [&](size_t i) { return uint64_t(rd->chunks[jobs[i].ck].n); }, &gend);
    const size_t ng = gend.size();
    mlz::SearchLayout lay;
    mlz::search_layout(jobs.size(), gend, [&](size_t i) { return uint64_t(rd->chunks[jobs[i].ck].out_off); }, [&](size_t i) { return uint64_t(rd->chunks[jobs[i].ck].n); }, L, &lay);
    const std::vector<uint64_t>& at = lay.at;
    const std::vector<mlz::SearchTile>& tiles = lay.tiles;
    const std::vector<size_t>& tile_end = lay.tile_end;
    const std::vector<uint32_t>& carry = lay.carry;
    const std::vector<uint64_t>& used = lay.used;
    const uint64_t scratch_max = lay.scratch_max;
    std::vector<size_t> place_end(ng);
    std::vector<PlaceDesc> places;   // stored chunks: copied from the stream
    for (size_t g = 0, j0 = 0; g < ng; j0 = gend[g++]) {
        for (size_t i = j0; i < gend[g]; i++) {
            const StreamChunk& ck = rd->chunks[jobs[i].ck];
            if (ck.type == kChunkUncompressed)
                for (size_t q = 0; q < ck.n; q += kPlacePiece) places.push_back(PlaceDesc{ck.body_off + q, at[i] + q, uint32_t(std::min<size_t>(kPlacePiece, ck.n - q)), 1});
        }
        place_end[g] = places.size();
    }
    const size_t nt = tiles.size(), np = places.size();
    if (nt > 0x7fffffffu) return -MLZ_ERR_ARG;
    // workspace: pattern | carried bytes | total | tiles | counts | prefix | bitmaps
    const size_t o_carry = mlz::kSearchMaxPattern, o_total = o_carry + mlz::kSearchMaxPattern, o_tiles = o_total + 16, o_counts = o_tiles + nt * sizeof(mlz::SearchTile),
                 o_prefix = (o_counts + nt * 4 + 15) & ~size_t(15), o_masks = o_prefix + nt * 8, ws_bytes = o_masks + nt * mlz::kSearchTileWords * 8;
    HIPCHK(c, c->d_rplan.ensure(ws_bytes));
    HIPCHK(c, c->d_range.ensure(size_t(scratch_max) + 64));
    if (np) HIPCHK(c, c->d_place.ensure(np * sizeof(PlaceDesc)));
    const size_t p_tiles = (chunk_jobs_pinned(jobs.size()) + 63) & ~size_t(63), p_places = p_tiles + nt * sizeof(mlz::SearchTile), p_pat = p_places + np * sizeof(PlaceDesc);
    int e = ensure_stream_objects(c, 0, p_pat + mlz::kSearchMaxPattern + 16);
    if (e) return e;
    uint8_t* pin = static_cast<uint8_t*>(c->pinned2);
    if (nt) std::memcpy(pin + p_tiles, tiles.data(), nt * sizeof(mlz::SearchTile));
    if (np) std::memcpy(pin + p_places, places.data(), np * sizeof(PlaceDesc));
    std::memcpy(pin + p_pat, pattern, L);
    uint8_t* ws = c->d_rplan.as<uint8_t>();
    uint8_t* scratch = c->d_range.as<uint8_t>();
    mlz::SearchTile* d_tiles = reinterpret_cast<mlz::SearchTile*>(ws + o_tiles);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(ws + o_counts);
    uint64_t* d_prefix = reinterpret_cast<uint64_t*>(ws + o_prefix);
    uint64_t* d_masks = reinterpret_cast<uint64_t*>(ws + o_masks);
    uint64_t* d_total = reinterpret_cast<uint64_t*>(ws + o_total);
    for (size_t i = 0; i < jobs.size(); i++) {
        const StreamChunk& ck = rd->chunks[jobs[i].ck];
        jobs[i].at = ck.type == kChunkUncompressed ? rd->d_src + ck.body_off : scratch + at[i];   // (a stored chunk's CRC: over the stream's own bytes)
    }
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(ws, pin + p_pat, L, hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemsetAsync(d_total, 0, 16, sm));
    if (nt) HIPCHK(c, hipMemcpyAsync(d_tiles, pin + p_tiles, nt * sizeof(mlz::SearchTile), hipMemcpyHostToDevice, sm));
    if (np) HIPCHK(c, hipMemcpyAsync(c->d_place.p, pin + p_places, np * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
    auto scan_group = [&](size_t g) -> int {
        const size_t t0 = g ? tile_end[g - 1] : 0, t1 = tile_end[g], q0 = g ? place_end[g - 1] : 0, q1 = place_end[g];
        if (q1 > q0) hipLaunchKernelGGL(stream_place2_kernel, dim3(uint32_t(q1 - q0)), dim3(256), 0, sm, rd->d_src, rd->d_src, scratch, c->d_place.as<PlaceDesc>() + q0);
        if (t1 > t0) hipLaunchKernelGGL(mlz::search_scan_kernel, dim3(uint32_t(t1 - t0)), dim3(256), 0, sm, scratch, d_tiles, uint32_t(t0), ws, L, d_masks, d_counts);
        if (carry[g]) {   // the run goes on in the next group: its last bytes in front of that group's first chunk
            HIPCHK(c, hipMemcpyAsync(ws + o_carry, scratch + used[g] - carry[g], carry[g], hipMemcpyDeviceToDevice, sm));
            HIPCHK(c, hipMemcpyAsync(scratch + mlz::kSearchPad - carry[g], ws + o_carry, carry[g], hipMemcpyDeviceToDevice, sm));
        }
        return 0;
    };
    const int64_t r = stream_run_chunk_jobs(c, sm, ignore_crc, rd->d_src, rd->chunks, jobs, gend, scan_group);
    if (r < 0) return r;
    if (nt == 0) return 0;
    hipLaunchKernelGGL(mlz::search_prefix_kernel, dim3(1), dim3(1024), 0, sm, d_counts, uint32_t(nt), d_prefix, d_total);
    if (cap) hipLaunchKernelGGL(mlz::search_write_kernel, dim3(uint32_t(nt)), dim3(mlz::kSearchTileWords), 0, sm, d_tiles, d_masks, d_prefix, cap, d_offsets);
    HIPCHK(c, hipMemcpyAsync(pin, d_total, 8, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    return int64_t(*reinterpret_cast<const uint64_t*>(pin));
}

}  // namespace

extern "C" int64_t mlz_dev_reader_search(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* pattern, size_t pattern_len, uint64_t* d_offsets, size_t cap,
                                         uint64_t* stats) {
    if (!rd || !pattern || pattern_len == 0 || pattern_len > mlz::kSearchMaxPattern || (!d_offsets && cap)) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return -MLZ_ERR_HIP; }
    if (cap && !on_device(c, d_offsets)) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    const int64_t r = dev_reader_search_locked(rd, static_cast<hipStream_t>(stream), flags, pattern, uint32_t(pattern_len), d_offsets, uint64_t(cap), stats);
    if (r < 0) (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));   // nothing of a failed call is left in flight
    return r;
}
