// mlz_stream_batch.hip.inc — batches of streams in HBM: many .mz streams walked, decoded or encoded by one call (included at the end of
// mlz_hip.hip, behind mlz_stream_walk.hip.inc and mlz_stream_ranges.hip.inc whose walk, chunk-list decode and framing kernels it uses).
//
// The contract of every stream of a batch is the single-stream call's (mlz_stream_decoded_len_device, mlz_stream_decode_device,
// mlz_stream_encode_gather_device over one range); what a batch saves is the fixed cost per stream: the six launches and two read-backs of
// the region walk, the decode's launch sequence and read-back, the Writer's.
//
//   walk     walk_batch_kernel<false>: a lane per stream steps through its chunk headers from offset 0 (mlz::batch_walk_lane: walk_headers, the step
//            walk_list_kernel runs inside one region, under a cap) and counts the table's entries; walk_scan_kernel turns the counts into places;
//            walk_batch_kernel<true> writes the records.  No region tables: 32 bytes per table entry, 8 bytes and a flag bit per stream.
//            A lane stops after kBatchWalkSteps headers; its stream is LONG and goes through stream_walk_device inside the same call.
//            Two read-backs: places, long flags and the sum; then the table.  walk_parse_table runs per stream on the host.
//   decode   the chunks of all streams form ONE job list (bodies relative to d_src, targets in d_dst) for the in-place decode of the
//            single-stream call (stream_decode_jobs_in_place: stored chunks of all streams by one stream_place_kernel launch, groups by
//            range_group_ends); per-job verdicts become per-stream ones by mlz::batch_stream_verdicts.
//   encode   the blocks of all streams through one encode_device_locked and one crc_device_locked; 12 bytes per block visit the host, which
//            lays every stream out as stream_gather_range and stream_foot do for one; bodies, heads and feet by one stream_place_kernel
//            launch (the heads and feet are host-made bytes, uploaded once), chunk headers by one stream_hdr_kernel launch.
//            With search tables (mlz_stream_encode_batch_device_tables, include/minlz_hip_encode_batch_tables.h): the tables of all blocks by
//            the pre-folded block-list kernels of mlz_search_tables.hip.inc — a block's slot in c->d_stab has the size its LENGTH allows
//            (stab_fold_block), not the 2^(B - 3) bytes of the call's block size —, 12 more bytes per block to the host (table bytes, R, CRC;
//            the CRCs by one more crc_device_locked over the kept tables, behind one more synchronisation), the tables placed by the same
//            stream_place_kernel launch (the heads' and feet's bytes then lie in c->d_stab behind the tables and records: one third source),
//            their chunk headers by one stream_tabhdr_kernel launch.

namespace mlz {

static_assert(kBatchErrCorrupt == MLZ_ERR_CORRUPT && kBatchErrCrc == MLZ_ERR_CRC, "mlz_stream_batch.h restates the error codes");

// A lane per stream, one wavefront per workgroup.  EMIT = false: counts[i] = the stream's table entries (0 for a long stream) and bit
// (i & 63) of long_flags[i / 64] = the stream is long.  EMIT = true: the records of stream i at table[first[i]], counts[i] of them.
template <bool EMIT>
__global__ __launch_bounds__(64) void walk_batch_kernel(const uint8_t* __restrict__ src, const mlz_block_desc* __restrict__ streams, uint32_t n_streams,
                                                        uint32_t* __restrict__ counts, const uint32_t* __restrict__ first, WalkChunk* __restrict__ table,
                                                        uint64_t* __restrict__ long_flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    bool is_long = false;
    uint32_t cnt = 0;
    if (i < n_streams) {
        const uint64_t off = streams[i].src_off, n = streams[i].src_len;
        if (!EMIT) cnt = batch_walk_lane<false>(src + off, n, kBatchWalkSteps, nullptr, 0, &is_long);
        else if (counts[i]) batch_walk_lane<true>(src + off, n, kBatchWalkSteps, table + first[i], counts[i], &is_long);
    }
    if (!EMIT) {
        if (i < n_streams) counts[i] = cnt;
        const uint64_t m = __ballot(is_long);
        if (threadIdx.x == 0) long_flags[blockIdx.x] = m;
    }
}

}  // namespace mlz

namespace {

constexpr int kBatchMaxStreams = 1 << 20;

// The walk of a batch: every stream's data chunks in front of its first framing error, and what stream_parse returns for it.
struct BatchWalk {
    std::vector<StreamChunk> chunks;        // body_off and hdr_off count from d_src, out_off inside the stream's own output
    std::vector<size_t> c0, c1;             // stream i's chunks: [c0[i], c1[i])
    std::vector<int64_t> parsed;
    size_t n_long = 0;
    // what the stream decodes to: its size, or the bytes of the chunks in front of its framing error
    uint64_t prefix(size_t i) const { return parsed[i] >= 0 ? uint64_t(parsed[i]) : c1[i] == c0[i] ? 0 : uint64_t(chunks[c1[i] - 1].out_off + chunks[c1[i] - 1].n); }
};

// [p, p + end) lies inside the allocation that holds p (a descriptor that leaves it would send a kernel out of bounds); true where the
// runtime cannot tell
bool span_inside_allocation(const void* p, uint64_t end) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return true; }
    const uintptr_t b = reinterpret_cast<uintptr_t>(base), q = reinterpret_cast<uintptr_t>(p);
    return q >= b && end <= uint64_t(b) + size - q;
}

// The arguments every batch call checks, in front of anything it launches or writes.  *run = the per-device context that serves the call.
// Returns 0, 1 (n_streams == 0: nothing to do) or -MLZ_ERR_ARG.
int batch_args(mlz_ctx* c, const uint8_t* d_src, const uint8_t* d_dst, bool with_dst, const mlz_block_desc* streams, int n_streams, const int64_t* out_len, mlz_ctx** run) {
    if (!c || n_streams < 0 || n_streams > kBatchMaxStreams) return -MLZ_ERR_ARG;
    if (n_streams == 0) return 1;
    if (!streams || !out_len || !d_src || (with_dst && !d_dst)) return -MLZ_ERR_ARG;
    if (!(c = owner_of(c, d_src)) || !on_device(c, d_src) || (with_dst && !on_device(c, d_dst))) return -MLZ_ERR_ARG;
    const size_t n = size_t(n_streams);
    uint64_t src_end = 0, dst_end = 0;
    std::vector<std::pair<uint64_t, uint64_t>> d;
    for (size_t i = 0; i < n; i++) {
        const mlz_block_desc& s = streams[i];
        if (s.src_len > kWalkMaxStream || s.src_off > ~uint64_t(0) - s.src_len) return -MLZ_ERR_ARG;
        if (s.src_len) src_end = std::max(src_end, s.src_off + s.src_len);
        if (!with_dst || !s.dst_cap) continue;
        if (s.dst_off > ~uint64_t(0) - s.dst_cap) return -MLZ_ERR_ARG;
        dst_end = std::max(dst_end, s.dst_off + s.dst_cap);
        d.emplace_back(s.dst_off, s.dst_cap);
    }
    // two destinations that overlap: one stream's bytes would change another's
    std::sort(d.begin(), d.end());
    for (size_t i = 1; i < d.size(); i++) if (d[i].first < d[i - 1].first + d[i - 1].second) return -MLZ_ERR_ARG;
    if (enter_device(c)) return -MLZ_ERR_ARG;
    if (!span_inside_allocation(d_src, src_end) || (with_dst && !span_inside_allocation(d_dst, dst_end))) return -MLZ_ERR_ARG;
    *run = c;
    return 0;
}

// The chunk walk of every stream of the batch.  Returns 0, -MLZ_ERR_ARG (more than 2^32 - 1 table entries could come) or -MLZ_ERR_HIP.
// Synchronous on st.  Caller holds c->mu.
int stream_batch_walk(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, const mlz_block_desc* streams, size_t n, BatchWalk* bw) {
    bw->chunks.clear();
    bw->c0.assign(n, 0); bw->c1.assign(n, 0); bw->parsed.assign(n, 0);
    bw->n_long = 0;
    c->batch_long = 0;
    HIPCHK(c, hipSetDevice(c->device));
    // the table's entries are counted in 32 bits: a lane adds at most one per step and per four bytes (and a stub)
    uint64_t most = 0;
    for (size_t i = 0; i < n; i++) most += std::min<uint64_t>(mlz::kBatchWalkSteps, streams[i].src_len / 4 + 1);
    if (most > 0xffffffffull) return -MLZ_ERR_ARG;
    const size_t nwg = (n + 63) / 64;
    Carve cv;   // counts | total | long flags | first: the last three come back together
    const auto r_cnt = cv.take<uint32_t>(n), r_total = cv.take<uint32_t>(4);
    const auto r_long = cv.take<uint64_t>(nwg);
    const auto r_first = cv.take<uint32_t>(n, 8);
    const size_t back = cv.bytes - r_total.off;
    HIPCHK(c, c->d_batch.ensure(cv.bytes));
    HIPCHK(c, c->d_batch_desc.ensure(n * sizeof(mlz_block_desc)));
    int r = ensure_stream_objects(c, 0, back);
    if (r) return r;
    void* ws = c->d_batch.p;
    uint32_t *counts = r_cnt.at(ws), *total = r_total.at(ws), *first = r_first.at(ws);
    uint64_t* long_flags = r_long.at(ws);
    mlz_block_desc* d_desc = c->d_batch_desc.as<mlz_block_desc>();
    std::vector<uint32_t> h_first(n + 1, 0);
    std::vector<uint64_t> h_long(nwg, 0);
    {
        WorkspaceOrder order(c, st);
        HIPCHK(c, hipMemcpyAsync(d_desc, streams, n * sizeof(mlz_block_desc), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mlz::walk_batch_kernel<false>, dim3(uint32_t(nwg)), dim3(64), 0, st, d_src, d_desc, uint32_t(n), counts, first, static_cast<mlz::WalkChunk*>(nullptr), long_flags);
        hipLaunchKernelGGL(mlz::walk_scan_kernel, dim3(1), dim3(1024), 0, st, counts, uint32_t(n), first, total);
        if ((r = fetch(c, st, c->pinned2, total, back))) return r;
        const uint8_t* h = static_cast<const uint8_t*>(c->pinned2);
        h_first[n] = *reinterpret_cast<const uint32_t*>(h);
        std::memcpy(h_long.data(), h + (r_long.off - r_total.off), nwg * sizeof(uint64_t));
        std::memcpy(h_first.data(), h + (r_first.off - r_total.off), n * sizeof(uint32_t));
        const size_t h_total = h_first[n];
        if (h_total) {
            HIPCHK(c, c->d_walk_tab.ensure(h_total * sizeof(mlz::WalkChunk)));
            if ((r = ensure_stream_objects(c, 0, h_total * sizeof(mlz::WalkChunk)))) return r;
            mlz::WalkChunk* tab = c->d_walk_tab.as<mlz::WalkChunk>();
            hipLaunchKernelGGL(mlz::walk_batch_kernel<true>, dim3(uint32_t(nwg)), dim3(64), 0, st, d_src, d_desc, uint32_t(n), counts, first, tab, long_flags);
            if ((r = fetch(c, st, c->pinned2, tab, h_total * sizeof(mlz::WalkChunk)))) return r;
        }
    }
    const mlz::WalkChunk* table = static_cast<const mlz::WalkChunk*>(c->pinned2);
    auto is_long = [&](size_t i) { return ((h_long[i >> 6] >> (i & 63)) & 1) != 0; };
    bw->chunks.reserve(h_first[n]);
    for (size_t i = 0; i < n; i++) {
        if (is_long(i)) { bw->n_long++; continue; }
        if (h_first[i + 1] < h_first[i]) { c->err = "stream_batch_walk: the table's places do not ascend"; return -MLZ_ERR_HIP; }
        const uint64_t base = streams[i].src_off;
        bw->c0[i] = bw->chunks.size();
        bw->parsed[i] = mlz::walk_parse_table(table + h_first[i], h_first[i + 1] - h_first[i], kMaxBlockSize, stream_chunk_sink(&bw->chunks, base));
        bw->c1[i] = bw->chunks.size();
    }
    // long streams: the region walk, one after the other (it takes c->pinned2 and c->d_walk_tab over: the batch's table is spent by now)
    std::vector<StreamChunk> one;
    for (size_t i = 0; bw->n_long && i < n; i++) {
        if (!is_long(i)) continue;
        const uint64_t base = streams[i].src_off;
        if ((r = stream_walk_device(c, st, d_src + base, size_t(streams[i].src_len), &one, &bw->parsed[i]))) return r;
        bw->c0[i] = bw->chunks.size();
        for (StreamChunk ck : one) { ck.body_off += size_t(base); ck.hdr_off += size_t(base); bw->chunks.push_back(ck); }
        bw->c1[i] = bw->chunks.size();
    }
    c->batch_long = bw->n_long;
    return 0;
}

// mlz_stream_decode_batch_device behind its argument checks.  Returns 0 or -MLZ_ERR_*; the streams' results go to out_len.
int64_t stream_decode_batch_locked(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* streams, size_t n, int64_t* out_len) {
    BatchWalk bw;
    int r = stream_batch_walk(c, sm, d_src, streams, n, &bw);
    if (r) return r;
    begin_decode_call(c);
    // one job list: every stream's chunks in its own order, stream after stream; a stream that does not fit its destination brings none
    std::vector<int64_t> verdict(bw.parsed);
    std::vector<size_t> job_first(n + 1, 0);
    std::vector<ChunkJob> jobs;
    jobs.reserve(bw.chunks.size());
    for (size_t i = 0; i < n; i++) {
        job_first[i] = jobs.size();
        if (bw.prefix(i) > streams[i].dst_cap) { verdict[i] = -MLZ_ERR_DST_TOO_SMALL; continue; }
        for (size_t k = bw.c0[i]; k < bw.c1[i]; k++) jobs.push_back(ChunkJob{k, d_dst + streams[i].dst_off + bw.chunks[k].out_off});
    }
    job_first[n] = jobs.size();
    std::vector<int64_t> job_rc;
    const int64_t e = stream_decode_jobs_in_place(c, sm, ignore_crc, d_src, bw.chunks, jobs, d_dst, &job_rc);
    if (e) return e;
    mlz::batch_stream_verdicts(verdict.data(), job_first.data(), job_rc.data(), n, out_len);
    return 0;
}

// mlz_stream_encode_batch_device and _tables behind their argument checks: stb.T = 0 gives plain streams, else every stream carries the
// search tables of that configuration, as stream_gather_range writes them for one range.
int64_t stream_encode_batch_locked(mlz_ctx* c, hipStream_t sm, int level, uint32_t bs, bool add_index, const StreamTables& stb, const uint8_t* d_src, uint8_t* d_dst,
                                   const mlz_block_desc* streams, size_t n, int64_t* out_len) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t ostride = (size_t(bs) + 16 + 63) & ~size_t(63);
    const uint32_t search_b = mlz::search_table_bits(bs), flen = stb.flen(), thdr = 12 + flen;   // thdr: a table chunk's bytes in front of its table
    std::vector<mlz::StabFoldBlock> tlist;   // with tables: every block's record, its slot carved from tab_bytes
    uint64_t tab_bytes = 0;
    uint32_t min_r0 = search_b;
    c->table_slot_bytes = 0;
    // the blocks of every stream that has room, stream after stream: block_first[i] = stream i's first
    std::vector<size_t> block_first(n + 1, 0);
    std::vector<mlz_block_desc> desc;
    size_t max_pieces = 0, misc_bound = 0;
    for (size_t i = 0; i < n; i++) {
        block_first[i] = desc.size();
        const uint64_t len = streams[i].src_len;
        out_len[i] = 0;
        if (streams[i].dst_cap < stream_bound(len, bs, add_index, stb)) { out_len[i] = -MLZ_ERR_DST_TOO_SMALL; continue; }
        const size_t cnt = size_t((len + bs - 1) / bs);
        for (size_t b = 0; b < cnt; b++) {
            const size_t q = desc.size();
            const uint64_t at = b * uint64_t(bs), blen = std::min<uint64_t>(bs, len - at);
            desc.push_back(mlz_block_desc{streams[i].src_off + at, blen, q * ostride, ostride});
            if (!stb.T) continue;
            const uint64_t before = tab_bytes;
            tlist.push_back(stab_fold_block(streams[i].src_off + at, uint32_t(blen), len - at - blen, stb.T, stb.field, stb.M, search_b, &tab_bytes));
            min_r0 = std::min(min_r0, tlist.back().r0);
            max_pieces += size_t((tab_bytes - before + kPlacePiece - 1) / kPlacePiece);
        }
        const size_t foot_bound = 16 + (add_index ? SeekIndex::bound(cnt) : 0);
        max_pieces += cnt * ((size_t(bs) + kPlacePiece - 1) / kPlacePiece + 1) + 2 + foot_bound / kPlacePiece;
        misc_bound += stb.head_bytes() + foot_bound;
    }
    block_first[n] = desc.size();
    const size_t nblk = desc.size();
    if (nblk > size_t(0x7fffffff)) return -MLZ_ERR_ARG;
    const size_t tcnt = stb.T ? nblk : 0;
    Carve pin;   // what comes back: sizes | CRCs | (table bytes or 0, R) | table CRCs; what goes up: pieces | chunk headers | table chunk headers | the heads' and feet's bytes | the tables' block list
    const auto r_len = pin.take<int64_t>(nblk);
    const auto r_crc = pin.take<uint32_t>(nblk);
    const auto r_tabinfo = pin.take<uint2>(tcnt);
    const auto r_tabcrc = pin.take<uint32_t>(tcnt);
    const auto r_place = pin.take<PlaceDesc>(max_pieces, 64);
    const auto r_hdr = pin.take<HdrDesc>(nblk);
    const auto r_tabhdr = pin.take<TabHdrDesc>(tcnt);
    const auto r_misc = pin.take<uint8_t>(misc_bound, 64);
    const auto r_tlist = pin.take<mlz::StabFoldBlock>(tcnt, 64);
    Carve tabs;   // c->d_stab with tables: the blocks' slots | their records | their block list | the heads' and feet's bytes (the place kernel's third source holds tables and these)
    const auto t_slots = tabs.take<uint8_t>(size_t(tab_bytes), 64);
    const auto t_info = tabs.take<uint2>(tcnt);
    const auto t_list = tabs.take<mlz::StabFoldBlock>(tcnt, 64);
    const auto t_misc = tabs.take<uint8_t>(misc_bound, 64);
    int r = ensure_stream_objects(c, 0, pin.bytes);
    if (r) return r;
    int64_t* h_len = r_len.at(c->pinned2);
    uint32_t* h_crc = r_crc.at(c->pinned2);
    PlaceDesc* h_place = r_place.at(c->pinned2);
    HdrDesc* h_hdr = r_hdr.at(c->pinned2);
    uint8_t* h_misc = r_misc.at(c->pinned2);
    uint2* h_tabinfo = r_tabinfo.at(c->pinned2);
    uint32_t* h_tabcrc = r_tabcrc.at(c->pinned2);
    TabHdrDesc* h_tabhdr = r_tabhdr.at(c->pinned2);
    { WorkspaceOrder order(c, sm); }   // (a batch of empty streams launches only the place kernel: ordered behind the workspace's last user all the same)
    if (stb.T) HIPCHK(c, c->d_stab.ensure(tabs.bytes + 64));
    uint8_t* d_out = nullptr;
    if (nblk) {
        HIPCHK(c, c->d_out.ensure(nblk * ostride + 64));
        HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * nblk));
        HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * nblk + 64));
        d_out = c->d_out.as<uint8_t>();
        if ((r = encode_device_locked(c, sm, level, d_src, d_out, desc.data(), int(nblk), c->d_len.as<int64_t>(), true))) return r;
        if ((r = crc_device_locked(c, sm, d_src, desc.data(), int(nblk), c->d_crc.as<uint32_t>()))) return r;
        if (tcnt) {
            mlz::StabFoldBlock* d_list = t_list.at(c->d_stab.p);
            std::memcpy(r_tlist.at(c->pinned2), tlist.data(), tcnt * sizeof(mlz::StabFoldBlock));
            HIPCHK(c, hipMemcpyAsync(d_list, r_tlist.at(c->pinned2), tcnt * sizeof(mlz::StabFoldBlock), hipMemcpyHostToDevice, sm));
            if ((r = search_tables_build_prefolded(c, sm, d_src, d_list, tcnt, bs, min_r0, tab_bytes, stb.T, stb.field, stb.M, search_b, c->d_stab.as<uint32_t>(), t_info.at(c->d_stab.p)))) return r;
            HIPCHK(c, hipMemcpyAsync(h_tabinfo, t_info.at(c->d_stab.p), sizeof(uint2) * tcnt, hipMemcpyDeviceToHost, sm));
        }
        HIPCHK(c, hipMemcpyAsync(h_len, c->d_len.p, sizeof(int64_t) * nblk, hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipMemcpyAsync(h_crc, c->d_crc.p, sizeof(uint32_t) * nblk, hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
        HIPCHK(c, hipGetLastError());
        c->table_slot_bytes = tab_bytes;
    }
    // a table goes in front of a block that was stored compressed (writer.go:528-540); its CRC is the stream's, over the table's bytes:
    // the kept tables through the CRC pass once more.  tab_at[b]: block b's place among them.
    std::vector<uint32_t> tab_at(tcnt, 0);
    size_t n_tabs = 0;
    if (tcnt) {
        std::vector<mlz_block_desc> tdesc;
        for (size_t b = 0; b < nblk; b++) {
            if (h_len[b] < 0 || chunk_shape(h_len[b], size_t(desc[b].src_len)).stored) h_tabinfo[b].x = 0;
            if (!h_tabinfo[b].x) continue;
            tab_at[b] = uint32_t(tdesc.size());
            tdesc.push_back(mlz_block_desc{tlist[b].tab_off, h_tabinfo[b].x, 0, 0});
        }
        n_tabs = tdesc.size();
        if (n_tabs) {
            HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * (nblk + n_tabs) + 64));
            if ((r = crc_device_locked(c, sm, c->d_stab.as<uint8_t>(), tdesc.data(), int(n_tabs), c->d_crc.as<uint32_t>()))) return r;
            HIPCHK(c, hipMemcpyAsync(h_tabcrc, c->d_crc.p, sizeof(uint32_t) * n_tabs, hipMemcpyDeviceToHost, sm));
            HIPCHK(c, hipStreamSynchronize(sm));
            HIPCHK(c, hipGetLastError());
        }
    }
    // every stream's layout: [identifier][type len24 crc body]...[EOF][index], from its dst_off on
    size_t n_place = 0, n_hdr = 0, n_misc = 0, n_tabhdr = 0;
    const size_t misc_base = stb.T ? t_misc.off : 0;   // where the heads' and feet's bytes start in the place kernel's third source
    auto put_piece = [&](const PlaceDesc& d) { h_place[n_place++] = d; };
    std::vector<uint32_t> framed;
    for (size_t i = 0; i < n; i++) {
        if (out_len[i] < 0) continue;
        const size_t b0 = block_first[i], cnt = block_first[i + 1] - b0;
        const uint64_t len = streams[i].src_len, base = streams[i].dst_off;
        int64_t bad = 0;
        for (size_t b = b0; b < b0 + cnt && !bad; b++) if (h_len[b] < 0) bad = h_len[b];
        if (bad) { out_len[i] = bad; continue; }
        framed.assign(cnt, 0);
        if (len > 0) {
            put_stream_head(h_misc + n_misc, bs, stb);
            put_piece(PlaceDesc{misc_base + n_misc, base, stb.head_bytes(), 2});
            n_misc += stb.head_bytes();
        }
        uint64_t o = base + stb.head_bytes();
        for (size_t b = b0; b < b0 + cnt; b++) {
            const ChunkShape s = chunk_shape(h_len[b], size_t(desc[b].src_len));
            if (tcnt && h_tabinfo[b].x) {   // 45 len24 | T M B | prefix field | R | crc32le | table (stream_gather_range's layout)
                const uint32_t tb = h_tabinfo[b].x, tlen = thdr - 4 + tb;
                TabHdrDesc& th = h_tabhdr[n_tabhdr++];
                th.dst_off = o; th.n = thdr;
                th.b[0] = mlz::kChunkSearchTable; th.b[1] = uint8_t(tlen); th.b[2] = uint8_t(tlen >> 8); th.b[3] = uint8_t(tlen >> 16);
                th.b[4] = uint8_t(stb.T); th.b[5] = uint8_t(stb.M); th.b[6] = uint8_t(search_b);
                const uint32_t inl = stb.T == 4 ? 0 : flen;   // the field's bytes inside the record
                std::memcpy(th.b + 7, stb.field, inl);
                th.b[7 + inl] = uint8_t(h_tabinfo[b].y);
                std::memcpy(th.b + 8 + inl, &h_tabcrc[tab_at[b]], 4);
                place_pieces(tlist[b].tab_off, o + thdr, tb, 2, put_piece);
                framed[b - b0] = thdr + tb;
                o += thdr + tb;
            }
            h_hdr[n_hdr].dst_off = o;
            put_chunk_header(h_hdr[n_hdr].b, s, h_crc[b]);
            n_hdr++;
            place_pieces(s.stored ? desc[b].src_off : desc[b].dst_off + 1, o + 8, s.body, s.stored ? 1 : 0, put_piece);
            framed[b - b0] += uint32_t(8 + s.body);
            o += 8 + s.body;
        }
        size_t at = 0;
        const std::vector<uint8_t> foot = stream_foot(size_t(len), bs, stb.head_bytes(), framed, add_index, &at);
        std::memcpy(h_misc + n_misc, foot.data(), foot.size());
        place_pieces(misc_base + n_misc, base + at, foot.size(), 2, put_piece);
        n_misc += foot.size();
        out_len[i] = int64_t(at + foot.size());
    }
    if (n_place > max_pieces || n_misc > misc_bound || n_tabhdr > n_tabs) { c->err = "stream_encode_batch: the layout passed its bound"; return -MLZ_ERR_HIP; }
    if (n_place) {
        Carve up;
        const auto u_place = up.take<PlaceDesc>(n_place);
        const auto u_hdr = up.take<HdrDesc>(n_hdr);
        const auto u_tabhdr = up.take<TabHdrDesc>(n_tabhdr);
        const auto u_misc = up.take<uint8_t>(stb.T ? 0 : n_misc, 64);
        HIPCHK(c, c->d_place.ensure(up.bytes));
        PlaceDesc* d_place = u_place.at(c->d_place.p);
        HdrDesc* d_hdr = u_hdr.at(c->d_place.p);
        // the third source: the heads' and feet's bytes; with tables c->d_stab, which holds them behind the tables
        uint8_t* d_third = stb.T ? c->d_stab.as<uint8_t>() : u_misc.at(c->d_place.p);
        HIPCHK(c, hipMemcpyAsync(d_place, h_place, n_place * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
        if (n_hdr) HIPCHK(c, hipMemcpyAsync(d_hdr, h_hdr, n_hdr * sizeof(HdrDesc), hipMemcpyHostToDevice, sm));
        HIPCHK(c, hipMemcpyAsync(d_third + misc_base, h_misc, n_misc, hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(stream_place_kernel, dim3(uint32_t(n_place)), dim3(256), 0, sm, d_out, d_src, d_third, d_dst, d_place);
        if (n_tabhdr) {
            TabHdrDesc* d_tabhdr = u_tabhdr.at(c->d_place.p);
            HIPCHK(c, hipMemcpyAsync(d_tabhdr, h_tabhdr, n_tabhdr * sizeof(TabHdrDesc), hipMemcpyHostToDevice, sm));
            TabLongField lf{};
            if (stb.T == 4) { lf.n = flen; std::memcpy(lf.b, stb.field, flen); }
            hipLaunchKernelGGL(stream_tabhdr_kernel, dim3(uint32_t((n_tabhdr + 63) / 64)), dim3(64), 0, sm, d_dst, d_tabhdr, uint32_t(n_tabhdr), lf);
        }
        if (n_hdr) hipLaunchKernelGGL(stream_hdr_kernel, dim3(uint32_t((n_hdr + 63) / 64)), dim3(64), 0, sm, d_dst, d_hdr, uint32_t(n_hdr));
        HIPCHK(c, hipStreamSynchronize(sm));
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

StreamTables sidecar_config(const mlz_search_config& q);   // mlz_stream_sidecar.hip.inc: the checks of the three single Writer calls, over the one struct of all four types

// An mlz_search_config (NULL: no tables) with the call's flags -> the Writer's configuration
StreamTables batch_tables_config(uint32_t flags, const mlz_search_config* cfg) {
    if (!cfg) return stream_tables_config(flags, nullptr);
    if (flags & (MLZ_STREAM_SEARCH_TABLES | MLZ_STREAM_SEARCH_MATCH_LEN(15))) return no_stream_tables();
    return sidecar_config(*cfg);
}

}  // namespace

extern "C" {

int mlz_stream_decoded_len_batch_device(mlz_ctx* c, void* stream, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, int64_t* out_len, uint64_t* prefix_len) {
    const int a = batch_args(c, d_src, nullptr, false, streams, n_streams, out_len, &c);
    if (a) return a < 0 ? a : 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    BatchWalk bw;
    const int r = int(settled(sm, stream_batch_walk(c, sm, d_src, streams, size_t(n_streams), &bw)));
    if (r) return r;
    for (size_t i = 0; i < size_t(n_streams); i++) {
        out_len[i] = bw.parsed[i];
        if (prefix_len) prefix_len[i] = bw.prefix(i);
    }
    return 0;
}

int mlz_stream_decode_batch_device(mlz_ctx* c, void* stream, uint32_t flags, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* streams, int n_streams,
                                   int64_t* out_len) {
    const int a = batch_args(c, d_src, d_dst, true, streams, n_streams, out_len, &c);
    if (a) return a < 0 ? a : 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return int(settled(sm, stream_decode_batch_locked(c, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, d_src, d_dst, streams, size_t(n_streams), out_len)));
}

int mlz_stream_encode_batch_device(mlz_ctx* c, void* stream, int level, uint32_t block_size, uint32_t flags, const uint8_t* d_src, uint8_t* d_dst,
                                   const mlz_block_desc* streams, int n_streams, int64_t* out_len) {
    if (!c || n_streams < 0 || n_streams > kBatchMaxStreams) return -MLZ_ERR_ARG;
    if (block_size < kMinStreamBlock || block_size > kMaxBlockSize) return -MLZ_ERR_ARG;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    if (flags & (MLZ_STREAM_SEARCH_TABLES | MLZ_STREAM_SEARCH_MATCH_LEN(15))) return -MLZ_ERR_ARG;   // tables in batches: out of scope
    const int a = batch_args(c, d_src, d_dst, true, streams, n_streams, out_len, &c);
    if (a) return a < 0 ? a : 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return int(settled(sm, stream_encode_batch_locked(c, sm, level, block_size, (flags & MLZ_STREAM_ADD_INDEX) != 0, StreamTables(), d_src, d_dst, streams, size_t(n_streams), out_len)));
}

// ---- include/minlz_hip_encode_batch_tables.h ----

int64_t mlz_stream_bound_config(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_config* cfg) {
    return stream_bound_checked(n, block_size, flags, batch_tables_config(flags, cfg));
}

int64_t mlz_search_table_prefold(uint64_t marks, uint32_t B, uint32_t table_type) {
    if (B < 8 || B > 23 || table_type < 1 || table_type > 4 || marks > (uint64_t(1) << 32)) return -MLZ_ERR_ARG;
    return int64_t(mlz::search_prefold(marks, B, mlz::search_fold_limit(table_type)));
}

int mlz_stream_encode_batch_device_tables(mlz_ctx* c, void* stream, int level, uint32_t block_size, uint32_t flags, const mlz_search_config* cfg, const uint8_t* d_src,
                                          uint8_t* d_dst, const mlz_block_desc* streams, int n_streams, int64_t* out_len) {
    if (!cfg) return mlz_stream_encode_batch_device(c, stream, level, block_size, flags, d_src, d_dst, streams, n_streams, out_len);
    if (!c || n_streams < 0 || n_streams > kBatchMaxStreams) return -MLZ_ERR_ARG;
    if (block_size < kMinStreamBlock || block_size > kMaxBlockSize) return -MLZ_ERR_ARG;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    if (flags & MLZ_STREAM_SEARCH_COMPRESS) return -MLZ_ERR_ARG;   // 0x46 in batches: out of scope (the header says why)
    const StreamTables stb = batch_tables_config(flags, cfg);
    if (!stb.valid) return -MLZ_ERR_ARG;
    const int a = batch_args(c, d_src, d_dst, true, streams, n_streams, out_len, &c);
    if (a) return a < 0 ? a : 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return int(settled(sm, stream_encode_batch_locked(c, sm, level, block_size, (flags & MLZ_STREAM_ADD_INDEX) != 0, stb, d_src, d_dst, streams, size_t(n_streams), out_len)));
}

}  // extern "C"
