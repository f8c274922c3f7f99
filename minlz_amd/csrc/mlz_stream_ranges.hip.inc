// mlz_stream_ranges.hip.inc — the device-resident ReadSeeker: range reads of a .mz stream that lies in HBM (included at the end of
// mlz_hip.hip, behind mlz_stream_walk.hip.inc whose walk and chunk-list decode it uses).
//
// Reader.ReadSeeker / ReadSeeker.ReadAt (reader.go:1322-1487) over Index.Find (index.go:114), with the chunk table of the device walk in
// the place of the seek index: mlz_stream_open_device walks the stream once and keeps the table of its data chunks on the host;
// mlz_dev_reader_read plans the ranges of a call against it (plan_ranges, mlz_stream_ranges.h: the touched chunks, each decoded once — in
// its place in the destination when one range covers it wholly, else in the context's scratch —, in groups of about 64 MiB), runs the
// groups through stream_run_chunk_jobs (decode, CRC over whole chunks, verdicts in stream order) and moves the wanted parts of partly
// wanted chunks, and of stored chunks from the stream itself, with ONE launch of stream_range_copy_kernel per group.

namespace mlz {

// Pieces of at most this many bytes are copied by 16 lanes each (four to a wavefront), longer ones by a workgroup each.  (0 builds the
// library with one workgroup per piece throughout: tools/stream_ranges_time.py times the copy both ways.)
#ifndef MLZ_RANGE_SHORT_MAX
#define MLZ_RANGE_SHORT_MAX 1024
#endif
constexpr uint32_t kRangeShortMax = MLZ_RANGE_SHORT_MAX;
constexpr uint32_t kRangeShortPerWg = 16;   // 256 threads / 16 lanes

// descs[0, n_long): a workgroup per piece (wg_copy, as stream_place_kernel); descs[n_long, n_all): 16 lanes per piece.  desc.pad selects the
// source (0 = the scratch, 1 = the stream: stored chunks).  The short form stores destination-aligned 16-byte vectors, lane i of a piece's
// 16 at aligned base + 16 i (+ 256 per further round); the ragged first and last vector are written bytewise by their lane; a full vector's
// 16 source bytes are loaded from where they lie, at whatever alignment, so no byte outside the piece is read or written.
__device__ __forceinline__ void lanes16_copy(uint8_t* o, const uint8_t* s, uint32_t len, uint32_t lane) {
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(o) & 15);
    s -= mis;   // s + x is the source of destination byte (o - mis) + x; only x in [mis, end) is touched
    o -= mis;
    const uint32_t end = mis + len;
    for (uint32_t lo = lane * 16; lo < end; lo += 256) {
        if (lo >= mis && lo + 16 <= end) {
            uint4 x;
            __builtin_memcpy(&x, s + lo, 16);
            *reinterpret_cast<uint4*>(o + lo) = x;
        } else {
            const uint32_t b = lo > mis ? lo : mis, e = lo + 16 < end ? lo + 16 : end;
            for (uint32_t k = b; k < e; k++) o[k] = s[k];
        }
    }
}

__global__ __launch_bounds__(256) void stream_range_copy_kernel(const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ stream, uint8_t* __restrict__ dst,
                                                                const PlaceDesc* __restrict__ descs, uint32_t n_long, uint32_t n_all) {
    if (blockIdx.x < n_long) {
        const PlaceDesc d = descs[blockIdx.x];
        wg_copy(dst + d.dst_off, (d.pad ? stream : scratch) + d.src_off, d.len, threadIdx.x, 256);
        return;
    }
    const uint32_t idx = n_long + (blockIdx.x - n_long) * kRangeShortPerWg + (threadIdx.x >> 4);
    if (idx >= n_all) return;
    const PlaceDesc d = descs[idx];
    lanes16_copy(dst + d.dst_off, (d.pad ? stream : scratch) + d.src_off, d.len, threadIdx.x & 15);
}

}  // namespace mlz

// A stream opened for range reads: the walk's result.  Refers to the caller's d_src and to the (per-device) context.
struct mlz_dev_reader {
    mlz_ctx* ctx = nullptr;
    void* d_chunks = nullptr;                 // `dchunks` where the plan kernels can read it, uploaded by the first mlz_dev_reader_read_device
    const uint8_t* d_src = nullptr;
    size_t n = 0;
    int64_t size = 0;
    std::vector<StreamChunk> chunks;          // the data chunks: body offset and length, decoded length, CRC, type, output offset
    std::vector<mlz::RdevChunk> dchunks;      // the planners' and the plan kernels' view of them
    uint32_t n_ident = 0;                     // stream identifiers in the stream (more than one: concatenated streams)
    uint8_t ident_byte = 0;                   // the first identifier's block-size byte, which a sidecar repeats
    // mlz_dev_reader_search: a stream's table sets — the configuration (T, M, B, prefix field) of each and every data chunk's table of each.
    // search[]: the one set of the stream's inline tables (its info chunk), found by the first search of the handle ([0]: table CRCs checked,
    // [1]: under MLZ_STREAM_IGNORE_CRC); side: the sets of the attached sidecar (mlz_dev_reader_attach_sidecar), which the searches use while side_on.
    struct SearchTables {
        bool ready = false;
        uint32_t ncfg = 0;                    // 0: no usable info chunk
        mlz::SearchConfig cfg[mlz::kSidecarMaxConfigs] = {};
        const uint8_t* base = nullptr;        // the tables' offsets count from here: the stream, or the sidecar
        void* d_tabs = nullptr;               // mlz::SearchTab per (set, data chunk), set by set; device memory the handle owns
        void* d_arena = nullptr;              // the expanded bitmaps of the sets' compressed tables (0x46), device memory the handle owns
        size_t arena_bytes = 0;
        std::vector<mlz::SearchTab> tabs;
    } search[2], side;
    bool side_on = false;
    // mlz_dev_reader_index_records: the positions of all delimiters of the decoded stream (8 bytes each; device memory the handle owns, not
    // part of the context's workspace), kept until the handle closes or another delimiter is indexed
    void* d_index = nullptr;
    uint64_t index_cap = 0, index_k = 0, index_n = 0;   // entries allocated, delimiters, records
    bool index_ready = false;
    uint8_t index_delim = 0;
    // mlz_dev_reader_grep_regex (mlz_stream_regex.hip.inc): the length of the index's longest record, found by the first such call and kept
    // beside the index; whatever replaces the index clears longest_ready
    uint64_t index_longest = 0;
    bool index_longest_ready = false;
    // mlz_stream_open_batch_device (mlz_stream_set.hip.inc): a set of streams behind one handle.  bases: count + 1 values, stream i's decoded
    // bytes are [bases[i], bases[i + 1]) of the handle ({0, size} for a handle of one stream); d_bases: the same where kernels can read them
    // (device memory the handle owns, uploaded by the first call that needs them).  A set searches without inline tables and takes no sidecar.
    bool set = false;
    std::vector<uint64_t> bases;
    void* d_bases = nullptr;
    // mlz_stream_open_batch_device_tables (mlz_stream_set_tables.hip.inc): a set whose searches use every stream's inline tables.  The open
    // leaves st (a descriptor's source span and its chunks in the handle's list; mode = whole or skipped); the first search finds the classes
    // (cls, prunable) once and every data chunk's table once per CRC mode (search[]: set c = class c, ncfg = the classes that prune).
    // d_chunks: mlz::SetTabChunk per data chunk; cross[0] / d_cross[0]: the streams' crossing flags of a position call, [1]: of a
    // record-bound call, made anew when the record index is replaced.  info: what mlz_dev_reader_set_tables_info reports.
    struct SetTabled {
        bool on = false, classed = false, cross_ready[2] = {false, false};
        uint32_t classes = 0, ncls = 0;
        uint64_t expansions = 0;             // 0x46 tables that stand expanded in search[]'s arenas
        std::vector<mlz::BatchPlanStream> st;
        std::vector<uint8_t> prunable, cross[2];
        mlz::SearchConfig cfg[mlz::kSidecarMaxConfigs] = {};
        void *d_chunks = nullptr, *d_cross[2] = {nullptr, nullptr};
        uint64_t info[mlz::kSetTabInfoValues] = {};
    } tabled;
};

namespace {

static_assert(sizeof(mlz_range) == sizeof(mlz::ByteRange) && offsetof(mlz_range, dst_off) == offsetof(mlz::ByteRange, dst_off), "mlz_range is the planner's ByteRange");

int64_t dev_reader_read_locked(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const mlz::RangePlan& plan, uint8_t* d_dst) {
    mlz_ctx* c = rd->ctx;
    const size_t nt = plan.touched.size();
    if (nt == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    size_t n_pieces = 0;
    for (const mlz::RangeSeg& sg : plan.segs) n_pieces += size_t((sg.len + kPlacePiece - 1) / kPlacePiece);
    if (plan.scratch_max) HIPCHK(c, c->d_range.ensure(size_t(plan.scratch_max)));
    if (n_pieces) HIPCHK(c, c->d_place.ensure(n_pieces * sizeof(PlaceDesc)));
    Carve pin;
    const ChunkJobResults res = take_chunk_job_results(&pin, nt);
    const auto r_place = pin.take<PlaceDesc>(n_pieces, 64);
    int r = ensure_stream_objects(c, 0, pin.bytes);
    if (r) return r;
    PlaceDesc* h_place = r_place.at(c->pinned2);
    const uint8_t* scratch = c->d_range.as<uint8_t>();
    std::vector<ChunkJob> jobs(nt);
    for (size_t t = 0; t < nt; t++) {
        const mlz::RangeTouched& tc = plan.touched[t];
        const StreamChunk& ck = rd->chunks[tc.chunk];
        jobs[t] = ChunkJob{tc.chunk, tc.where == mlz::kRangeDirect ? d_dst + tc.at : tc.where == mlz::kRangeScratch ? scratch + tc.at : rd->d_src + ck.body_off};
    }
    std::vector<size_t> gend(plan.groups.size());
    for (size_t g = 0; g < gend.size(); g++) gend[g] = plan.groups[g].t1;
    size_t placed = 0;
    // a group's segments, cut into pieces of 64 KiB: the long ones in front, the short ones behind; built while the group's decode runs
    auto copy_group = [&](size_t g) -> int {
        const mlz::RangeGroup& gr = plan.groups[g];
        size_t n_long = 0, n_short = 0;
        for (size_t s = gr.s0; s < gr.s1; s++) {
            const uint64_t len = plan.segs[s].len, full = len / kPlacePiece, rest = len % kPlacePiece;
            n_long += size_t(full);
            if (rest) (rest <= mlz::kRangeShortMax ? n_short : n_long)++;
        }
        if (n_long + n_short == 0) return 0;
        PlaceDesc* out = h_place + placed;
        size_t ql = 0, qs = n_long;
        for (size_t s = gr.s0; s < gr.s1; s++) {
            const mlz::RangeSeg& sg = plan.segs[s];
            const mlz::RangeTouched& tc = plan.touched[sg.touched];
            const bool stored = tc.where == mlz::kRangeStored;
            const uint64_t from = (stored ? uint64_t(rd->chunks[tc.chunk].body_off) : tc.at) + sg.rel;
            place_pieces(from, sg.dst_off, sg.len, stored ? 1u : 0u, [&](const PlaceDesc& d) { out[d.len <= mlz::kRangeShortMax ? qs++ : ql++] = d; });
        }
        PlaceDesc* d_place = c->d_place.as<PlaceDesc>() + placed;
        HIPCHK(c, hipMemcpyAsync(d_place, out, (n_long + n_short) * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
        const size_t grid = n_long + (n_short + mlz::kRangeShortPerWg - 1) / mlz::kRangeShortPerWg;
        hipLaunchKernelGGL(mlz::stream_range_copy_kernel, dim3(uint32_t(grid)), dim3(256), 0, sm, scratch, rd->d_src, d_dst, d_place, uint32_t(n_long), uint32_t(n_long + n_short));
        placed += n_long + n_short;
        return 0;
    };
    {   // (a call that only copies stored chunks launches nothing else: its copies are ordered behind the workspace's last user all the same)
        WorkspaceOrder order(c, sm);
    }
    return stream_run_chunk_jobs(c, sm, ignore_crc, rd->d_src, rd->chunks, jobs, gend, res, copy_group);
}

}  // namespace

extern "C" {

int64_t mlz_stream_open_device(mlz_ctx* c, void* stream, const uint8_t* d_src, size_t n, mlz_dev_reader** out) {
    if (out) *out = nullptr;
    if (!out || !(c = stream_ctx(c, d_src, n))) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    mlz_dev_reader* rd = new (std::nothrow) mlz_dev_reader;
    if (!rd) return -MLZ_ERR_HIP;
    int64_t parsed = 0;
    const int e = stream_walk_device(c, static_cast<hipStream_t>(stream), d_src, n, &rd->chunks, &parsed, &rd->n_ident, &rd->ident_byte);
    if (e || parsed < 0) { delete rd; return e ? e : parsed; }   // a framing error: no handle
    rd->ctx = c; rd->d_src = d_src; rd->n = n; rd->size = parsed;
    rd->bases = {0, uint64_t(parsed)};
    rd->dchunks.reserve(rd->chunks.size());
    for (const StreamChunk& ck : rd->chunks) rd->dchunks.push_back(mlz::RdevChunk{uint64_t(ck.out_off), uint64_t(ck.body_off), uint32_t(ck.n), ck.type});
    *out = rd;
    return parsed;
}

int64_t mlz_dev_reader_size(const mlz_dev_reader* rd) { return rd ? rd->size : -MLZ_ERR_ARG; }

int64_t mlz_dev_reader_read(mlz_dev_reader* rd, void* stream, uint32_t flags, const mlz_range* ranges, size_t n_ranges, uint8_t* d_dst, size_t dst_cap) {
    if (!rd || (!ranges && n_ranges) || (!d_dst && dst_cap)) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    mlz::RangePlan plan;
    const int pr = mlz::plan_ranges(rd->dchunks.data(), rd->dchunks.size(), uint64_t(rd->size), reinterpret_cast<const mlz::ByteRange*>(ranges), n_ranges, uint64_t(dst_cap), &plan);
    if (pr < 0) return pr;
    if (plan.total && !on_device(c, d_dst)) return -MLZ_ERR_ARG;   // the destination: on the handle's device
    begin_decode_call(c);
    c->range_chunks = plan.touched.size();
    c->range_scratch = plan.scratch_total;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const int64_t r = settled(sm, dev_reader_read_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, plan, d_dst));
    return r < 0 ? r : int64_t(plan.total);
}

void mlz_dev_reader_close(mlz_dev_reader* rd) {
    if (rd && (rd->d_chunks || rd->search[0].d_tabs || rd->search[1].d_tabs || rd->side.d_tabs || rd->d_index || rd->d_bases || rd->tabled.d_chunks)) {
        std::lock_guard<std::mutex> lk(rd->ctx->mu);
        if (hipSetDevice(rd->ctx->device) == hipSuccess)
            for (void* p : {rd->d_chunks, rd->search[0].d_tabs, rd->search[1].d_tabs, rd->side.d_tabs, rd->search[0].d_arena, rd->search[1].d_arena, rd->side.d_arena, rd->d_index, rd->d_bases,
                            rd->tabled.d_chunks, rd->tabled.d_cross[0], rd->tabled.d_cross[1]})
                if (p) (void)hipFree(p);
    }
    delete rd;
}

}  // extern "C"
