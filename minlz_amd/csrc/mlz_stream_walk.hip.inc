// mlz_stream_walk.hip.inc — the device-resident Reader: the chunk walk of a .mz stream that lies in HBM, and its decode in place
// (included at the end of mlz_hip.hip, behind mlz_stream.hip.inc whose chunk types, chunk list (StreamChunk, ChunkJob, chunk_group_descs)
// and decode helpers it uses; the framing rules themselves are mlz_stream_walk.h's, the same code the host Reader runs).
//
// A stream carries no table of its chunks, but every chunk type advances the Reader by 4 + clen (walk_headers: every step does), so
// next(p) = p + 4 + clen(p) is defined for EVERY byte offset p and the chunk starts are the orbit of offset 0 under next.  A parse that
// starts at a wrong offset never falls in step with the real one (unlike a token stream: mlz_decode.hip.inc D2 guesses, this cannot), so the
// exits are kept for every offset and the orbit is followed top-down through two sizes of region:
//
//   W1 exits   walk_exit_kernel    a workgroup per 4 KiB region (kWalkR0), bytes staged in LDS with 16-byte loads; next(i) for each of its
//                                  offsets, finished to the region's EXIT (the first orbit point behind the region) by pointer jumping in LDS:
//                                  one round for the usual region (garbage lengths average 8 MiB), ten for a region of empty chunks.
//                                  x0[p] = exit - region base, a u32 per stream byte.
//   W2 lift    walk_lift_kernel    a lane per four offsets: x1[p] = exit of p's 256 KiB region (kWalkR1), by following x0 while it stays inside
//                                  (about one offset in 60 has to take a second hop).
//   W3 top     walk_top_kernel     ONE lane follows x1 from offset 0 and notes the entry of every 256 KiB region the orbit visits: a chain of
//                                  min(chunks, n / 256 KiB) dependent loads — bounded by the stream's size, not by its chunk count.
//   W4 mid     walk_mid_kernel     a lane per entered 256 KiB region follows x0 from its entry (at most 64 hops) and notes the entry of every
//                                  4 KiB region on the way.
//   W5 count / scan / emit         a lane per entered 4 KiB region steps through the chunk headers inside it (walk_headers; usually one), counts
//                                  those that enter the table, and after an exclusive scan of the counts writes their records (walk_classify,
//                                  mlz_stream_walk.h) in stream order.  Skippable chunks that lie inside the stream never enter the table —
//                                  but for the walk of a sidecar, which keeps the chunks of types 0x44, 0x45 and 0x47.
//
// The table (32 bytes per chunk) is read back and the Reader's running state (block size, header / EOF bookkeeping, output offsets, the
// first error: WalkReader) is applied to it on the host by walk_parse_table — the state the host Reader and the host check run (a serial
// pass over 32-byte records; streams of very many DATA chunks would want it as scans on the device).  Decode and CRC then run on the stream where it lies: descriptors point into
// d_src (token-only mode, nothing is patched) and d_dst, stored chunks are copied by one kernel over a descriptor list.
// Every device-resident call stages its chunk list for stream_run_chunk_jobs in one of two ways, written here once: in place (stream_decode_jobs_in_place:
// this call and the batch decode) or through the scratch (ScratchDecode: the searches, the grep, the record index and the sidecar build).
// Workspace: 8 bytes per stream byte (x0, x1) + 12 bytes per 4 KiB + 32 bytes per table entry.

namespace mlz {

constexpr int kWalkR0Log = 12, kWalkR1Log = 18;
constexpr uint32_t kWalkR0 = 1u << kWalkR0Log, kWalkR1 = 1u << kWalkR1Log;
constexpr uint32_t kWalkStop = 0xffffffffu;     // no header can be read at this offset (fewer than 4 bytes left): the orbit ends here
constexpr uint32_t kWalkNoEntry = 0xffffffffu;
constexpr uint64_t kWalkNoEntry64 = ~uint64_t(0);
constexpr uint32_t kWalkThreads = 256, kWalkPer = kWalkR0 / kWalkThreads;

// W1.  LDS: 4 KiB + 3 bytes of the stream (+ up to 15 in front: the loads are 16-byte aligned) and a u32 per offset = 20.1 KiB.
__global__ __launch_bounds__(kWalkThreads) void walk_exit_kernel(const uint8_t* __restrict__ src, uint64_t n, uint32_t* __restrict__ x0) {
    __shared__ uint4 bufv[(kWalkR0 + 3 + 15 + 15) / 16 + 1];
    __shared__ uint32_t t[kWalkR0];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = uint64_t(blockIdx.x) << kWalkR0Log;
    const uint32_t rem = uint32_t(n - base < kWalkR0 + 3 ? n - base : kWalkR0 + 3);   // bytes of the stream from base on that matter here
    const uint8_t* g = src + base;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(g) & 15);
    // aligned 16-byte loads: the first holds g[0] and the last g[rem - 1], so every one of them touches a byte of the stream's own pages
    const uint4* ga = reinterpret_cast<const uint4*>(g - mis);
    const uint32_t nvec = (mis + rem + 15) >> 4;
    for (uint32_t k = tid; k < nvec; k += kWalkThreads) bufv[k] = ga[k];
    __syncthreads();
    const uint8_t* buf = reinterpret_cast<const uint8_t*>(bufv) + mis;
    uint32_t v[kWalkPer];
#pragma unroll
    for (uint32_t k = 0; k < kWalkPer; k++) {
        const uint32_t i = k * kWalkThreads + tid;
        uint32_t h = 0;
        const bool ok = i + 4 <= rem;
        if (ok) __builtin_memcpy(&h, buf + i, 4);
        v[k] = ok ? i + 4 + (h >> 8) : kWalkStop;
        t[i] = v[k];
    }
    // pointer jumping in place: t[i] is always a point of i's orbit and only moves forward, so a value read while its owner replaces it
    // is as good as the old one
    for (;;) {
        __syncthreads();
        bool more = false;
#pragma unroll
        for (uint32_t k = 0; k < kWalkPer; k++) {
            if (v[k] < kWalkR0) {
                v[k] = t[v[k]];
                t[k * kWalkThreads + tid] = v[k];
                more = more || v[k] < kWalkR0;
            }
        }
        if (!__syncthreads_or(more)) break;
    }
    const uint32_t own = uint32_t(n - base < kWalkR0 ? n - base : kWalkR0);
#pragma unroll
    for (uint32_t k = 0; k < kWalkPer; k++) {
        const uint32_t i = k * kWalkThreads + tid;
        if (i < own) x0[base + i] = v[k];
    }
}

// W2.  x0 and x1 are 16-byte aligned and padded to a multiple of four entries.
__global__ __launch_bounds__(256) void walk_lift_kernel(uint64_t n, const uint32_t* __restrict__ x0, uint32_t* __restrict__ x1) {
    const uint64_t p0 = (uint64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    const uint4 in = *reinterpret_cast<const uint4*>(x0 + p0);
    uint32_t v[4] = {in.x, in.y, in.z, in.w};
    const uint64_t base1 = p0 & ~uint64_t(kWalkR1 - 1), end1 = base1 + kWalkR1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (p0 + j >= n) { v[j] = kWalkStop; continue; }
        uint64_t base0 = p0 & ~uint64_t(kWalkR0 - 1);
        uint32_t x = v[j];
        for (;;) {
            if (x == kWalkStop) break;
            const uint64_t e = base0 + x;     // (strictly behind the offset it was read at: the loop ends)
            if (e >= end1 || e >= n) { x = uint32_t(e - base1); break; }
            base0 = e & ~uint64_t(kWalkR0 - 1);
            x = x0[e];
        }
        v[j] = x;
    }
    *reinterpret_cast<uint4*>(x1 + p0) = make_uint4(v[0], v[1], v[2], v[3]);
}

// W3.
__global__ __launch_bounds__(64) void walk_top_kernel(uint64_t n, const uint32_t* __restrict__ x1, uint64_t* __restrict__ entry1) {
    if (threadIdx.x != 0) return;
    uint64_t e = 0;
    while (e < n) {
        const uint64_t r1 = e >> kWalkR1Log;
        entry1[r1] = e;
        const uint32_t x = x1[e];
        if (x == kWalkStop) break;
        e = (r1 << kWalkR1Log) + x;
    }
}

// W4.
__global__ __launch_bounds__(64) void walk_mid_kernel(uint64_t n, uint32_t nreg1, const uint32_t* __restrict__ x0, const uint64_t* __restrict__ entry1,
                                                      uint32_t* __restrict__ entry0) {
    const uint32_t r1 = blockIdx.x * 64 + threadIdx.x;
    if (r1 >= nreg1) return;
    uint64_t e = entry1[r1];
    if (e == kWalkNoEntry64) return;
    const uint64_t end1 = (uint64_t(r1) + 1) << kWalkR1Log;
    while (e < end1 && e < n) {
        const uint64_t r0 = e >> kWalkR0Log;
        entry0[r0] = uint32_t(e & (kWalkR0 - 1));
        const uint32_t x = x0[e];
        if (x == kWalkStop) break;
        e = (r0 << kWalkR0Log) + x;
    }
}

// W5: the chunk headers of one entered 4 KiB region, in order (walk_headers).  EMIT = false counts the table's entries, EMIT = true writes them.
// keep_search: the walk of a sidecar, whose info, table and reference chunks (0x44, 0x45, 0x47) enter the table like the others.
template <bool EMIT>
__global__ __launch_bounds__(64) void walk_list_kernel(const uint8_t* __restrict__ src, uint64_t n, uint32_t nreg0, const uint32_t* __restrict__ entry0,
                                                       uint32_t* __restrict__ counts, const uint32_t* __restrict__ first, WalkChunk* __restrict__ table, bool keep_search) {
    const uint32_t r0 = blockIdx.x * 64 + threadIdx.x;
    if (r0 >= nreg0) return;
    const uint32_t ent = entry0[r0];
    uint32_t cnt = 0;
    if (ent != kWalkNoEntry) {
        const uint64_t base = uint64_t(r0) << kWalkR0Log;
        const uint64_t end = base + kWalkR0 < n ? base + kWalkR0 : n;
        const uint32_t at = EMIT ? first[r0] : 0;
        walk_headers(src, n, base + ent, end, keep_search, kWalkNoCap, [&](uint64_t e) {
            if (EMIT) table[at + cnt] = walk_classify(src, n, e);
            cnt++;
            return true;
        });
    }
    if (!EMIT) counts[r0] = cnt;
}

// Exclusive scan of the per-region counts by one workgroup: a contiguous slab per thread, the slab sums scanned in LDS.  total[0] = the sum.
__global__ __launch_bounds__(1024) void walk_scan_kernel(const uint32_t* __restrict__ counts, uint32_t nreg0, uint32_t* __restrict__ first, uint32_t* __restrict__ total) {
    __shared__ uint32_t sums[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (nreg0 + 1023) / 1024;
    const uint32_t b = tid * per < nreg0 ? tid * per : nreg0, e = b + per < nreg0 ? b + per : nreg0;
    uint32_t s = 0;
    for (uint32_t i = b; i < e; i++) s += counts[i];
    uint32_t sum, run = wg_scan<1024>(s, sums, tid, [](uint32_t x, uint32_t y) { return x + y; }, &sum);
    for (uint32_t i = b; i < e; i++) { first[i] = run; run += counts[i]; }
    if (tid == 1023) total[0] = sum;
}

}  // namespace mlz

namespace {

constexpr uint64_t kWalkMaxStream = uint64_t(1) << 36;   // (the table's entries are counted in 32 bits: one per 4 bytes at the most)

// The per-device context that serves a call on the stream d_src[0, n) (an empty stream: any device), or nullptr: an argument error
mlz_ctx* stream_ctx(mlz_ctx* c, const uint8_t* d_src, size_t n) {
    if (!c || (!d_src && n) || uint64_t(n) > kWalkMaxStream) return nullptr;
    if (n && !(c = owner_of(c, d_src))) return nullptr;
    return c->kids.empty() ? c : c->kids[0];
}

bool on_device(const mlz_ctx* c, const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->device) { (void)hipGetLastError(); return false; }
    return true;
}

// An entry point's first word to the runtime: the calling thread works on the context's device
int enter_device(mlz_ctx* c) { return hipSetDevice(c->device) == hipSuccess ? 0 : ((void)hipGetLastError(), -MLZ_ERR_HIP); }

// `bytes` from device memory to the host, waited for; an error of anything sm was given before shows here too
int fetch(mlz_ctx* c, hipStream_t sm, void* host, const void* dev, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The result of a call's body as the entry point returns it: nothing of a failed call is left in flight
int64_t settled(hipStream_t sm, int64_t r) {
    if (r < 0) (void)hipStreamSynchronize(sm);
    return r;
}

// The chunk walk of d_src[0, n) on c's device: `chunks` = the data chunks in front of the first framing error, *parsed = what stream_parse
// returns for the same bytes.  Returns 0 or -MLZ_ERR_HIP.  Synchronous on st.  Caller holds c->mu.
// n_ident, ident_byte (may be NULL): the stream identifiers the table holds and the first one's block-size byte.  side (may be NULL): the walk of a sidecar — its search chunks (0x44, 0x45,
// 0x47) enter the table, *side receives the whole table (which also stays in c->d_walk_tab for the caller's kernels), and the Reader's
// state is applied to the other records.
int stream_walk_device(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, size_t n, std::vector<StreamChunk>* chunks, int64_t* parsed, uint32_t* n_ident = nullptr,
                       uint8_t* ident_byte = nullptr, std::vector<mlz::WalkChunk>* side = nullptr) {
    chunks->clear();
    *parsed = 0;
    if (n_ident) *n_ident = 0;
    if (side) side->clear();
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t nreg0 = (uint64_t(n) + kWalkR0 - 1) >> kWalkR0Log, nreg1 = (uint64_t(n) + kWalkR1 - 1) >> kWalkR1Log;
    const size_t xlen = (size_t(n) + 3) & ~size_t(3);
    Carve cv;   // x0 | x1 | entry1 | entry0 | counts | first | total; entry1 and entry0 lie side by side: one memset clears both
    const auto r_x0 = cv.take<uint32_t>(xlen), r_x1 = cv.take<uint32_t>(xlen);
    const auto r_e1 = cv.take<uint64_t>(size_t(nreg1));
    const auto r_e0 = cv.take<uint32_t>(size_t(nreg0), 4), r_cnt = cv.take<uint32_t>(size_t(nreg0), 4), r_first = cv.take<uint32_t>(size_t(nreg0), 4), r_total = cv.take<uint32_t>(4);
    HIPCHK(c, c->d_walk.ensure(cv.bytes));
    int r = ensure_stream_objects(c, 0, 64);
    if (r) return r;
    void* ws = c->d_walk.p;
    uint32_t *x0 = r_x0.at(ws), *x1 = r_x1.at(ws), *entry0 = r_e0.at(ws), *counts = r_cnt.at(ws), *first = r_first.at(ws), *total = r_total.at(ws);
    uint64_t* entry1 = r_e1.at(ws);
    uint32_t h_total = 0;
    {
        WorkspaceOrder order(c, st);
        HIPCHK(c, hipMemsetAsync(entry1, 0xff, r_cnt.off - r_e1.off, st));   // entry1 and entry0: no entry
        hipLaunchKernelGGL(mlz::walk_exit_kernel, dim3(uint32_t(nreg0)), dim3(mlz::kWalkThreads), 0, st, d_src, uint64_t(n), x0);
        hipLaunchKernelGGL(mlz::walk_lift_kernel, dim3(uint32_t((xlen / 4 + 255) / 256)), dim3(256), 0, st, uint64_t(n), x0, x1);
        hipLaunchKernelGGL(mlz::walk_top_kernel, dim3(1), dim3(64), 0, st, uint64_t(n), x1, entry1);
        hipLaunchKernelGGL(mlz::walk_mid_kernel, dim3(uint32_t((nreg1 + 63) / 64)), dim3(64), 0, st, uint64_t(n), uint32_t(nreg1), x0, entry1, entry0);
        hipLaunchKernelGGL(mlz::walk_list_kernel<false>, dim3(uint32_t((nreg0 + 63) / 64)), dim3(64), 0, st, d_src, uint64_t(n), uint32_t(nreg0), entry0, counts, first,
                           static_cast<mlz::WalkChunk*>(nullptr), side != nullptr);
        hipLaunchKernelGGL(mlz::walk_scan_kernel, dim3(1), dim3(1024), 0, st, counts, uint32_t(nreg0), first, total);
        if ((r = fetch(c, st, c->pinned2, total, 4))) return r;
        h_total = *static_cast<uint32_t*>(c->pinned2);
        if (h_total) {
            HIPCHK(c, c->d_walk_tab.ensure(size_t(h_total) * sizeof(mlz::WalkChunk)));
            r = ensure_stream_objects(c, 0, size_t(h_total) * sizeof(mlz::WalkChunk));
            if (r) return r;
            mlz::WalkChunk* tab = c->d_walk_tab.as<mlz::WalkChunk>();
            hipLaunchKernelGGL(mlz::walk_list_kernel<true>, dim3(uint32_t((nreg0 + 63) / 64)), dim3(64), 0, st, d_src, uint64_t(n), uint32_t(nreg0), entry0, counts, first, tab,
                               side != nullptr);
            if ((r = fetch(c, st, c->pinned2, tab, size_t(h_total) * sizeof(mlz::WalkChunk)))) return r;
        }
    }
    const mlz::WalkChunk* table = static_cast<const mlz::WalkChunk*>(c->pinned2);
    size_t n_table = h_total;
    std::vector<mlz::WalkChunk> others;
    if (side) {   // the Reader never sees a search chunk that lies inside the stream
        side->assign(table, table + h_total);
        for (const mlz::WalkChunk& w : *side)
            if (!(mlz::walk_search_chunk(uint8_t(w.tl >> 24)) && !(w.flags & (mlz::kWalkTrunc | mlz::kWalkStub)))) others.push_back(w);
        table = others.data(); n_table = others.size();
    }
    if (n_ident)
        for (size_t i = 0; i < n_table; i++)
            if (!(table[i].flags & mlz::kWalkStub) && (table[i].tl >> 24) == 0xff && (*n_ident)++ == 0 && ident_byte) *ident_byte = uint8_t(table[i].val);
    chunks->reserve(n_table);
    *parsed = mlz::walk_parse_table(table, n_table, kMaxBlockSize, stream_chunk_sink(chunks));
    return 0;
}

// What comes back per job, in c->pinned2: the caller takes the regions from its carve of that buffer, in front of its last ensure
struct ChunkJobResults { Region<int64_t> len; Region<uint32_t> crc; };
ChunkJobResults take_chunk_job_results(Carve* pin, size_t nj) { return ChunkJobResults{pin->take<int64_t>(nj), pin->take<uint32_t>(nj, 4)}; }

// The decode / CRC / verdict of a list of chunks of a stream that lies at d_src, shared by the whole-stream call and the range read.  jobs: in
// stream order; gend[g]: one past the last job of group g (range_group_ends: about 64 MiB of chunk output).  Per group one decode launch
// sequence (token-only mode: d_src is not touched) and one CRC launch over all its chunks — 0x01 / 0x02 over the bytes at `at`, 0x03 over the
// token bytes in the stream —, each with the lowest target address as its base pointer and the targets' distances from it in the descriptors
// (chunk_group_descs, which the host decode's pipeline fills its launches from as well);
// after_group(g) is then called with sm still running (the range read enqueues the group's copy there).  One synchronise at the end; per chunk
// 8 + 4 bytes of results come back, to `res`.  The caller has begun the decode call, sized c->pinned2 for its carve (res is part of it)
// and holds c->mu.  Returns 0 or the error of the first failing chunk of the list.  per_job (the batch calls, whose list holds many streams):
// receives every job's own verdict (mlz::chunk_job_verdict), and the chunks' errors are then not the call's: it returns 0.
template <class AfterGroup>
int64_t stream_run_chunk_jobs(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const std::vector<StreamChunk>& chunks,
                              const std::vector<ChunkJob>& jobs, const std::vector<size_t>& gend, const ChunkJobResults& res, AfterGroup after_group,
                              std::vector<int64_t>* per_job = nullptr) {
    const size_t nj = jobs.size();
    if (per_job) per_job->assign(nj, 0);
    if (nj == 0) return 0;
    HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * nj));
    HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * nj + 64));
    if (c->pinned2_cap < res.crc.off + sizeof(uint32_t) * nj) { c->err = "stream_run_chunk_jobs: the result buffer was not sized"; return -MLZ_ERR_HIP; }
    int64_t* h_len = res.len.at(c->pinned2);
    uint32_t* h_crc = res.crc.at(c->pinned2);
    ChunkGroupDescs gd;
    std::vector<size_t> res_idx(nj, 0);
    size_t n_dec = 0;
    int r = 0;
    for (size_t g = 0, j0 = 0; g < gend.size(); j0 = gend[g++]) {
        const size_t j1 = gend[g];
        chunk_group_descs(d_src, 0, chunks, jobs.data(), j0, j1, n_dec, res_idx.data(), &gd);
        if (!gd.dec.empty()) {
            r = decode_device_locked(c, sm, d_src, reinterpret_cast<uint8_t*>(gd.dbase), gd.dec.data(), int(gd.dec.size()), c->d_len.as<int64_t>() + n_dec, true, nullptr, false);
            if (r) return r;
        }
        if (!ignore_crc) {
            r = crc_device_locked(c, sm, reinterpret_cast<const uint8_t*>(gd.cbase), gd.crc.data(), int(j1 - j0), c->d_crc.as<uint32_t>() + j0);
            if (r) return r;
        }
        n_dec += gd.dec.size();
        r = after_group(g);
        if (r) return r;
    }
    if (n_dec) HIPCHK(c, hipMemcpyAsync(h_len, c->d_len.p, sizeof(int64_t) * n_dec, hipMemcpyDeviceToHost, sm));
    if (!ignore_crc) HIPCHK(c, hipMemcpyAsync(h_crc, c->d_crc.p, sizeof(uint32_t) * nj, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    for (size_t j = 0; j < nj; j++) {
        const StreamChunk& ck = chunks[jobs[j].ck];
        const bool compressed = ck.type != kChunkUncompressed;
        const int64_t v = mlz::chunk_job_verdict(compressed, compressed ? h_len[res_idx[j]] : 0, ck.n, !ignore_crc, ignore_crc ? 0 : h_crc[j], ck.crc);
        if (per_job) (*per_job)[j] = v;
        else if (v) return v;
    }
    return 0;
}

// The scratch decode: a list of a handle's chunks decoded group by group into the context's scratch (c->d_range), which every group reuses,
// for the calls that read decoded bytes without keeping them (the searches, the grep, the record index, the sidecar build).  The caller
// fills jobs (ck; in stream order), gend and at (every job's offset in the scratch; scratch_decode_whole: for all chunks); the rest is the rule of mlz_stream_scratch.h.
struct ScratchDecode {
    std::vector<ChunkJob> jobs;
    std::vector<size_t> gend;
    std::vector<uint64_t> at;
    mlz::ScratchPlaces sp;
    ChunkJobResults res;
    Region<PlaceDesc> hplaces;

    // Its regions of the caller's carve of the pinned buffer, in front of the caller's ensure_stream_objects; the scratch, the copies' descriptors
    int take(mlz_ctx* c, const std::vector<StreamChunk>& chunks, Carve* pin) {
        sp = mlz::scratch_places(jobs.size(), gend, [&](size_t i) -> const StreamChunk& { return chunks[jobs[i].ck]; }, at);
        res = take_chunk_job_results(pin, jobs.size());
        hplaces = pin->take<PlaceDesc>(sp.places.size(), 8);
        HIPCHK(c, c->d_range.ensure(size_t(sp.scratch_max) + 64));
        if (!sp.places.empty()) HIPCHK(c, c->d_place.ensure(sp.places.size() * sizeof(PlaceDesc)));
        return 0;
    }
    // Decodes the list; per group the stored chunks' copies are enqueued and after_group(g) is called with the group's bytes in place (sm still running).
    // per_job: stream_run_chunk_jobs' (a list that holds many streams' chunks: every job's own verdict)
    template <class AfterGroup>
    int64_t run(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const std::vector<StreamChunk>& chunks, AfterGroup after_group,
                std::vector<int64_t>* per_job = nullptr) {
        uint8_t* scratch = c->d_range.as<uint8_t>();
        const size_t np = sp.places.size();
        for (size_t i = 0; i < jobs.size(); i++) {
            const StreamChunk& ck = chunks[jobs[i].ck];
            jobs[i].at = ck.type == kChunkUncompressed ? d_src + ck.body_off : scratch + at[i];   // (a stored chunk's CRC: over the stream's own bytes)
        }
        if (np) {
            std::memcpy(hplaces.at(c->pinned2), sp.places.data(), np * sizeof(PlaceDesc));
            HIPCHK(c, hipMemcpyAsync(c->d_place.p, hplaces.at(c->pinned2), np * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
        }
        return stream_run_chunk_jobs(c, sm, ignore_crc, d_src, chunks, jobs, gend, res, [&](size_t g) -> int {
            const size_t q0 = g ? sp.place_end[g - 1] : 0, q1 = sp.place_end[g];
            if (q1 > q0) hipLaunchKernelGGL(stream_place_kernel, dim3(uint32_t(q1 - q0)), dim3(256), 0, sm, d_src, d_src, nullptr, scratch, c->d_place.as<PlaceDesc>() + q0);
            return after_group(g);
        }, per_job);
    }
};

// The whole-stream decode of a handle's chunk table (mlz::whole_stream_list): jobs, gend and at of *dec; *w keeps every group's first decoded
// position and bytes.  size: the stream's decoded bytes; `call` names the entry point in an error's text.  An empty stream (size 0, no chunk with bytes) passes with no job and no group: a caller that launches per group must be ready for none.
int scratch_decode_whole(mlz_ctx* c, const char* call, const std::vector<StreamChunk>& chunks, uint64_t size, ScratchDecode* dec, mlz::WholeStreamList* w) {
    const std::vector<size_t> dc = mlz::chunks_with_bytes(chunks.size(), [&](size_t k) { return chunks[k].n; });
    mlz::range_group_ends(dc.size(), [&](size_t i) { return uint64_t(chunks[dc[i]].n); }, &dec->gend);
    *w = mlz::whole_stream_list(dc, dec->gend, [&](size_t k) { return uint64_t(chunks[k].n); }, [&](size_t k) { return uint64_t(chunks[k].out_off); }, size);
    if (w->status != mlz::kWholeOk) {
        c->err = std::string(call) + (w->status == mlz::kWholeNotContiguous ? ": the chunks' output offsets are not contiguous" : ": the groups do not tile the stream");
        return -MLZ_ERR_HIP;
    }
    for (size_t k : dc) dec->jobs.push_back(ChunkJob{k, nullptr});
    dec->at = w->at;
    return 0;
}

// The in-place decode: a job list whose targets all lie in d_dst, where the chunks finally lie.  Stored chunks by one stream_place_kernel launch over
// their 64 KiB pieces, then decode and CRC group by group (range_group_ends, stream_run_chunk_jobs and its per_job).  The caller has begun the decode call.
int64_t stream_decode_jobs_in_place(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const std::vector<StreamChunk>& chunks, const std::vector<ChunkJob>& jobs,
                                    uint8_t* d_dst, std::vector<int64_t>* per_job = nullptr) {
    std::vector<uint64_t> at(jobs.size());   // the stored chunks' pieces: the rule of the scratch decode for one group that is d_dst
    for (size_t j = 0; j < jobs.size(); j++) at[j] = uint64_t(jobs[j].at - d_dst);
    const std::vector<PlaceDesc> places = mlz::scratch_places(jobs.size(), {jobs.size()}, [&](size_t j) -> const StreamChunk& { return chunks[jobs[j].ck]; }, at).places;
    const size_t np = places.size();
    Carve pin;
    const ChunkJobResults res = take_chunk_job_results(&pin, jobs.size());
    const auto r_place = pin.take<PlaceDesc>(np, 64);
    if (const int r = ensure_stream_objects(c, 0, pin.bytes)) return r;
    { WorkspaceOrder order(c, sm); }
    if (np) {
        HIPCHK(c, c->d_place.ensure(np * sizeof(PlaceDesc)));
        std::memcpy(r_place.at(c->pinned2), places.data(), np * sizeof(PlaceDesc));
        HIPCHK(c, hipMemcpyAsync(c->d_place.p, r_place.at(c->pinned2), np * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(stream_place_kernel, dim3(uint32_t(np)), dim3(256), 0, sm, d_src, d_src, nullptr, d_dst, c->d_place.as<PlaceDesc>());
    }
    std::vector<size_t> gend;
    mlz::range_group_ends(jobs.size(), [&](size_t j) { return uint64_t(chunks[jobs[j].ck].n); }, &gend);
    return stream_run_chunk_jobs(c, sm, ignore_crc, d_src, chunks, jobs, gend, res, [](size_t) { return 0; }, per_job);
}

// All chunks of a walked stream, where they lie in d_dst.  Returns 0 or the first chunk's error in stream order.
int64_t stream_decode_chunks_device(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const std::vector<StreamChunk>& chunks, uint8_t* d_dst) {
    begin_decode_call(c);
    if (chunks.empty()) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<ChunkJob> jobs(chunks.size());
    for (size_t i = 0; i < jobs.size(); i++) jobs[i] = ChunkJob{i, d_dst + chunks[i].out_off};
    return stream_decode_jobs_in_place(c, sm, ignore_crc, d_src, chunks, jobs, d_dst);
}

}  // namespace

extern "C" {

int64_t mlz_stream_decoded_len_device(mlz_ctx* c, void* stream, const uint8_t* d_src, size_t n, uint64_t* prefix_len) {
    if (!(c = stream_ctx(c, d_src, n))) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    std::vector<StreamChunk> chunks;
    int64_t r = 0;
    const int e = stream_walk_device(c, static_cast<hipStream_t>(stream), d_src, n, &chunks, &r);
    if (e) return e;
    if (prefix_len) *prefix_len = r >= 0 ? uint64_t(r) : chunks.empty() ? 0 : uint64_t(chunks.back().out_off + chunks.back().n);
    return r;
}

int64_t mlz_stream_decode_device(mlz_ctx* c, void* stream, uint32_t flags, const uint8_t* d_src, size_t n, uint8_t* d_dst, size_t dst_cap) {
    if ((!d_dst && dst_cap) || !(c = stream_ctx(c, d_src, n))) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0;
    std::vector<StreamChunk> chunks;
    int64_t parsed = 0;
    const int e = stream_walk_device(c, st, d_src, n, &chunks, &parsed);
    if (e) return e;
    // as stream_decode_over: the chunks in front of a framing error are decoded and checked first
    const size_t total = parsed >= 0 ? size_t(parsed) : chunks.empty() ? 0 : chunks.back().out_off + chunks.back().n;
    if (total > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;
    const int64_t r = (parsed >= 0 || total) ? stream_decode_chunks_device(c, st, ignore_crc, d_src, chunks, d_dst) : 0;
    return r < 0 ? r : parsed;
}

}  // extern "C"
