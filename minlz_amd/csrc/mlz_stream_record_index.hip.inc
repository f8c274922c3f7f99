// mlz_stream_record_index.hip.inc — the record index of a .mz stream in HBM: the positions of all delimiters of the decoded stream, built by
// one decode, and the calls that read records by number and number positions by record (included at the end of mlz_hip.hip, behind the
// records search, whose slab and the range read in device memory it uses).  The rules are those of mlz_stream_record_index.h, which the
// host check runs as plain loops.
//
// Build (mlz_dev_reader_index_records): the handle's data chunks with bytes are decoded group by group (about 64 MiB, range_group_ends) into
// the ReadSeeker's scratch, side by side from scratch[0] on (scratch_decode_whole, ScratchDecode, mlz_stream_walk.hip.inc; stored chunks are copied there).  Per group:
//   count   rindex_count_kernel: a workgroup per 64 KiB tile, a 16-byte load per lane and step, the popcounts reduced to one word per tile;
//   scan    rindex_scan_kernel (one workgroup): the tiles' exclusive bases and the group's total, which comes home (8 bytes); the host adds
//           it to the running base and grows the table to fit (exactly with one group, else geometrically with a device-to-device copy);
//   emit    rindex_emit_kernel: same tiling; the lane's 16 masks stay in registers, a wavefront scan per step gives the lower lanes' hits,
//           the 64 (step, wavefront) totals are scanned in LDS by one wavefront, and each delimiter's position goes to table[base + rank].
// The table is built beside the handle's old one and replaces it only when every chunk has passed its decode and CRC verdicts.
// Read: rindex_spans_kernel and rindex_numbers_kernel, a lane per item; 16 bytes come home from either.  mlz_dev_reader_read_records puts
// the spans into context workspace and hands them to dev_reader_read_device_locked.  No kernel waits for another workgroup.

#include "mlz_stream_record_index.h"

namespace mlz {

// The mask of the block at bs.  whole: the tile lies inside the region (uniform over the workgroup), every block is one load.
__device__ __forceinline__ uint32_t rindex_mask_at(const uint8_t* __restrict__ al, int64_t bs, int64_t ylo, int64_t yhi, uint8_t delim, bool whole) {
    if (whole) {
        const uint4 x = *reinterpret_cast<const uint4*>(al + bs);
        const uint32_t v[4] = {x.x, x.y, x.z, x.w};
        return rindex_vec_mask(v, rindex_splat(delim));
    }
    return rindex_block_mask(bs, ylo, yhi, delim,
                             [&](int64_t y, uint32_t* v) { const uint4 x = *reinterpret_cast<const uint4*>(al + y); v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; },
                             [&](int64_t y) { return al[y]; });
}

struct RindexRegion { const uint8_t* al; int64_t ylo, yhi; bool whole; };
__device__ __forceinline__ RindexRegion rindex_region(const uint8_t* base, uint64_t n, uint64_t tile) {
    const int64_t mis = int64_t(reinterpret_cast<uintptr_t>(base) & 15), t0 = int64_t(tile) * kRindexTile;
    return RindexRegion{base - mis, mis, mis + int64_t(n), t0 >= mis && t0 + int64_t(kRindexTile) <= mis + int64_t(n)};
}

// tile_count[t] = the delimiters among the bytes of base[0, n) that tile t covers
__global__ __launch_bounds__(kRindexThreads) void rindex_count_kernel(const uint8_t* __restrict__ base, uint64_t n, uint8_t delim, uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t wsum[kRindexWaves];
    const uint32_t tid = threadIdx.x;
    const RindexRegion rg = rindex_region(base, n, blockIdx.x);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t s = 0; s < kRindexSteps; s++) cnt += rindex_popcount(rindex_mask_at(rg.al, rindex_block_at(blockIdx.x, s, tid), rg.ylo, rg.yhi, delim, rg.whole));
    for (int d = 32; d; d >>= 1) cnt += uint32_t(__shfl_xor(int(cnt), d));
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) tile_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup.  tile_base[t] = the hits of the tiles in front of t; *total = the group's hits.
__global__ __launch_bounds__(kRecordsScanThreads) void rindex_scan_kernel(const uint32_t* __restrict__ tile_count, uint64_t ntiles, uint32_t* __restrict__ tile_base, uint64_t* __restrict__ total) {
    __shared__ uint64_t lds[kRecordsScanThreads];
    const uint32_t tid = threadIdx.x;
    const RecordsSlab sl = records_slab(ntiles, tid);
    uint64_t sum = 0, tot = 0;
    for (uint64_t t = sl.b; t < sl.e; t++) sum += tile_count[t];
    uint64_t run = wg_scan<kRecordsScanThreads>(sum, lds, tid, [](uint64_t x, uint64_t y) { return x + y; }, &tot);
    for (uint64_t t = sl.b; t < sl.e; t++) { tile_base[t] = uint32_t(run); run += tile_count[t]; }
    if (tid == 0) *total = tot;
}

// table[rank] = first + the offset in base[0, n) of the group's rank-th delimiter, for every rank < limit (the group's total)
__global__ __launch_bounds__(kRindexThreads) void rindex_emit_kernel(const uint8_t* __restrict__ base, uint64_t n, uint8_t delim, const uint32_t* __restrict__ tile_base, uint64_t first,
                                                                     uint64_t limit, uint64_t* __restrict__ table) {
    __shared__ uint32_t slot_base[kRindexSlots];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RindexRegion rg = rindex_region(base, n, blockIdx.x);
    uint32_t m[kRindexSteps], below[kRindexSteps];   // the lane's masks (16 bits each) and the hits of its wavefront's lower lanes, per step
#pragma unroll
    for (uint32_t s = 0; s < kRindexSteps; s++) {
        m[s] = rindex_mask_at(rg.al, rindex_block_at(blockIdx.x, s, tid), rg.ylo, rg.yhi, delim, rg.whole);
        const uint32_t c = rindex_popcount(m[s]), incl = wave_incl_scan(c);   // (at most 16 * 64 per wavefront and step, 65 536 per tile)
        below[s] = incl - c;
        if (lane == 63) slot_base[rindex_slot(s, wave)] = incl;
    }
    __syncthreads();
    if (wave == 0) {   // the 64 slot totals -> their exclusive prefix
        const uint32_t v = slot_base[lane], incl = wave_incl_scan(v);
        slot_base[lane] = incl - v;
    }
    __syncthreads();
    const uint64_t t0 = tile_base[blockIdx.x];
#pragma unroll
    for (uint32_t s = 0; s < kRindexSteps; s++) {
        if (!m[s]) continue;
        rindex_emit(m[s], t0 + slot_base[rindex_slot(s, wave)] + below[s], limit, rindex_block_at(blockIdx.x, s, tid),
                    [&](uint64_t rank, int64_t y) { table[rank] = first + uint64_t(y - rg.ylo); });
    }
}

// off[i], len[i] = the span of record idx[i]; hdr->total += the lengths, hdr->bad = 1 for an index >= N (hdr: zeroed by the caller)
__global__ __launch_bounds__(256) void rindex_spans_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t N, uint64_t size, const uint64_t* __restrict__ idx, uint64_t n,
                                                           uint64_t* __restrict__ off, uint64_t* __restrict__ len, RindexSums* __restrict__ hdr) {
    __shared__ uint64_t lds[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = uint64_t(blockIdx.x) * 256 + tid;
    uint64_t l = 0, tot = 0;
    if (i < n) {
        const uint64_t r = idx[i];
        RindexSpan sp{0, 0};
        if (r >= N) hdr->bad = 1;
        else sp = rindex_span([&](uint64_t j) { return D[j]; }, k, size, r);
        off[i] = sp.off; len[i] = sp.len;
        l = sp.len;
    }
    wg_scan<256>(l, lds, tid, [](uint64_t x, uint64_t y) { return x + y; }, &tot);
    if (tid == 0 && tot) atomicAdd(reinterpret_cast<unsigned long long*>(&hdr->total), static_cast<unsigned long long>(tot));
}

// no[i] = the record number of position pos[i], or kRindexNoRecord for a position >= size; hdr->total += the positions < size
__global__ __launch_bounds__(256) void rindex_numbers_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t size, const uint64_t* __restrict__ pos, uint64_t n,
                                                             uint64_t* __restrict__ no, RindexSums* __restrict__ hdr) {
    __shared__ uint64_t lds[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = uint64_t(blockIdx.x) * 256 + tid;
    uint64_t in = 0, tot = 0;
    if (i < n) {
        const uint64_t p = pos[i];
        in = p < size ? 1 : 0;
        no[i] = in ? rindex_number([&](uint64_t j) { return D[j]; }, k, p) : kRindexNoRecord;
    }
    wg_scan<256>(in, lds, tid, [](uint64_t x, uint64_t y) { return x + y; }, &tot);
    if (tid == 0 && tot) atomicAdd(reinterpret_cast<unsigned long long*>(&hdr->total), static_cast<unsigned long long>(tot));
}

}  // namespace mlz

namespace {

// The table under construction: device memory that becomes the handle's when the build has passed
struct RindexTable {
    uint64_t* p = nullptr;
    uint64_t cap = 0;   // entries
    ~RindexTable() { if (p) (void)hipFree(p); }
};

int64_t dev_reader_index_records_locked(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, uint8_t delim, uint64_t* decoded) {
    mlz_ctx* c = rd->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t size = uint64_t(rd->size);
    ScratchDecode dec;
    mlz::WholeStreamList groups;
    int e = scratch_decode_whole(c, "mlz_dev_reader_index_records", rd->chunks, size, &dec, &groups);
    if (e) return e;
    const size_t nd = dec.jobs.size(), ng = dec.gend.size();
    Carve cv, pin;   // workspace: the group's total | tile counts | tile bases; pinned: the decode's | the total
    if ((e = dec.take(c, rd->chunks, &pin))) return e;
    const uint64_t tiles_max = mlz::rindex_tiles(15, dec.sp.scratch_max);
    const auto r_total = cv.take<uint64_t>(2);
    const auto r_count = cv.take<uint32_t>(size_t(tiles_max)), r_base = cv.take<uint32_t>(size_t(tiles_max));
    const auto h_total_r = pin.take<uint64_t>(2);
    HIPCHK(c, c->d_records.ensure(cv.bytes));
    if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
    void* ws = c->d_records.p;
    uint8_t* scratch = c->d_range.as<uint8_t>();
    uint64_t *d_total = r_total.at(ws), *h_total = h_total_r.at(c->pinned2);
    uint32_t *d_count = r_count.at(ws), *d_base = r_base.at(ws);
    { WorkspaceOrder order(c, sm); }
    RindexTable tab;
    uint64_t k = 0;
    // a group's bytes are in the scratch: count, scan, the total home, room in the table, emit
    auto index_group = [&](size_t g) -> int {
        const uint64_t n = groups.bytes[g], ntiles = mlz::rindex_tiles(reinterpret_cast<uintptr_t>(scratch) & 15, n);
        if (ntiles == 0 || ntiles > tiles_max) { c->err = "mlz_dev_reader_index_records: a group's tiles do not fit the workspace"; return -MLZ_ERR_HIP; }
        hipLaunchKernelGGL(mlz::rindex_count_kernel, dim3(uint32_t(ntiles)), dim3(mlz::kRindexThreads), 0, sm, scratch, n, delim, d_count);
        hipLaunchKernelGGL(mlz::rindex_scan_kernel, dim3(1), dim3(mlz::kRecordsScanThreads), 0, sm, d_count, ntiles, d_base, d_total);
        int r = fetch(c, sm, h_total, d_total, sizeof(uint64_t));
        if (r) return r;
        const uint64_t total = h_total[0];
        if (total > n) { c->err = "mlz_dev_reader_index_records: more delimiters than bytes"; return -MLZ_ERR_HIP; }
        if (total == 0) return 0;
        if (k + total > tab.cap) {   // exactly for a stream of one group, else geometric
            const uint64_t want = ng == 1 ? total : std::max(k + total, 2 * tab.cap);
            uint64_t* fresh = nullptr;
            HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&fresh), size_t(want) * sizeof(uint64_t)));
            if (k) {
                const hipError_t ce = hipMemcpyAsync(fresh, tab.p, size_t(k) * sizeof(uint64_t), hipMemcpyDeviceToDevice, sm);
                if (ce != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) { (void)hipFree(fresh); c->err = "mlz_dev_reader_index_records: the table's copy failed"; return -MLZ_ERR_HIP; }
            }
            if (tab.p) (void)hipFree(tab.p);
            tab.p = fresh; tab.cap = want;
        }
        hipLaunchKernelGGL(mlz::rindex_emit_kernel, dim3(uint32_t(ntiles)), dim3(mlz::kRindexThreads), 0, sm, scratch, n, delim, d_base, groups.first[g], total, tab.p + k);
        k += total;
        return 0;
    };
    const int64_t r = dec.run(c, sm, ignore_crc, rd->d_src, rd->chunks, index_group);
    if (r < 0) return r;
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    bool last_is_delim = false;
    if (k) {
        if ((e = fetch(c, sm, h_total, tab.p + (k - 1), sizeof(uint64_t)))) return e;
        if (h_total[0] >= size) { c->err = "mlz_dev_reader_index_records: a delimiter beyond the stream"; return -MLZ_ERR_HIP; }
        last_is_delim = h_total[0] == size - 1;
    }
    // the build has passed: the table is the handle's
    if (rd->d_index) (void)hipFree(rd->d_index);
    rd->d_index = tab.p; rd->index_cap = tab.cap;
    tab.p = nullptr;
    rd->index_ready = true; rd->index_delim = delim; rd->index_k = k;
    rd->index_longest_ready = false;
    rd->tabled.cross_ready[1] = false;   // (the joined flags of a set that keeps its tables belong to the index)
    rd->index_n = mlz::rindex_records(k, size, last_is_delim);
    *decoded = nd;
    return int64_t(rd->index_n);
}

// The header of a spans or numbers launch, zeroed; d_records holds at least `bytes`
int rindex_header(mlz_ctx* c, hipStream_t sm, size_t bytes) {
    HIPCHK(c, c->d_records.ensure(bytes));
    int e = ensure_stream_objects(c, 0, 64);
    if (e) return e;
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemsetAsync(c->d_records.p, 0, sizeof(mlz::RindexSums), sm));
    return 0;
}

// The spans of n record numbers into off / len (device memory); *sums = what came home
int64_t dev_reader_record_spans_locked(mlz_dev_reader* rd, hipStream_t sm, const uint64_t* d_idx, uint64_t n, uint64_t* d_off, uint64_t* d_len, mlz::RindexSums* sums) {
    mlz_ctx* c = rd->ctx;
    mlz::RindexSums* hdr = static_cast<mlz::RindexSums*>(c->d_records.p);
    hipLaunchKernelGGL(mlz::rindex_spans_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, rd->index_n,
                       uint64_t(rd->size), d_idx, n, d_off, d_len, hdr);
    const int e = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::RindexSums));
    if (e) return e;
    *sums = *static_cast<const mlz::RindexSums*>(c->pinned2);
    return 0;
}

// The entry checks the calls on an index share: the handle, its index, the count, the device
int rindex_enter(mlz_dev_reader* rd, size_t n) {
    if (!rd || !rd->index_ready || uint64_t(n) > mlz::kRindexMaxItems) return -MLZ_ERR_ARG;
    return 0;
}

}  // namespace

extern "C" {

int64_t mlz_dev_reader_index_records(mlz_dev_reader* rd, void* stream, uint32_t flags, uint8_t delimiter, uint64_t* info) {
    if (!rd) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t decoded = 0;
    if (!(rd->index_ready && rd->index_delim == delimiter)) {
        if (enter_device(c)) return -MLZ_ERR_HIP;
        begin_decode_call(c);
        hipStream_t sm = static_cast<hipStream_t>(stream);
        const int64_t r = settled(sm, dev_reader_index_records_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, delimiter, &decoded));
        if (r < 0) return r;   // (the handle keeps what it had)
    }
    if (info) { info[0] = rd->index_n; info[1] = rd->index_k; info[2] = rd->index_cap * sizeof(uint64_t); info[3] = decoded; }
    return int64_t(rd->index_n);
}

int64_t mlz_dev_reader_record_count(const mlz_dev_reader* rd) {
    if (!rd) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    return rd->index_ready ? int64_t(rd->index_n) : -MLZ_ERR_ARG;
}

int64_t mlz_dev_reader_record_spans(mlz_dev_reader* rd, void* stream, const uint64_t* d_idx, size_t n, uint64_t* d_off, uint64_t* d_len) {
    if (!rd || (n && (!d_idx || !d_off || !d_len))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (rindex_enter(rd, n)) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_idx) || !on_device(c, d_off) || !on_device(c, d_len)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    mlz::RindexSums sums{};
    int64_t r = rindex_header(c, sm, sizeof(mlz::RindexSums));
    if (r == 0) r = dev_reader_record_spans_locked(rd, sm, d_idx, uint64_t(n), d_off, d_len, &sums);
    if (r < 0) return settled(sm, r);
    return sums.bad ? -MLZ_ERR_ARG : int64_t(sums.total);
}

int64_t mlz_dev_reader_read_records(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint64_t* d_idx, size_t n, uint8_t* d_dst, size_t dst_cap, uint64_t* d_starts) {
    if (!rd || (n && !d_idx) || (!d_dst && dst_cap)) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (rindex_enter(rd, n)) return -MLZ_ERR_ARG;
    c->range_plan_host = 0;
    if (n == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_idx) || (d_dst && !on_device(c, d_dst)) || (d_starts && !on_device(c, d_starts))) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    c->range_chunks = c->range_scratch = 0;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    Carve cv;   // what lives across the read: the header | the offsets | the lengths
    const auto r_hdr = cv.take<mlz::RindexSums>(1);
    const auto r_off = cv.take<uint64_t>(n), r_len = cv.take<uint64_t>(n);
    int64_t r = rindex_header(c, sm, cv.bytes);
    if (r < 0) return r;
    void* ws = c->d_records.p;
    (void)r_hdr;
    mlz::RindexSums sums{};
    if ((r = dev_reader_record_spans_locked(rd, sm, d_idx, uint64_t(n), r_off.at(ws), r_len.at(ws), &sums)) < 0) return settled(sm, r);
    // both refusals are decided here: nothing has been written to d_dst or d_starts
    if (sums.bad) return -MLZ_ERR_ARG;
    if (sums.total > uint64_t(dst_cap)) return -MLZ_ERR_DST_TOO_SMALL;
    uint64_t total = 0;
    r = settled(sm, dev_reader_read_device_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, r_off.at(ws), r_len.at(ws), uint64_t(n), d_dst, uint64_t(dst_cap), d_starts, &total));
    return r < 0 ? r : int64_t(total);
}

int64_t mlz_dev_reader_record_numbers(mlz_dev_reader* rd, void* stream, const uint64_t* d_pos, size_t n, uint64_t* d_no) {
    if (!rd || (n && (!d_pos || !d_no))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (rindex_enter(rd, n)) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_pos) || !on_device(c, d_no)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    int64_t r = rindex_header(c, sm, sizeof(mlz::RindexSums));
    if (r < 0) return r;
    mlz::RindexSums* hdr = static_cast<mlz::RindexSums*>(c->d_records.p);
    hipLaunchKernelGGL(mlz::rindex_numbers_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, uint64_t(rd->size), d_pos,
                       uint64_t(n), d_no, hdr);
    if ((r = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::RindexSums))) < 0) return settled(sm, r);
    return int64_t(static_cast<const mlz::RindexSums*>(c->pinned2)->total);
}

int64_t mlz_dev_reader_record_range(mlz_dev_reader* rd, uint64_t first, uint64_t count, uint64_t* off, uint64_t* len) {
    if (!rd || !off || !len) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!rd->index_ready || first > rd->index_n || count > rd->index_n - first) return -MLZ_ERR_ARG;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    const uint64_t k = rd->index_k, size = uint64_t(rd->size), last = count ? first + count - 1 : first;
    // the two entries of the table that the range's ends need
    uint64_t before = 0, behind = 0;
    const uint64_t* D = static_cast<const uint64_t*>(rd->d_index);
    if (first > 0 && first <= k) HIPCHK(c, hipMemcpy(&before, D + (first - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (count && last < k) HIPCHK(c, hipMemcpy(&behind, D + last, sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t s = first == 0 ? 0 : first <= k ? before + 1 : size;   // (rindex_span's start and end, an entry each)
    const uint64_t e = count ? (last < k ? behind : size) : s;
    if (e < s || e > size) { c->err = "mlz_dev_reader_record_range: the table's entries do not ascend"; return -MLZ_ERR_HIP; }
    *off = s; *len = e - s;
    return 0;
}

}  // extern "C"
