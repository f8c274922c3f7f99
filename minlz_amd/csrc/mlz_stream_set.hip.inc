// mlz_stream_set.hip.inc — a batch of streams in HBM opened as ONE ReadSeeker handle, and the calls that translate between the handle's
// positions and record numbers and (stream, position or record inside the stream) (included at the end of mlz_hip.hip, behind
// mlz_stream_batch.hip.inc whose walk and argument checks it uses and mlz_stream_record_index.hip.inc whose header and range read it uses).
// The rules are those of mlz_stream_set.h, which the host check runs as plain loops.
//
// Open (mlz_stream_open_batch_device): stream_batch_walk yields every stream's data chunks with body_off counted from d_src, which is all a
// handle is; the healthy streams' chunks are appended in descriptor order with out_off + bases[i].  Every handle call then works on the
// concatenation as it does on one stream: none of them asks that body_off ascends (the decode's descriptors hold distances from the lowest
// address of a group, chunk_group_descs), and the one that walks the stream from d_src[0] on, dev_reader_search_tables, is never run: the
// handle counts as having no usable inline table.
//   locate          set_locate_kernel: a lane per position, a bisection of the bases.
//   read_streams    set_ranges_kernel: a lane per range checks it and writes its place in the handle into context workspace;
//                   dev_reader_read_device_locked does the rest, as for mlz_dev_reader_read_records.
//   stream_records  set_records_kernel: a lane per stream bisects the delimiter table for first[i] and for its last byte.
//   locate_records  set_locate_records_kernel: a lane per record number: one table entry, a bisection of the bases, one of the table.
// No kernel waits for another workgroup; the counts are summed per workgroup and added with one atomicAdd whose result is not used.

#include "mlz_stream_set.h"

namespace mlz {

// hdr->total += the lanes' values: summed over the workgroup (lds: 256 values), one add per workgroup
__device__ __forceinline__ void set_add_total(uint64_t mine, uint64_t* lds, SetSums* __restrict__ hdr) {
    uint64_t tot = 0;
    wg_scan<256>(mine, lds, threadIdx.x, [](uint64_t x, uint64_t y) { return x + y; }, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(reinterpret_cast<unsigned long long*>(&hdr->total), static_cast<unsigned long long>(tot));
}

// which[i], local[i] = the stream of position pos[i] and the position inside it; hdr->total += the positions below the size (hdr: zeroed by the caller)
__global__ __launch_bounds__(256) void set_locate_kernel(const uint64_t* __restrict__ bases, uint32_t ns, const uint64_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ which,
                                                         uint64_t* __restrict__ local, SetSums* __restrict__ hdr) {
    __shared__ uint64_t lds[256];
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    uint64_t in = 0;
    if (i < n) {
        uint32_t w;
        uint64_t l;
        in = set_locate(bases, ns, pos[i], &w, &l) ? 1 : 0;
        which[i] = w; local[i] = l;
    }
    set_add_total(in, lds, hdr);
}

// goff[i] = the place in the handle of range i (which[i], off[i], len[i]); hdr->bad = 1 for a range that fails the check
__global__ __launch_bounds__(256) void set_ranges_kernel(const uint64_t* __restrict__ bases, uint32_t ns, const uint32_t* __restrict__ which, const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ len, uint64_t n, uint64_t* __restrict__ goff, SetSums* __restrict__ hdr) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t g;
    if (!set_range_ok(bases, ns, which[i], off[i], len[i], &g)) hdr->bad = 1;
    goff[i] = g;
}

// out[i] = first[i] for i <= ns; out[ns + 1 + i] = 1 when stream i is joined to the next one, else 0, for i < ns
__global__ __launch_bounds__(256) void set_records_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t N, const uint64_t* __restrict__ bases, uint32_t ns,
                                                          uint64_t* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i > ns) return;
    auto at = [&](uint64_t j) { return D[j]; };
    out[i] = set_first(at, k, N, bases[i]);
    if (i < ns) out[uint64_t(ns) + 1 + i] = set_joined(at, k, bases, ns, uint32_t(i)) ? 1 : 0;
}

// which[i], local_no[i] = the stream in which record no[i] starts and its number inside that stream; hdr->total += the numbers below N
__global__ __launch_bounds__(256) void set_locate_records_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t N, const uint64_t* __restrict__ bases, uint32_t ns,
                                                                 const uint64_t* __restrict__ no, uint64_t n, uint32_t* __restrict__ which, uint64_t* __restrict__ local_no,
                                                                 SetSums* __restrict__ hdr) {
    __shared__ uint64_t lds[256];
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    uint64_t in = 0;
    if (i < n) {
        uint32_t w;
        uint64_t l;
        in = set_locate_record([&](uint64_t j) { return D[j]; }, k, N, bases, ns, no[i], &w, &l) ? 1 : 0;
        which[i] = w; local_no[i] = l;
    }
    set_add_total(in, lds, hdr);
}

}  // namespace mlz

namespace {

// The handle's bases where kernels can read them, uploaded by the first call that needs them (a handle of one stream: {0, size})
int dev_reader_bases(mlz_dev_reader* rd, const uint64_t** d_bases) {
    mlz_ctx* c = rd->ctx;
    if (!rd->d_bases) {
        HIPCHK(c, hipMalloc(&rd->d_bases, rd->bases.size() * sizeof(uint64_t)));
        HIPCHK(c, hipMemcpy(rd->d_bases, rd->bases.data(), rd->bases.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    *d_bases = static_cast<const uint64_t*>(rd->d_bases);
    return 0;
}

uint32_t set_grid(uint64_t n) { return uint32_t((n + 255) / 256); }

// mlz_stream_open_batch_device behind its argument checks: the walk, then the handle's table.  Returns the handle's size.
int64_t stream_open_batch_locked(mlz_ctx* c, hipStream_t sm, const uint8_t* d_src, const mlz_block_desc* streams, size_t n, int64_t* out_len, mlz_dev_reader* rd) {
    BatchWalk bw;
    const int r = stream_batch_walk(c, sm, d_src, streams, n, &bw);
    if (r) return r;
    std::vector<uint64_t> size(n, 0);
    uint64_t total = 0, src_end = 0;
    size_t nck = 0;
    for (size_t i = 0; i < n; i++) {
        out_len[i] = bw.parsed[i];
        if (streams[i].src_len) src_end = std::max(src_end, streams[i].src_off + streams[i].src_len);
        if (bw.parsed[i] < 0) continue;   // a framing error: nothing of the stream enters the handle
        size[i] = uint64_t(bw.parsed[i]);
        if (size[i] > uint64_t(INT64_MAX) - total) return -MLZ_ERR_ARG;
        total += size[i];
        nck += bw.c1[i] - bw.c0[i];
    }
    if (rd->tabled.on) rd->tabled.st.assign(n, mlz::BatchPlanStream{0, 0, 0, 0, mlz::kBatchPlanSkip, 0});
    if (nck > 0xffffffffull) return -MLZ_ERR_ARG;   // the planners count chunks in 32 bits
    rd->bases.assign(n + 1, 0);
    mlz::set_bases(size.data(), n, rd->bases.data());
    rd->chunks.reserve(nck);
    rd->dchunks.reserve(nck);
    for (size_t i = 0; i < n; i++) {
        if (bw.parsed[i] < 0) continue;
        if (rd->tabled.on)   // the stream's source span up to its first data chunk's body, and its chunks in the handle's list
            rd->tabled.st[i] = mlz::BatchPlanStream{streams[i].src_off, bw.c1[i] > bw.c0[i] ? uint64_t(bw.chunks[bw.c0[i]].body_off) : streams[i].src_off + streams[i].src_len,
                                                    uint32_t(rd->chunks.size()), uint32_t(rd->chunks.size() + (bw.c1[i] - bw.c0[i])), mlz::kBatchPlanWhole, 0};
        for (size_t k = bw.c0[i]; k < bw.c1[i]; k++) {
            StreamChunk ck = bw.chunks[k];
            ck.out_off += size_t(rd->bases[i]);
            rd->chunks.push_back(ck);
            rd->dchunks.push_back(mlz::RdevChunk{uint64_t(ck.out_off), uint64_t(ck.body_off), uint32_t(ck.n), ck.type});
        }
    }
    rd->n = size_t(src_end);
    rd->size = int64_t(total);
    return rd->size;
}

// The entry checks of the calls that translate n items: the handle, the count
int set_enter(mlz_dev_reader* rd, size_t n) { return !rd || uint64_t(n) > mlz::kSetMaxItems ? -MLZ_ERR_ARG : 0; }

// mlz_stream_open_batch_device, and with `tabled` mlz_stream_open_batch_device_tables (mlz_stream_set_tables.hip.inc)
int64_t stream_open_batch_handle(mlz_ctx* c, void* stream, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, int64_t* out_len, mlz_dev_reader** out, bool tabled) {
    if (out) *out = nullptr;
    if (!out) return -MLZ_ERR_ARG;
    const int a = batch_args(c, d_src, nullptr, false, streams, n_streams, out_len, &c);
    if (a < 0) return a;
    if (a > 0) c = c->kids.empty() ? c : c->kids[0];   // no stream: the handle of the first device, as for an empty single stream
    std::lock_guard<std::mutex> lk(c->mu);
    mlz_dev_reader* rd = new (std::nothrow) mlz_dev_reader;
    if (!rd) return -MLZ_ERR_HIP;
    rd->ctx = c; rd->d_src = d_src; rd->set = true;
    rd->bases.assign(1, 0);
    // no inline tables on a plain set: dev_reader_search_tables' hops would run from one stream into another (a tabled set finds them stream
    // by stream: dev_reader_set_tables)
    rd->search[0].ready = rd->search[1].ready = !tabled;
    rd->tabled.on = tabled;
    if (a == 0) {
        hipStream_t sm = static_cast<hipStream_t>(stream);
        const int64_t r = settled(sm, stream_open_batch_locked(c, sm, d_src, streams, size_t(n_streams), out_len, rd));
        if (r < 0) { delete rd; return r; }
    }
    *out = rd;
    return rd->size;
}

}  // namespace

extern "C" {

int64_t mlz_stream_open_batch_device(mlz_ctx* c, void* stream, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, int64_t* out_len, mlz_dev_reader** out) {
    return stream_open_batch_handle(c, stream, d_src, streams, n_streams, out_len, out, false);
}

int64_t mlz_dev_reader_stream_count(const mlz_dev_reader* rd) { return rd ? int64_t(rd->bases.size() - 1) : -MLZ_ERR_ARG; }

int64_t mlz_dev_reader_stream_bases(const mlz_dev_reader* rd, uint64_t* bases) {
    if (!rd || !bases) return -MLZ_ERR_ARG;
    std::memcpy(bases, rd->bases.data(), rd->bases.size() * sizeof(uint64_t));
    return int64_t(rd->bases.size() - 1);
}

int64_t mlz_dev_reader_locate(mlz_dev_reader* rd, void* stream, const uint64_t* d_pos, size_t n, uint32_t* d_which, uint64_t* d_local) {
    if (set_enter(rd, n) || (n && (!d_pos || !d_which || !d_local))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (n == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_pos) || !on_device(c, d_which) || !on_device(c, d_local)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const uint64_t* d_bases = nullptr;
    int64_t r = dev_reader_bases(rd, &d_bases);
    if (r == 0) r = rindex_header(c, sm, sizeof(mlz::SetSums));
    if (r < 0) return r;
    mlz::SetSums* hdr = static_cast<mlz::SetSums*>(c->d_records.p);
    hipLaunchKernelGGL(mlz::set_locate_kernel, dim3(set_grid(n)), dim3(256), 0, sm, d_bases, uint32_t(rd->bases.size() - 1), d_pos, uint64_t(n), d_which, d_local, hdr);
    if ((r = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::SetSums))) < 0) return settled(sm, r);
    return int64_t(static_cast<const mlz::SetSums*>(c->pinned2)->total);
}

int64_t mlz_dev_reader_read_streams_device(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint32_t* d_which, const uint64_t* d_off, const uint64_t* d_len, size_t n_ranges,
                                           uint8_t* d_dst, size_t dst_cap, uint64_t* d_starts) {
    if (!rd || (n_ranges && (!d_which || !d_off || !d_len)) || (!d_dst && dst_cap) || uint64_t(n_ranges) > mlz::kRdevMaxRanges) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    c->range_plan_host = 0;
    if (n_ranges == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_which) || !on_device(c, d_off) || !on_device(c, d_len) || (d_dst && !on_device(c, d_dst)) || (d_starts && !on_device(c, d_starts))) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    c->range_chunks = c->range_scratch = 0;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const uint64_t* d_bases = nullptr;
    int64_t r = dev_reader_bases(rd, &d_bases);
    if (r < 0) return r;
    Carve cv;   // what lives across the read: the header | the ranges' places in the handle
    const auto r_hdr = cv.take<mlz::SetSums>(1);
    const auto r_goff = cv.take<uint64_t>(n_ranges);
    if ((r = rindex_header(c, sm, cv.bytes)) < 0) return r;
    void* ws = c->d_records.p;
    mlz::SetSums* hdr = r_hdr.at(ws);
    hipLaunchKernelGGL(mlz::set_ranges_kernel, dim3(set_grid(n_ranges)), dim3(256), 0, sm, d_bases, uint32_t(rd->bases.size() - 1), d_which, d_off, d_len, uint64_t(n_ranges), r_goff.at(ws), hdr);
    if ((r = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::SetSums))) < 0) return settled(sm, r);
    // the refusal is decided here: nothing has been written to d_dst or d_starts
    if (static_cast<const mlz::SetSums*>(c->pinned2)->bad) return -MLZ_ERR_ARG;
    uint64_t total = 0;
    r = settled(sm, dev_reader_read_device_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, r_goff.at(ws), d_len, uint64_t(n_ranges), d_dst, uint64_t(dst_cap), d_starts, &total));
    return r < 0 ? r : int64_t(total);
}

int64_t mlz_dev_reader_stream_records(mlz_dev_reader* rd, void* stream, uint64_t* first, uint64_t* joined) {
    if (!rd || !first) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (rindex_enter(rd, 0)) return -MLZ_ERR_ARG;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const size_t ns = rd->bases.size() - 1;
    const uint64_t* d_bases = nullptr;
    int64_t r = dev_reader_bases(rd, &d_bases);
    if (r < 0) return r;
    Carve cv;   // the header (unused here, zeroed all the same) | first[ns + 1] | the joined flags[ns]
    (void)cv.take<mlz::SetSums>(1);
    const auto r_out = cv.take<uint64_t>(2 * ns + 1);
    if ((r = rindex_header(c, sm, cv.bytes)) < 0) return r;
    if ((r = ensure_stream_objects(c, 0, (2 * ns + 1) * sizeof(uint64_t))) < 0) return r;
    uint64_t* d_out = r_out.at(c->d_records.p);
    hipLaunchKernelGGL(mlz::set_records_kernel, dim3(set_grid(ns + 1)), dim3(256), 0, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, rd->index_n, d_bases, uint32_t(ns), d_out);
    if ((r = fetch(c, sm, c->pinned2, d_out, (2 * ns + 1) * sizeof(uint64_t))) < 0) return settled(sm, r);
    const uint64_t* h = static_cast<const uint64_t*>(c->pinned2);
    std::memcpy(first, h, (ns + 1) * sizeof(uint64_t));
    uint64_t j = 0;
    for (size_t i = 0; i < ns; i++) j += h[ns + 1 + i];
    if (joined) *joined = j;
    return int64_t(rd->index_n);
}

int64_t mlz_dev_reader_locate_records(mlz_dev_reader* rd, void* stream, const uint64_t* d_rec_no, size_t n, uint32_t* d_which, uint64_t* d_local_no) {
    if (set_enter(rd, n) || (n && (!d_rec_no || !d_which || !d_local_no))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (rindex_enter(rd, n)) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_rec_no) || !on_device(c, d_which) || !on_device(c, d_local_no)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const uint64_t* d_bases = nullptr;
    int64_t r = dev_reader_bases(rd, &d_bases);
    if (r == 0) r = rindex_header(c, sm, sizeof(mlz::SetSums));
    if (r < 0) return r;
    mlz::SetSums* hdr = static_cast<mlz::SetSums*>(c->d_records.p);
    hipLaunchKernelGGL(mlz::set_locate_records_kernel, dim3(set_grid(n)), dim3(256), 0, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, rd->index_n, d_bases,
                       uint32_t(rd->bases.size() - 1), d_rec_no, uint64_t(n), d_which, d_local_no, hdr);
    if ((r = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::SetSums))) < 0) return settled(sm, r);
    return int64_t(static_cast<const mlz::SetSums*>(c->pinned2)->total);
}

}  // extern "C"
