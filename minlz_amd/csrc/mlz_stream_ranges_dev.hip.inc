// mlz_stream_ranges_dev.hip.inc — the device-resident ReadSeeker with its RANGES in device memory (included at the end of mlz_hip.hip, behind
// mlz_stream_ranges.hip.inc whose handle, copy forms and chunk-list decode it uses).
//
// mlz_dev_reader_read_device: offsets and lengths lie in HBM (a sampler's, a top-k's or an index look-up's output) and are validated, located,
// classified and copied by kernels; the rules are those of mlz_stream_ranges_dev.h, which the host check runs as plain loops.  What visits the
// host is proportional to the TOUCHED CHUNKS, never to the ranges: 32 bytes of header (error word, total, pieces, touched chunks), then 16
// bytes per touched chunk down and 16 up (mlz_get_counter 9 counts them), and the decode's 12 bytes of results per chunk as ever.
//
//   R1  rdev_range_kernel    a lane per four ranges, a workgroup per block of 1024: bounds, first and last touched chunk, the difference
//                            arrays (combined in LDS when the stream has few chunks, else within the wavefront, before one non-returning
//                            atomic per distinct word goes to memory), block-local prefixes of lengths and long pieces + block sums.
//   R2  rdev_chunk_kernel    ONE workgroup: scans the block sums (-> starts, total, pieces), then the difference arrays over the chunks
//                            (a slab per lane): count and sole toucher, rdev_chunk_rule, the touched chunks compacted in stream order.
//   R3  rdev_starts_kernel   only when d_starts is wanted, and only once the call is known to go ahead.
//   R4  rdev_gather_kernel   one launch per group (from stream_run_chunk_jobs' after_group), straight from the range arrays: workgroups
//                            [0, pieces) copy one long piece each, the rest serve 16 short ranges each with 16 lanes.  With several groups
//                            every launch visits every range and piece and skips what belongs to another group.
// No kernel waits for another workgroup; the adds are atomicAdd on u32 whose results are not used.

#include "mlz_stream_ranges_dev.h"

namespace mlz {

constexpr uint32_t kRdevThreads = 256, kRdevPer = kRdevBlock / kRdevThreads;
constexpr uint32_t kRdevLdsChunks = 2048;   // streams of fewer chunks: the difference arrays of a workgroup's 1024 ranges are summed in LDS first
constexpr int kRdevCombineRounds = 8;       // else: this many distinct words per wavefront instruction are combined, the rest go one by one

// add (dc, dw) at word `key` of the two difference arrays for every active lane; lanes of a wavefront that meet on a word send one add
__device__ __forceinline__ void rdev_wave_add(uint32_t* __restrict__ cntd, uint32_t* __restrict__ whod, bool active, uint32_t key, uint32_t dc, uint32_t dw) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t todo = __ballot(active);
    for (int round = 0; round < kRdevCombineRounds && todo; round++) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t k = __shfl(key, leader);
        const bool mine = active && key == k;
        const uint64_t m = __ballot(mine);
        uint32_t sw = mine ? dw : 0;
        if (m & (m - 1))
            for (int d = 32; d; d >>= 1) sw += __shfl_xor(sw, d);
        if (lane == uint32_t(leader)) {
            atomicAdd(&cntd[k], dc * uint32_t(__popcll(m)));
            atomicAdd(&whod[k], sw);
        }
        todo &= ~m;
    }
    if (active && (todo >> lane & 1)) {
        atomicAdd(&cntd[key], dc);
        atomicAdd(&whod[key], dw);
    }
}

// R1.  Range i of block b is lane (i % 1024) / 4's: a lane's four ranges are neighbours, so its running sums are the prefix.
struct RdevSums { uint64_t l, p; };   // lengths and long pieces: one scan for both
__global__ __launch_bounds__(kRdevThreads) void rdev_range_kernel(const RdevChunk* __restrict__ ck, uint32_t nck, uint64_t size, uint64_t avg, const uint64_t* __restrict__ d_off,
                                                                  const uint64_t* __restrict__ d_len, uint64_t n, uint32_t short_max, uint32_t* __restrict__ first,
                                                                  uint64_t* __restrict__ len_local, uint32_t* __restrict__ piece_local, uint64_t* __restrict__ len_block,
                                                                  uint64_t* __restrict__ piece_block, uint32_t* __restrict__ cntd, uint32_t* __restrict__ whod, RdevHeader* __restrict__ hdr) {
    __shared__ uint32_t lc[kRdevLdsChunks], lw[kRdevLdsChunks];
    __shared__ RdevSums ss[kRdevThreads];
    const uint32_t tid = threadIdx.x;
    const bool in_lds = nck < kRdevLdsChunks;   // nck + 1 words
    if (in_lds) {
        for (uint32_t k = tid; k <= nck; k += kRdevThreads) { lc[k] = 0; lw[k] = 0; }
        __syncthreads();
    }
    const uint64_t i0 = uint64_t(blockIdx.x) * kRdevBlock + tid * kRdevPer;
    uint64_t lens[kRdevPer], pcs[kRdevPer], tl = 0, tp = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t k = 0; k < kRdevPer; k++) {
        const uint64_t i = i0 + k;
        RdevRange r{0, 0, 0, false, false};
        lens[k] = 0;
        if (i < n) {
            const uint64_t off = d_off[i], len = d_len[i];
            r = rdev_range_rule(ck, nck, size, avg, off, len, short_max, kPlacePiece);
            bad = bad || r.bad;
            lens[k] = r.bad ? 0 : len;
            first[i] = r.j0;
        }
        pcs[k] = r.pieces;
        tl = rdev_sat_add(tl, lens[k]);
        tp = rdev_sat_add(tp, pcs[k]);
        if (in_lds) {
            if (r.live) {
                atomicAdd(&lc[r.j0], 1u); atomicAdd(&lw[r.j0], uint32_t(i));
                atomicAdd(&lc[r.j1 + 1], ~0u); atomicAdd(&lw[r.j1 + 1], 0u - uint32_t(i));
            }
        } else {
            rdev_wave_add(cntd, whod, r.live, r.j0, 1u, uint32_t(i));
            rdev_wave_add(cntd, whod, r.live, r.j1 + 1, ~0u, 0u - uint32_t(i));
        }
    }
    if (bad) hdr->err = 1;
    // exclusive prefix of the lanes' sums over the workgroup
    RdevSums sum;
    const RdevSums run = wg_scan<kRdevThreads>(RdevSums{tl, tp}, ss, tid, [](RdevSums x, RdevSums y) { return RdevSums{rdev_sat_add(x.l, y.l), rdev_sat_add(x.p, y.p)}; }, &sum);
    uint64_t rl = run.l, rp = run.p;
#pragma unroll
    for (uint32_t k = 0; k < kRdevPer; k++) {
        if (i0 + k < n) { len_local[i0 + k] = rl; piece_local[i0 + k] = uint32_t(rp); }
        rl = rdev_sat_add(rl, lens[k]); rp = rdev_sat_add(rp, pcs[k]);
    }
    if (tid == kRdevThreads - 1) { len_block[blockIdx.x] = sum.l; piece_block[blockIdx.x] = sum.p; }
    if (in_lds) {   // (the LDS adds were all made in front of the scan's first barrier)
        for (uint32_t k = tid; k <= nck; k += kRdevThreads) {
            if (lc[k]) atomicAdd(&cntd[k], lc[k]);
            if (lw[k]) atomicAdd(&whod[k], lw[k]);
        }
    }
}

constexpr uint32_t kRdevScanThreads = 1024;

struct RdevPair { uint32_t c, w; };

// R2.  len_block / piece_block: block sums in, exclusive block offsets out.
__global__ __launch_bounds__(kRdevScanThreads) void rdev_chunk_kernel(const RdevChunk* __restrict__ ck, uint32_t nck, const uint64_t* __restrict__ d_off, const uint64_t* __restrict__ d_len,
                                                                      uint64_t nb, uint64_t* __restrict__ len_block, uint64_t* __restrict__ piece_block,
                                                                      const uint64_t* __restrict__ len_local, const uint32_t* __restrict__ cntd, const uint32_t* __restrict__ whod,
                                                                      uint32_t* __restrict__ slot, RdevTouched* __restrict__ touched, RdevHeader* __restrict__ hdr) {
    __shared__ uint64_t s64[kRdevScanThreads];
    __shared__ RdevPair s32[kRdevScanThreads];
    const uint32_t tid = threadIdx.x;
    auto sat = [](uint64_t a, uint64_t b) { return rdev_sat_add(a, b); };
    {   // the block sums: a slab per lane
        const uint64_t per = (nb + kRdevScanThreads - 1) / kRdevScanThreads;
        const uint64_t b = tid * per < nb ? tid * per : nb, e = b + per < nb ? b + per : nb;
        uint64_t sl = 0, sp = 0, tot_l = 0, tot_p = 0;
        for (uint64_t k = b; k < e; k++) { sl = rdev_sat_add(sl, len_block[k]); sp = rdev_sat_add(sp, piece_block[k]); }
        uint64_t rl = wg_scan<kRdevScanThreads>(sl, s64, tid, sat, &tot_l);
        uint64_t rp = wg_scan<kRdevScanThreads>(sp, s64, tid, sat, &tot_p);
        for (uint64_t k = b; k < e; k++) {
            const uint64_t l = len_block[k], p = piece_block[k];
            len_block[k] = rl; piece_block[k] = rp;
            rl = rdev_sat_add(rl, l); rp = rdev_sat_add(rp, p);
        }
        if (tid == 0) { hdr->total = tot_l; hdr->pieces = tot_p; }
        __syncthreads();   // the block offsets are read below by other lanes (rdev_start)
    }
    // the chunks: a slab per lane
    const uint32_t per = (nck + kRdevScanThreads - 1) / kRdevScanThreads;
    const uint32_t b = uint64_t(tid) * per < nck ? tid * per : nck, e = nck - b > per ? b + per : nck;
    RdevPair s{0, 0}, tot{0, 0};
    for (uint32_t j = b; j < e; j++) { s.c += cntd[j]; s.w += whod[j]; }
    const RdevPair run0 = wg_scan<kRdevScanThreads>(s, s32, tid, [](RdevPair x, RdevPair y) { return RdevPair{x.c + y.c, x.w + y.w}; }, &tot);
    RdevTouched t;
    uint32_t mine = 0;
    RdevPair run = run0;
    for (uint32_t j = b; j < e; j++) {
        run.c += cntd[j]; run.w += whod[j];
        mine += rdev_chunk_rule(ck[j], j, run.c, run.w, d_off, d_len, len_block, len_local, &t) ? 1u : 0u;
    }
    RdevPair nt{0, 0};
    uint32_t at = wg_scan<kRdevScanThreads>(RdevPair{mine, 0}, s32, tid, [](RdevPair x, RdevPair y) { return RdevPair{x.c + y.c, 0}; }, &nt).c;
    run = run0;
    for (uint32_t j = b; j < e; j++) {
        run.c += cntd[j]; run.w += whod[j];
        if (rdev_chunk_rule(ck[j], j, run.c, run.w, d_off, d_len, len_block, len_local, &t)) { slot[j] = at; touched[at++] = t; }
    }
    if (tid == 0) hdr->touched = nt.c;
}

// R3.
__global__ __launch_bounds__(256) void rdev_starts_kernel(uint64_t n, const uint64_t* __restrict__ len_block, const uint64_t* __restrict__ len_local, const RdevHeader* __restrict__ hdr,
                                                          uint64_t* __restrict__ d_starts) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) d_starts[i] = rdev_start(len_block, len_local, i);
    else if (i == n) d_starts[n] = hdr->total;
}

struct RdevGatherArgs {
    const RdevChunk* ck; const uint64_t *d_off, *d_len, *len_block, *len_local, *piece_block; const uint32_t *piece_local, *first, *slot; const RdevPlace* place;
    const uint8_t *scratch, *stream; uint8_t* dst;
    uint64_t n, nb, avg; uint32_t nck, n_pieces, group, short_max;
};

// R4.
__global__ __launch_bounds__(256) void rdev_gather_kernel(const RdevGatherArgs a) {
    uint64_t src, dst;
    uint32_t len;
    bool from_stream;
    if (blockIdx.x < a.n_pieces) {   // a long piece: bytes [q * 64 KiB, + 64 KiB) of its range, through the chunks it meets
        uint64_t q;
        const uint64_t i = rdev_piece_owner(a.piece_block, a.piece_local, a.n, a.nb, blockIdx.x, &q);
        const uint64_t off = a.d_off[i], end = off + a.d_len[i], start = rdev_start(a.len_block, a.len_local, i);
        const uint64_t wb = off + q * kPlacePiece, we = end - wb > kPlacePiece ? wb + kPlacePiece : end;
        for (uint32_t j = q ? range_locate(a.ck, a.nck, a.avg, wb) : a.first[i]; j < a.nck && a.ck[j].out_off < we; j++) {
            const RdevChunk c = a.ck[j];
            if (!c.n) continue;
            if (rdev_intersect(c, a.place[a.slot[j]], a.group, off, start, wb, we, &src, &dst, &len, &from_stream))
                wg_copy(a.dst + dst, (from_stream ? a.stream : a.scratch) + src, len, threadIdx.x, 256);
        }
        return;
    }
    const uint64_t i = uint64_t(blockIdx.x - a.n_pieces) * kRangeShortPerWg + (threadIdx.x >> 4);
    if (i >= a.n) return;
    const uint64_t rlen = a.d_len[i];
    if (!rlen || rlen > a.short_max) return;
    const uint64_t off = a.d_off[i], end = off + rlen, start = rdev_start(a.len_block, a.len_local, i);
    for (uint32_t j = a.first[i]; j < a.nck && a.ck[j].out_off < end; j++) {
        const RdevChunk c = a.ck[j];
        if (!c.n) continue;
        if (rdev_intersect(c, a.place[a.slot[j]], a.group, off, start, off, end, &src, &dst, &len, &from_stream))
            lanes16_copy(a.dst + dst, (from_stream ? a.stream : a.scratch) + src, len, threadIdx.x & 15);
    }
}

}  // namespace mlz

namespace {

int64_t dev_reader_read_device_locked(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const uint64_t* d_off, const uint64_t* d_len, uint64_t n, uint8_t* d_dst, uint64_t dst_cap,
                                      uint64_t* d_starts, uint64_t* total_out) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    HIPCHK(c, hipSetDevice(c->device));
    if (nck && !rd->d_chunks) {   // once per handle: the chunk table where kernels can read it
        HIPCHK(c, hipMalloc(&rd->d_chunks, nck * sizeof(mlz::RdevChunk)));
        HIPCHK(c, hipMemcpy(rd->d_chunks, rd->dchunks.data(), nck * sizeof(mlz::RdevChunk), hipMemcpyHostToDevice));
    }
    const uint64_t nb = (n + mlz::kRdevBlock - 1) / mlz::kRdevBlock;
    // header | count differences | index differences | slot | touched, then places | first | piece prefix | length prefix | block sums
    Carve cv;   // (the header and the difference arrays lie in front: one memset clears them)
    const auto r_hdr = cv.take<mlz::RdevHeader>(1);
    const auto r_cntd = cv.take<uint32_t>(nck + 1), r_whod = cv.take<uint32_t>(nck + 1), r_slot = cv.take<uint32_t>(nck);
    const auto r_touched = cv.take<mlz::RdevTouched>(nck);
    const auto r_first = cv.take<uint32_t>(size_t(n)), r_plocal = cv.take<uint32_t>(size_t(n));
    const auto r_llocal = cv.take<uint64_t>(size_t(n)), r_lblock = cv.take<uint64_t>(size_t(nb)), r_pblock = cv.take<uint64_t>(size_t(nb));
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    int r = ensure_stream_objects(c, 0, 64);
    if (r) return r;
    void* ws = c->d_rplan.p;
    mlz::RdevHeader* hdr = r_hdr.at(ws);
    mlz::RdevTouched* touched = r_touched.at(ws);
    uint32_t *cntd = r_cntd.at(ws), *whod = r_whod.at(ws), *slot = r_slot.at(ws), *first = r_first.at(ws), *piece_local = r_plocal.at(ws);
    uint64_t *len_local = r_llocal.at(ws), *len_block = r_lblock.at(ws), *piece_block = r_pblock.at(ws);
    const mlz::RdevChunk* ck = static_cast<const mlz::RdevChunk*>(rd->d_chunks);
    const uint64_t size = uint64_t(rd->size), avg = std::max<uint64_t>(1, nck ? size / nck : 1);

    WorkspaceOrder order(c, sm);
    HIPCHK(c, hipMemsetAsync(ws, 0, r_slot.off, sm));   // header and difference arrays
    hipLaunchKernelGGL(mlz::rdev_range_kernel, dim3(uint32_t(nb)), dim3(mlz::kRdevThreads), 0, sm, ck, uint32_t(nck), size, avg, d_off, d_len, n, mlz::kRangeShortMax, first, len_local,
                       piece_local, len_block, piece_block, cntd, whod, hdr);
    hipLaunchKernelGGL(mlz::rdev_chunk_kernel, dim3(1), dim3(mlz::kRdevScanThreads), 0, sm, ck, uint32_t(nck), d_off, d_len, nb, len_block, piece_block, len_local, cntd, whod, slot,
                       touched, hdr);
    if ((r = fetch(c, sm, c->pinned2, hdr, sizeof(mlz::RdevHeader)))) return r;
    const mlz::RdevHeader h = *static_cast<const mlz::RdevHeader*>(c->pinned2);
    c->range_plan_host = sizeof(mlz::RdevHeader);
    if (h.err) return -MLZ_ERR_ARG;
    if (h.total > dst_cap || h.total == ~uint64_t(0)) return -MLZ_ERR_DST_TOO_SMALL;
    const uint64_t grid = h.pieces + (n + mlz::kRangeShortPerWg - 1) / mlz::kRangeShortPerWg;
    if (h.pieces > mlz::kRdevMaxGrid || grid > mlz::kRdevMaxGrid) return -MLZ_ERR_ARG;
    *total_out = h.total;
    if (d_starts) hipLaunchKernelGGL(mlz::rdev_starts_kernel, dim3(uint32_t((n + 1 + 255) / 256)), dim3(256), 0, sm, n, len_block, len_local, hdr, d_starts);
    const size_t nt = h.touched;
    if (nt == 0) {
        if (d_starts) { HIPCHK(c, hipStreamSynchronize(sm)); HIPCHK(c, hipGetLastError()); }
        return 0;
    }
    // the touched chunks come down, their places go up: behind the part of the pinned buffer that stream_run_chunk_jobs uses
    Carve pin;
    const ChunkJobResults res = take_chunk_job_results(&pin, nt);
    const auto r_htouched = pin.take<mlz::RdevTouched>(nt, 64);
    const auto r_hplace = pin.take<mlz::RdevPlace>(nt);
    r = ensure_stream_objects(c, 0, pin.bytes);
    if (r) return r;
    mlz::RdevTouched* h_touched = r_htouched.at(c->pinned2);
    mlz::RdevPlace* h_place = r_hplace.at(c->pinned2);
    if ((r = fetch(c, sm, h_touched, touched, nt * sizeof(mlz::RdevTouched)))) return r;
    std::vector<mlz::RdevPlace> places;
    std::vector<size_t> gend;
    std::vector<uint8_t> group_copies;
    uint64_t scratch_total = 0, scratch_max = 0;
    for (size_t t = 0; t < nt; t++)
        if (h_touched[t].chunk >= nck) { c->err = "mlz_dev_reader_read_device: the plan names a chunk the stream does not have"; return -MLZ_ERR_HIP; }
    mlz::rdev_host_places(h_touched, nt, [&](uint32_t j) { return uint64_t(rd->chunks[j].n); }, &places, &gend, &group_copies, &scratch_total, &scratch_max);
    c->range_chunks = nt;
    c->range_scratch = scratch_total;
    c->range_plan_host += nt * (sizeof(mlz::RdevTouched) + sizeof(mlz::RdevPlace));
    if (scratch_max) HIPCHK(c, c->d_range.ensure(size_t(scratch_max)));
    const uint8_t* scratch = c->d_range.as<uint8_t>();
    std::vector<ChunkJob> jobs(nt);
    for (size_t t = 0; t < nt; t++) {
        const mlz::RdevTouched& tc = h_touched[t];
        if (tc.where == mlz::kRangeDirect && (tc.at > h.total || rd->chunks[tc.chunk].n > h.total - tc.at)) { c->err = "mlz_dev_reader_read_device: a direct chunk's place lies outside the destination"; return -MLZ_ERR_HIP; }
        jobs[t] = ChunkJob{tc.chunk, tc.where == mlz::kRangeDirect ? d_dst + tc.at : tc.where == mlz::kRangeScratch ? scratch + places[t].base : rd->d_src + rd->chunks[tc.chunk].body_off};
        h_place[t] = places[t];
    }
    mlz::RdevPlace* d_place = reinterpret_cast<mlz::RdevPlace*>(touched);   // (the list has been read: its memory takes the places)
    HIPCHK(c, hipMemcpyAsync(d_place, h_place, nt * sizeof(mlz::RdevPlace), hipMemcpyHostToDevice, sm));
    mlz::RdevGatherArgs ga{ck, d_off, d_len, len_block, len_local, piece_block, piece_local, first, slot, d_place, scratch, rd->d_src, d_dst,
                           n, nb, avg, uint32_t(nck), uint32_t(h.pieces), 0, mlz::kRangeShortMax};
    auto copy_group = [&](size_t g) -> int {
        if (!group_copies[g]) return 0;   // (every chunk of the group decodes straight into its place)
        ga.group = uint32_t(g);
        hipLaunchKernelGGL(mlz::rdev_gather_kernel, dim3(uint32_t(grid)), dim3(256), 0, sm, ga);
        return 0;
    };
    return stream_run_chunk_jobs(c, sm, ignore_crc, rd->d_src, rd->chunks, jobs, gend, res, copy_group);
}

}  // namespace

extern "C" int64_t mlz_dev_reader_read_device(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint64_t* d_off, const uint64_t* d_len, size_t n_ranges, uint8_t* d_dst,
                                              size_t dst_cap, uint64_t* d_starts) {
    if (!rd || (n_ranges && (!d_off || !d_len)) || (!d_dst && dst_cap) || uint64_t(n_ranges) > mlz::kRdevMaxRanges) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    c->range_plan_host = 0;
    if (n_ranges == 0) return 0;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_off) || !on_device(c, d_len) || (d_dst && !on_device(c, d_dst)) || (d_starts && !on_device(c, d_starts))) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    c->range_chunks = c->range_scratch = 0;
    uint64_t total = 0;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const int64_t r = settled(sm, dev_reader_read_device_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, d_off, d_len, uint64_t(n_ranges), d_dst, uint64_t(dst_cap), d_starts, &total));
    return r < 0 ? r : int64_t(total);
}
