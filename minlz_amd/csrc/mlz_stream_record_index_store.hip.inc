// mlz_stream_record_index_store.hip.inc — the record index of a handle saved as a blob in HBM, loaded from one without a decode, and built
// from raw bytes (included from mlz_hip.hip behind mlz_stream_record_index.hip.inc; the C ABI is include/minlz_hip_record_index_store.h).
// The layout and every rule are mlz_stream_record_index_store.h's, which the host check runs as plain loops.
//
// Save (rstore_save_locked, from D[0, k) in device memory):
//   rstore_bounds_kernel   a lane per tile boundary bisects D (rindex_number): the rank of the first delimiter of every 64 KiB tile;
//   rstore_scan_kernel     a workgroup per section over its <= 1024 tiles (wg_scan): every tile's payload offset, the section's length and its
//                          dense tiles; 8 bytes per section come home, the host lays out directory and chunks, checks dst_cap, and sends up
//                          8 bytes per section and the header chunk, which it makes itself;
//   rstore_pack_kernel     a workgroup per tile.  Sparse: a lane per entry, u16 stores side by side.  Dense: the 8 KiB bitmap zeroed in LDS,
//                          filled with LDS atomic OR, written with dword stores.  Lane 0: the tile's count, and in a section's first tile its header;
//   the CRC pass           crc_device_locked over the sections as they lie in d_dst;
//   rstore_place_kernel    the identifier and header chunk, every section's chunk header and CRC, the EOF chunk.
// Load (dev_reader_load_record_index_locked): the host fetches the header chunk, checks it (rstore_parse_fixed, rstore_match,
//   rstore_parse_directory: what mlz_record_index_parse runs), allocates 8 k bytes (k <= size has been checked) and sends up 16 bytes per section;
//   rstore_frames_kernel   a lane per section: its chunk header, and its CRC against the CRC pass's unless MLZ_STREAM_IGNORE_CRC; the EOF chunk;
//   rstore_expand_kernel   a workgroup per tile checks before it reads (rstore_tile_plan: section header, counts, ranks, the payload's place
//                          inside the section, which the directory has bounded by len), then expands: sparse a lane per entry (ascending,
//                          below the size), dense 8 words per lane, ranked by popcount and a wavefront scan (popcount = count, no bit beyond
//                          the size).  No rank at or beyond k is written.  Verdicts are ORed into one record; 16 bytes come home.
// Both directions take the dword path when the blob is 4-aligned and a bytewise path otherwise (the template parameter A).
// Build (mlz_record_index_build_device): rindex_count_kernel / rindex_scan_kernel / rindex_emit_kernel over the raw bytes (first = 0, the
// buffer's misalignment as a scratch group's) into context workspace, then the save path.  No kernel waits for another workgroup.

#include "../../include/minlz_hip_record_index_store.h"
#include "mlz_stream_record_index_store.h"

static_assert(mlz::kRstoreErrCorrupt == MLZ_ERR_CORRUPT && mlz::kRstoreErrUnsupported == MLZ_ERR_UNSUPPORTED && mlz::kRstoreErrCrc == MLZ_ERR_CRC &&
              mlz::kRstoreErrDstTooSmall == MLZ_ERR_DST_TOO_SMALL && mlz::kRstoreErrArg == MLZ_ERR_ARG, "mlz_stream_record_index_store.h restates the header");
static_assert(mlz::kRstoreSectionTiles == mlz::kRecordsScanThreads, "a lane per tile of a section");

namespace mlz {

template <bool A> __device__ __forceinline__ uint32_t rstore_ld32(const uint8_t* p) { return A ? *reinterpret_cast<const uint32_t*>(p) : rstore_get32(p); }
template <bool A> __device__ __forceinline__ uint32_t rstore_ld16(const uint8_t* p) { return A ? uint32_t(*reinterpret_cast<const uint16_t*>(p)) : rstore_get16(p); }
template <bool A> __device__ __forceinline__ void rstore_st32(uint8_t* p, uint32_t v) { if (A) *reinterpret_cast<uint32_t*>(p) = v; else rstore_put32(p, v); }
template <bool A> __device__ __forceinline__ void rstore_st16(uint8_t* p, uint32_t v) { if (A) *reinterpret_cast<uint16_t*>(p) = uint16_t(v); else { p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); } }

// first[t] = the rank of the first delimiter at or behind t * 65536, for t <= ntiles (first[ntiles] = k)
__global__ __launch_bounds__(kRstoreThreads) void rstore_bounds_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t ntiles, uint64_t* __restrict__ first) {
    const uint64_t t = uint64_t(blockIdx.x) * kRstoreThreads + threadIdx.x;
    if (t <= ntiles) first[t] = rstore_first([&](uint64_t j) { return D[j]; }, k, ntiles, t);
}

// A workgroup per section: tile_off[t] = where tile t's payload lies in its section; sec_out[s] = (the section's length, its dense tiles)
__global__ __launch_bounds__(kRstoreSectionTiles) void rstore_scan_kernel(const uint64_t* __restrict__ first, uint64_t ntiles, uint32_t* __restrict__ tile_off, uint2* __restrict__ sec_out) {
    __shared__ uint32_t lds[kRstoreSectionTiles];
    __shared__ uint32_t dense;
    const uint32_t tid = threadIdx.x, s = blockIdx.x, tiles = rstore_section_tiles(ntiles, s);
    const uint64_t t = uint64_t(s) * kRstoreSectionTiles + tid;
    uint32_t bytes = 0, tot = 0;
    bool dn = false;
    if (tid < tiles) {
        const uint32_t c = uint32_t(first[t + 1] - first[t]);
        bytes = rstore_payload_bytes(c);
        dn = rstore_dense(c);
    }
    if (tid == 0) dense = 0;
    const uint32_t off = wg_scan<kRstoreSectionTiles>(bytes, lds, tid, [](uint32_t x, uint32_t y) { return x + y; }, &tot);
    if (dn) atomicAdd(&dense, 1u);
    __syncthreads();
    if (tid < tiles) tile_off[t] = rstore_section_head(tiles) + off;
    if (tid == 0) sec_out[s] = make_uint2(rstore_section_head(tiles) + tot, dense);
}

// A workgroup per tile: its payload, its count, and in a section's first tile the section's header.  sec_off[s]: where section s's bytes lie in dst.
template <bool A>
__global__ __launch_bounds__(kRstoreThreads) void rstore_pack_kernel(const uint64_t* __restrict__ D, const uint64_t* __restrict__ first, const uint32_t* __restrict__ tile_off,
                                                                     const uint64_t* __restrict__ sec_off, uint64_t ntiles, uint8_t* __restrict__ dst) {
    __shared__ uint32_t bitmap[kRstoreBitmap / 4];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x, s = t / kRstoreSectionTiles;
    const uint32_t i = uint32_t(t % kRstoreSectionTiles), tiles = rstore_section_tiles(ntiles, s);
    uint8_t* sec = dst + sec_off[s];
    const uint64_t f0 = first[t], f1 = first[t + 1], fs = first[s * kRstoreSectionTiles];
    const uint32_t c = uint32_t(f1 - f0);
    if (tid == 0) {
        if (i == 0) {
            rstore_st32<A>(sec, uint32_t(s)); rstore_st32<A>(sec + 4, tiles);
            rstore_st32<A>(sec + 8, uint32_t(fs)); rstore_st32<A>(sec + 12, uint32_t(fs >> 32));
            rstore_st32<A>(sec + 16, 0);
        }
        rstore_st32<A>(sec + 20 + 4 * i, uint32_t(f1 - fs));
    }
    uint8_t* out = sec + tile_off[t];
    const auto at = [&](uint64_t j) { return D[j]; };
    if (!rstore_dense(c)) {
        for (uint32_t j = tid; j < c + (c & 1); j += kRstoreThreads) rstore_st16<A>(out + 2 * j, rstore_sparse_entry(at, f0, c, t, j));
        return;
    }
    for (uint32_t w = tid; w < kRstoreBitmap / 4; w += kRstoreThreads) bitmap[w] = 0;
    __syncthreads();
    for (uint32_t j = tid; j < c; j += kRstoreThreads) {
        const uint64_t rel = D[f0 + j] - (t << kRstoreTileLog);   // (< 65536 by the bisection of an ascending table)
        if (rel < kRstoreTile) atomicOr(&bitmap[uint32_t(rel) >> 5], 1u << (uint32_t(rel) & 31));
    }
    __syncthreads();
    for (uint32_t w = tid; w < kRstoreBitmap / 4; w += kRstoreThreads) rstore_st32<A>(out + 4 * w, bitmap[w]);
}

// The identifier and the header chunk (head[0, head_n)), every section's chunk header and CRC, the EOF chunk at eof_at
__global__ __launch_bounds__(kRstoreThreads) void rstore_place_kernel(const uint8_t* __restrict__ head, uint32_t head_n, const uint64_t* __restrict__ sec_off, const uint2* __restrict__ sec_out,
                                                                      const uint32_t* __restrict__ crc, uint32_t nsections, uint64_t eof_at, uint8_t* __restrict__ dst) {
    const uint32_t g = blockIdx.x * kRstoreThreads + threadIdx.x;
    for (uint32_t j = g; j < head_n; j += gridDim.x * kRstoreThreads) dst[j] = head[j];
    if (g < nsections) {
        uint8_t* p = dst + sec_off[g] - 8;
        rstore_chunk_header(p, kRstoreChunkSection, 4 + sec_out[g].x);
        rstore_put32(p + 4, crc[g]);
    }
    if (g == 0) rstore_put_eof(dst + eof_at);
}

// A lane per section: its chunk header against the directory's entry, its CRC (crc == nullptr: not looked at); lane 0: the EOF chunk
__global__ __launch_bounds__(kRstoreThreads) void rstore_frames_kernel(const uint8_t* __restrict__ blob, const RstoreSection* __restrict__ secs, const uint32_t* __restrict__ crc,
                                                                       uint32_t nsections, uint64_t eof_at, RstoreVerdict* __restrict__ out) {
    const uint32_t g = blockIdx.x * kRstoreThreads + threadIdx.x;
    if (g < nsections) {
        const uint8_t* p = blob + secs[g].off - 8;
        const uint32_t len24 = uint32_t(p[1]) | uint32_t(p[2]) << 8 | uint32_t(p[3]) << 16;
        if (p[0] != kRstoreChunkSection || len24 != 4 + secs[g].len) atomicOr(&out->bad, kRstoreBadSection);
        if (crc && rstore_get32(p + 4) != crc[g]) atomicOr(&out->crc_bad, 1u);
    }
    if (g == 0) {
        const uint8_t* e = blob + eof_at;
        if (e[0] != 0x20 || e[1] != 1 || e[2] || e[3] || e[4]) atomicOr(&out->bad, kRstoreBadSection);
    }
}

// A workgroup per tile: table[rank] = the position of the tile's delimiters, after the checks of rstore_tile_plan.  secs: from the directory,
// every section inside the blob.  *out: zeroed by the caller.
template <bool A>
__global__ __launch_bounds__(kRstoreThreads) void rstore_expand_kernel(const uint8_t* __restrict__ blob, const RstoreSection* __restrict__ secs, uint64_t ntiles, uint64_t nsections,
                                                                       uint64_t size, uint64_t k, uint64_t* __restrict__ table, RstoreVerdict* __restrict__ out) {
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t t = blockIdx.x, s = t / kRstoreSectionTiles;
    const uint32_t i = uint32_t(t % kRstoreSectionTiles), tiles = rstore_section_tiles(ntiles, s);
    const RstoreSection sec = secs[s];
    const auto ld32 = [&](uint64_t off) { return rstore_ld32<A>(blob + off); };
    // the payload bytes of the section's tiles in front of this one (the counts lie inside the section's head, which the directory has bounded)
    uint32_t part = 0;
    for (uint32_t j = tid; j < i; j += kRstoreThreads) part += rstore_count_bytes(ld32(sec.off + 16 + 4 * uint64_t(j)), ld32(sec.off + 20 + 4 * uint64_t(j)));
    for (int d = 32; d; d >>= 1) part += uint32_t(__shfl_xor(int(part), d));
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    const uint32_t before = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    uint64_t next_first = k;
    if (i + 1 == tiles && s + 1 < nsections) {
        const uint64_t no = secs[s + 1].off;
        next_first = uint64_t(ld32(no + 8)) | uint64_t(ld32(no + 12)) << 32;
    }
    const RstoreTilePlan p = rstore_tile_plan(ld32, sec, s, tiles, i, before, next_first, k);
    if (p.bad) {
        if (tid == 0) atomicOr(&out->bad, p.bad);
        return;
    }
    const uint64_t t0 = t << kRstoreTileLog;
    const uint32_t limit = size - t0 < kRstoreTile ? uint32_t(size - t0) : kRstoreTile;
    const uint8_t* pay = blob + p.payload;
    uint32_t bad = 0, last = 0;
    if (!rstore_dense(p.c)) {
        for (uint32_t j = tid; j < p.c + (p.c & 1); j += kRstoreThreads) {
            const uint32_t v = rstore_ld16<A>(pay + 2 * j), prev = j ? rstore_ld16<A>(pay + 2 * j - 2) : 0;
            bad |= rstore_sparse_check(v, prev, j > 0, j == p.c, limit);
            if (j < p.c) {
                table[p.rank + j] = t0 + v;   // (rank + c <= k by the plan)
                last |= t0 + v + 1 == size ? 1u : 0u;
            }
        }
    } else {
        uint32_t w[8], pc = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            w[q] = rstore_ld32<A>(pay + 4 * (8 * tid + q));
            bad |= rstore_dense_check(w[q], 8 * tid + q, limit);
            pc += rindex_popcount(w[q]);
        }
        const uint32_t incl = wave_incl_scan(pc);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t r = incl - pc;
        for (uint32_t v = 0; v < wave; v++) r += wsum[v];
        if (wsum[0] + wsum[1] + wsum[2] + wsum[3] != p.c) bad |= kRstoreBadDense;
#pragma unroll
        for (uint32_t q = 0; q < 8; q++)
            for (uint32_t m = w[q]; m; m &= m - 1, r++) {
                const uint64_t pos = t0 + 32 * (8 * tid + q) + uint32_t(__ffs(int(m)) - 1);
                if (r < p.c) table[p.rank + r] = pos;
                last |= pos + 1 == size ? 1u : 0u;
            }
    }
    if (bad) atomicOr(&out->bad, bad);
    if (last) atomicOr(&out->last_is_delim, 1u);
}

}  // namespace mlz

namespace {

// What binds a blob to the handle: the tag over its data chunks with bytes
mlz::RstoreTag rstore_tag_of(const mlz_dev_reader* rd) {
    mlz::RstoreTag tg;
    for (const StreamChunk& ck : rd->chunks)
        if (ck.n) tg.add(uint32_t(ck.n), ck.crc, ck.type);
    return tg;
}

bool rstore_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The blob of the index D[0, k) (device memory) of `size` decoded bytes into d_dst[0, cap); proto: flags, delimiter, N, longest and the binding.
// info (may be NULL): bytes, sections, sparse tiles, dense tiles.  -> the blob's bytes
int64_t rstore_save_locked(mlz_ctx* c, hipStream_t sm, const uint64_t* D, uint64_t k, uint64_t size, mlz::RstoreHeader h, uint8_t* d_dst, uint64_t cap, uint64_t* info) {
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t nt = mlz::rstore_ntiles(size), ns = mlz::rstore_nsections(size);
    const uint32_t head_n = uint32_t(mlz::kRstoreDirAt + 4 * ns);
    Carve cv, pin;   // workspace: first | tile offsets | (length, dense) per section | section offsets, head (go up as one block) | CRCs; pinned: what comes home | what goes up
    const auto r_first = cv.take<uint64_t>(size_t(nt) + 1);
    const auto r_toff = cv.take<uint32_t>(size_t(nt));
    const auto r_out = cv.take<uint2>(size_t(ns));
    const auto r_up = cv.take<uint8_t>(size_t(8 * ns) + head_n);
    const auto r_crc = cv.take<uint32_t>(size_t(ns));
    const auto h_out_r = pin.take<uint2>(size_t(ns));
    const auto h_up_r = pin.take<uint8_t>(size_t(8 * ns) + head_n, 64);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    int e = ensure_stream_objects(c, 0, pin.bytes);
    if (e) return e;
    void* ws = c->d_rplan.p;
    uint2* h_out = h_out_r.at(c->pinned2);
    uint8_t* h_up = h_up_r.at(c->pinned2);
    uint64_t* h_off = reinterpret_cast<uint64_t*>(h_up);
    { WorkspaceOrder order(c, sm); }
    uint64_t dense = 0, at = head_n;
    if (ns) {
        hipLaunchKernelGGL(mlz::rstore_bounds_kernel, dim3(uint32_t((nt + 1 + mlz::kRstoreThreads - 1) / mlz::kRstoreThreads)), dim3(mlz::kRstoreThreads), 0, sm, D, k, nt, r_first.at(ws));
        hipLaunchKernelGGL(mlz::rstore_scan_kernel, dim3(uint32_t(ns)), dim3(mlz::kRstoreSectionTiles), 0, sm, r_first.at(ws), nt, r_toff.at(ws), r_out.at(ws));
        if ((e = fetch(c, sm, h_out, r_out.at(ws), size_t(ns) * sizeof(uint2)))) return e;
    }
    std::vector<uint32_t> dir(size_t(ns), 0);
    std::vector<mlz_block_desc> desc(size_t(ns), mlz_block_desc{});
    for (uint64_t s = 0; s < ns; s++) {
        const uint32_t tiles = mlz::rstore_section_tiles(nt, s), n = h_out[s].x, lo = mlz::rstore_section_head(tiles);
        if (n < lo || n > lo + uint64_t(mlz::kRstoreBitmap) * tiles || (n & 3) || h_out[s].y > tiles) { c->err = "record index store: a section's length is out of its bounds"; return -MLZ_ERR_HIP; }
        dir[size_t(s)] = n;
        h_off[s] = at + 8;
        desc[size_t(s)] = mlz_block_desc{at + 8, n, 0, 0};
        at += 8 + uint64_t(n);
        dense += h_out[s].y;
    }
    const uint64_t total = at + mlz::kRstoreEof;
    if (info) { info[0] = total; info[1] = ns; info[2] = nt - dense; info[3] = dense; }
    if (total > cap) return -MLZ_ERR_DST_TOO_SMALL;
    h.nsections = uint32_t(ns);
    mlz::rstore_put_head(h_up + 8 * ns, h, dir.data());
    HIPCHK(c, hipMemcpyAsync(r_up.at(ws), h_up, size_t(8 * ns) + head_n, hipMemcpyHostToDevice, sm));
    const uint64_t* d_off = reinterpret_cast<const uint64_t*>(r_up.at(ws));
    if (ns) {
        if (rstore_aligned(d_dst)) hipLaunchKernelGGL(mlz::rstore_pack_kernel<true>, dim3(uint32_t(nt)), dim3(mlz::kRstoreThreads), 0, sm, D, r_first.at(ws), r_toff.at(ws), d_off, nt, d_dst);
        else hipLaunchKernelGGL(mlz::rstore_pack_kernel<false>, dim3(uint32_t(nt)), dim3(mlz::kRstoreThreads), 0, sm, D, r_first.at(ws), r_toff.at(ws), d_off, nt, d_dst);
        if ((e = crc_device_locked(c, sm, d_dst, desc.data(), int(ns), r_crc.at(ws)))) return e;
    }
    const uint32_t items = std::max<uint32_t>(head_n, uint32_t(ns));
    hipLaunchKernelGGL(mlz::rstore_place_kernel, dim3((items + mlz::kRstoreThreads - 1) / mlz::kRstoreThreads), dim3(mlz::kRstoreThreads), 0, sm, r_up.at(ws) + 8 * ns, head_n, d_off,
                       r_out.at(ws), r_crc.at(ws), uint32_t(ns), at, d_dst);
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    return int64_t(total);
}

int64_t dev_reader_load_record_index_locked(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const uint8_t* d_blob, uint64_t len) {
    mlz_ctx* c = rd->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t size = uint64_t(rd->size), nt = mlz::rstore_ntiles(size), ns = mlz::rstore_nsections(size);
    const uint64_t head_n = mlz::kRstoreDirAt + 4 * ns, have = std::min<uint64_t>(len, head_n);
    Carve cv, pin;   // workspace: the verdict | the sections | CRCs; pinned: the header chunk | the sections | the verdict
    const auto r_verdict = cv.take<mlz::RstoreVerdict>(1);
    const auto r_secs = cv.take<mlz::RstoreSection>(size_t(ns));
    const auto r_crc = cv.take<uint32_t>(size_t(ns));
    const auto h_head_r = pin.take<uint8_t>(size_t(head_n), 64);
    const auto h_secs_r = pin.take<mlz::RstoreSection>(size_t(ns));
    const auto h_verdict_r = pin.take<mlz::RstoreVerdict>(1);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    int e = ensure_stream_objects(c, 0, pin.bytes);
    if (e) return e;
    void* ws = c->d_rplan.p;
    uint8_t* h_head = h_head_r.at(c->pinned2);
    mlz::RstoreSection* h_secs = h_secs_r.at(c->pinned2);
    mlz::RstoreVerdict* h_verdict = h_verdict_r.at(c->pinned2);
    { WorkspaceOrder order(c, sm); }
    if (have && (e = fetch(c, sm, h_head, d_blob, size_t(have)))) return e;
    mlz::RstoreHeader h{};
    const mlz_block_desc none{};
    if ((e = mlz::rstore_parse_fixed(h_head, size_t(have), &h))) return -e;
    if (h.size != size) return -MLZ_ERR_ARG;
    if ((e = mlz::rstore_parse_directory(h_head, size_t(have), len, h, ignore_crc, h_secs))) return -e;
    const mlz::RstoreTag tg = rstore_tag_of(rd);
    if ((e = mlz::rstore_match(h, size, tg.tag(), tg.chunks))) return -e;
    const uint64_t k = h.k;
    RindexTable tab;
    if (k) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&tab.p), size_t(k) * sizeof(uint64_t)));
        tab.cap = k;
    }
    HIPCHK(c, hipMemsetAsync(r_verdict.at(ws), 0, sizeof(mlz::RstoreVerdict), sm));
    if (ns) HIPCHK(c, hipMemcpyAsync(r_secs.at(ws), h_secs, size_t(ns) * sizeof(mlz::RstoreSection), hipMemcpyHostToDevice, sm));
    if (ns && !ignore_crc) {
        std::vector<mlz_block_desc> desc(size_t(ns), none);
        for (uint64_t s = 0; s < ns; s++) desc[size_t(s)] = mlz_block_desc{h_secs[s].off, h_secs[s].len, 0, 0};
        if ((e = crc_device_locked(c, sm, d_blob, desc.data(), int(ns), r_crc.at(ws)))) return e;
    }
    hipLaunchKernelGGL(mlz::rstore_frames_kernel, dim3(uint32_t((std::max<uint64_t>(ns, 1) + mlz::kRstoreThreads - 1) / mlz::kRstoreThreads)), dim3(mlz::kRstoreThreads), 0, sm, d_blob,
                       r_secs.at(ws), ignore_crc ? nullptr : r_crc.at(ws), uint32_t(ns), len - mlz::kRstoreEof, r_verdict.at(ws));
    if (ns) {
        if (rstore_aligned(d_blob)) hipLaunchKernelGGL(mlz::rstore_expand_kernel<true>, dim3(uint32_t(nt)), dim3(mlz::kRstoreThreads), 0, sm, d_blob, r_secs.at(ws), nt, ns, size, k, tab.p, r_verdict.at(ws));
        else hipLaunchKernelGGL(mlz::rstore_expand_kernel<false>, dim3(uint32_t(nt)), dim3(mlz::kRstoreThreads), 0, sm, d_blob, r_secs.at(ws), nt, ns, size, k, tab.p, r_verdict.at(ws));
    }
    if ((e = fetch(c, sm, h_verdict, r_verdict.at(ws), sizeof(mlz::RstoreVerdict)))) return e;
    if (h_verdict->crc_bad) return -MLZ_ERR_CRC;
    if (h_verdict->bad) return -MLZ_ERR_CORRUPT;
    if (h.N != mlz::rindex_records(k, size, h_verdict->last_is_delim != 0)) return -MLZ_ERR_CORRUPT;
    // every check has passed: the table is the handle's
    if (rd->d_index) (void)hipFree(rd->d_index);
    rd->d_index = tab.p; rd->index_cap = tab.cap;
    tab.p = nullptr;
    rd->index_ready = true; rd->index_delim = h.delim; rd->index_k = k; rd->index_n = h.N;
    rd->index_longest_ready = (h.flags & mlz::kRstoreLongest) != 0;
    rd->index_longest = rd->index_longest_ready ? h.longest : 0;
    rd->tabled.cross_ready[1] = false;   // (the joined flags of a set that keeps its tables belong to the index)
    return int64_t(rd->index_n);
}

// The index of d_raw[0, n) for `delim` into the context's workspace (c->d_range, 8 bytes per delimiter): *k delimiters, *last_is_delim
int64_t rstore_index_raw_locked(mlz_ctx* c, hipStream_t sm, const uint8_t* d_raw, uint64_t n, uint8_t delim, uint64_t* k, bool* last_is_delim) {
    HIPCHK(c, hipSetDevice(c->device));
    *k = 0; *last_is_delim = false;
    if (n == 0) return 0;
    const uint64_t ntiles = mlz::rindex_tiles(reinterpret_cast<uintptr_t>(d_raw) & 15, n);
    Carve cv;   // workspace: the total | tile counts | tile bases
    const auto r_total = cv.take<uint64_t>(2);
    const auto r_count = cv.take<uint32_t>(size_t(ntiles)), r_base = cv.take<uint32_t>(size_t(ntiles));
    HIPCHK(c, c->d_records.ensure(cv.bytes));
    int e = ensure_stream_objects(c, 0, 64);
    if (e) return e;
    void* ws = c->d_records.p;
    uint64_t* h_total = static_cast<uint64_t*>(c->pinned2);
    { WorkspaceOrder order(c, sm); }
    hipLaunchKernelGGL(mlz::rindex_count_kernel, dim3(uint32_t(ntiles)), dim3(mlz::kRindexThreads), 0, sm, d_raw, n, delim, r_count.at(ws));
    hipLaunchKernelGGL(mlz::rindex_scan_kernel, dim3(1), dim3(mlz::kRecordsScanThreads), 0, sm, r_count.at(ws), ntiles, r_base.at(ws), r_total.at(ws));
    if ((e = fetch(c, sm, h_total, r_total.at(ws), sizeof(uint64_t)))) return e;
    const uint64_t total = h_total[0];
    if (total > n) { c->err = "mlz_record_index_build_device: more delimiters than bytes"; return -MLZ_ERR_HIP; }
    if (total == 0) return 0;
    HIPCHK(c, c->d_range.ensure(size_t(total) * sizeof(uint64_t)));
    uint64_t* D = c->d_range.as<uint64_t>();
    hipLaunchKernelGGL(mlz::rindex_emit_kernel, dim3(uint32_t(ntiles)), dim3(mlz::kRindexThreads), 0, sm, d_raw, n, delim, r_base.at(ws), uint64_t(0), total, D);
    if ((e = fetch(c, sm, h_total, D + (total - 1), sizeof(uint64_t)))) return e;
    if (h_total[0] >= n) { c->err = "mlz_record_index_build_device: a delimiter beyond the bytes"; return -MLZ_ERR_HIP; }
    *k = total; *last_is_delim = h_total[0] == n - 1;
    return 0;
}

}  // namespace

extern "C" {

int64_t mlz_dev_reader_record_index_bound(const mlz_dev_reader* rd) {
    if (!rd) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    return rd->index_ready ? int64_t(mlz::rstore_bound(uint64_t(rd->size), rd->index_k)) : -MLZ_ERR_ARG;
}

int64_t mlz_dev_reader_save_record_index(mlz_dev_reader* rd, void* stream, uint8_t* d_dst, size_t dst_cap, uint64_t* info) {
    if (!rd || !d_dst) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!rd->index_ready) return -MLZ_ERR_ARG;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_dst)) return -MLZ_ERR_ARG;
    const mlz::RstoreTag tg = rstore_tag_of(rd);
    mlz::RstoreHeader h{};
    h.flags = mlz::kRstoreBound | (rd->index_longest_ready ? mlz::kRstoreLongest : 0u);
    h.delim = rd->index_delim; h.size = uint64_t(rd->size); h.k = rd->index_k; h.N = rd->index_n;
    h.longest = rd->index_longest_ready ? rd->index_longest : ~uint64_t(0);
    h.tag = tg.tag(); h.data_chunks = tg.chunks;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, rstore_save_locked(c, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, uint64_t(rd->size), h, d_dst, uint64_t(dst_cap), info));
}

int64_t mlz_dev_reader_load_record_index(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* d_blob, size_t len, uint64_t* info) {
    if (!rd || !d_blob || len == 0 || (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC))) return -MLZ_ERR_ARG;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_blob)) return -MLZ_ERR_ARG;
    c->range_chunks = c->range_scratch = 0;   // (nothing is decoded)
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const int64_t r = settled(sm, dev_reader_load_record_index_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, d_blob, uint64_t(len)));
    if (r < 0) return r;   // (the handle keeps what it had)
    if (info) { info[0] = rd->index_n; info[1] = rd->index_k; info[2] = rd->index_cap * sizeof(uint64_t); info[3] = 0; }
    return r;
}

int64_t mlz_record_index_bound(uint64_t raw_len) {
    if (raw_len > mlz::kRstoreMaxBuild) return -MLZ_ERR_TOO_LARGE;
    return int64_t(mlz::rstore_bound(raw_len, raw_len));
}

int64_t mlz_record_index_build_device(mlz_ctx* ctx, void* stream, const uint8_t* d_raw, size_t raw_len, uint8_t delimiter, uint8_t* d_dst, size_t dst_cap, uint64_t* info) {
    if (!ctx || !d_dst || (!d_raw && raw_len)) return -MLZ_ERR_ARG;
    if (uint64_t(raw_len) > mlz::kRstoreMaxBuild) return -MLZ_ERR_TOO_LARGE;
    mlz_ctx* c = owner_of(ctx, d_dst);
    if (!c) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_dst) || (raw_len && !on_device(c, d_raw))) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    uint64_t k = 0;
    bool last_is_delim = false;
    int64_t r = rstore_index_raw_locked(c, sm, d_raw, uint64_t(raw_len), delimiter, &k, &last_is_delim);
    if (r < 0) return settled(sm, r);
    mlz::RstoreHeader h{};
    h.delim = delimiter; h.size = uint64_t(raw_len); h.k = k; h.N = mlz::rindex_records(k, uint64_t(raw_len), last_is_delim);
    h.longest = ~uint64_t(0);
    return settled(sm, rstore_save_locked(c, sm, c->d_range.as<uint64_t>(), k, uint64_t(raw_len), h, d_dst, uint64_t(dst_cap), info));
}

int64_t mlz_record_index_parse(const uint8_t* blob, size_t len, uint64_t* info) {
    if (!blob || !info) return -MLZ_ERR_ARG;
    mlz::RstoreHeader h{};
    int e = mlz::rstore_parse_fixed(blob, len, &h);
    if (e == 0) e = mlz::rstore_parse_directory(blob, len, len, h, false, nullptr);
    if (e) return -e;
    info[0] = h.flags; info[1] = h.delim; info[2] = h.size; info[3] = h.k; info[4] = h.N; info[5] = h.longest; info[6] = h.tag; info[7] = h.data_chunks;
    return int64_t(h.nsections);
}

}  // extern "C"
