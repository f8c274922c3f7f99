// mlz_stream_sidecar_extract.hip.inc — a stream's inline search tables moved into a sidecar, and the stream written again without them, in
// HBM (included from mlz_hip.hip behind mlz_stream_sidecar.hip.inc; the C ABI is include/minlz_hip_sidecar_extract.h).
//
// The reference's ExtractSidecar (sidecar.go:546-771) for one stream: the 0x44 / 0x45 / 0x46 chunks are copied as they are, nothing is
// decoded.  The handle's chunk table holds the data chunks only, so the work is on the GAPS between them (mlz_stream_sidecar_extract.h):
//   extract_gap_kernel    a lane per gap steps through its headers and sums what goes where: 64 bytes per gap visit the host
//   the layout            on the host (extract_layout): the stripped main's offsets, then the references' lengths, then the sidecar's
//                         offsets; 48 bytes per gap go up (16 in front of the gap pass, 32 behind it), and the foot of the stripped main
//                         (its EOF chunk and the fresh seek index, SeekIndex as the Writer's) with them.  No chunk body visits the host.
//   extract_emit_kernel   a lane per gap walks it again and writes the descriptors of its chunks' pieces and of the data chunk behind it,
//                         that chunk's 0x47 and, at the EOF chunk, the sidecar's EOF and the foot's descriptors; block 0: the identifiers
//   extract_copy_kernel   a workgroup per long piece (wg_copy), 16 lanes per short piece (lanes16_copy), as stream_range_copy_kernel
// The copies: both helpers store destination-aligned 16-byte vectors; the 16 source bytes of a vector are loaded from where they lie, so
// where source and destination differ modulo 16 (almost every chunk) the stores are vector-wide and aligned and the loads are 16-byte loads
// at an unaligned address.

namespace mlz {

__global__ __launch_bounds__(64) void extract_gap_kernel(const uint8_t* __restrict__ src, const ExtractSpan* __restrict__ span, uint32_t n_gaps, ExtractGap* __restrict__ out) {
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g < n_gaps) out[g] = extract_gap_scan(src, span[g].begin, span[g].end);
}

struct ExtractEmitArgs {
    const uint8_t* src;
    const ExtractSpan* span;
    const ExtractBase* base;
    uint8_t *side, *main;      // main = nullptr: mode a
    PlaceDesc* descs;
    uint64_t foot_n;
    uint32_t n_gaps, n_long;
    uint8_t ident[10];
};

__global__ __launch_bounds__(64) void extract_emit_kernel(const ExtractEmitArgs a) {
    if (blockIdx.x == 0 && threadIdx.x < 10) {
        a.side[threadIdx.x] = a.ident[threadIdx.x];
        if (a.main) a.main[threadIdx.x] = a.ident[threadIdx.x];
    }
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= a.n_gaps) return;
    const bool last = g + 1 == a.n_gaps;
    extract_emit_gap(a.src, a.span[g], last ? 0 : a.span[g + 1].begin, last, a.base[g], a.main != nullptr, a.foot_n, a.side, a.descs, a.n_long);
}

// descs[0, n_long): a workgroup per piece; descs[n_long, n_all): 16 lanes per piece.  desc.pad: kExtractToMain, kExtractFromFoot
__global__ __launch_bounds__(256) void extract_copy_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ foot, uint8_t* __restrict__ side, uint8_t* __restrict__ main,
                                                           const PlaceDesc* __restrict__ descs, uint32_t n_long, uint32_t n_all) {
    if (blockIdx.x < n_long) {
        const PlaceDesc d = descs[blockIdx.x];
        wg_copy(((d.pad & kExtractToMain) ? main : side) + d.dst_off, ((d.pad & kExtractFromFoot) ? foot : src) + d.src_off, d.len, threadIdx.x, 256);
        return;
    }
    const uint32_t idx = n_long + (blockIdx.x - n_long) * kRangeShortPerWg + (threadIdx.x >> 4);
    if (idx >= n_all) return;
    const PlaceDesc d = descs[idx];
    lanes16_copy(((d.pad & kExtractToMain) ? main : side) + d.dst_off, ((d.pad & kExtractFromFoot) ? foot : src) + d.src_off, d.len, threadIdx.x & 15);
}

}  // namespace mlz

namespace {

static_assert(mlz::kExtractShortMax == mlz::kRangeShortMax || mlz::kRangeShortMax == 0, "short pieces as the range copy's");

constexpr size_t kExtractEofBound = 4 + 10;
size_t extract_foot_bound(size_t n_chunks) { return kExtractEofBound + SeekIndex::bound(n_chunks); }

uint64_t extract_chunk_end(const StreamChunk& ck) { return uint64_t(ck.body_off) + ck.body_len; }

// The handles the call serves: 0, or the error both entry points return
int extract_refusal(const mlz_dev_reader* rd) {
    if (rd->set || rd->n_ident > 1) return -MLZ_ERR_UNSUPPORTED;   // a set of streams, concatenated streams: the line mlz_dev_reader_attach_sidecar draws
    if (rd->n_ident == 0) return -MLZ_ERR_CORRUPT;                 // (an empty stream: no identifier to repeat)
    return 0;
}

int64_t dev_reader_extract_sidecar_locked(mlz_dev_reader* rd, hipStream_t sm, uint8_t* d_side, uint64_t side_cap, uint8_t* d_main, uint64_t main_cap, mlz_sidecar_extract_result* out) {
    mlz_ctx* c = rd->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nck = rd->chunks.size(), ng = nck + 1;
    const bool strip = d_main != nullptr;
    const uint64_t max_block = sidecar_max_block(rd);
    const size_t foot_cap = extract_foot_bound(nck);
    Carve cv, pin;   // workspace: spans | bases | foot | gaps; pinned: the same (bases | foot go up as one block)
    const auto r_span = cv.take<mlz::ExtractSpan>(ng);
    const auto r_base = cv.take<mlz::ExtractBase>(ng);
    const auto r_foot = cv.take<uint8_t>(foot_cap);
    const auto r_gap = cv.take<mlz::ExtractGap>(ng);
    const auto h_span_r = pin.take<mlz::ExtractSpan>(ng);
    const auto h_up_r = pin.take<uint8_t>(r_gap.off - r_base.off, 64);
    const auto h_gap_r = pin.take<mlz::ExtractGap>(ng);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    int e = ensure_stream_objects(c, 0, pin.bytes);
    if (e) return e;
    void* ws = c->d_rplan.p;
    mlz::ExtractSpan* h_span = h_span_r.at(c->pinned2);
    uint8_t* h_up = h_up_r.at(c->pinned2);
    mlz::ExtractBase* h_base = reinterpret_cast<mlz::ExtractBase*>(h_up);
    uint8_t* h_foot = h_up + (r_foot.off - r_base.off);
    mlz::ExtractGap* h_gap = h_gap_r.at(c->pinned2);
    for (size_t g = 0; g < ng; g++)
        h_span[g] = mlz::ExtractSpan{g ? extract_chunk_end(rd->chunks[g - 1]) : 0, g < nck ? uint64_t(rd->chunks[g].hdr_off) : uint64_t(rd->n)};
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(r_span.at(ws), h_span, ng * sizeof(mlz::ExtractSpan), hipMemcpyHostToDevice, sm));
    const uint32_t grid = uint32_t((ng + 63) / 64);
    hipLaunchKernelGGL(mlz::extract_gap_kernel, dim3(grid), dim3(64), 0, sm, rd->d_src, r_span.at(ws), uint32_t(ng), r_gap.at(ws));
    if ((e = fetch(c, sm, h_gap, r_gap.at(ws), ng * sizeof(mlz::ExtractGap)))) return e;

    const mlz::ExtractLayout L = mlz::extract_layout(
        nck, max_block, strip, [&](size_t g) -> const mlz::ExtractGap& { return h_gap[g]; }, [&](size_t k) { return uint64_t(rd->chunks[k].hdr_off); },
        [&](size_t k) { return extract_chunk_end(rd->chunks[k]) - rd->chunks[k].hdr_off; }, [&](size_t k) { return uint64_t(rd->chunks[k].n); },
        [&](const mlz::ExtractLayout& l) {   // the foot: emitEOFChunk(decoded size), then Index.add per data chunk and appendTo(decoded size, -1)
            SeekIndex idx;
            idx.reset(int64_t(max_block));
            for (size_t k = 0; k < nck; k++) idx.add(int64_t(l.new_hdr[k]), int64_t(rd->chunks[k].out_off));
            const size_t v = put_uvarint64(h_foot + 4, uint64_t(rd->size));
            h_foot[0] = 0x20; h_foot[1] = uint8_t(v); h_foot[2] = h_foot[3] = 0;
            return uint64_t(4 + v + idx.append_to(h_foot + 4 + v, rd->size, -1));
        });
    if (L.status != mlz::kExtractOk) return -int64_t(L.status);
    out->side_len = L.side_len; out->main_len = L.main_len;
    if (L.side_len > side_cap || L.main_len > main_cap) return -MLZ_ERR_DST_TOO_SMALL;   // (the sizes stay in *out)
    for (size_t g = 0; g < ng; g++) h_base[g] = L.base[g];
    const uint32_t n_all = L.n_long + L.n_short;
    HIPCHK(c, c->d_place.ensure(size_t(std::max<uint32_t>(n_all, 1)) * sizeof(mlz::PlaceDesc)));
    HIPCHK(c, hipMemcpyAsync(r_base.at(ws), h_up, (r_foot.off - r_base.off) + L.foot_n, hipMemcpyHostToDevice, sm));
    mlz::ExtractEmitArgs a{};
    a.src = rd->d_src; a.span = r_span.at(ws); a.base = r_base.at(ws); a.side = d_side; a.main = d_main; a.descs = c->d_place.as<mlz::PlaceDesc>();
    a.foot_n = L.foot_n; a.n_gaps = uint32_t(ng); a.n_long = L.n_long;
    std::memcpy(a.ident, kMagicChunk, 9);
    a.ident[9] = rd->ident_byte;
    hipLaunchKernelGGL(mlz::extract_emit_kernel, dim3(grid), dim3(64), 0, sm, a);
    if (n_all) {
        const uint32_t cgrid = L.n_long + (L.n_short + mlz::kRangeShortPerWg - 1) / mlz::kRangeShortPerWg;
        hipLaunchKernelGGL(mlz::extract_copy_kernel, dim3(cgrid), dim3(256), 0, sm, rd->d_src, r_foot.at(ws), d_side, d_main, a.descs, L.n_long, n_all);
    }
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    out->blocks = L.blocks; out->info_chunks = L.info; out->tables = L.tables; out->tables_compressed = L.tables46;
    out->passed_bytes = L.passed; out->dropped_bytes = L.dropped;
    return int64_t(L.side_len);
}

}  // namespace

extern "C" {

int64_t mlz_dev_reader_extract_sidecar_bound(const mlz_dev_reader* rd, uint64_t* main_bound) {
    if (main_bound) *main_bound = 0;
    if (!rd) return -MLZ_ERR_ARG;
    if (const int e = extract_refusal(rd)) return e;
    uint64_t data = 0;
    for (const StreamChunk& ck : rd->chunks) data += extract_chunk_end(ck) - ck.hdr_off;
    if (main_bound) *main_bound = uint64_t(rd->n) + extract_foot_bound(rd->chunks.size());
    return int64_t(10 + (uint64_t(rd->n) - data) + uint64_t(rd->chunks.size()) * mlz::kSidecarRefBound + 5);
}

int64_t mlz_dev_reader_extract_sidecar(mlz_dev_reader* rd, void* stream, uint32_t flags, uint8_t* d_side, size_t side_cap, uint8_t* d_main, size_t main_cap,
                                       mlz_sidecar_extract_result* out) {
    if (!rd || !d_side || !out || (d_main && !main_cap) || (!d_main && main_cap) || (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC))) return -MLZ_ERR_ARG;
    *out = mlz_sidecar_extract_result{};
    if (const int e = extract_refusal(rd)) return e;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_side) || (d_main && !on_device(c, d_main))) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_extract_sidecar_locked(rd, sm, d_side, uint64_t(side_cap), d_main, uint64_t(main_cap), out));
}

}  // extern "C"
