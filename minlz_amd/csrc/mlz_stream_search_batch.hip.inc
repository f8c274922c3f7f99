// mlz_stream_search_batch.hip.inc — mlz_stream_search_batch_device: which streams of a batch in HBM hold which of up to 4096 byte strings, and
// where (included behind mlz_stream_batch.hip.inc, whose walk and argument checks it uses, and mlz_stream_search_many.hip.inc, whose pattern
// index, decode helpers and scan kernel it runs).
//
// The batch is laid out as ONE decoded sequence with a one-byte hole behind every stream (mlz_stream_search_batch.h: the virtual positions),
// so search_layout, the scratch decode and search_many_kernel run as they do for one stream: the chunks of all healthy streams form one job
// list in descriptor order, decoded group by group into the scratch; per group SearchManyScan::count_prefix_write counts, continues the running
// prefix over ALL tiles and writes (virtual position, pattern) below cap, and SearchManyScan::mark_streams sets the presence bits.  The scan is
// prepared once for the call and takes its regions anew in every pass.  search_batch_finish_kernel then gives every stream its count (the prefix at its tiles' ends) and turns every written
// virtual position into (stream, position).  A stream whose decode or CRC fails is known only when the job results come back, with its garbage
// scanned: it is then dropped from the list and the whole scan runs once more over the rest (failures are deterministic: two passes at the most).

#include "mlz_stream_search_batch.h"

namespace mlz {

// After the last group.  A lane per stream: counts[i] (and stream_counts[i], when given) = the pairs of stream i's tiles.  A lane per written
// triple: hit_stream[k] = the stream of the virtual position hit_pos[k], which becomes the position inside that stream.  vbase: n + 1 values.
__global__ __launch_bounds__(256) void search_batch_finish_kernel(const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ total, uint32_t nt,
                                                                  const uint32_t* __restrict__ tile_first, const uint64_t* __restrict__ vbase, uint32_t n,
                                                                  uint64_t* __restrict__ counts, uint64_t* __restrict__ stream_counts, uint64_t cap,
                                                                  uint32_t* __restrict__ hit_stream, uint64_t* __restrict__ hit_pos) {
    const uint64_t all = *total, written = all < cap ? all : cap, step = uint64_t(gridDim.x) * 256;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += step) {
        const uint64_t v = batch_stream_count([&](size_t t) { return prefix[t]; }, nt, all, tile_first, size_t(i));
        counts[i] = v;
        if (stream_counts) stream_counts[i] = v;
    }
    for (uint64_t k = uint64_t(blockIdx.x) * 256 + threadIdx.x; k < written; k += step) {
        const uint64_t v = hit_pos[k];
        const size_t s = batch_stream_of(vbase, n, v);
        hit_stream[k] = uint32_t(s);
        hit_pos[k] = v - vbase[s];
    }
}

}  // namespace mlz

namespace {

struct SearchBatchOut {
    uint64_t *d_stream_counts, *d_pattern_counts;
    uint32_t* d_present;
    uint32_t* d_hit_stream;
    uint64_t* d_hit_pos;
    uint32_t* d_hit_which;
    uint64_t cap;
};

// One pass: the streams with alive[i] are decoded and scanned.  rc[i] = 0 or the stream's first failing chunk's error; *total and counts[i]
// are valid (and the device outputs written) when no stream failed.  *n_jobs: the chunks the pass decoded.  take (may be NULL: every chunk
// that has bytes): a byte per chunk of the walk, the plan of the pruned call (mlz_stream_search_batch_prune.hip.inc).
int64_t stream_search_batch_pass(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const BatchWalk& bw, size_t n, const std::vector<uint8_t>& alive, const uint8_t* take,
                                 SearchManyScan& scan, const SearchBatchOut& out, std::vector<int64_t>* rc, std::vector<uint64_t>* counts, uint64_t* total, size_t* n_jobs,
                                 bool* failed) {
    // the virtual positions and the one job list: every alive stream's chunks that have bytes, in descriptor order
    std::vector<uint64_t> size(n, 0), vbase(n + 1, 0);
    for (size_t i = 0; i < n; i++) if (alive[i]) size[i] = bw.prefix(i);
    mlz::batch_vbases(size.data(), n, vbase.data());
    SearchDecode sd;
    std::vector<ChunkJob>& jobs = sd.dec.jobs;
    std::vector<size_t> job_first(n + 1, 0);
    std::vector<uint64_t> voff;
    for (size_t i = 0; i < n; i++) {
        job_first[i] = jobs.size();
        for (size_t k = bw.c0[i]; alive[i] && k < bw.c1[i]; k++)
            if (bw.chunks[k].n && (!take || take[k])) { jobs.push_back(ChunkJob{k, nullptr}); voff.push_back(vbase[i] + bw.chunks[k].out_off); }
    }
    job_first[n] = jobs.size();
    *n_jobs = jobs.size();
    search_decode_layout(bw.chunks, [&](size_t j) { return voff[j]; }, scan.index.lmin, scan.index.lmax, mlz::kSearchManyTile, &sd);
    const size_t nt = sd.lay.tiles.size();
    if (nt > 0x7fffffffu) return -MLZ_ERR_ARG;
    std::vector<uint32_t> tile_stream(nt), tile_first(n + 1);
    if (!mlz::batch_tile_streams(sd.lay.tiles.data(), nt, vbase.data(), n, tile_stream.data(), tile_first.data())) {
        c->err = "stream_search_batch: a tile crosses a stream";
        return -MLZ_ERR_HIP;
    }
    const size_t words = (scan.n + 31) / 32;
    Carve cv, pin;   // workspace: the scan's (pattern counts | total | the index | tile counts | prefix) | tile streams | tile firsts | vbase | stream counts | the decode's
    scan.take(&cv, &pin, &nt);
    // (tile streams | tile firsts | vbase go up as one block; stream counts | total come back as one)
    Carve blk;
    const auto u_ts = blk.take<uint32_t>(nt, 4), u_tf = blk.take<uint32_t>(n + 1, 4);
    const auto u_vb = blk.take<uint64_t>(n + 1, 8);
    const auto r_blk = cv.take<uint8_t>(blk.bytes), h_blk = pin.take<uint8_t>(blk.bytes);
    const auto r_sc = cv.take<uint64_t>(n + 1);
    const auto h_sc = pin.take<uint64_t>(n + 1);
    int e = search_decode_ready(c, bw.chunks, &sd, &cv, &pin);
    if (e) return e;
    void* ws = c->d_rplan.p;
    uint64_t* d_sc = r_sc.at(ws);
    uint8_t *d_blk = r_blk.at(ws), *hb = h_blk.at(c->pinned2);
    const uint32_t *d_ts = u_ts.at(d_blk), *d_tf = u_tf.at(d_blk);
    const uint64_t* d_vb = u_vb.at(d_blk);
    const uint64_t *d_prefix = scan.prefixes.at(ws), *d_total = scan.total.at(ws);
    if (nt) std::memcpy(u_ts.at(hb), tile_stream.data(), nt * 4);
    std::memcpy(u_tf.at(hb), tile_first.data(), (n + 1) * 4);
    std::memcpy(u_vb.at(hb), vbase.data(), (n + 1) * 8);
    { WorkspaceOrder order(c, sm); }
    if ((e = scan.clear(c, sm))) return e;
    if (out.d_present) HIPCHK(c, hipMemsetAsync(out.d_present, 0, n * words * 4, sm));
    HIPCHK(c, hipMemcpyAsync(d_blk, hb, blk.bytes, hipMemcpyHostToDevice, sm));
    if ((e = scan.send(c, sm, sd.tiles.at(ws)))) return e;
    std::vector<int64_t> job_rc;
    const int64_t r = search_decode_run(c, d_src, bw.chunks, sm, ignore_crc, &sd, [&](size_t, size_t t0, size_t t1) {
        scan.count_prefix_write(t0, t1, out.cap, out.d_hit_pos, out.d_hit_which);
        if (out.d_present) scan.mark_streams(t0, t1, d_ts, out.d_present, uint32_t(words));
        return 0;
    }, &job_rc);
    if (r < 0) return r;
    std::vector<int64_t> zero(n, 0);
    rc->assign(n, 0);
    mlz::batch_stream_verdicts(zero.data(), job_first.data(), job_rc.data(), n, rc->data());
    *failed = false;
    for (size_t i = 0; i < n; i++) *failed = *failed || (*rc)[i] < 0;
    if (*failed) {   // what this pass wrote is void; the caller clears the triples it may have written: it needs the pass's total for that
        if (nt == 0) { *total = 0; return 0; }
        if ((e = fetch(c, sm, c->pinned2, d_total, 8))) return e;
        *total = *static_cast<const uint64_t*>(c->pinned2);
        return 0;
    }
    const uint64_t lanes = std::max<uint64_t>(n, out.cap);
    hipLaunchKernelGGL(mlz::search_batch_finish_kernel, dim3(uint32_t(std::min<uint64_t>((lanes + 255) / 256, 4096))), dim3(256), 0, sm, d_prefix, d_total, uint32_t(nt), d_tf, d_vb,
                       uint32_t(n), d_sc, out.d_stream_counts, out.cap, out.d_hit_stream, out.d_hit_pos);
    if (out.d_pattern_counts) HIPCHK(c, hipMemcpyAsync(out.d_pattern_counts, scan.pat_counts.at(ws), scan.n * 8, hipMemcpyDeviceToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(d_sc + n, d_total, 8, hipMemcpyDeviceToDevice, sm));
    uint64_t* h = h_sc.at(c->pinned2);
    if ((e = fetch(c, sm, h, d_sc, (n + 1) * 8))) return e;
    counts->assign(h, h + n);
    *total = h[n];
    return 0;
}

// The passes of both calls behind the walk: the first over every stream without a framing error, a second over the rest when a stream's
// decode failed.  out_count[i] and the device outputs as the contract says; four[0 .. 3] = the call's first four stats.  take: the pass's.
int64_t stream_search_batch_passes(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const BatchWalk& bw, size_t n, const uint8_t* take, SearchManyScan& scan,
                                   int64_t* out_count, const SearchBatchOut& out, uint64_t* four) {
    // a stream with a framing error keeps the walk's code, and nothing of it is searched
    std::vector<uint8_t> alive(n);
    std::vector<int64_t> verdict(n, 0), rc;
    for (size_t i = 0; i < n; i++) { alive[i] = bw.parsed[i] >= 0; if (!alive[i]) verdict[i] = bw.parsed[i]; }
    std::vector<uint64_t> counts(n, 0);
    uint64_t total = 0, decoded = 0, bad = 0, passes = 0;
    for (;;) {
        size_t n_jobs = 0;
        bool failed = false;
        const int64_t e = stream_search_batch_pass(c, sm, ignore_crc, d_src, bw, n, alive, take, scan, out, &rc, &counts, &total, &n_jobs, &failed);
        if (e < 0) return e;
        decoded += n_jobs;
        passes += n_jobs ? 1 : 0;
        if (!failed) break;
        if (passes > 1) { c->err = "stream_search_batch: a stream failed in the second pass only"; return -MLZ_ERR_HIP; }
        for (size_t i = 0; i < n; i++) if (rc[i] < 0) { alive[i] = 0; verdict[i] = rc[i]; bad++; }
        // the triples the void pass wrote: cleared (never anything at cap or beyond)
        const uint64_t wrote = std::min<uint64_t>(total, out.cap);
        if (wrote) {
            HIPCHK(c, hipMemsetAsync(out.d_hit_pos, 0, wrote * 8, sm));
            HIPCHK(c, hipMemsetAsync(out.d_hit_which, 0, wrote * 4, sm));
        }
    }
    for (size_t i = 0; i < n; i++) out_count[i] = verdict[i] < 0 ? verdict[i] : int64_t(counts[i]);
    c->search_chunks = decoded;
    four[0] = bw.chunks.size(); four[1] = decoded; four[2] = bad; four[3] = passes;
    return int64_t(total);
}

// mlz_stream_search_batch_device behind its argument checks.  Returns the number of all triples or -MLZ_ERR_*; the streams' results go to out_count.
int64_t stream_search_batch_locked(mlz_ctx* c, hipStream_t sm, uint32_t flags, const uint8_t* d_src, const mlz_block_desc* streams, size_t n, const uint8_t* patterns,
                                   const uint32_t* pattern_len, size_t np, int64_t* out_count, const SearchBatchOut& out, uint64_t* stats) {
    BatchWalk bw;
    int r = stream_batch_walk(c, sm, d_src, streams, n, &bw);
    if (r) return r;
    begin_decode_call(c);
    c->search_chunks = c->search_tables = c->search_compressed = 0;
    SearchManyScan scan;
    scan.prepare(flags, patterns, pattern_len, np);
    uint64_t four[4];
    const int64_t total = stream_search_batch_passes(c, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, d_src, bw, n, nullptr, scan, out_count, out, four);
    if (total >= 0 && stats) for (int i = 0; i < 4; i++) stats[i] = four[i];
    return total;
}

// The argument checks of both calls.  Returns 0 with *run = the context that serves the call and its lock still to be taken, 1 (n_streams == 0) or -MLZ_ERR_ARG.
int search_batch_args(mlz_ctx* c, uint32_t flags, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, const uint8_t* patterns, const uint32_t* pattern_len,
                      size_t n_patterns, const int64_t* out_count, const uint32_t* d_hit_stream, const uint64_t* d_hit_pos, const uint32_t* d_hit_which, size_t cap, mlz_ctx** run) {
    if (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC | MLZ_SEARCH_IGNORE_CASE | MLZ_SEARCH_NO_TABLES)) return -MLZ_ERR_ARG;
    if (n_patterns == 0 || search_pattern_list(patterns, pattern_len, n_patterns) < 0 || (cap && (!d_hit_stream || !d_hit_pos || !d_hit_which))) return -MLZ_ERR_ARG;
    return batch_args(c, d_src, nullptr, false, streams, n_streams, out_count, run);
}

// ... and those of the device outputs, under the context's lock
bool search_batch_outputs_on_device(mlz_ctx* c, const SearchBatchOut& out) {
    for (const void* p : {static_cast<const void*>(out.d_stream_counts), static_cast<const void*>(out.d_pattern_counts), static_cast<const void*>(out.d_present)})
        if (p && !on_device(c, p)) return false;
    return !out.cap || (on_device(c, out.d_hit_stream) && on_device(c, out.d_hit_pos) && on_device(c, out.d_hit_which));
}

}  // namespace

extern "C" int64_t mlz_stream_search_batch_device(mlz_ctx* c, void* stream, uint32_t flags, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams,
                                                  const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns, int64_t* out_count, uint64_t* d_stream_counts,
                                                  uint64_t* d_pattern_counts, uint32_t* d_present, uint32_t* d_hit_stream, uint64_t* d_hit_pos, uint32_t* d_hit_which, size_t cap,
                                                  uint64_t* stats) {
    const int a = search_batch_args(c, flags, d_src, streams, n_streams, patterns, pattern_len, n_patterns, out_count, d_hit_stream, d_hit_pos, d_hit_which, cap, &c);
    if (a) {
        if (a > 0 && stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
        return a < 0 ? a : 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    const SearchBatchOut out{d_stream_counts, d_pattern_counts, d_present, d_hit_stream, d_hit_pos, d_hit_which, uint64_t(cap)};
    if (!search_batch_outputs_on_device(c, out)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, stream_search_batch_locked(c, sm, flags, d_src, streams, size_t(n_streams), patterns, pattern_len, n_patterns, out_count, out, stats));
}
