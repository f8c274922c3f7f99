// mlz_stream_grep.hip.inc — mlz_dev_reader_grep_records: grep over the record index of a .mz stream in HBM — many patterns, inverted match,
// context records, record numbers out (included at the end of mlz_hip.hip, behind the record index, whose table it reads, and the search for
// many patterns, whose plan, decode and walk it runs).  The rules are those of mlz_stream_grep.h, which the host check runs as plain loops.
//
//   mark      the search phase of mlz_dev_reader_search_many (SearchManyScan, dev_reader_search_plan, search_decode_plan / ready / run) with
//             SearchManyScan::mark_records on every group: one pass of search_many_kernel<kSearchManyMarkRecords>, a verified pair sets the
//             bit of its position's record in a bitmap of N bits in the workspace.  No count pass, no prefix, no position list.
//   select    grep_select_kernel (one workgroup, a slab of words per lane, as rindex_scan_kernel and records_number_kernel run): the
//             complement under MLZ_GREP_INVERT, the forward and the backward scan of the nearest selected record, a word's context bits from
//             the two, the popcounts' exclusive prefix; R and |S|.
//   compact   grep_compact_kernel, a lane per word: numbers and kinds of the ranks below rec_cap, and end - start of every record (two
//             loads of D) summed into the bytes written and the bytes of all R records: two 64-bit atomics per workgroup.
// 32 bytes come home, behind the decode's verdicts; the caller's arrays are written by the compact kernel alone, which runs behind them.
// No kernel waits for another workgroup.  The regex grep (mlz_stream_regex.hip.inc) shares grep_enter, GrepWork and grep_select_compact.

#include "mlz_stream_grep.h"

namespace mlz {

// One workgroup.  sel: the marked words in, S out; ctx: C; above: the backward scan's value per word; rank: the records of C in front of a word
__global__ __launch_bounds__(kGrepScanThreads) void grep_select_kernel(uint32_t* __restrict__ sel, uint32_t* __restrict__ ctx, uint32_t* __restrict__ above, uint32_t* __restrict__ rank,
                                                                       uint64_t W, uint64_t N, uint32_t invert, uint64_t before, uint64_t after, GrepTotals* __restrict__ tot) {
    __shared__ uint32_t lds[kGrepScanThreads];
    const uint32_t tid = threadIdx.x;
    auto most = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
    auto plus = [](uint32_t x, uint32_t y) { return x + y; };
    const GrepSlab sl = grep_slab(W, tid);
    uint32_t last = 0, first = 0, nsel = 0;
    for (uint64_t w = sl.b; w < sl.e; w++) {
        const uint32_t s = grep_select_word(sel[w], w, N, invert != 0);
        sel[w] = s;
        nsel += rindex_popcount(s);
        last = most(last, grep_last_key(s, w));
        first = most(first, grep_first_key(s, w, N));
    }
    uint32_t below = wg_scan<kGrepScanThreads>(last, lds, tid, most);                           // over the lanes in front
    uint32_t beyond = wg_scan<kGrepScanThreads>(first, lds, kGrepScanThreads - 1 - tid, most);  // the lanes in reverse: over those behind
    for (uint64_t w = sl.e; w > sl.b; w--) {
        above[w - 1] = beyond;
        beyond = most(beyond, grep_first_key(sel[w - 1], w - 1, N));
    }
    uint32_t cnt = 0, total = 0, selected = 0;
    for (uint64_t w = sl.b; w < sl.e; w++) {
        const uint32_t s = sel[w], cw = grep_context_word(s, w, below, above[w], before, after, N);
        ctx[w] = cw;
        cnt += rindex_popcount(cw);
        below = most(below, grep_last_key(s, w));
    }
    uint32_t run = wg_scan<kGrepScanThreads>(cnt, lds, tid, plus, &total);   // (at most N < 2^32)
    for (uint64_t w = sl.b; w < sl.e; w++) { rank[w] = run; run += rindex_popcount(ctx[w]); }
    wg_scan<kGrepScanThreads>(nsel, lds, tid, plus, &selected);
    if (tid == 0) { tot->records = total; tot->selected = selected; }
}

struct GrepBytes { uint64_t written, bytes; };

// A lane per word of C.  rec_no[rank], rec_kind[rank] (may be NULL) for the ranks below rec_cap; tot->written, tot->bytes += the records' lengths
__global__ __launch_bounds__(kGrepCompactThreads) void grep_compact_kernel(const uint32_t* __restrict__ ctx, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ rank, uint64_t W,
                                                                           const uint64_t* __restrict__ D, uint64_t k, uint64_t size, uint64_t rec_cap, uint64_t* __restrict__ rec_no,
                                                                           uint8_t* __restrict__ rec_kind, GrepTotals* __restrict__ tot) {
    __shared__ GrepBytes lds[kGrepCompactThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t w = uint64_t(blockIdx.x) * kGrepCompactThreads + tid;
    GrepBytes mine{0, 0}, sum{0, 0};
    if (w < W) {
        const uint32_t cw = ctx[w];
        if (cw)
            grep_emit_word(cw, sel[w], w, rank[w], rec_cap, [&](uint64_t r) { return rindex_span([&](uint64_t j) { return D[j]; }, k, size, r).len; },
                           [&](uint64_t at, uint64_t r, uint8_t kind) { rec_no[at] = r; if (rec_kind) rec_kind[at] = kind; }, &mine.written, &mine.bytes);
    }
    wg_scan<kGrepCompactThreads>(mine, lds, tid, [](GrepBytes x, GrepBytes y) { return GrepBytes{x.written + y.written, x.bytes + y.bytes}; }, &sum);
    if (tid == 0) {
        if (sum.written) atomicAdd(reinterpret_cast<unsigned long long*>(&tot->written), static_cast<unsigned long long>(sum.written));
        if (sum.bytes) atomicAdd(reinterpret_cast<unsigned long long*>(&tot->bytes), static_cast<unsigned long long>(sum.bytes));
    }
}

}  // namespace mlz

namespace {

struct GrepOut { uint64_t* d_rec_no; uint8_t* d_rec_kind; uint64_t rec_cap; };

// What both greps run under the context's lock, in front of their bodies: the index is there and small enough, the call's own checks pass
// (call_ok()), the device, the outputs lie on it, the decode call begun; *out = the outputs as the kernels take them.  Returns 0 or the call's error.
template <class Ok>
int grep_enter(mlz_dev_reader* rd, Ok call_ok, uint64_t* d_rec_no, uint8_t* d_rec_kind, size_t rec_cap, GrepOut* out) {
    mlz_ctx* c = rd->ctx;
    if (!rd->index_ready || rd->index_n >= mlz::kGrepMaxRecords || !call_ok()) return -MLZ_ERR_ARG;
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (rec_cap && (!on_device(c, d_rec_no) || (d_rec_kind && !on_device(c, d_rec_kind)))) return -MLZ_ERR_ARG;
    begin_decode_call(c);
    *out = GrepOut{rec_cap ? d_rec_no : nullptr, rec_cap ? d_rec_kind : nullptr, uint64_t(rec_cap)};
    return 0;
}

void grep_zero_totals(uint64_t* totals) { if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0; }

// A grep's regions of the workspace (c->d_rplan): the totals | the marked words, then S | C | the backward scan | ranks, W words each.
// take: from the caller's carve; clear, behind the caller's ensure: the regions as pointers, the totals and the marks zeroed.
struct GrepWork {
    mlz::GrepTotals* tot = nullptr;
    uint32_t *sel = nullptr, *ctx = nullptr, *above = nullptr, *rank = nullptr;
    void take(Carve* cv, uint64_t words) {
        W = size_t(words); r_tot = cv->take<mlz::GrepTotals>(1);
        for (Region<uint32_t>& r : r_words) r = cv->take<uint32_t>(W);
    }
    int clear(mlz_ctx* c, hipStream_t sm) {
        void* ws = c->d_rplan.p;
        tot = r_tot.at(ws); sel = r_words[0].at(ws); ctx = r_words[1].at(ws); above = r_words[2].at(ws); rank = r_words[3].at(ws);
        HIPCHK(c, hipMemsetAsync(tot, 0, sizeof(mlz::GrepTotals), sm));
        HIPCHK(c, hipMemsetAsync(sel, 0, W * 4, sm));
        return 0;
    }
private:
    size_t W = 0; Region<mlz::GrepTotals> r_tot{}; Region<uint32_t> r_words[4]{};
};

// What every grep runs behind its mark phase, whose bits are in w.sel: select and compact, the totals home and their check against the index.
// Returns R; `call` names the entry point in an error's text.
int64_t grep_select_compact(mlz_dev_reader* rd, hipStream_t sm, const char* call, bool invert, uint64_t before, uint64_t after, const GrepOut& out, const GrepWork& w, uint64_t* totals) {
    mlz_ctx* c = rd->ctx;
    const uint64_t N = rd->index_n, W = mlz::grep_words(N);
    const uint64_t* D = static_cast<const uint64_t*>(rd->d_index);
    hipLaunchKernelGGL(mlz::grep_select_kernel, dim3(1), dim3(mlz::kGrepScanThreads), 0, sm, w.sel, w.ctx, w.above, w.rank, W, N, invert ? 1u : 0u, mlz::grep_clamp(before, N),
                       mlz::grep_clamp(after, N), w.tot);
    hipLaunchKernelGGL(mlz::grep_compact_kernel, dim3(uint32_t((W + mlz::kGrepCompactThreads - 1) / mlz::kGrepCompactThreads)), dim3(mlz::kGrepCompactThreads), 0, sm,
                       static_cast<const uint32_t*>(w.ctx), static_cast<const uint32_t*>(w.sel), static_cast<const uint32_t*>(w.rank), W, D, rd->index_k, uint64_t(rd->size), out.rec_cap,
                       out.d_rec_no, out.d_rec_kind, w.tot);
    const int e = fetch(c, sm, c->pinned2, w.tot, sizeof(mlz::GrepTotals));
    if (e) return e;
    const mlz::GrepTotals t = *static_cast<const mlz::GrepTotals*>(c->pinned2);
    if (t.records > N || t.selected > t.records || t.written > t.bytes || t.bytes > uint64_t(rd->size)) {
        c->err = std::string(call) + ": the totals do not fit the index";
        return -MLZ_ERR_HIP;
    }
    if (totals) { totals[0] = t.records; totals[1] = t.selected; totals[2] = t.written; totals[3] = t.bytes; }
    return int64_t(t.records);
}

int64_t dev_reader_grep_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* patterns, const uint32_t* pattern_len, size_t n, uint64_t before, uint64_t after,
                               const GrepOut& out, uint64_t* totals, uint64_t* stats) {
    mlz_ctx* c = rd->ctx;
    const size_t nck = rd->chunks.size();
    search_begin(rd, stats);
    grep_zero_totals(totals);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t N = rd->index_n;
    if (N == 0) return 0;
    SearchManyScan scan;
    scan.prepare(flags, patterns, pattern_len, n);
    std::vector<uint8_t> take(nck, 0);
    size_t n_take = 0;
    if (n && nck) {
        const int64_t pr = dev_reader_search_plan(rd, sm, flags, scan.patterns, scan.index.off, n, &take, &n_take, stats, true, true);   // (record-bound)
        if (pr) return pr;
    }
    Carve cv, pin;   // workspace: the grep's (totals | marks, then S | C | the backward scan | ranks) | the index | the decode's; pinned: the index | the decode's
    GrepWork w;
    w.take(&cv, mlz::grep_words(N));
    SearchDecode sd;
    if (n_take) {
        search_decode_plan(rd->chunks, take, n_take, scan.index.lmin, scan.index.lmax, mlz::kSearchManyTile, &sd);
        if (sd.lay.tiles.size() > 0x7fffffffu) return -MLZ_ERR_ARG;
        scan.take(&cv, &pin, nullptr);   // (nothing is counted)
        const int e = search_decode_ready(rd->ctx, rd->chunks, &sd, &cv, &pin);
        if (e) return e;
    } else {
        HIPCHK(c, c->d_rplan.ensure(cv.bytes));
        const int e = ensure_stream_objects(c, 0, 64);
        if (e) return e;
    }
    { WorkspaceOrder order(c, sm); }
    int e = w.clear(c, sm);
    if (e) return e;
    if (n_take) {
        if ((e = scan.send(c, sm, sd.tiles.at(c->d_rplan.p)))) return e;
        const uint64_t* D = static_cast<const uint64_t*>(rd->d_index);
        const int64_t r = search_decode_run(rd->ctx, rd->d_src, rd->chunks, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, &sd, [&](size_t, size_t t0, size_t t1) {
            scan.mark_records(t0, t1, D, rd->index_k, w.sel);
            return 0;
        });
        if (r < 0) return r;   // (nothing has been written to the caller's arrays)
    }
    return grep_select_compact(rd, sm, "mlz_dev_reader_grep_records", (flags & MLZ_GREP_INVERT) != 0, before, after, out, w, totals);
}

}  // namespace

extern "C" int64_t mlz_dev_reader_grep_records(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns, uint64_t before,
                                               uint64_t after, uint64_t* d_rec_no, uint8_t* d_rec_kind, size_t rec_cap, uint64_t* totals, uint64_t* stats) {
    const int64_t blob = rd ? search_pattern_list(patterns, pattern_len, n_patterns) : -1;
    if (blob < 0 || (rec_cap && !d_rec_no)) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    // a line search cannot match across lines; records are split at the delimiter's own byte, which is never folded
    auto pattern_ok = [&] { return !(blob && std::memchr(patterns, rd->index_delim, size_t(blob))) && !((flags & MLZ_SEARCH_IGNORE_CASE) && mlz::search_is_letter(rd->index_delim)); };
    GrepOut out;
    if (const int e = grep_enter(rd, pattern_ok, d_rec_no, d_rec_kind, rec_cap, &out)) return e;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_grep_locked(rd, sm, flags, patterns, pattern_len, n_patterns, before, after, out, totals, stats));
}
