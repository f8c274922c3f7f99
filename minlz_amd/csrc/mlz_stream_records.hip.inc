// mlz_stream_records.hip.inc — mlz_dev_reader_search_records: the records (lines) of a .mz stream in HBM that hold a byte string (included at
// the end of mlz_hip.hip, behind the pattern search and the range read in device memory, whose locked forms it calls).
//
// Two phases under one lock; the rules are those of mlz_stream_records.h, which the host check runs as plain loops.
//   phase 1  dev_reader_search_scan_locked: the search's plan, decode and scan.  The total comes home, the context's records buffer is sized
//            by it, and search_write_kernel puts ALL occurrences there (the search's bitmaps live in c->d_rplan, which phase 2 carves anew).
//   windows  records_window_kernel: does the window [p - W, p + L + W) of an occurrence open a merged window; records_window_scan_kernel
//            (one workgroup, a slab of occurrences per lane) numbers the windows and compacts them into offsets and lengths.
//   phase 2  dev_reader_read_device_locked over those arrays into the context's window buffer, with the starts: every chunk a window touches
//            is decoded once, also the chunks that the tables pruned in phase 1 and a record reaches into.
//   bounds   records_bounds_kernel, a wavefront per occurrence: the delimiter backwards from p and forwards from p + L in the window buffer,
//            16 bytes per lane and step, a ballot, the highest lane backwards and the lowest forwards.
//   records  records_number_kernel (one workgroup): opening flags from the neighbour's s, a scan for the record numbers, per record e and the
//            right cut of its last occurrence, a scan of the lengths, the cut at the caps; a 48-byte header comes home.
//   copy     records_copy_kernel, in the shape of rdev_gather_kernel: workgroups [0, pieces) copy 64 KiB of a long record each, the rest serve
//            16 records each with 16 lanes and write the records' entries of the caller's arrays.
// No kernel waits for another workgroup.

#include "mlz_stream_records.h"

namespace mlz {

constexpr uint32_t kRecordsScanThreads = 1024;

// The slab of lane `tid` of a one-workgroup pass over n items
struct RecordsSlab { uint64_t b, e; };
__device__ __forceinline__ RecordsSlab records_slab(uint64_t n, uint32_t tid) {
    const uint64_t per = (n + kRecordsScanThreads - 1) / kRecordsScanThreads;
    const uint64_t b = tid * per < n ? tid * per : n;
    return RecordsSlab{b, n - b > per ? b + per : n};
}

// win_of[i] = 1 when occurrence i's window opens a merged window, else 0
__global__ __launch_bounds__(256) void records_window_kernel(const uint64_t* __restrict__ off, uint64_t n, uint32_t L, uint32_t W, uint64_t size, uint32_t* __restrict__ win_of) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const RecordsWindow w = records_window(off[i], L, W, size);
    win_of[i] = i == 0 || records_window_opens(w.lo, records_window(off[i - 1], L, W, size).hi) ? 1u : 0u;
}

// win_of[i]: the flag in, the merged window's number out.  woff[w], wlen[w]: lo of window w's first occurrence, hi of its last - that lo.
__global__ __launch_bounds__(kRecordsScanThreads) void records_window_scan_kernel(const uint64_t* __restrict__ off, uint64_t n, uint32_t L, uint32_t W, uint64_t size,
                                                                                   uint32_t* __restrict__ win_of, uint64_t* __restrict__ woff, uint64_t* __restrict__ wlen,
                                                                                   RecordsWindows* __restrict__ hdr) {
    __shared__ uint64_t lds[kRecordsScanThreads];
    const uint32_t tid = threadIdx.x;
    auto plus = [](uint64_t x, uint64_t y) { return x + y; };
    const RecordsSlab sl = records_slab(n, tid);
    uint64_t cnt = 0, nw = 0;
    for (uint64_t i = sl.b; i < sl.e; i++) cnt += win_of[i];
    uint64_t run = wg_scan<kRecordsScanThreads>(cnt, lds, tid, plus, &nw);
    for (uint64_t i = sl.b; i < sl.e; i++) {
        const uint32_t opens = win_of[i];
        run += opens;
        const uint64_t w = run - 1;
        win_of[i] = uint32_t(w);
        const RecordsWindow wd = records_window(off[i], L, W, size);
        if (opens) woff[w] = wd.lo;
        if (i + 1 == n || records_window_opens(records_window(off[i + 1], L, W, size).lo, wd.hi)) wlen[w] = wd.hi;   // (its end, until the pass below)
    }
    __threadfence_block();
    __syncthreads();   // a window's first and last occurrence may be two lanes'
    const RecordsSlab ws = records_slab(nw, tid);
    uint64_t sum = 0, total = 0;
    for (uint64_t w = ws.b; w < ws.e; w++) {
        const uint64_t l = wlen[w] - woff[w];
        wlen[w] = l;
        sum += l;
    }
    wg_scan<kRecordsScanThreads>(sum, lds, tid, plus, &total);
    if (tid == 0) { hdr->n = nw; hdr->bytes = total; }
}

// A wavefront per occurrence.  win: the merged windows' bytes, packed; window w's byte for stream position x lies at wstart[w] + (x - woff[w]).
// Only bytes of [lo, p) and [p + L, hi) are read, which lie in the occurrence's merged window.
__global__ __launch_bounds__(256) void records_bounds_kernel(const uint8_t* __restrict__ win, const uint64_t* __restrict__ off, const uint32_t* __restrict__ win_of,
                                                             const uint64_t* __restrict__ woff, const uint64_t* __restrict__ wstart, uint64_t n, uint32_t L, uint32_t W, uint64_t size,
                                                             uint8_t delim, uint64_t* __restrict__ s_out, uint64_t* __restrict__ e_out, uint8_t* __restrict__ cut_out) {
    const uint64_t i = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= n) return;   // (the whole wavefront)
    const uint64_t p = off[i];
    const uint32_t w = win_of[i];
    const RecordsWindow wd = records_window(p, L, W, size);
    const int64_t x0 = int64_t(wstart[w]) - int64_t(woff[w]);   // win + x0 is where position 0 would lie
    const int64_t mis = int64_t((reinterpret_cast<uintptr_t>(win) + uintptr_t(x0)) & 15);
    const uint8_t* al = win + (x0 - mis);   // al + y is the address of y = x + mis: 16-byte aligned where y % 16 == 0
    auto vec = [&](int64_t y, uint32_t* v) {
        const uint4 x = *reinterpret_cast<const uint4*>(al + y);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    };
    auto byte = [&](int64_t y) { return al[y]; };
    uint8_t cut = 0;
    bool found = false;
    uint64_t at = 0;
    {   // backwards over [lo, p)
        const int64_t ylo = int64_t(wd.lo) + mis, yp = int64_t(p) + mis, ytop = (yp + 15) & ~int64_t(15);
        for (uint32_t step = 0; ytop - int64_t(step) * kRecordsStep > ylo; step++) {
            const uint32_t m = records_block_mask(records_back_block(ytop, step, lane), ylo, yp, delim, vec, byte);
            const uint64_t hit = __ballot(m != 0);
            if (hit) {
                const uint32_t hl = 63u - uint32_t(__clzll(static_cast<long long>(hit)));
                const uint32_t hm = uint32_t(__shfl(int(m), int(hl)));
                at = uint64_t(records_back_block(ytop, step, hl) + int64_t(31 - __clz(int(hm))) - mis);
                found = true;
                break;
            }
        }
    }
    const uint64_t s = records_left(found, at, wd.lo, &cut);
    found = false;
    {   // forwards over [p + L, hi)
        const int64_t yq = int64_t(p + L) + mis, yhi = int64_t(wd.hi) + mis, ybot = yq & ~int64_t(15);
        for (uint32_t step = 0; ybot + int64_t(step) * kRecordsStep < yhi; step++) {
            const uint32_t m = records_block_mask(records_fwd_block(ybot, step, lane), yq, yhi, delim, vec, byte);
            const uint64_t hit = __ballot(m != 0);
            if (hit) {
                const uint32_t hl = uint32_t(__ffsll(static_cast<long long>(hit))) - 1u;
                const uint32_t hm = uint32_t(__shfl(int(m), int(hl)));
                at = uint64_t(records_fwd_block(ybot, step, hl) + int64_t(__ffs(int(hm)) - 1) - mis);
                found = true;
                break;
            }
        }
    }
    const uint64_t e = records_right(found, at, wd.hi, size, &cut);
    if (lane == 0) { s_out[i] = s; e_out[i] = e; cut_out[i] = cut; }
}

struct RecordsSums { uint64_t len, pieces, flagged; };

// One workgroup.  Records out: rec_s, rec_e, rec_win (the merged window that holds it), rec_fl (its flags; rec_fr: scratch for the right cut),
// rec_start and rec_piece (n + 1 values each: the exclusive prefixes of the lengths and of the long pieces, and their totals), the header.
__global__ __launch_bounds__(kRecordsScanThreads) void records_number_kernel(const uint64_t* __restrict__ s, const uint64_t* __restrict__ e, const uint8_t* __restrict__ cut,
                                                                              const uint32_t* __restrict__ win_of, uint64_t n, uint64_t rec_cap, uint64_t dst_cap, uint32_t short_max,
                                                                              uint32_t piece, uint64_t* __restrict__ rec_s, uint64_t* __restrict__ rec_e, uint32_t* __restrict__ rec_win,
                                                                              uint8_t* __restrict__ rec_fl, uint8_t* __restrict__ rec_fr, uint64_t* __restrict__ rec_start,
                                                                              uint64_t* __restrict__ rec_piece, RecordsHeader* __restrict__ hdr) {
    __shared__ uint64_t lds[kRecordsScanThreads];
    __shared__ RecordsSums lds3[kRecordsScanThreads];
    const uint32_t tid = threadIdx.x;
    auto plus = [](uint64_t x, uint64_t y) { return x + y; };
    const RecordsSlab sl = records_slab(n, tid);
    uint64_t cnt = 0, nr = 0;
    for (uint64_t i = sl.b; i < sl.e; i++) cnt += records_opens(i, s[i], i ? s[i - 1] : 0) ? 1 : 0;
    uint64_t run = wg_scan<kRecordsScanThreads>(cnt, lds, tid, plus, &nr);
    for (uint64_t i = sl.b; i < sl.e; i++) {
        const bool opens = records_opens(i, s[i], i ? s[i - 1] : 0);
        run += opens ? 1 : 0;
        const uint64_t r = run - 1;
        if (opens) { rec_s[r] = s[i]; rec_win[r] = win_of[i]; rec_fl[r] = cut[i] & kRecordCutLeft; }
        if (i + 1 == n || records_opens(i + 1, s[i + 1], s[i])) { rec_e[r] = e[i]; rec_fr[r] = cut[i] & kRecordCutRight; }   // the record's last occurrence
    }
    __threadfence_block();
    __syncthreads();   // a record's first and last occurrence may be two lanes'
    const RecordsSlab rs = records_slab(nr, tid);
    RecordsSums sum{0, 0, 0}, tot{0, 0, 0};
    for (uint64_t r = rs.b; r < rs.e; r++) {
        const uint64_t len = rec_e[r] - rec_s[r];
        sum.len += len;
        sum.pieces += records_pieces(len, short_max, piece);
        sum.flagged += (rec_fl[r] | rec_fr[r]) ? 1 : 0;
    }
    RecordsSums pre = wg_scan<kRecordsScanThreads>(sum, lds3, tid, [](RecordsSums x, RecordsSums y) { return RecordsSums{x.len + y.len, x.pieces + y.pieces, x.flagged + y.flagged}; }, &tot);
    uint64_t fit = 0, k = 0;
    for (uint64_t r = rs.b; r < rs.e; r++) {
        const uint64_t len = rec_e[r] - rec_s[r];
        rec_start[r] = pre.len;
        rec_piece[r] = pre.pieces;
        rec_fl[r] = rec_fl[r] | rec_fr[r];
        pre.len += len;
        pre.pieces += records_pieces(len, short_max, piece);
        fit += records_fits(r, pre.len, rec_cap, dst_cap) ? 1 : 0;
    }
    if (tid == 0) { rec_start[nr] = tot.len; rec_piece[nr] = tot.pieces; }
    wg_scan<kRecordsScanThreads>(fit, lds, tid, plus, &k);
    __threadfence_block();
    __syncthreads();
    if (tid == 0) *hdr = RecordsHeader{nr, tot.len, tot.flagged, k, rec_start[k], rec_piece[k]};
}

struct RecordsCopyArgs {
    const uint8_t* win; const uint64_t *woff, *wstart, *rec_s, *rec_e, *rec_start, *rec_piece; const uint32_t* rec_win; const uint8_t* rec_fl;
    uint8_t* dst; uint64_t *d_rec_off, *d_rec_start; uint8_t* d_rec_flags;
    uint64_t k; uint32_t n_pieces, short_max;
};

// Records [0, k) to dst, packed, and their entries of the caller's arrays (d_rec_start: k + 1 values).
__global__ __launch_bounds__(256) void records_copy_kernel(const RecordsCopyArgs a) {
    auto src_of = [&](uint64_t r) { const uint32_t w = a.rec_win[r]; return a.win + a.wstart[w] + (a.rec_s[r] - a.woff[w]); };
    if (blockIdx.x < a.n_pieces) {   // a long piece: the last record whose piece prefix is at most the piece's number owns it (records without pieces share their successor's prefix)
        uint64_t lo = 0, hi = a.k;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.rec_piece[mid] <= blockIdx.x) lo = mid; else hi = mid;
        }
        const uint64_t r = lo, len = a.rec_e[r] - a.rec_s[r], pb = (blockIdx.x - a.rec_piece[r]) * uint64_t(kPlacePiece);
        wg_copy(a.dst + a.rec_start[r] + pb, src_of(r) + pb, uint32_t(len - pb > kPlacePiece ? kPlacePiece : len - pb), threadIdx.x, 256);
        return;
    }
    const uint64_t r = uint64_t(blockIdx.x - a.n_pieces) * kRangeShortPerWg + (threadIdx.x >> 4);
    const uint32_t lane = threadIdx.x & 15;
    if (r > a.k) return;
    if (r == a.k) {
        if (lane == 0 && a.d_rec_start) a.d_rec_start[r] = a.rec_start[r];
        return;
    }
    if (lane == 0) {
        a.d_rec_off[r] = a.rec_s[r];
        if (a.d_rec_start) a.d_rec_start[r] = a.rec_start[r];
        if (a.d_rec_flags) a.d_rec_flags[r] = a.rec_fl[r];
    }
    const uint64_t len = a.rec_e[r] - a.rec_s[r];
    if (len <= a.short_max) lanes16_copy(a.dst + a.rec_start[r], src_of(r), uint32_t(len), lane);
}

}  // namespace mlz

namespace {

struct RecordsOut { uint8_t* d_dst; uint64_t dst_cap; uint64_t *d_rec_off, *d_rec_start; uint8_t* d_rec_flags; uint64_t rec_cap; };

int64_t dev_reader_search_records_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* pattern, uint32_t L, uint8_t delim, uint32_t W, const RecordsOut& out,
                                         uint64_t* totals, uint64_t* stats) {
    mlz_ctx* c = rd->ctx;
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0;
    const uint64_t size = uint64_t(rd->size);
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
    // phase 1
    SearchFound found;
    int64_t r = dev_reader_search_scan_locked(rd, sm, flags, pattern, L, stats, &found);
    if (r < 0) return r;
    if ((r = search_found_total(c, sm, found)) <= 0) return r;
    const uint64_t n = uint64_t(r);
    if (totals) totals[2] = n;
    if (n > mlz::kRecordsMaxOccurrences) return -MLZ_ERR_ARG;
    // what lives across the read phase: per occurrence | per merged window | per record (there are at most n of either)
    Carve cv;
    const auto r_hdr = cv.take<mlz::RecordsHeader>(1);
    const auto r_whdr = cv.take<mlz::RecordsWindows>(1);
    const auto r_off = cv.take<uint64_t>(size_t(n)), r_s = cv.take<uint64_t>(size_t(n)), r_e = cv.take<uint64_t>(size_t(n));
    const auto r_woff = cv.take<uint64_t>(size_t(n)), r_wlen = cv.take<uint64_t>(size_t(n)), r_wstart = cv.take<uint64_t>(size_t(n) + 1);
    const auto r_rs = cv.take<uint64_t>(size_t(n)), r_re = cv.take<uint64_t>(size_t(n)), r_rstart = cv.take<uint64_t>(size_t(n) + 1), r_rpiece = cv.take<uint64_t>(size_t(n) + 1);
    const auto r_winof = cv.take<uint32_t>(size_t(n)), r_rwin = cv.take<uint32_t>(size_t(n));
    const auto r_cut = cv.take<uint8_t>(size_t(n)), r_fl = cv.take<uint8_t>(size_t(n)), r_fr = cv.take<uint8_t>(size_t(n));
    HIPCHK(c, c->d_records.ensure(cv.bytes));
    void* ws = c->d_records.p;
    uint64_t *d_off = r_off.at(ws), *d_s = r_s.at(ws), *d_e = r_e.at(ws), *d_woff = r_woff.at(ws), *d_wlen = r_wlen.at(ws), *d_wstart = r_wstart.at(ws);
    uint64_t *d_rs = r_rs.at(ws), *d_re = r_re.at(ws), *d_rstart = r_rstart.at(ws), *d_rpiece = r_rpiece.at(ws);
    uint32_t *d_winof = r_winof.at(ws), *d_rwin = r_rwin.at(ws);
    uint8_t *d_cut = r_cut.at(ws), *d_fl = r_fl.at(ws), *d_fr = r_fr.at(ws);
    mlz::RecordsHeader* d_hdr = r_hdr.at(ws);
    mlz::RecordsWindows* d_whdr = r_whdr.at(ws);
    search_found_write(sm, found, n, d_off);
    // windows
    hipLaunchKernelGGL(mlz::records_window_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, sm, d_off, n, L, W, size, d_winof);
    hipLaunchKernelGGL(mlz::records_window_scan_kernel, dim3(1), dim3(mlz::kRecordsScanThreads), 0, sm, d_off, n, L, W, size, d_winof, d_woff, d_wlen, d_whdr);
    int e = fetch(c, sm, c->pinned2, d_whdr, sizeof(mlz::RecordsWindows));
    if (e) return e;
    const mlz::RecordsWindows wh = *static_cast<const mlz::RecordsWindows*>(c->pinned2);
    if (wh.n == 0 || wh.n > n || wh.bytes > size) { c->err = "mlz_dev_reader_search_records: the windows do not fit the stream"; return -MLZ_ERR_HIP; }
    // phase 2
    HIPCHK(c, c->d_rwin.ensure(size_t(wh.bytes)));
    uint8_t* d_win = c->d_rwin.as<uint8_t>();
    uint64_t got = 0;
    if ((r = dev_reader_read_device_locked(rd, sm, ignore_crc, d_woff, d_wlen, wh.n, d_win, wh.bytes, d_wstart, &got)) < 0) return r;
    if (got != wh.bytes) { c->err = "mlz_dev_reader_search_records: the read phase returned other bytes than the windows hold"; return -MLZ_ERR_HIP; }
    // bounds, records
    hipLaunchKernelGGL(mlz::records_bounds_kernel, dim3(uint32_t((n + 3) / 4)), dim3(256), 0, sm, d_win, d_off, d_winof, d_woff, d_wstart, n, L, W, size, delim, d_s, d_e, d_cut);
    hipLaunchKernelGGL(mlz::records_number_kernel, dim3(1), dim3(mlz::kRecordsScanThreads), 0, sm, d_s, d_e, d_cut, d_winof, n, out.rec_cap, out.dst_cap, mlz::kRangeShortMax,
                       kPlacePiece, d_rs, d_re, d_rwin, d_fl, d_fr, d_rstart, d_rpiece, d_hdr);
    if ((e = fetch(c, sm, c->pinned2, d_hdr, sizeof(mlz::RecordsHeader)))) return e;
    const mlz::RecordsHeader h = *static_cast<const mlz::RecordsHeader*>(c->pinned2);
    if (h.records == 0 || h.records > n || h.k > h.records || h.k > out.rec_cap || h.written > out.dst_cap || h.written > h.bytes) {
        c->err = "mlz_dev_reader_search_records: the records do not fit the occurrences or the caps";
        return -MLZ_ERR_HIP;
    }
    if (totals) { totals[0] = h.records; totals[1] = h.bytes; totals[3] = h.flagged; }
    // copy
    const uint64_t grid = h.pieces + (h.k + 1 + mlz::kRangeShortPerWg - 1) / mlz::kRangeShortPerWg;
    if (grid > mlz::kRdevMaxGrid) return -MLZ_ERR_ARG;
    if (h.k || out.d_rec_start) {
        const mlz::RecordsCopyArgs ca{d_win, d_woff, d_wstart, d_rs, d_re, d_rstart, d_rpiece, d_rwin, d_fl, out.d_dst, out.d_rec_off, out.d_rec_start, out.d_rec_flags,
                                      h.k, uint32_t(h.pieces), mlz::kRangeShortMax};
        hipLaunchKernelGGL(mlz::records_copy_kernel, dim3(uint32_t(grid)), dim3(256), 0, sm, ca);
        HIPCHK(c, hipStreamSynchronize(sm));
        HIPCHK(c, hipGetLastError());
    }
    return int64_t(h.records);
}

}  // namespace

extern "C" int64_t mlz_dev_reader_search_records(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* pattern, size_t pattern_len, uint8_t delimiter, uint32_t max_reach,
                                                 uint8_t* d_dst, size_t dst_cap, uint64_t* d_rec_off, uint64_t* d_rec_start, uint8_t* d_rec_flags, size_t rec_cap, uint64_t* totals,
                                                 uint64_t* stats) {
    if (!rd || !pattern || pattern_len == 0 || pattern_len > mlz::kSearchMaxPattern || max_reach > MLZ_RECORDS_MAX_REACH || (!d_dst && dst_cap) || (!d_rec_off && rec_cap))
        return -MLZ_ERR_ARG;
    if (std::memchr(pattern, delimiter, pattern_len)) return -MLZ_ERR_ARG;   // a line search cannot match across lines
    if ((flags & MLZ_SEARCH_IGNORE_CASE) && mlz::search_is_letter(delimiter)) return -MLZ_ERR_ARG;   // records are split at the delimiter's own byte, which is never folded
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if ((dst_cap && !on_device(c, d_dst)) || (rec_cap && !on_device(c, d_rec_off)) || (d_rec_start && !on_device(c, d_rec_start)) ||
        (rec_cap && d_rec_flags && !on_device(c, d_rec_flags)))
        return -MLZ_ERR_ARG;
    begin_decode_call(c);
    c->range_plan_host = 0;
    c->range_chunks = c->range_scratch = 0;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const RecordsOut out{d_dst, uint64_t(dst_cap), d_rec_off, d_rec_start, rec_cap ? d_rec_flags : nullptr, uint64_t(rec_cap)};
    return settled(sm, dev_reader_search_records_locked(rd, sm, flags, pattern, uint32_t(pattern_len), delimiter, max_reach ? max_reach : mlz::kRecordsDefaultReach, out, totals, stats));
}
