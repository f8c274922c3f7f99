// mlz_search_tables_compress.hip.inc — compressed block search tables (chunk 0x46) on the write side: bitmaps in device memory -> their
// huff0 sections (`h0_bs h0_tc | table descriptions | sub-blocks`), byte for byte what cst_compress_host (mlz_search_compressed.h) and
// the model's default writer (tests/search_compressed_model.py) make of them.  Included in mlz_hip.hip.  gfx950, wave64.
//
// Three kernels, 256 threads (four wavefronts) a workgroup:
//   cstw_plan_kernel    a workgroup per (bitmap, sub-block).  Wavefront q counts the byte values of quarter q, which is stream q of a
//                       tabled sub-block, in a histogram of its own in LDS; their sum is the sub-block's.  One value: RLE.  Else the exact
//                       length of the sparse table (each thread's first and last set bit, a max-scan for the set bit in front of a
//                       thread's bytes, the 255-escapes counted per gap; skipped where the set bits alone rule sparse out), the code
//                       lengths (wavefront 0: up to 255 merges, each two wave-wide minima over the live nodes, four a lane, keyed by
//                       (weight, smallest symbol); built again with halved counts while deeper than 11), the canonical codes (a thread
//                       per symbol), the description (one lane: cst_w_description) and every stream's bits.  It leaves a record (kind,
//                       description and body bytes, stream sizes), the description and the 256 (code, length) pairs in workspace.
//   cstw_layout_kernel  a thread per bitmap: the records' places in the section (`h0_bs h0_tc`, descriptions in table order, sub-blocks),
//                       the section's length against the item's capacity, the length or the item's error to d_len.
//   cstw_encode_kernel  a workgroup per (bitmap, sub-block), a wavefront per stream.  A lane owns a run of consecutive symbols; a suffix
//                       scan of the runs' bits gives each run its bit offset from the stream's end; runs are packed in a 64-bit register
//                       and go to the stream's image in LDS 32 bits at a time with ds_or (words shared by two lanes merge there; no
//                       global atomics); the image leaves with dword stores.  Raw, RLE and sparse sub-blocks are written here too (sparse:
//                       the scan of the plan again, and a prefix sum of the threads' byte counts).
// Nothing is written outside an item's [dst_off, dst_off + section length), and nothing at all for an item with an error.
// The device Writer (stream_gather_range) and the sidecar build (sidecar_build_pass) hand their kept tables to the same launch sequence, each with
// one byte less of room than the table has: a section that is no shorter is then that item's error and the chunk stays 0x45.

namespace mlz {

constexpr uint32_t kCstwThreads = 256;
constexpr uint32_t kCstwStreamLds = 22544;   // a stream's image: at most 16384 symbols of 11 bits and the end marker, in whole 16-byte units

__device__ __forceinline__ unsigned long long cstw_wave_min(unsigned long long v) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_xor(uint32_t(v), d), hi = __shfl_xor(uint32_t(v >> 32), d);
        const unsigned long long o = (unsigned long long)(hi) << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

// The sparse table of a sub-block, thread t's share: its bytes are b[t * ch, (t + 1) * ch), ch = max(1, sub / 256).  -> the bytes its set
// bits take in the table; *prev_out: one behind the last set bit in front of its bytes (0: none).  scan: 256 words of LDS.  All threads call.
__device__ uint32_t cstw_sparse_share(const uint8_t* __restrict__ b, uint32_t sub, uint32_t t, uint32_t* scan, uint32_t* prev_out) {
    const uint32_t ch = sub >= kCstwThreads ? sub / kCstwThreads : 1, lo = t * ch;
    uint32_t first = 0xffffffffu, last1 = 0, inner = 0;   // last1: one behind the thread's last set bit
    if (lo < sub)
        for (uint32_t i = 0; i < ch; i++)
            for (uint32_t v = b[lo + i]; v; v &= v - 1) {
                const uint32_t pos = 8 * (lo + i) + uint32_t(__builtin_ctz(v));
                if (first == 0xffffffffu) first = pos;
                else inner += cst_w_gap_bytes(pos - last1);
                last1 = pos + 1;
            }
    scan[t] = last1;
    __syncthreads();
    for (uint32_t d = 1; d < kCstwThreads; d <<= 1) {      // inclusive max-scan: positions grow with t, 0 is "none"
        const uint32_t o = t >= d ? scan[t - d] : 0;
        __syncthreads();
        if (o > scan[t]) scan[t] = o;
        __syncthreads();
    }
    const uint32_t prev = t ? scan[t - 1] : 0;
    __syncthreads();
    *prev_out = prev;
    return first == 0xffffffffu ? 0 : inner + cst_w_gap_bytes(first - prev);
}

__global__ __launch_bounds__(kCstwThreads) void cstw_plan_kernel(const uint8_t* __restrict__ src, const CstwJob* __restrict__ jobs, CstwRec* __restrict__ recs,
                                                                 uint32_t* __restrict__ codes, uint8_t* __restrict__ descs) {
    __shared__ uint32_t hist4[4][256], hist[256], code[256], scan[kCstwThreads];
    __shared__ CstHuffScratch hs;
    __shared__ CstFseScratch fs;
    __shared__ uint8_t depth[256], w[256], desc[1 + kCstFseOutCap + 7];
    __shared__ uint32_t sh_sparse, sh_deepest, sh_dlen, sh_bits[4];
    const uint32_t t = threadIdx.x, q = t >> 6, lane = t & 63;
    const CstwJob jb = jobs[blockIdx.x];
    const uint8_t* b = src + jb.src_off;
    const uint32_t sub = jb.sub, seg = sub >> 2;
    CstwRec* rec = recs + blockIdx.x;

    for (uint32_t i = 0; i < 4; i++) hist4[i][t] = 0;
    if (t < 4) sh_bits[t] = 0;
    if (t == 0) sh_sparse = 0;
    __syncthreads();
    if (seg >= 256) {   // (src_off is the caller's: dwords are read where the quarter starts at one)
        const uint8_t* p = b + q * seg;
        if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            for (uint32_t i = lane; i < seg / 4; i += 64) {
                const uint32_t v = reinterpret_cast<const uint32_t*>(p)[i];
                atomicAdd(&hist4[q][v & 255], 1u);
                atomicAdd(&hist4[q][(v >> 8) & 255], 1u);
                atomicAdd(&hist4[q][(v >> 16) & 255], 1u);
                atomicAdd(&hist4[q][v >> 24], 1u);
            }
        } else {
            for (uint32_t i = lane; i < seg; i += 64) atomicAdd(&hist4[q][p[i]], 1u);
        }
    } else {
        for (uint32_t i = lane; i < seg; i += 64) atomicAdd(&hist4[q][b[q * seg + i]], 1u);
    }
    __syncthreads();
    const uint32_t mine = hist4[0][t] + hist4[1][t] + hist4[2][t] + hist4[3][t];
    hist[t] = mine;
    const int values = __syncthreads_count(mine != 0);
    if (values == 1) {
        if (mine) *rec = CstwRec{kCstRle, 0, 2, t, 0, 0, {0, 0, 0, 0}, 0, 0, 0, {0, 0, 0}};
        return;
    }
    // the set bits from the histogram: sparse takes a byte a bit at least, so with bits + 3 >= sub raw is never larger and wins the tie
    atomicAdd(&sh_sparse, mine * uint32_t(__popc(t)));
    __syncthreads();
    const bool sparse_can = sh_sparse + 3 < sub;
    __syncthreads();
    if (sparse_can) {
        if (t == 0) sh_sparse = 0;
        uint32_t prev;
        const uint32_t share = cstw_sparse_share(b, sub, t, scan, &prev);
        if (share) atomicAdd(&sh_sparse, share);
    }

    // code lengths: slot i * 64 + lane of wavefront 0 holds symbol i * 64 + lane's node
    for (uint32_t shift = 0;; shift++) {
        __syncthreads();
        uint32_t nodes = 256;
        if (q == 0) {
            uint32_t key[4], node[4];
            for (uint32_t i = 0; i < 4; i++) { key[i] = cst_w_key(hist[i * 64 + lane], shift, i * 64 + lane); node[i] = i * 64 + lane; }
            for (int live = values; live > 1; live--) {
                unsigned long long m[2];
                uint32_t nd[2];
                for (uint32_t r = 0; r < 2; r++) {
                    unsigned long long best = ~0ull;
                    for (uint32_t i = 0; i < 4; i++) {
                        const unsigned long long k = (unsigned long long)(key[i]) << 8 | (i * 64 + lane);
                        best = k < best ? k : best;
                    }
                    m[r] = cstw_wave_min(best);
                    const uint32_t slot = uint32_t(m[r]) & 255;
                    uint32_t n_ = 0;
                    for (uint32_t i = 0; i < 4; i++)
                        if ((slot & 63) == lane && (slot >> 6) == i) { n_ = node[i]; if (r == 0) key[i] = kCstNoNode; }
                    nd[r] = __shfl(n_, int(slot & 63));
                }
                const uint32_t sa = uint32_t(m[0]) & 255, sb = uint32_t(m[1]) & 255;
                const uint32_t merged = cst_w_merge_key(uint32_t(m[0] >> 8), uint32_t(m[1] >> 8));
                for (uint32_t i = 0; i < 4; i++) {
                    if ((sa & 63) == lane && (sa >> 6) == i) { key[i] = merged; node[i] = nodes; }
                    if ((sb & 63) == lane && (sb >> 6) == i) key[i] = kCstNoNode;
                }
                if (lane == 0) { hs.parent[nd[0]] = uint16_t(nodes); hs.parent[nd[1]] = uint16_t(nodes); }
                nodes++;
            }
        }
        __syncthreads();
        if (t == 0) sh_deepest = cst_w_depths(hist, 255 + uint32_t(values), &hs, depth);
        __syncthreads();
        if (sh_deepest <= kCstMaxTableLog) break;
    }
    const uint32_t log = sh_deepest;
    // weights and canonical codes, a thread per symbol: symbols by ascending weight, by value within a weight
    const uint32_t wt = depth[t] ? log + 1 - depth[t] : 0;
    w[t] = uint8_t(wt);
    __syncthreads();
    uint32_t at = 0;
    if (wt)
        for (uint32_t s = 0; s < 256; s++) {
            const uint32_t x = w[s];
            if (x && x < wt) at += 1u << (x - 1);
            else if (x == wt && s < t) at += 1u << (wt - 1);
        }
    const uint32_t cd = wt ? (at >> (wt - 1)) | (log + 1 - wt) << 16 : 0;
    code[t] = cd;
    codes[size_t(blockIdx.x) * 256 + t] = cd;
    for (uint32_t i = 0; i < 4; i++)
        if (hist4[i][t]) atomicAdd(&sh_bits[i], hist4[i][t] * (cd >> 16));
    if (t == 0) {
        uint32_t top = 255;
        while (!hist[top]) top--;
        sh_dlen = cst_w_description(w, top, desc, &fs);
    }
    __syncthreads();
    const uint32_t dlen = sh_dlen;
    if (t < dlen) descs[size_t(blockIdx.x) * kCstwDescSlot + t] = desc[t];
    if (t == 0) {
        const uint32_t sparse_len = sparse_can ? sh_sparse : 0xffffffu;
        const uint32_t bits = sh_bits[0] + sh_bits[1] + sh_bits[2] + sh_bits[3];
        const uint32_t kind = cst_w_pick(sub, sparse_len, dlen, bits);
        CstwRec r{kind, 0, 0, 0, 0, 0, {0, 0, 0, 0}, 0, 0, 0, {0, 0, 0}};
        if (kind == kCstRaw) r.body_len = 1 + sub;
        else if (kind == kCstSparse) { r.sparse_len = sparse_len; r.body_len = 1 + cst_w_uvarint_len(sparse_len) + sparse_len; }
        else {
            r.desc_len = dlen;
            r.four_len = 6;
            for (uint32_t i = 0; i < 4; i++) { r.slen[i] = sh_bits[i] / 8 + 1; r.four_len += r.slen[i]; }
            r.body_len = 1 + cst_w_uvarint_len(r.four_len) + r.four_len;
        }
        *rec = r;
    }
}

__global__ __launch_bounds__(64) void cstw_layout_kernel(const CstwItem* __restrict__ items, uint32_t n, CstwRec* __restrict__ recs, uint8_t* __restrict__ dst,
                                                         int64_t* __restrict__ d_len, uint32_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const CstwItem it = items[i];
    ok[i] = 0;
    if (!it.n) { d_len[i] = -MLZ_ERR_ARG; return; }
    CstwRec* r = recs + it.first_job;
    uint32_t tc = 0, at = 2;
    for (uint32_t j = 0; j < it.nsub; j++)
        if (r[j].kind == 0) { r[j].table = tc++; r[j].desc_off = at; at += r[j].desc_len; }
    for (uint32_t j = 0; j < it.nsub; j++) { r[j].out_off = at; at += r[j].body_len; }
    if (at > it.dst_cap) { d_len[i] = -MLZ_ERR_DST_TOO_SMALL; return; }
    dst[it.dst_off] = uint8_t(it.bs);
    dst[it.dst_off + 1] = uint8_t(tc);
    d_len[i] = int64_t(at);
    ok[i] = 1;
}

// src[0, n) in LDS or global memory -> dst[0, n) in global memory by `lanes` workers: bytes up to dst's first dword, dwords, bytes
__device__ __forceinline__ void cstw_store(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t lane, uint32_t lanes) {
    uint32_t head = uint32_t(-reinterpret_cast<uintptr_t>(dst)) & 3;
    head = head < n ? head : n;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t words = (n - head) >> 2;
    for (uint32_t i = lane; i < words; i += lanes) {
        uint32_t v;
        __builtin_memcpy(&v, src + head + 4 * i, 4);
        *reinterpret_cast<uint32_t*>(dst + head + 4 * i) = v;
    }
    const uint32_t done = head + 4 * words;
    if (lane < n - done) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(kCstwThreads) void cstw_encode_kernel(const uint8_t* __restrict__ src, const CstwJob* __restrict__ jobs, const CstwItem* __restrict__ items,
                                                                   const CstwRec* __restrict__ recs, const uint32_t* __restrict__ codes,
                                                                   const uint8_t* __restrict__ descs, const uint32_t* __restrict__ ok, uint8_t* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t image[4][kCstwStreamLds];
    __shared__ uint32_t code[256], scan[kCstwThreads];
    const uint32_t t = threadIdx.x, q = t >> 6, lane = t & 63;
    const CstwJob jb = jobs[blockIdx.x];
    if (!ok[jb.item]) return;
    const CstwRec rec = recs[blockIdx.x];
    const uint8_t* b = src + jb.src_off;
    uint8_t* section = dst + items[jb.item].dst_off;
    uint8_t* out = section + rec.out_off;
    const uint32_t sub = jb.sub;
    if (rec.kind == kCstRle) {
        if (t == 0) { out[0] = uint8_t(kCstRle); out[1] = uint8_t(rec.rle); }
        return;
    }
    if (rec.kind == kCstRaw) {
        if (t == 0) out[0] = uint8_t(kCstRaw);
        cstw_store(out + 1, b, sub, t, kCstwThreads);
        return;
    }
    if (rec.kind == kCstSparse) {
        uint32_t prev;
        const uint32_t share = cstw_sparse_share(b, sub, t, scan, &prev);
        scan[t] = share;
        __syncthreads();
        for (uint32_t d = 1; d < kCstwThreads; d <<= 1) {   // inclusive prefix sum of the threads' bytes
            const uint32_t o = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += o;
            __syncthreads();
        }
        uint8_t uv[5];
        const uint32_t un = cst_w_put_uvarint(uv, rec.sparse_len);
        if (t == 0) { out[0] = uint8_t(kCstSparse); for (uint32_t i = 0; i < un; i++) out[1 + i] = uv[i]; }
        if (share && scan[t] <= rec.sparse_len) {
            uint8_t* p = out + 1 + un + (scan[t] - share);
            const uint32_t ch = sub >= kCstwThreads ? sub / kCstwThreads : 1, lo = t * ch;
            for (uint32_t i = 0; i < ch; i++)
                for (uint32_t v = b[lo + i]; v; v &= v - 1) {
                    const uint32_t pos = 8 * (lo + i) + uint32_t(__builtin_ctz(v));
                    uint32_t gap = pos - prev;
                    for (; gap >= 255; gap -= 255) *p++ = 255;
                    *p++ = uint8_t(gap);
                    prev = pos + 1;
                }
        }
        return;
    }
    // a table of its own: the description, the record's head, four streams
    code[t] = codes[size_t(blockIdx.x) * 256 + t];
    if (t < rec.desc_len) section[rec.desc_off + t] = descs[size_t(blockIdx.x) * kCstwDescSlot + t];
    uint8_t uv[5];
    const uint32_t un = cst_w_put_uvarint(uv, rec.four_len);
    if (t == 0) {
        out[0] = uint8_t(rec.table);
        for (uint32_t i = 0; i < un; i++) out[1 + i] = uv[i];
        for (uint32_t i = 0; i < 3; i++) { out[1 + un + 2 * i] = uint8_t(rec.slen[i]); out[2 + un + 2 * i] = uint8_t(rec.slen[i] >> 8); }
    }
    const uint32_t slen = rec.slen[q], seg = sub >> 2;
    uint32_t* img = reinterpret_cast<uint32_t*>(image[q]);
    for (uint32_t i = lane; i < (slen + 3) / 4; i += 64) img[i] = 0;
    __syncthreads();
    {
        const uint8_t* s = b + q * seg;
        const uint32_t run = seg >= 64 ? seg / 64 : 1, lo = lane * run, hi = lo < seg ? lo + run : lo;   // the lane's symbols [lo, hi)
        uint32_t mybits = 0;
        for (uint32_t i = lo; i < hi; i++) mybits += code[s[i]] >> 16;
        uint32_t behind = mybits;                             // the bits of this lane's run and of every run behind it
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_down(behind, d);
            if (lane + d < 64) behind += o;
        }
        uint32_t pos = behind - mybits;                       // the last symbol of the run lies here, counted from the stream's end
        uint64_t acc = 0;
        uint32_t nbit = pos & 31, wi = pos >> 5;
        for (uint32_t i = hi; i-- > lo;) {
            const uint32_t c = code[s[i]];
            acc |= uint64_t(c & 0xffff) << nbit;
            nbit += c >> 16;
            if (nbit >= 32) { atomicOr(&img[wi++], uint32_t(acc)); acc >>= 32; nbit -= 32; }
        }
        if (lane == 0) { acc |= uint64_t(1) << nbit; nbit++; }   // the end marker above the first symbol
        if (nbit) atomicOr(&img[wi], uint32_t(acc));
        if (nbit > 32) atomicOr(&img[wi + 1], uint32_t(acc >> 32));
    }
    __syncthreads();
    uint32_t off = 1 + un + 6;
    for (uint32_t i = 0; i < q; i++) off += rec.slen[i];
    cstw_store(out + off, image[q], slen, lane, 64);
}

}  // namespace mlz

namespace {

// The three kernels over n items, enqueued on st (caller holds c->mu; workspace: c->d_cstw).  The item and job lists stay in the context
// until the next call: a caller may synchronise later.  One call's launches must have run before the next call's lists are made, which
// every caller's own synchronisation sees to.
int search_bitmaps_compress_locked(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* tables, int n, int64_t* d_len) {
    HIPCHK(c, hipSetDevice(c->device));
    WorkspaceOrder order(c, st);
    c->call_seq++;
    std::vector<mlz::CstwItem>& items = c->h_cstw_items;
    std::vector<mlz::CstwJob>& jobs = c->h_cstw_jobs;
    items.assign(static_cast<size_t>(n), mlz::CstwItem{});
    jobs.clear();
    for (int i = 0; i < n; i++) {
        const mlz_block_desc& d = tables[i];
        mlz::CstwItem it{d.dst_off, d.dst_cap, 0, uint32_t(jobs.size()), 0, 0};
        if (mlz::cst_w_size_ok(d.src_len)) {
            it.n = uint32_t(d.src_len);
            it.bs = mlz::cst_w_bs(it.n);
            it.nsub = it.n >> it.bs;
            for (uint32_t j = 0; j < it.nsub; j++) jobs.push_back(mlz::CstwJob{d.src_off + (uint64_t(j) << it.bs), uint32_t(i), 1u << it.bs});
        }
        items[size_t(i)] = it;
    }
    const size_t m = jobs.size();
    Carve cv;
    const auto r_items = cv.take<mlz::CstwItem>(size_t(n));
    const auto r_jobs = cv.take<mlz::CstwJob>(m);
    const auto r_recs = cv.take<mlz::CstwRec>(m);
    const auto r_codes = cv.take<uint32_t>(m * 256);
    const auto r_descs = cv.take<uint8_t>(m * mlz::kCstwDescSlot);
    const auto r_ok = cv.take<uint32_t>(size_t(n));
    HIPCHK(c, c->d_cstw.ensure(cv.bytes));
    void* ws = c->d_cstw.p;
    HIPCHK(c, hipMemcpyAsync(r_items.at(ws), items.data(), items.size() * sizeof(mlz::CstwItem), hipMemcpyHostToDevice, st));
    if (m) {
        HIPCHK(c, hipMemcpyAsync(r_jobs.at(ws), jobs.data(), m * sizeof(mlz::CstwJob), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mlz::cstw_plan_kernel, dim3(uint32_t(m)), dim3(mlz::kCstwThreads), 0, st, d_src, r_jobs.at(ws), r_recs.at(ws), r_codes.at(ws), r_descs.at(ws));
    }
    hipLaunchKernelGGL(mlz::cstw_layout_kernel, dim3(uint32_t((n + 63) / 64)), dim3(64), 0, st, r_items.at(ws), uint32_t(n), r_recs.at(ws), d_dst, d_len, r_ok.at(ws));
    if (m)
        hipLaunchKernelGGL(mlz::cstw_encode_kernel, dim3(uint32_t(m)), dim3(mlz::kCstwThreads), 0, st, d_src, r_jobs.at(ws), r_items.at(ws), r_recs.at(ws), r_codes.at(ws),
                           r_descs.at(ws), r_ok.at(ws), d_dst);
    HIPCHK(c, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int64_t mlz_search_bitmap_compress(const uint8_t* bitmap, size_t n, uint8_t* dst, size_t cap) {
    if (!bitmap || (!dst && cap) || !mlz::cst_w_size_ok(n)) return -MLZ_ERR_ARG;
    const int64_t r = mlz::cst_compress_host(bitmap, uint32_t(n), dst, cap);
    return r < 0 ? -MLZ_ERR_DST_TOO_SMALL : r;
}

extern "C" int mlz_search_bitmaps_compress_device(mlz_ctx* c, void* stream, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* tables, int n, int64_t* d_len) {
    if (!c || n < 0 || (n && (!tables || !d_src || !d_dst || !d_len))) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    mlz_ctx* const root = c;
    if (!(c = owner_of(root, d_src)) || owner_of(root, d_dst) != c || owner_of(root, d_len) != c) return -MLZ_ERR_ARG;   // all three on one device the context holds
    std::lock_guard<std::mutex> lk(c->mu);
    const int r = search_bitmaps_compress_locked(c, static_cast<hipStream_t>(stream), d_src, d_dst, tables, n, d_len);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return 0;
}
