// mlz_search_tables.hip.inc — the device-resident Writer's block search tables (included in mlz_hip.hip in front of mlz_stream.hip.inc, whose
// stream_gather_range calls search_tables_build).
//
// The reference's Writer with search tables (SPEC_SEARCH.md; search_table.go, search_index.go:30-63, unsafe_disabled.go:52-87), table type 1:
// a bitmap of 2^B bits per block, bit HashValue(window of M bytes, B, M) set for every position of the block — the last M - 1 positions take
// their missing bytes from the next block, zeros beyond it; the stream's last block has no such positions —, dropped when more than 70 % of
// its bits are set, else folded in halves while a quarter of the folded bits at the most are set and 32 bytes at the least remain.
// Table types 2 and 3 (SPEC_SEARCH.md 3.3; search_index.go:85-137): only the positions q >= 1 of a block whose preceding byte block[q - 1]
// is one of the configured prefix bytes; a block that is not the stream's last indexes position n too (the window that lies wholly in the
// next block's first M bytes, behind a prefix byte that is the block's last one), the stream's last block the positions up to n - M; a fold
// is accepted while a tenth of the folded bits at the most are set.
//
// stab_build_kernel: a workgroup keeps the bitmap (B <= 20: all of it, 128 KiB at the most; above: one slice of 2^20 bits, so 2, 4 or 8
//   workgroups hash a block's windows and each keeps the bits of its slice) in LDS, where a set bit is one non-returning ds_or; a device-scope
//   atomic per window would cost several times the whole encode (DESIGN.md section 0).  Few large blocks: several workgroups take parts of a
//   block and merge into the zeroed table in HBM with non-returning dword atomicOr (words that are not zero only).
//   stab_build_kernel<true> is the prefix form: a lane's 16 bytes start one byte in front of its 8 positions, the 256-bit set of prefix bytes
//   lies in 32 bytes of LDS (a per-lane byte indexes it with one ds_read), and the hash and the ds_or run for positions behind a prefix byte only:
//   a lane first gathers its 8 positions' verdicts into a bit mask and then loops over the set bits.
// Table type 4 (SPEC_SEARCH.md 3.3.4; search_index.go: buildTablePrefixLong, the overlap tail and the straddling prefix, whose union this is):
//   every start p of the K-byte prefix in the block — all of 0 .. n - 1 with a block behind, 0 .. n - K - M - E in the stream's last block —
//   sets the E + 1 bits of the windows at p + K + j; prefix and windows run into the K - 1 + M + E bytes that follow the block, the windows
//   into zeros beyond the stream's end (a prefix never does).
// stab_build_long_kernel is that form: a lane's 8 positions are prefix starts and every read goes forward.  Stage one compares the first
//   min(K, 8) prefix bytes in registers with the lane's 16 loaded bytes and gathers 8 verdicts into a bit mask; stage two loops over the set
//   bits only, compares the rest of the prefix (in LDS behind the bitmap) and hashes the E + 1 windows.
// Every kernel also has the block-list form (StabCommon::list: blocks of uneven sizes anywhere in a buffer, each with its own overlap behind it —
//   the chunks of a decoded stream, for a sidecar's tables): stab_share reads the block's place from the list, and nothing else differs.
// Both forms share stab_zero, stab_share, stab_positions, stab_mark and stab_flush (the zeroing of the bitmap, a workgroup's (part, slice, block)
//   and its positions, the slice-filtered bit and the write-out or merge); they stay kernels of their own: the short forms keep the bytes behind
//   the range in a register, the long form in LDS.
// The pre-folded block-list form (stab_build_kernel<*, true>, stab_build_long_kernel<true>, stab_reduce_fold_kernel; the batch Writer,
//   mlz_stream_batch.hip.inc): a table's size comes from the call's block size, and in a batch every stream's last block is short, often its
//   only one.  A block's record (StabFoldBlock) names r0 = search_prefold of the positions its length lets it index and its table's place:
//   the block gets a slot of 2^(B - r0 - 3) bytes, its workgroup zeroes, marks (bit h & (2^(B - r0) - 1)) and writes 2^(min(B - r0, 20) - 5)
//   words, a table that fits one slice uses slice 0 only (the grid stays one workgroup per (block, slice, part); the surplus ones return at
//   once), and the reduce starts at R = r0.  The same (table, R) as the full build: mlz_stream_search.h says why.
// stab_reduce_kernel: a workgroup per block counts the bits, applies the rules above fold by fold (search_reduce_rule's conditions) and leaves
//   the table compact at the front of its slot; 8 bytes per block (table bytes or 0, R) go to the host next to the sizes and CRCs.

namespace mlz {

constexpr uint32_t kStabSliceBits = 20, kStabThreads = 1024, kStabPerThread = 8;

// The block-list form (a sidecar's tables over the chunks of a decoded stream, mlz_stream_sidecar.hip.inc): block b lies at src + off, and
// `over` bytes of the stream that follow it (the next data chunk's first ones, cut at that chunk's length) lie behind its last byte; beyond them zeros
struct StabBlock { uint64_t off; uint32_t bytes, over; };
static_assert(sizeof(StabBlock) == 16, "a record shared with the host");
// The pre-folded form's record: the block is built folded r0 times, its table of 2^(B - r0 - 3) bytes lies tab_off bytes (a multiple of 32) into tabs
struct StabFoldBlock : StabBlock { uint32_t r0, pad; uint64_t tab_off; };
static_assert(sizeof(StabFoldBlock) == 32, "a record shared with the host");

// What every build kernel is told
struct StabCommon {
    const uint8_t* src;      // the range
    uint64_t len;            // its bytes
    uint32_t tail_n;         // how many bytes behind the range (the next range's first ones) exist (0: the range ends the stream)
    uint32_t bs, cnt, B, M, parts, slices;
    uint32_t* tabs;          // cnt tables of 2^B bits
    const StabBlock* list;   // nullptr: block b is src[b * bs ...) of the range; else the block-list form (len, bs and the tail are unused, tail_n is 0);
                             // the pre-folded kernels: an array of StabFoldBlock
};
struct StabArgs : StabCommon {
    uint64_t tail;           // the bytes behind the range, little-endian
    uint32_t mask[8];        // the prefix form: byte v is a prefix byte when mask[v >> 5] >> (v & 31) & 1
};

// A workgroup's bitmap in LDS: all 2^B bits, or its slice of 2^20
__device__ __forceinline__ uint32_t stab_words(const StabCommon& a) { return 1u << ((a.B < kStabSliceBits ? a.B : kStabSliceBits) - 5); }
__device__ __forceinline__ void stab_zero(uint32_t* bits, uint32_t words) {
    for (uint32_t i = threadIdx.x; i < words; i += kStabThreads) bits[i] = 0;
}
// The workgroup's share: part `part` of block b's positions, the bits of slice `slice`.  next: a block follows this one in the stream;
// end: where the bytes that can be read at src end for this block (the range's end; the list form: the end of the block's overlap)
struct StabShare { uint32_t part, slice, b, blen; uint64_t b0, end; bool next; };
template <bool kFold = false>
__device__ __forceinline__ StabShare stab_share(const StabCommon& a) {
    StabShare w;
    w.part = blockIdx.x % a.parts; w.slice = (blockIdx.x / a.parts) % a.slices; w.b = blockIdx.x / (a.parts * a.slices);
    if (kFold || a.list) {
        const StabBlock blk = kFold ? static_cast<const StabBlock&>(static_cast<const StabFoldBlock*>(a.list)[w.b]) : a.list[w.b];
        w.b0 = blk.off; w.blen = blk.bytes; w.end = blk.off + blk.bytes + blk.over; w.next = blk.over != 0;
        return w;
    }
    w.b0 = uint64_t(w.b) * a.bs;
    w.blen = uint32_t(a.len - w.b0 < a.bs ? a.len - w.b0 : a.bs);
    w.end = a.len;
    w.next = w.b + 1 < a.cnt || a.tail_n != 0;
    return w;
}
// [*p0, *p1): the part's positions of the block's npos, a multiple of a lane's 8 each
__device__ __forceinline__ void stab_positions(const StabCommon& a, uint32_t part, uint32_t npos, uint32_t* p0, uint32_t* p1) {
    const uint32_t per = ((npos + a.parts - 1) / a.parts + kStabPerThread - 1) & ~(kStabPerThread - 1);
    *p0 = part * per; *p1 = *p0 + per < npos ? *p0 + per : npos;
}
// bit h of the table, when it falls into this workgroup's slice
__device__ __forceinline__ void stab_mark(uint32_t* bits, uint32_t slice, uint32_t h) {
    if ((h >> kStabSliceBits) == slice) {
        const uint32_t x = h & ((1u << kStabSliceBits) - 1);
        atomicOr(&bits[x >> 5], 1u << (x & 31));
    }
}
// The pre-folded form, read from the block's record in front of everything else: the workgroup's bitmap words, the mask of a hash, where its
// slice of the table goes, and skip = the block's folded table has no such slice
struct StabFold { uint32_t words, mask; uint32_t* out; bool skip; };
__device__ __forceinline__ StabFold stab_fold(const StabCommon& a) {
    const uint32_t slice = (blockIdx.x / a.parts) % a.slices;
    const StabFoldBlock& blk = static_cast<const StabFoldBlock*>(a.list)[blockIdx.x / (a.parts * a.slices)];
    const uint32_t bits = a.B - blk.r0, lbits = bits < kStabSliceBits ? bits : kStabSliceBits;
    StabFold f;
    f.words = 1u << (lbits - 5); f.mask = (1u << bits) - 1;
    f.out = a.tabs + (blk.tab_off >> 2) + (size_t(slice) << (kStabSliceBits - 5));
    f.skip = slice >= (1u << (bits - lbits));
    return f;
}
// The bitmap to the block's table in HBM: written out, or, when several parts share the (zeroed) table, merged by its words that are not zero
__device__ __forceinline__ void stab_flush_to(uint32_t* out, uint32_t parts, const uint32_t* bits, uint32_t words);
__device__ __forceinline__ void stab_flush(const StabCommon& a, const StabShare& w, const uint32_t* bits, uint32_t words) {
    stab_flush_to(a.tabs + (size_t(w.b) << (a.B - 5)) + (size_t(w.slice) << (kStabSliceBits - 5)), a.parts, bits, words);
}
__device__ __forceinline__ void stab_flush_to(uint32_t* out, uint32_t parts, const uint32_t* bits, uint32_t words) {
    if (parts == 1) {
        for (uint32_t i = threadIdx.x; i < words; i += kStabThreads) out[i] = bits[i];
    } else {
        for (uint32_t i = threadIdx.x; i < words; i += kStabThreads) {
            const uint32_t v = bits[i];
            if (v) atomicOr(&out[i], v);
        }
    }
}

// byte q of the range, continued by the next range's first bytes and zeros (end: StabShare::end)
__device__ __forceinline__ uint64_t stab_byte(const StabArgs& a, uint64_t end, uint64_t q) {
    if (q < end) return a.src[q];
    const uint64_t over = q - end;
    return over < a.tail_n ? (a.tail >> (8 * over)) & 0xff : 0;
}

template <bool kPrefix, bool kFold = false>
__global__ __launch_bounds__(kStabThreads) void stab_build_kernel(const StabArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* bits = reinterpret_cast<uint32_t*>(smem);
    [[maybe_unused]] StabFold fold{};
    if constexpr (kFold) { fold = stab_fold(a); if (fold.skip) return; }
    const uint32_t tid = threadIdx.x, words = kFold ? fold.words : stab_words(a);
    stab_zero(bits, words);
    [[maybe_unused]] const uint32_t* pmask = bits + words;   // the prefix form: 32 bytes behind the bitmap
    if constexpr (kPrefix) { if (tid < 8) bits[words + tid] = a.mask[tid]; }
    __syncthreads();
    const StabShare w = stab_share<kFold>(a);
    const uint64_t b0 = w.b0;
    const uint32_t blen = w.blen;
    // positions [0, npos): every one with a next block, else those whose window lies inside the block.  The prefix form: position 0 is
    // never indexed (it belongs to the block before), position blen of a block with a next one is (its window lies in the next block)
    const uint32_t npos = kPrefix ? (w.next ? blen + 1 : (blen >= a.M ? blen - a.M + 1 : 0)) : (w.next ? blen : (blen >= a.M ? blen - a.M + 1 : 0));
    uint32_t p0, p1;
    stab_positions(a, w.part, npos, &p0, &p1);
    const uint32_t M = a.M, B = a.B;
    auto mark = [&](uint64_t v) { stab_mark(bits, w.slice, kFold ? search_hash(v, B, M) & fold.mask : search_hash(v, B, M)); };
    for (uint32_t i = p0 + tid * kStabPerThread; i < p1; i += kStabThreads * kStabPerThread) {
        // the prefix form reads from one byte in front of its first position (a part's first position looks at the part before it); the
        // block's first lane has no such byte and shifts a zero in, for position 0, which is skipped
        const uint32_t back = kPrefix && i ? 1 : 0;
        const uint64_t q = b0 + i - back;
        uint64_t lo, hi;
        if (q + 16 <= w.end) {
            __builtin_memcpy(&lo, a.src + q, 8);
            __builtin_memcpy(&hi, a.src + q + 8, 8);
        } else {
            lo = hi = 0;
            for (uint32_t j = 0; j < 8; j++) { lo |= stab_byte(a, w.end, q + j) << (8 * j); hi |= stab_byte(a, w.end, q + 8 + j) << (8 * j); }
        }
        if constexpr (kPrefix) {
            if (!back) { hi = (hi << 8) | (lo >> 56); lo <<= 8; }
            // bit j of todo: position i + j lies behind a prefix byte (byte j of lo).  Then one hash per set bit: a wave runs as many
            // rounds as its busiest lane has such positions, not 8 (a branch around the hash would run it in nearly every round: some
            // lane of the 64 almost always has a prefix byte at a given j)
            uint32_t todo = 0;
#pragma unroll
            for (uint32_t j = 0; j < kStabPerThread; j++) {
                const uint32_t pb = uint32_t(lo >> (8 * j)) & 0xff;
                todo |= ((pmask[pb >> 5] >> (pb & 31)) & 1) << j;
            }
            if (p1 - i < kStabPerThread) todo &= (1u << (p1 - i)) - 1;   // the part's last positions
            if (i == 0) todo &= ~1u;                                      // position 0 belongs to the block before
            for (; todo; todo &= todo - 1) {
                const uint32_t sh = 8 * (uint32_t(__builtin_ctz(todo)) + 1);   // the window starts one byte behind its prefix byte
                mark(sh < 64 ? (lo >> sh) | (hi << (64 - sh)) : hi);
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kStabPerThread; j++) {
                if (i + j >= p1) break;
                mark(j ? (lo >> (8 * j)) | (hi << (64 - 8 * j)) : lo);
            }
        }
    }
    __syncthreads();
    if constexpr (kFold) stab_flush_to(fold.out, a.parts, bits, words);
    else stab_flush(a, w, bits, words);
}

// The long-prefix form (table type 4).  The bytes behind the range (K - 1 + M + E at the most) and the prefix travel in the kernel arguments.
constexpr uint32_t kStabLongTail = 272;   // >= 255 + 16
struct StabLongArgs : StabCommon {
    uint32_t E, K;
    uint8_t pfx[kSearchMaxPrefix];
    uint8_t tail[kStabLongTail];   // the bytes behind the range
};

template <bool kFold = false>
__global__ __launch_bounds__(kStabThreads) void stab_build_long_kernel(const StabLongArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* bits = reinterpret_cast<uint32_t*>(smem);
    [[maybe_unused]] StabFold fold{};
    if constexpr (kFold) { fold = stab_fold(a); if (fold.skip) return; }
    const uint32_t tid = threadIdx.x, words = kFold ? fold.words : stab_words(a);
    stab_zero(bits, words);
    uint8_t* lpfx = smem + words * 4;            // the prefix and, behind it, the bytes that follow the range
    uint8_t* ltail = lpfx + kSearchMaxPrefix;
    if (tid < a.K) lpfx[tid] = a.pfx[tid];
    if (tid < kStabLongTail) ltail[tid] = tid < a.tail_n ? a.tail[tid] : 0;
    __syncthreads();
    const uint32_t M = a.M, B = a.B, E = a.E, K = a.K;
    const StabShare w = stab_share<kFold>(a);
    const uint64_t b0 = w.b0, end = w.end, real = end + a.tail_n;   // real: where the stream's bytes that this block can see end
    // prefix starts [0, npos): every position with a block behind, else those whose prefix and windows lie inside the block
    const uint32_t npos = w.next ? w.blen : (w.blen >= K + M + E ? w.blen - K - M - E + 1 : 0);
    uint32_t p0, p1;
    stab_positions(a, w.part, npos, &p0, &p1);
    auto byte_at = [&](uint64_t q) -> uint64_t {   // byte q of the range, continued by the bytes behind it and zeros
        if (q < end) return a.src[q];
        const uint64_t over = q - end;
        return over < kStabLongTail ? ltail[over] : 0;
    };
    auto load8 = [&](uint64_t q) -> uint64_t {
        uint64_t v = 0;
        if (q + 8 <= end) __builtin_memcpy(&v, a.src + q, 8);
        else for (uint32_t j = 0; j < 8; j++) v |= byte_at(q + j) << (8 * j);
        return v;
    };
    const uint32_t k8 = K < 8 ? K : 8;
    const uint64_t m8 = k8 == 8 ? ~uint64_t(0) : (uint64_t(1) << (8 * k8)) - 1;
    uint64_t p8 = 0;
    for (uint32_t j = 0; j < k8; j++) p8 |= uint64_t(lpfx[j]) << (8 * j);
    for (uint32_t i = p0 + tid * kStabPerThread; i < p1; i += kStabThreads * kStabPerThread) {
        const uint64_t q = b0 + i;
        const uint64_t lo = load8(q), hi = load8(q + 8);
        // bit j of todo: the prefix's first bytes stand at position i + j.  Then one round per set bit: a wave runs as many rounds as its
        // busiest lane has such positions
        uint32_t todo = 0;
#pragma unroll
        for (uint32_t j = 0; j < kStabPerThread; j++) {
            const uint64_t v = j ? (lo >> (8 * j)) | (hi << (64 - 8 * j)) : lo;
            todo |= uint32_t((v & m8) == p8) << j;
        }
        if (p1 - i < kStabPerThread) todo &= (1u << (p1 - i)) - 1;   // the part's last positions
        for (; todo; todo &= todo - 1) {
            const uint64_t s = q + uint32_t(__builtin_ctz(todo));
            if (s + K > real) continue;                               // a prefix does not run beyond the stream's end
            uint32_t t = 8;
            while (t < K && byte_at(s + t) == lpfx[t]) t++;
            if (t < K) continue;
            for (uint32_t e = 0; e <= E; e++) stab_mark(bits, w.slice, kFold ? search_hash(load8(s + K + e), B, M) & fold.mask : search_hash(load8(s + K + e), B, M));
        }
    }
    __syncthreads();
    if constexpr (kFold) stab_flush_to(fold.out, a.parts, bits, words);
    else stab_flush(a, w, bits, words);
}

// The rules over one table t of `words` words that was built folded R times (0: as the full kernels build it): *out = (table bytes or 0, R);
// the table of 2^(B - R) bits is left at the front of its slot.  (A pre-folded table is never dropped: it holds a quarter of 2^(B - 1) bits at the most.)
__device__ __forceinline__ void stab_reduce(uint32_t* __restrict__ t, uint32_t words, uint32_t R, uint32_t B, uint32_t fold_limit, uint2* __restrict__ out) {
    __shared__ uint32_t wsum[kStabThreads / 64];
    const uint32_t tid = threadIdx.x;
    // the workgroup's sum of `mine`
    auto total = [&](uint32_t mine) -> uint32_t {
        for (int o = 32; o; o >>= 1) mine += __shfl_down(mine, o);
        __syncthreads();
        if ((tid & 63) == 0) wsum[tid >> 6] = mine;
        __syncthreads();
        uint32_t s = 0;
        for (uint32_t w = 0; w < kStabThreads / 64; w++) s += wsum[w];
        return s;
    };
    uint32_t pop = 0;
    for (uint32_t i = tid; i < words; i += kStabThreads) pop += uint32_t(__popc(t[i]));
    pop = total(pop);
    if (search_table_dropped(pop, B)) {
        if (tid == 0) *out = make_uint2(0, 0);
        return;
    }
    while (words * 4 >= 64) {
        const uint32_t half = words >> 1;
        uint32_t p = 0;
        for (uint32_t i = tid; i < half; i += kStabThreads) p += uint32_t(__popc(t[i] | t[half + i]));
        p = total(p);
        if (!search_fold_accepted(p, uint64_t(half) * 32, fold_limit)) break;
        for (uint32_t i = tid; i < half; i += kStabThreads) t[i] |= t[half + i];
        __syncthreads();
        words = half; R++;
    }
    if (tid == 0) *out = make_uint2(words * 4, R);
}
// info[b] = block b's record, its table at the front of its slot of 2^(B - 3) bytes
__global__ __launch_bounds__(kStabThreads) void stab_reduce_kernel(uint32_t* __restrict__ tabs, uint32_t B, uint32_t fold_limit /* per cent */, uint2* __restrict__ info) {
    const uint32_t b = blockIdx.x;
    stab_reduce(tabs + (size_t(b) << (B - 5)), 1u << (B - 5), 0, B, fold_limit, info + b);
}
// The pre-folded form: block b's table of 2^(B - r0) bits lies where its record says
__global__ __launch_bounds__(kStabThreads) void stab_reduce_fold_kernel(uint32_t* __restrict__ tabs, const StabFoldBlock* __restrict__ list, uint32_t B, uint32_t fold_limit,
                                                                        uint2* __restrict__ info) {
    const uint32_t b = blockIdx.x;
    const StabFoldBlock blk = list[b];
    stab_reduce(tabs + (blk.tab_off >> 2), 1u << (B - blk.r0 - 5), blk.r0, B, fold_limit, info + b);
}

}  // namespace mlz

namespace {

// The launch both callers share: a.src, a.len / a.list, a.bs (the largest block), a.cnt, a.tail_n and a.tabs are set; `info` receives cnt records.
// fold: the pre-folded form — a.list names StabFoldBlock records, the launch's largest table has 2^fold->bits bits, all tables together fold->bytes bytes.
struct StabFoldLaunch { uint32_t bits; size_t bytes; };
int stab_launch(mlz_ctx* c, hipStream_t sm, mlz::StabCommon a, uint32_t T, const uint8_t* field, uint32_t M, uint32_t B, const uint8_t* tail, uint2* info,
                const StabFoldLaunch* fold = nullptr) {
    const size_t slot = size_t(1) << (B - 3), cnt = a.cnt;
    const uint32_t lbits = std::min(fold ? fold->bits : B, mlz::kStabSliceBits), lds = 1u << (lbits - 3);   // dynamic LDS: the launch's largest bitmap
    constexpr uint32_t kBitmap = 1u << (mlz::kStabSliceBits - 3), kLong = kBitmap + mlz::kSearchMaxPrefix + mlz::kStabLongTail;
    if (int r = raise_lds_once(c, c->stab_attr, Kernels{{mlz::stab_build_kernel<false>, kBitmap}, {mlz::stab_build_kernel<true>, kBitmap + 32}, {mlz::stab_build_long_kernel<false>, kLong},
                                                        {mlz::stab_build_kernel<false, true>, kBitmap}, {mlz::stab_build_kernel<true, true>, kBitmap + 32},
                                                        {mlz::stab_build_long_kernel<true>, kLong}})) return r;
    a.B = B; a.M = M;
    a.slices = 1u << ((fold ? fold->bits : B) - lbits);
    // few large blocks: parts of at least 64 KiB, until the device has about two workgroups per CU
    const uint64_t want = std::max<uint64_t>(1, uint64_t(2 * std::max(c->n_cus, 1)) / (cnt * a.slices));
    a.parts = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(want, a.bs >> 16)));
    if (a.parts > 1) HIPCHK(c, hipMemsetAsync(a.tabs, 0, fold ? fold->bytes : cnt * slot, sm));
    if (cnt * a.slices * a.parts > 0x7fffffffull) { c->err = "search tables: more workgroups than a launch takes"; return -MLZ_ERR_ARG; }
    const dim3 grid(uint32_t(cnt * a.slices * a.parts)), wg(mlz::kStabThreads);
    if (T == 4) {
        mlz::StabLongArgs la{};
        static_cast<mlz::StabCommon&>(la) = a;
        la.E = mlz::search_long_e(field); la.K = mlz::search_long_k(field);
        std::memcpy(la.pfx, mlz::search_long_prefix(field), la.K);
        if (a.tail_n) std::memcpy(la.tail, tail, a.tail_n);
        hipLaunchKernelGGL((fold ? mlz::stab_build_long_kernel<true> : mlz::stab_build_long_kernel<false>), grid, wg, lds + mlz::kSearchMaxPrefix + mlz::kStabLongTail, sm, la);
    } else {
        mlz::StabArgs sa{};
        static_cast<mlz::StabCommon&>(sa) = a;
        if (a.tail_n) std::memcpy(&sa.tail, tail, a.tail_n);
        if (T == 1) hipLaunchKernelGGL((fold ? mlz::stab_build_kernel<false, true> : mlz::stab_build_kernel<false>), grid, wg, lds, sm, sa);
        else {
            mlz::search_prefix_mask(T, field, sa.mask);
            hipLaunchKernelGGL((fold ? mlz::stab_build_kernel<true, true> : mlz::stab_build_kernel<true>), grid, wg, lds + 32, sm, sa);
        }
    }
    if (fold)
        hipLaunchKernelGGL(mlz::stab_reduce_fold_kernel, dim3(uint32_t(cnt)), dim3(mlz::kStabThreads), 0, sm, a.tabs, static_cast<const mlz::StabFoldBlock*>(a.list), B,
                           mlz::search_fold_limit(T), info);
    else hipLaunchKernelGGL(mlz::stab_reduce_kernel, dim3(uint32_t(cnt)), dim3(mlz::kStabThreads), 0, sm, a.tabs, B, mlz::search_fold_limit(T), info);
    return 0;
}

// Where a caller's own bytes start in c->d_stab behind the cnt slots and records of search_tables_build (whole 64-byte units)
size_t search_tables_extra_off(size_t cnt, uint32_t B) { return (cnt * (size_t(1) << (B - 3)) + cnt * sizeof(uint2) + 64 + 63) & ~size_t(63); }

// The tables of the cnt blocks of a range (len bytes at d_src), built and reduced on sm: c->d_stab then holds cnt slots of 2^(B - 3) bytes, each
// with its block's table at the front, and behind them (at *info_off) cnt records (table bytes or 0, R).  tail: the tail_n bytes that follow
// the range in the stream (the next range's first ones, StreamTables::overlap() at the most; host memory).  T, field: the table type and
// its prefix field.  Caller holds c->mu.
// The short forms take the first 8 of them, in a register.  They come as M - 1 (type 1) or M (types 2, 3) bytes: search_hash reads only the
// M low bytes of its argument, so zeros behind them give the bits that more of the stream's bytes would.  The kernels read "a block
// follows" from tail_n != 0: type 1 with M = 1 reaches no byte behind its block (tail_n is 0 there), and with or without a following block
// its blocks index all their blen positions.
int search_tables_build(mlz_ctx* c, hipStream_t sm, const uint8_t* d_src, size_t len, uint32_t bs, size_t cnt, uint32_t T, const uint8_t* field, uint32_t M, uint32_t B,
                        const uint8_t* tail, uint32_t tail_n, size_t* info_off, size_t extra = 0 /* bytes the caller wants behind the records, from search_tables_extra_off on */) {
    const size_t slot = size_t(1) << (B - 3);
    *info_off = cnt * slot;
    HIPCHK(c, c->d_stab.ensure(search_tables_extra_off(cnt, B) + extra));
    mlz::StabCommon a{};
    a.src = d_src; a.len = len; a.bs = bs; a.cnt = uint32_t(cnt);
    a.tail_n = std::min(tail_n, T == 4 ? mlz::kStabLongTail : 8u);
    a.tabs = c->d_stab.as<uint32_t>();
    return stab_launch(c, sm, a, T, field, M, B, tail, reinterpret_cast<uint2*>(c->d_stab.as<uint8_t>() + *info_off));
}

// The block-list form: the tables of the cnt blocks d_list names inside d_src (a decoded group in the scratch), of one configuration, to
// `tabs` (cnt slots of 2^(B - 3) bytes in c->d_stab, which the caller has sized) and their records to `info`.  max_block: the largest block.
int search_tables_build_list(mlz_ctx* c, hipStream_t sm, const uint8_t* d_src, const mlz::StabBlock* d_list, size_t cnt, uint32_t max_block, uint32_t T, const uint8_t* field,
                             uint32_t M, uint32_t B, uint32_t* tabs, uint2* info) {
    mlz::StabCommon a{};
    a.src = d_src; a.list = d_list; a.bs = max_block; a.cnt = uint32_t(cnt);
    a.tabs = tabs;
    return stab_launch(c, sm, a, T, field, M, B, nullptr, info);
}

// A block's record of the pre-folded form by the Writer's rule: the block of `bytes` bytes at d_src + off with `behind` bytes of its stream
// behind it (0: the stream's last block, which indexes only what lies inside it) sees min(overlap, behind) of them and zeros beyond, never
// another stream's bytes.  Its slot of 2^(B - r0 - 3) bytes starts at *tab_bytes, which moves on.
mlz::StabFoldBlock stab_fold_block(uint64_t off, uint32_t bytes, uint64_t behind, uint32_t T, const uint8_t* field, uint32_t M, uint32_t B, uint64_t* tab_bytes) {
    mlz::StabFoldBlock blk{};
    blk.off = off; blk.bytes = bytes;
    blk.over = uint32_t(std::min<uint64_t>(mlz::search_overlap(T, M, field), behind));
    blk.r0 = mlz::search_prefold(mlz::search_table_marks(T, M, field, bytes, behind != 0), B, mlz::search_fold_limit(T));
    blk.tab_off = *tab_bytes;
    *tab_bytes += uint64_t(1) << (B - blk.r0 - 3);
    return blk;
}

// The pre-folded block-list form: the tables of the cnt blocks d_list names inside d_src (records made by stab_fold_block, on the device), of
// one configuration, to `tabs` (tab_bytes bytes, which the caller has sized) and their records to `info`.  max_block: the largest block;
// min_r0: the smallest r0 of the list.
int search_tables_build_prefolded(mlz_ctx* c, hipStream_t sm, const uint8_t* d_src, const mlz::StabFoldBlock* d_list, size_t cnt, uint32_t max_block, uint32_t min_r0,
                                  uint64_t tab_bytes, uint32_t T, const uint8_t* field, uint32_t M, uint32_t B, uint32_t* tabs, uint2* info) {
    mlz::StabCommon a{};
    a.src = d_src; a.list = d_list; a.bs = max_block; a.cnt = uint32_t(cnt);
    a.tabs = tabs;
    const StabFoldLaunch fold{B - min_r0, size_t(tab_bytes)};
    return stab_launch(c, sm, a, T, field, M, B, nullptr, info, &fold);
}

}  // namespace
