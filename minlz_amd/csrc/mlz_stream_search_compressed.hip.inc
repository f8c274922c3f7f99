// mlz_stream_search_compressed.hip.inc — compressed block search tables (chunk 0x46) on the read side (included in mlz_hip.hip in front of
// mlz_stream_search.hip.inc, whose per-handle locate step and the sidecar attach call cst_resolve).
//
// The locate kernels take a fitting 0x46 chunk as a CANDIDATE (SearchTab::pad = kSearchTabArena, off = the chunk's body, bytes = its
// length).  Once per handle and locate round cst_resolve expands the candidates into one arena the handle owns: the arena's layout is a
// prefix sum over 2^(B - R - 3) of the candidates; cst_parse_kernel (a lane per candidate) runs the shared parse (mlz_search_compressed.h)
// and leaves up to 16 job records per chunk; cst_expand_kernel (a wavefront per chunk) builds the chunk's decode tables in LDS and decodes,
// copies or fills the sub-blocks; the CRC pass then runs over the arena's bitmaps as it does over 0x45 bodies.  A candidate that fails the
// parse, the decode or the CRC is passed over through the caller's skip[] round.  What is left is a table like any other, its bytes at
// arena + off: search_plan_kernel selects the base by SearchTab::pad and probes as before.

namespace mlz {

struct CstItem { uint64_t src_off, arena_off; uint32_t clen, f, B, n; };   // a candidate: its body in the stream, its bitmap's place and size in the arena

__global__ __launch_bounds__(64) void cst_parse_kernel(const uint8_t* __restrict__ base, const CstItem* __restrict__ items, uint32_t m, CstPlan* __restrict__ plans) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= m) return;
    const CstItem it = items[i];
    CstPlan* pl = plans + i;   // (filled in place: the record is too large for registers)
    if (cst_parse(base + it.src_off, it.clen, it.f, it.B, pl) && pl->n != it.n) pl->ok = 0;   // (the arena was laid out for it.n bytes)
}

// One wavefront per chunk.  LDS: 16 decode tables of 2^11 two-byte entries (64 KiB), a description, its weights and its symbols' places.
// The weights of a description are decoded by one lane, its table is filled by all; then a lane per (sub-block, stream) decodes the
// tabled sub-blocks (at most 16 x 4 = 64 lanes), and the wavefront as a whole writes the raw and the repeated ones with 16-byte stores and
// walks the sparse ones 64 gap bytes a round.  arena + it.arena_off is 16-byte aligned: cst_resolve gives every bitmap whole 16-byte units
// (cst_arena_slot), and a bitmap is a power of two of at least 32 bytes (cst_fixed_fields).
// LDS in all: 66 736 bytes (the tables' 64 KiB, the description, weights, places, FSE scratch and logs), of the 160 KiB a workgroup may declare on gfx950.
__global__ __launch_bounds__(64) void cst_expand_kernel(const uint8_t* __restrict__ base, const CstItem* __restrict__ items, CstPlan* __restrict__ plans,
                                                        uint8_t* __restrict__ arena) {
    __shared__ uint16_t tabs[kCstMaxTables][kCstTableEntries];
    __shared__ uint16_t start[256];
    __shared__ uint8_t w[256];
    __shared__ uint32_t logs[kCstMaxTables];
    __shared__ uint8_t desc[132];          // a table description, copied in by all lanes: its one reader walks it byte by byte
    __shared__ CstFseScratch fse;
    __shared__ uint32_t bad;
    const uint32_t lane = threadIdx.x;
    const CstItem it = items[blockIdx.x];
    CstPlan* pl = plans + blockIdx.x;
    if (!pl->ok) return;
    const uint8_t* body = base + it.src_off;
    uint8_t* out = arena + it.arena_off;
    const uint32_t tc = pl->tc, nsub = pl->nsub, sub = 1u << pl->bs;
    if (lane == 0) bad = 0;
    for (uint32_t t = 0; t < tc; t++) {
        const uint32_t off = pl->tab_off[t], dlen = cst_desc_len(body + off, it.clen - off);   // (at most 129 bytes)
        __syncthreads();
        for (uint32_t i = lane; i < dlen; i += 64) desc[i] = body[off + i];
        __syncthreads();
        if (lane == 0) {
            const uint32_t log = cst_weights(desc, dlen, w, &fse);
            if (log) cst_table_starts(w, log, start);
            else bad = 1;
            logs[t] = log;
        }
        __syncthreads();
        if (logs[t]) cst_table_fill(w, start, logs[t], tabs[t], lane, 64);
    }
    __syncthreads();
    if (bad) { if (lane == 0) pl->ok = 0; return; }

    bool fail = false;
    {
        const uint32_t j = lane >> 2, q = lane & 3;
        if (j < nsub && pl->job[j].kind < 16) {
            const CstJob jb = pl->job[j];
            CstStream st;
            fail = !cst_stream_of(body + jb.src_off, jb.src_len, sub, q, &st) ||
                   !cst_decode_stream(body + jb.src_off + st.off, st.len, tabs[jb.table], logs[jb.table], out + jb.dst_off + st.dst_off, st.count);
        }
    }
    for (uint32_t j = 0; j < nsub; j++) {
        const CstJob jb = pl->job[j];
        if (jb.kind < 16) continue;
        uint8_t* dst = out + jb.dst_off;
        const uint8_t* src = body + jb.src_off;
        if (jb.kind == kCstRaw) {
            for (uint32_t i = lane * 16; i < sub; i += 64 * 16) {
                uint4 v;
                __builtin_memcpy(&v, src + i, 16);
                *reinterpret_cast<uint4*>(dst + i) = v;
            }
            continue;
        }
        const uint32_t x = jb.kind == kCstRle ? jb.rle * 0x01010101u : 0u;
        for (uint32_t i = lane * 16; i < sub; i += 64 * 16) *reinterpret_cast<uint4*>(dst + i) = uint4{x, x, x, x};
        if (jb.kind != kCstSparse) continue;
        __threadfence();   // the zeros are in place before a bit is set
        // byte i sets a bit when it is not 255, at (the sum of the bytes 0 .. i) + (the setting bytes in front of i)
        const uint32_t len = jb.src_len, nbits = sub * 8;
        uint32_t sum_base = 0, cnt_base = 0;
        for (uint32_t r = 0; r < len; r += 64) {
            const uint32_t i = r + lane;
            const uint32_t b = i < len ? src[i] : 0;
            const bool sets = i < len && b != 255;
            uint32_t s = b;
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(s, d);
                if (lane >= d) s += up;
            }
            const uint64_t m = __ballot(sets);
            const uint32_t pos = sum_base + s + cnt_base + uint32_t(__popcll(m & ((uint64_t(1) << lane) - 1)));
            if (sets) {
                if (pos >= nbits) fail = true;
                else atomicOr(reinterpret_cast<uint32_t*>(dst) + (pos >> 5), 1u << (pos & 31));
            }
            sum_base += __shfl(s, 63);
            cnt_base += uint32_t(__popcll(m));
        }
        if (len && src[len - 1] == 255) fail = true;
    }
    if (fail) bad = 1;
    __syncthreads();
    if (bad && lane == 0) pl->ok = 0;
}

}  // namespace mlz

namespace {

// A handle's table sets give up what they own on the device
void search_tables_release(mlz_dev_reader::SearchTables* st) {
    if (st->d_tabs) (void)hipFree(st->d_tabs);
    if (st->d_arena) (void)hipFree(st->d_arena);
    st->d_tabs = st->d_arena = nullptr;
    st->arena_bytes = 0;
}

// One locate round's 0x46 candidates among tabs (set s's table of chunk k at tabs[s * per_set + k], its configuration st->cfg[s]; d_base:
// the stream or the sidecar) -> tables in st->d_arena, by cst_settle's rule: off = the bitmap's place in the arena, bytes = its size; a
// candidate that is refused (parse, decode, or unless ignore_crc the CRC) gets skip[i]++ and *again = true: the caller locates once more
// (every round expands all of its candidates anew: a broken table costs one more expansion; broken tables are the rare case).  If the
// arena cannot be allocated the candidates count as no table.  Whenever a round without refusals had candidates, the tables as they now
// stand go up to d_tabs, which the locate kernel left with the candidates in it: the plan kernel never sees a candidate.
// Temporary device memory of its own (once per handle and round); synchronous on sm.  Caller holds c->mu.
int cst_resolve(mlz_ctx* c, hipStream_t sm, const uint8_t* d_base, mlz_dev_reader::SearchTables* st, std::vector<mlz::SearchTab>* tabs, size_t per_set, bool ignore_crc,
                std::vector<uint32_t>* skip, bool* again, void* d_tabs) {
    std::vector<mlz::CstItem> items;
    std::vector<size_t> who;
    std::vector<uint64_t> sizes, offs;
    uint64_t arena = 0;
    for (size_t i = 0; i < tabs->size(); i++) {
        const mlz::SearchTab& t = (*tabs)[i];
        if (t.R == mlz::kSearchNoTable || t.pad != mlz::kSearchTabArena) continue;
        const mlz::SearchConfig& cf = st->cfg[i / per_set];
        items.push_back(mlz::CstItem{t.off, arena, t.bytes, mlz::search_field_len(cf.T, cf.field), cf.B, 1u << (cf.B - t.R - 3)});
        who.push_back(i);
        sizes.push_back(items.back().n);
        offs.push_back(arena);
        arena += mlz::cst_arena_slot(sizes.back());
    }
    const size_t m = items.size();
    if (m == 0) return 0;
    auto publish = [&]() -> int {
        HIPCHK(c, hipMemcpyAsync(d_tabs, tabs->data(), tabs->size() * sizeof(mlz::SearchTab), hipMemcpyHostToDevice, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
        return 0;
    };
    if (arena > st->arena_bytes) {
        if (st->d_arena) (void)hipFree(st->d_arena);
        st->d_arena = nullptr;
        st->arena_bytes = 0;
        if (hipMalloc(&st->d_arena, arena) != hipSuccess) {   // without an arena these tables count as none: the search stays exact and decodes more
            (void)hipGetLastError();
            st->d_arena = nullptr;
            mlz::cst_settle(tabs, who, offs.data(), sizes.data(), nullptr, nullptr, skip);
            return publish();
        }
        st->arena_bytes = arena;
    }
    Carve cv;
    const auto r_items = cv.take<mlz::CstItem>(m);
    const auto r_plans = cv.take<mlz::CstPlan>(m);
    const auto r_crc = cv.take<uint32_t>(m);
    void* ws = nullptr;
    HIPCHK(c, hipMalloc(&ws, cv.bytes));
    struct Free { void* p; ~Free() { (void)hipFree(p); } } free_ws{ws};
    std::vector<mlz::CstPlan> plans(m);
    std::vector<uint32_t> crc(m), ok(m);
    uint8_t* d_arena = static_cast<uint8_t*>(st->d_arena);
    HIPCHK(c, hipMemcpyAsync(r_items.at(ws), items.data(), m * sizeof(mlz::CstItem), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::cst_parse_kernel, dim3(uint32_t((m + 63) / 64)), dim3(64), 0, sm, d_base, r_items.at(ws), uint32_t(m), r_plans.at(ws));
    hipLaunchKernelGGL(mlz::cst_expand_kernel, dim3(uint32_t(m)), dim3(64), 0, sm, d_base, r_items.at(ws), r_plans.at(ws), d_arena);
    int r = fetch(c, sm, plans.data(), r_plans.at(ws), m * sizeof(mlz::CstPlan));
    if (r) return r;
    if (!ignore_crc) {
        std::vector<mlz_block_desc> desc(m);
        for (size_t i = 0; i < m; i++) desc[i] = mlz_block_desc{items[i].arena_off, sizes[i], 0, 0};   // (a refused chunk's bytes are whatever the arena held)
        if ((r = crc_device_locked(c, sm, d_arena, desc.data(), int(m), r_crc.at(ws)))) return r;
        if ((r = fetch(c, sm, crc.data(), r_crc.at(ws), m * 4))) return r;
    }
    for (size_t i = 0; i < m; i++) ok[i] = plans[i].ok;
    if (mlz::cst_settle(tabs, who, offs.data(), sizes.data(), ok.data(), ignore_crc ? nullptr : crc.data(), skip)) { *again = true; return 0; }
    return publish();
}

}  // namespace

extern "C" int64_t mlz_search_table_expand(const uint8_t* body, size_t len, uint8_t* bitmap, size_t cap, uint32_t* out_R, uint32_t flags) {
    if (!body || (!bitmap && cap) || len > 0xffffffu || (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC))) return -MLZ_ERR_ARG;
    mlz::CstPlan plan;
    const int64_t n = mlz::cst_expand_host(body, uint32_t(len), bitmap, cap, &plan);
    if (n == 0) return -MLZ_ERR_CORRUPT;
    if (n < 0) return -MLZ_ERR_DST_TOO_SMALL;
    if (!(flags & MLZ_STREAM_IGNORE_CRC) && mlz::cst_crc_host(bitmap, size_t(n)) != plan.crc) return -MLZ_ERR_CRC;
    if (out_R) *out_R = plan.R;
    return n;
}
