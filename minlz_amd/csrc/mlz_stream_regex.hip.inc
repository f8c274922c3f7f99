// mlz_stream_regex.hip.inc — include/minlz_hip_regex.h: regular expressions compiled on the host (mlz_regex_compile.h) and
// mlz_dev_reader_grep_regex, the grep over the record index with its mark phase decided by the compiled automaton (included at the end of
// mlz_hip.hip, behind the grep, whose select and compact kernels it runs).  The rules are those of mlz_stream_regex.h, which the host check
// runs as plain loops.
//
//   longest   regex_longest_kernel, on the first call on an index: the maximum of end - start over the records, 8 bytes home, kept on the handle.
//             An index with a record beyond MLZ_REGEX_MAX_RECORD is refused here, before any chunk is decoded.
//   bounds    regex_bounds_kernel, a lane per decode group: the group's first and last record (two bisections), 16 bytes per group home: they size
//             the mark launches.
//   mark      every data chunk with bytes is decoded once, group by group into the scratch (scratch_decode_whole, the index build's list; its groups are the RegexGroups).  Per group
//             regex_mark_kernel: class map and table into LDS by 16-byte loads; a lane per record walks its bytes in 16-byte aligned blocks of the
//             scratch, a step being one add and one 16-bit LDS read (the class of each of a block's bytes is read in front of the chain); a lane
//             leaves its loop at dead or matched, a wavefront when no lane is left; the verdicts' ballot goes out as two words ORed into the
//             bitmap by lanes 0 and 32, and the one lane that runs into the group's end writes the carry.  A workgroup takes slices of 256
//             records in turn, so a large group loads the table kRegexMaxGrid times at the most.
//   select, compact   grep_select_compact (mlz_stream_grep.hip.inc, as are grep_enter and GrepWork).
// No kernel waits for another workgroup; the bitmap takes no atomics.  The table is looked up through the class map; a table indexed by the byte
// itself (S * 256 entries) was not built, so there is no measurement of it against this one.

#include "../../include/minlz_hip_regex.h"
#include "mlz_regex_compile.h"

static_assert(mlz::kRegexErrArg == MLZ_ERR_ARG && mlz::kRegexErrUnsupported == MLZ_ERR_UNSUPPORTED, "the compiler's codes are the ABI's");
static_assert(mlz::kRegexIgnoreCase == MLZ_REGEX_IGNORE_CASE && mlz::kRegexMaxRecord == MLZ_REGEX_MAX_RECORD, "mlz_stream_regex.h restates the header");

struct mlz_regex { mlz::RegexProgram prog; };

namespace mlz {

// *longest = max(*longest, the longest of records 0 .. k) (zeroed by the caller)
__global__ __launch_bounds__(kRegexLongestThreads) void regex_longest_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t size, uint64_t* __restrict__ longest) {
    __shared__ uint64_t lds[kRegexLongestThreads];
    const uint32_t tid = threadIdx.x;
    uint64_t mine = 0, most = 0;
    for (uint64_t j = uint64_t(blockIdx.x) * kRegexLongestThreads + tid; j <= k; j += uint64_t(gridDim.x) * kRegexLongestThreads) {
        const uint64_t l = regex_record_len([&](uint64_t i) { return D[i]; }, k, size, j);
        mine = l > mine ? l : mine;
    }
    wg_scan<kRegexLongestThreads>(mine, lds, tid, [](uint64_t x, uint64_t y) { return x > y ? x : y; }, &most);
    if (tid == 0 && most) atomicMax(reinterpret_cast<unsigned long long*>(longest), static_cast<unsigned long long>(most));
}

// bounds[g] = the records of group g, a lane per group
__global__ __launch_bounds__(64) void regex_bounds_kernel(const uint64_t* __restrict__ D, uint64_t k, const RegexGroup* __restrict__ groups, uint32_t ng, RegexBounds* __restrict__ bounds) {
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g < ng) bounds[g] = regex_bounds([&](uint64_t i) { return D[i]; }, k, groups[g]);
}

// What both mark kernels (this one and regex_mark_runs_kernel, mlz_stream_regex_prune.hip.inc) do around their lanes' rule.
// The class map and the table, image_bytes of them, into LDS by 16-byte loads
__device__ __forceinline__ void regex_load_image(uint4* lds, const uint4* __restrict__ image, uint32_t image_bytes, uint32_t tid) {
    for (uint32_t i = tid; i < image_bytes / 16; i += kRegexThreads) lds[i] = image[i];
}
// regex_walk_blocks over the bytes y in [from, to) of memory: al is a 16-byte boundary, the region [ylo, yhi) counts from it
__device__ __forceinline__ uint32_t regex_walk_memory(const uint16_t* next, const uint8_t* cmap, uint32_t C, const uint8_t* al, int64_t ylo, int64_t yhi, int64_t from, int64_t to, uint32_t state) {
    return regex_walk_blocks(next, cmap, C,
                             [&](int64_t y, uint32_t* v) { const uint4 x = *reinterpret_cast<const uint4*>(al + y); v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; },
                             [&](int64_t y) { return al[y]; }, ylo, yhi, from, to, state);
}
// The verdicts of a wavefront's 64 records, the first of which is r - lane, into the bitmap: the ballot's halves by lanes 0 and 32
__device__ __forceinline__ void regex_put_marks(uint32_t verdict, uint64_t r, uint32_t lane, uint32_t* __restrict__ sel, uint64_t W) {
    const uint64_t ballot = __ballot(verdict != 0);
    const uint32_t half = lane >> 5, bits = uint32_t(ballot >> (32 * half));
    const uint64_t w = regex_word(r - lane, half);
    if ((lane & 31) == 0 && bits && w < W) sel[w] |= bits;
}

// The group's bytes lie at base[0, g.n).  image: the class map and the table (image_bytes, a multiple of 16, at a 16-byte boundary).  in / out:
// the carry slots this group reads and writes.  sel: the bitmap, W words.
__global__ __launch_bounds__(kRegexThreads) void regex_mark_kernel(const uint8_t* __restrict__ base, RegexGroup g, uint64_t size, const uint64_t* __restrict__ D, uint64_t k, RegexBounds b,
                                                                   const uint4* __restrict__ image, uint32_t image_bytes, uint32_t C, uint32_t start, uint32_t end_hi,
                                                                   const RegexCarry* __restrict__ in, RegexCarry* __restrict__ out, uint32_t* __restrict__ sel, uint64_t W) {
    extern __shared__ uint4 regex_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    regex_load_image(regex_lds, image, image_bytes, tid);
    __syncthreads();
    const uint8_t* cmap = reinterpret_cast<const uint8_t*>(regex_lds);
    const uint16_t* next = reinterpret_cast<const uint16_t*>(cmap + 256);
    const int64_t mis = int64_t(reinterpret_cast<uintptr_t>(base) & 15), ylo = mis, yhi = mis + int64_t(g.n);
    const uint8_t* al = base - mis;
    const RegexCarry carried = *in;
    auto at = [&](uint64_t j) { return D[j]; };
    auto walk = [&](uint64_t from, uint64_t to, uint32_t state) { return regex_walk_memory(next, cmap, C, al, ylo, yhi, int64_t(from - g.first) + mis, int64_t(to - g.first) + mis, state); };
    const uint64_t slices = regex_slices(b);
    for (uint64_t s = blockIdx.x; s < slices; s += gridDim.x) {
        const uint64_t r = regex_lane_record(b, s * kRegexThreads + tid);
        uint32_t verdict = 0;
        if (r >= b.r_lo && r <= b.r_hi) {
            const RegexLaneOut o = regex_run_lane(at, k, size, g, r, carried, start, C, end_hi, walk);
            if (o.finished) verdict = o.verdict;
            else *out = o.carry;
        }
        regex_put_marks(verdict, r, lane, sel, W);
    }
}

}  // namespace mlz

namespace {

// The longest record of the handle's index, for both regex greps: the reduction into *d_longest (zeroed by the caller) where the handle does not
// know it yet; behind the caller's fetch regex_longest_keep; regex_longest_check refuses what no lane can walk, before any chunk is decoded.
void regex_longest_launch(mlz_dev_reader* rd, hipStream_t sm, uint64_t* d_longest) {
    const uint64_t items = rd->index_k + 1;
    const uint32_t grid = uint32_t(std::min<uint64_t>((items + mlz::kRegexLongestThreads - 1) / mlz::kRegexLongestThreads, 1024));
    hipLaunchKernelGGL(mlz::regex_longest_kernel, dim3(grid), dim3(mlz::kRegexLongestThreads), 0, sm, static_cast<const uint64_t*>(rd->d_index), rd->index_k, uint64_t(rd->size), d_longest);
}
void regex_longest_keep(mlz_dev_reader* rd, uint64_t longest) { rd->index_longest = longest; rd->index_longest_ready = true; }
int regex_longest_check(mlz_dev_reader* rd, const char* call) {
    if (rd->index_longest > uint64_t(rd->size)) { rd->ctx->err = std::string(call) + ": a record longer than the stream"; return -MLZ_ERR_HIP; }
    return rd->index_longest > MLZ_REGEX_MAX_RECORD ? -MLZ_ERR_UNSUPPORTED : 0;
}

int64_t dev_reader_grep_regex_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const mlz::RegexProgram& pr, uint64_t before, uint64_t after, const GrepOut& out,
                                     uint64_t* totals, uint64_t* stats) {
    mlz_ctx* c = rd->ctx;
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0;
    search_begin(rd, stats);
    grep_zero_totals(totals);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t N = rd->index_n, W = mlz::grep_words(N), size = uint64_t(rd->size);
    if (N == 0) return 0;
    ScratchDecode dec;
    mlz::WholeStreamList whole;
    int e = scratch_decode_whole(c, "mlz_dev_reader_grep_regex", rd->chunks, size, &dec, &whole);
    if (e) return e;
    const size_t nd = dec.jobs.size(), ng = dec.gend.size();
    std::vector<mlz::RegexGroup> groups(ng);
    for (size_t g = 0; g < ng; g++) { groups[g].first = whole.first[g]; groups[g].n = whole.bytes[g]; }
    const uint32_t image_bytes = pr.image_bytes();
    Carve cv, pin;   // workspace: the grep's (totals | marks, then S | C | the backward scan | ranks) | longest, bounds | groups | carry slots | image; pinned: the decode's | the same four
    GrepWork w;
    w.take(&cv, W);
    const auto r_home = cv.take<uint64_t>(2 + 2 * ng);   // the longest record (and a pad) | the bounds: what comes home in front of the decode
    const auto r_groups = cv.take<mlz::RegexGroup>(ng);
    const auto r_carry = cv.take<mlz::RegexCarry>(2);
    const auto r_image = cv.take<uint8_t>(image_bytes);
    if ((e = dec.take(c, rd->chunks, &pin))) return e;
    const auto h_home_r = pin.take<uint64_t>(2 + 2 * ng);
    const auto h_groups_r = pin.take<mlz::RegexGroup>(ng);
    const auto h_image_r = pin.take<uint8_t>(image_bytes);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
    void* ws = c->d_rplan.p;
    uint64_t *d_home = r_home.at(ws), *h_home = h_home_r.at(c->pinned2);
    mlz::RegexGroup *d_groups = r_groups.at(ws), *h_groups = h_groups_r.at(c->pinned2);
    mlz::RegexCarry* d_carry = r_carry.at(ws);
    uint8_t *d_image = r_image.at(ws), *h_image = h_image_r.at(c->pinned2);
    const uint64_t* D = static_cast<const uint64_t*>(rd->d_index);
    { WorkspaceOrder order(c, sm); }
    if ((e = w.clear(c, sm))) return e;
    HIPCHK(c, hipMemsetAsync(d_home, 0, 2 * sizeof(uint64_t), sm));
    HIPCHK(c, hipMemsetAsync(d_carry, 0xff, 2 * sizeof(mlz::RegexCarry), sm));   // (no record has that number)
    std::memcpy(h_groups, groups.data(), ng * sizeof(mlz::RegexGroup));
    pr.image(h_image);
    HIPCHK(c, hipMemcpyAsync(d_groups, h_groups, ng * sizeof(mlz::RegexGroup), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(d_image, h_image, image_bytes, hipMemcpyHostToDevice, sm));
    if (!rd->index_longest_ready) regex_longest_launch(rd, sm, d_home);
    mlz::RegexBounds* d_bounds = reinterpret_cast<mlz::RegexBounds*>(d_home + 2);
    hipLaunchKernelGGL(mlz::regex_bounds_kernel, dim3(uint32_t((ng + 63) / 64)), dim3(64), 0, sm, D, rd->index_k, static_cast<const mlz::RegexGroup*>(d_groups), uint32_t(ng), d_bounds);
    if ((e = fetch(c, sm, h_home, d_home, (2 + 2 * ng) * sizeof(uint64_t)))) return e;
    if (!rd->index_longest_ready) regex_longest_keep(rd, h_home[0]);
    if ((e = regex_longest_check(rd, "mlz_dev_reader_grep_regex"))) return e;   // (no chunk has been decoded)
    std::vector<mlz::RegexBounds> bounds(ng);
    std::memcpy(bounds.data(), h_home + 2, ng * sizeof(mlz::RegexBounds));   // (the decode reuses the pinned buffer)
    for (size_t g = 0; g < ng; g++) {
        const mlz::RegexBounds& b = bounds[g];
        if (b.r_lo > b.r_hi || b.r_hi >= N || (g && (b.r_lo < bounds[g - 1].r_hi || b.r_lo > bounds[g - 1].r_hi + 1))) {
            c->err = "mlz_dev_reader_grep_regex: a group's records do not fit the index";
            return -MLZ_ERR_HIP;
        }
    }
    const uint8_t* scratch = c->d_range.as<uint8_t>();
    c->search_chunks = nd;
    if (stats) stats[1] = nd;
    const int64_t r = dec.run(c, sm, ignore_crc, rd->d_src, rd->chunks, [&](size_t g) -> int {
        const uint32_t grid = uint32_t(std::min<uint64_t>(mlz::regex_slices(bounds[g]), mlz::kRegexMaxGrid));
        hipLaunchKernelGGL(mlz::regex_mark_kernel, dim3(grid), dim3(mlz::kRegexThreads), image_bytes, sm, scratch, groups[g], size, D, rd->index_k, bounds[g],
                           reinterpret_cast<const uint4*>(d_image), image_bytes, pr.C, pr.start, pr.end_hi, static_cast<const mlz::RegexCarry*>(d_carry + (g & 1)), d_carry + ((g + 1) & 1),
                           w.sel, W);
        return 0;
    });
    if (r < 0) return r;   // (nothing has been written to the caller's arrays)
    return grep_select_compact(rd, sm, "mlz_dev_reader_grep_regex", (flags & MLZ_GREP_INVERT) != 0, before, after, out, w, totals);
}

}  // namespace

extern "C" {

int mlz_regex_compile(const uint8_t* exprs, const uint32_t* expr_len, size_t n_exprs, uint32_t flags, mlz_regex** out, uint64_t* where) {
    if (!out) return -MLZ_ERR_ARG;
    *out = nullptr;
    mlz_regex* re = new (std::nothrow) mlz_regex;
    if (!re) return -MLZ_ERR_ARG;
    const int r = mlz::regex_compile(exprs, expr_len, n_exprs, flags, &re->prog, where);
    if (r) { delete re; return r; }
    *out = re;
    return 0;
}

void mlz_regex_free(mlz_regex* re) { delete re; }

int mlz_regex_info(const mlz_regex* re, uint64_t* info) {
    if (!re || !info) return -MLZ_ERR_ARG;
    info[0] = re->prog.S; info[1] = re->prog.C; info[2] = re->prog.image_bytes(); info[3] = re->prog.empty_ok ? 1 : 0;
    return 0;
}

int mlz_regex_test(const mlz_regex* re, const uint8_t* record, size_t len) {
    if (!re || (!record && len)) return -MLZ_ERR_ARG;
    return mlz::regex_test(re->prog, record, len);
}

int64_t mlz_dev_reader_grep_regex(mlz_dev_reader* rd, void* stream, uint32_t flags, const mlz_regex* re, uint64_t before, uint64_t after, uint64_t* d_rec_no, uint8_t* d_rec_kind,
                                  size_t rec_cap, uint64_t* totals, uint64_t* stats) {
    if (!rd || !re || (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC | MLZ_GREP_INVERT)) || (rec_cap && !d_rec_no)) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    GrepOut out;
    if (const int e = grep_enter(rd, [] { return true; }, d_rec_no, d_rec_kind, rec_cap, &out)) return e;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_grep_regex_locked(rd, sm, flags, re->prog, before, after, out, totals, stats));
}

}  // extern "C"
