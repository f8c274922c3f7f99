// mlz_stream_regex_prune.hip.inc — include/minlz_hip_regex_prune.h: mlz_regex_literals and mlz_dev_reader_grep_regex_pruned, the regex grep that
// decodes only what the block search tables admit for the expression's required literals (included at the end of mlz_hip.hip, behind the regex
// grep, whose longest-record and bounds kernels, carry and walk it runs).  The rules are those of mlz_stream_regex_prune.h, which the host check
// runs as plain loops.
//
//   longest   on the first call on an index regex_longest_kernel, 8 bytes home: a record beyond MLZ_REGEX_MAX_RECORD is refused in front of everything else.
//   plan      the literals without those that hold the delimiter go through dev_reader_search_plan as the patterns of a search for many: one byte
//             per chunk comes back.  No literals, MLZ_SEARCH_NO_TABLES, a set handle, a literal the tables do not serve, the case flag with a
//             letter as the delimiter: every chunk with bytes.  Literals that all hold the delimiter: no chunk, M is empty.
//   widen     regex_widen_kernel, a lane per taken chunk, when the plan left a chunk out: the span of the records that hold the chunk's first and
//             its last byte (two bisections each), 16 bytes per taken chunk home; the host adds every chunk that intersects a span (regex_widen_take).
//   decode    the widened list through ScratchDecode in groups (range_group_ends), a group's chunks side by side; regex_run_table says which
//             pieces of runs a group holds.  A group with more than kRegexMaxRuns pieces makes the call take every chunk (one run) instead.
//   mark      regex_mark_runs_kernel, one launch per group: regex_mark_kernel's lanes, word ownership and carry; the group's run table lies in
//             LDS behind the automaton's image, a lane finds its record's piece there by bisection and is idle unless a run holds the record
//             whole (regex_run_lane_of).  The walk is regex_walk_blocks over the group's used scratch.
//   select, compact   grep_select_compact.
// With every chunk taken the call is the unpruned one on one run per group: the same kernels, no threshold.

#include "../../include/minlz_hip_regex_prune.h"

namespace mlz {

// spans[i] = what the records of taken chunk i need, a lane per chunk
__global__ __launch_bounds__(kRegexWidenThreads) void regex_widen_kernel(const uint64_t* __restrict__ D, uint64_t k, uint64_t size, const RegexTaken* __restrict__ taken, uint32_t n,
                                                                         RegexWiden* __restrict__ spans) {
    const uint32_t i = blockIdx.x * kRegexWidenThreads + threadIdx.x;
    if (i < n) spans[i] = regex_widen([&](uint64_t j) { return D[j]; }, k, size, taken[i]);
}

// regex_mark_kernel for a group with holes: its bytes lie at base[0, used), piece j of runs[0, n_runs) at base + runs[j].at.  The launch's
// dynamic LDS holds the image and, behind it, the run table (n_runs * sizeof(RegexRun)).
__global__ __launch_bounds__(kRegexThreads) void regex_mark_runs_kernel(const uint8_t* __restrict__ base, uint64_t used, uint64_t size, const uint64_t* __restrict__ D, uint64_t k, RegexBounds b,
                                                                        const uint4* __restrict__ image, uint32_t image_bytes, uint32_t C, uint32_t start, uint32_t end_hi,
                                                                        const RegexCarry* __restrict__ in, RegexCarry* __restrict__ out, uint32_t* __restrict__ sel, uint64_t W,
                                                                        const uint64_t* __restrict__ runs, uint32_t n_runs, uint64_t head_first, uint64_t tail_end) {
    extern __shared__ uint4 regex_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    regex_load_image(regex_lds, image, image_bytes, tid);
    uint64_t* table = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(regex_lds) + image_bytes);
    for (uint32_t i = tid; i < n_runs * 3; i += kRegexThreads) table[i] = runs[i];
    __syncthreads();
    const uint8_t* cmap = reinterpret_cast<const uint8_t*>(regex_lds);
    const uint16_t* next = reinterpret_cast<const uint16_t*>(cmap + 256);
    const int64_t mis = int64_t(reinterpret_cast<uintptr_t>(base) & 15), ylo = mis, yhi = mis + int64_t(used);
    const uint8_t* al = base - mis;
    const RegexCarry carried = *in;
    auto at = [&](uint64_t j) { return D[j]; };
    auto run_at = [&](uint32_t j) { return RegexRun{table[3 * j], table[3 * j + 1], table[3 * j + 2]}; };
    const uint64_t slices = regex_slices(b);
    for (uint64_t s = blockIdx.x; s < slices; s += gridDim.x) {
        const uint64_t r = regex_lane_record(b, s * kRegexThreads + tid);
        uint32_t verdict = 0;
        if (r >= b.r_lo && r <= b.r_hi) {
            const RindexSpan sp = rindex_span(at, k, size, r);
            const RegexRunLane rl = regex_run_lane_of(run_at, n_runs, head_first, tail_end, sp.off, sp.off + sp.len);
            if (rl.active) {
                const RegexRun p = run_at(rl.piece);
                const int64_t shift = int64_t(p.at) - int64_t(p.first) + mis;   // a decoded position of the piece -> y
                const RegexLaneOut o = regex_lane_result(rl.lane, r, carried, start, C, end_hi, [&](uint64_t from, uint64_t to, uint32_t state) {
                    return regex_walk_memory(next, cmap, C, al, ylo, yhi, int64_t(from) + shift, int64_t(to) + shift, state);
                });
                if (o.finished) verdict = o.verdict;
                else *out = o.carry;
            }
        }
        regex_put_marks(verdict, r, lane, sel, W);
    }
}

}  // namespace mlz

namespace {

constexpr uint32_t kRegexRunsLds = mlz::kRegexLdsMax + mlz::kRegexMaxRuns * uint32_t(sizeof(mlz::RegexRun));   // the most a mark launch asks for
static_assert(kRegexRunsLds <= 160u << 10, "a workgroup's LDS");
static_assert(mlz::kRegexMaxLiteralLen == mlz::kSearchMaxPattern, "a literal is a pattern of the search");

int64_t dev_reader_grep_regex_pruned_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const mlz::RegexProgram& pr, uint64_t before, uint64_t after, const GrepOut& out,
                                            uint64_t* totals, uint64_t* stats) {
    const char* call = "mlz_dev_reader_grep_regex_pruned";
    mlz_ctx* c = rd->ctx;
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0, fold = (pr.flags & mlz::kRegexIgnoreCase) != 0;
    search_begin(rd, stats);
    grep_zero_totals(totals);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t N = rd->index_n, W = mlz::grep_words(N), size = uint64_t(rd->size);
    if (N == 0) return 0;
    const std::vector<StreamChunk>& chunks = rd->chunks;
    const size_t nck = chunks.size();
    const uint64_t* D = static_cast<const uint64_t*>(rd->d_index);
    int e = 0;

    // the longest record, on the first call on an index: 8 bytes home, and the refusal of what no lane can walk, before the plan and any decode
    if (!rd->index_longest_ready) {
        HIPCHK(c, c->d_rplan.ensure(2 * sizeof(uint64_t)));
        if ((e = ensure_stream_objects(c, 0, 64))) return e;
        uint64_t* d_longest = c->d_rplan.as<uint64_t>();
        { WorkspaceOrder order(c, sm); }
        HIPCHK(c, hipMemsetAsync(d_longest, 0, 2 * sizeof(uint64_t), sm));
        regex_longest_launch(rd, sm, d_longest);
        if ((e = fetch(c, sm, c->pinned2, d_longest, sizeof(uint64_t)))) return e;
        regex_longest_keep(rd, *static_cast<const uint64_t*>(c->pinned2));
    }
    if ((e = regex_longest_check(rd, call))) return e;

    // a. the plan: one byte per chunk
    std::vector<uint8_t> take(nck, 0);
    size_t n_take = 0, n_data = 0;
    for (size_t k = 0; k < nck; k++) n_data += chunks[k].n ? 1 : 0;
    const bool everything = pr.literals.empty() || (flags & MLZ_SEARCH_NO_TABLES) || (rd->set && !rd->tabled.on) || (fold && mlz::search_is_letter(rd->index_delim));
    if (everything) {
        for (size_t k = 0; k < nck; k++) take[k] = chunks[k].n ? 1 : 0;
        n_take = n_data;
    } else {
        std::vector<uint8_t> blob;   // the literals that can lie inside a record
        std::vector<uint32_t> off(1, 0);
        for (const std::string& l : pr.literals) {
            if (std::memchr(l.data(), rd->index_delim, l.size())) continue;
            blob.insert(blob.end(), l.begin(), l.end());
            off.push_back(uint32_t(blob.size()));
        }
        if (off.size() > 1) {
            const uint32_t plan_flags = (flags & MLZ_STREAM_IGNORE_CRC) | (fold ? uint32_t(MLZ_SEARCH_IGNORE_CASE) : 0u);
            const int64_t r = dev_reader_search_plan(rd, sm, plan_flags, blob.data(), off, off.size() - 1, &take, &n_take, nullptr, true, true);   // (record-bound)
            if (r) return r;
        }
    }
    const size_t n_planned = n_take;
    auto report = [&](size_t decoded) {
        c->search_chunks = decoded;
        if (stats) { stats[1] = decoded; stats[2] = c->search_tables; stats[3] = n_planned; }
    };
    report(0);

    // b. the widening, when the plan left a chunk with bytes out
    if (n_take > 0 && n_take < n_data) {
        Carve cv, pin;   // workspace and pinned: the spans | the taken chunks
        const size_t nw = n_take;
        const auto r_spans = cv.take<mlz::RegexWiden>(nw);
        const auto r_taken = cv.take<mlz::RegexTaken>(nw);
        const auto h_spans_r = pin.take<mlz::RegexWiden>(nw);
        const auto h_taken_r = pin.take<mlz::RegexTaken>(nw);
        HIPCHK(c, c->d_rplan.ensure(cv.bytes));
        if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
        mlz::RegexWiden *d_spans = r_spans.at(c->d_rplan.p), *spans = h_spans_r.at(c->pinned2);
        mlz::RegexTaken *d_taken = r_taken.at(c->d_rplan.p), *h_taken = h_taken_r.at(c->pinned2);
        { WorkspaceOrder order(c, sm); }
        {
            size_t i = 0;
            for (size_t k = 0; k < nck; k++) {
                if (!take[k]) continue;
                const uint64_t first = uint64_t(chunks[k].out_off), n = chunks[k].n;
                if (n == 0 || first >= size || n > size - first) { c->err = std::string(call) + ": a taken chunk lies outside the stream"; return -MLZ_ERR_HIP; }
                h_taken[i++] = mlz::RegexTaken{first, first + n - 1};
            }
            HIPCHK(c, hipMemcpyAsync(d_taken, h_taken, nw * sizeof(mlz::RegexTaken), hipMemcpyHostToDevice, sm));
            hipLaunchKernelGGL(mlz::regex_widen_kernel, dim3(uint32_t((nw + mlz::kRegexWidenThreads - 1) / mlz::kRegexWidenThreads)), dim3(mlz::kRegexWidenThreads), 0, sm, D, rd->index_k, size,
                               static_cast<const mlz::RegexTaken*>(d_taken), uint32_t(nw), d_spans);
        }
        if ((e = fetch(c, sm, spans, d_spans, nw * sizeof(mlz::RegexWiden)))) return e;
        {
            for (size_t i = 0; i < nw; i++)
                if (spans[i].start > spans[i].end || spans[i].end > size || (i && (spans[i].start < spans[i - 1].start || spans[i].end < spans[i - 1].end))) {
                    c->err = std::string(call) + ": the widened spans do not fit the index";
                    return -MLZ_ERR_HIP;
                }
            n_take = mlz::regex_widen_take(nck, [&](size_t k) { return uint64_t(chunks[k].out_off); }, [&](size_t k) { return uint64_t(chunks[k].n); }, spans, nw, &take);
        }
    }

    // c. the decode list, its groups and their pieces of runs; a group whose table does not fit takes the call to the list of every chunk
    ScratchDecode dec;
    mlz::RegexRunTable rt;
    for (int pass = 0; pass < 2; pass++) {
        dec = ScratchDecode();
        for (size_t k = 0; k < nck; k++) if (take[k]) dec.jobs.push_back(ChunkJob{k, nullptr});
        mlz::range_group_ends(dec.jobs.size(), [&](size_t i) { return uint64_t(chunks[dec.jobs[i].ck].n); }, &dec.gend);
        rt = mlz::regex_run_table(dec.jobs.size(), dec.gend, [&](size_t i) { return uint64_t(chunks[dec.jobs[i].ck].out_off); }, [&](size_t i) { return uint64_t(chunks[dec.jobs[i].ck].n); });
        bool fits = true;
        for (const mlz::RegexRunGroup& g : rt.groups) fits = fits && g.r1 - g.r0 <= mlz::kRegexMaxRuns;
        if (fits) break;
        for (size_t k = 0; k < nck; k++) take[k] = chunks[k].n ? 1 : 0;   // (contiguous chunks: one piece per group)
        n_take = n_data;
    }
    dec.at = rt.at;
    const size_t nd = dec.jobs.size(), ng = dec.gend.size(), nr = rt.runs.size();
    std::vector<mlz::RegexGroup> groups(ng);
    for (size_t g = 0; g < ng; g++) {
        const mlz::RegexRunGroup& gr = rt.groups[g];
        if (gr.r1 == gr.r0 || gr.r1 - gr.r0 > mlz::kRegexMaxRuns || rt.runs[gr.r1 - 1].end > size) { c->err = std::string(call) + ": a group's runs do not fit the stream"; return -MLZ_ERR_HIP; }
        groups[g] = mlz::RegexGroup{rt.runs[gr.r0].first, rt.runs[gr.r1 - 1].end - rt.runs[gr.r0].first};
    }
    const uint32_t image_bytes = pr.image_bytes();
    Carve cv, pin;   // workspace: the grep's | bounds | groups | carry slots | image | runs; pinned: the decode's | the same four without the carry
    GrepWork w;
    w.take(&cv, W);
    const auto r_bounds = cv.take<mlz::RegexBounds>(ng);
    const auto r_groups = cv.take<mlz::RegexGroup>(ng);
    const auto r_carry = cv.take<mlz::RegexCarry>(2);
    const auto r_image = cv.take<uint8_t>(image_bytes);
    const auto r_runs = cv.take<mlz::RegexRun>(nr);
    if ((e = dec.take(c, chunks, &pin))) return e;
    const auto h_bounds_r = pin.take<mlz::RegexBounds>(ng);
    const auto h_groups_r = pin.take<mlz::RegexGroup>(ng);
    const auto h_image_r = pin.take<uint8_t>(image_bytes);
    const auto h_runs_r = pin.take<mlz::RegexRun>(nr);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
    if ((e = raise_lds_once(c, c->regex_runs_attr, Kernels{{mlz::regex_mark_runs_kernel, kRegexRunsLds}}))) return e;
    void* ws = c->d_rplan.p;
    mlz::RegexBounds *d_bounds = r_bounds.at(ws), *h_bounds = h_bounds_r.at(c->pinned2);
    mlz::RegexGroup *d_groups = r_groups.at(ws), *h_groups = h_groups_r.at(c->pinned2);
    mlz::RegexCarry* d_carry = r_carry.at(ws);
    uint8_t *d_image = r_image.at(ws), *h_image = h_image_r.at(c->pinned2);
    mlz::RegexRun *d_runs = r_runs.at(ws), *h_runs = h_runs_r.at(c->pinned2);
    { WorkspaceOrder order(c, sm); }
    if ((e = w.clear(c, sm))) return e;
    std::vector<mlz::RegexBounds> bounds(ng);
    if (ng) {
        HIPCHK(c, hipMemsetAsync(d_carry, 0xff, 2 * sizeof(mlz::RegexCarry), sm));   // (no record has that number)
        std::memcpy(h_groups, groups.data(), ng * sizeof(mlz::RegexGroup));
        std::memcpy(h_runs, rt.runs.data(), nr * sizeof(mlz::RegexRun));
        pr.image(h_image);
        HIPCHK(c, hipMemcpyAsync(d_groups, h_groups, ng * sizeof(mlz::RegexGroup), hipMemcpyHostToDevice, sm));
        HIPCHK(c, hipMemcpyAsync(d_image, h_image, image_bytes, hipMemcpyHostToDevice, sm));
        HIPCHK(c, hipMemcpyAsync(d_runs, h_runs, nr * sizeof(mlz::RegexRun), hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(mlz::regex_bounds_kernel, dim3(uint32_t((ng + 63) / 64)), dim3(64), 0, sm, D, rd->index_k, static_cast<const mlz::RegexGroup*>(d_groups), uint32_t(ng), d_bounds);
        if ((e = fetch(c, sm, h_bounds, d_bounds, ng * sizeof(mlz::RegexBounds)))) return e;
        std::memcpy(bounds.data(), h_bounds, ng * sizeof(mlz::RegexBounds));   // (the decode reuses the pinned buffer)
        for (size_t g = 0; g < ng; g++) {
            const mlz::RegexBounds& b = bounds[g];
            if (b.r_lo > b.r_hi || b.r_hi >= N || (g && b.r_lo < bounds[g - 1].r_hi)) { c->err = std::string(call) + ": a group's records do not fit the index"; return -MLZ_ERR_HIP; }
        }
    }
    const uint8_t* scratch = c->d_range.as<uint8_t>();
    report(nd);
    if (nd) {
        const int64_t r = dec.run(c, sm, ignore_crc, rd->d_src, chunks, [&](size_t g) -> int {
            const mlz::RegexRunGroup& gr = rt.groups[g];
            const uint32_t n_runs = uint32_t(gr.r1 - gr.r0), lds = image_bytes + n_runs * uint32_t(sizeof(mlz::RegexRun));
            const uint32_t grid = uint32_t(std::min<uint64_t>(mlz::regex_slices(bounds[g]), mlz::kRegexMaxGrid));
            hipLaunchKernelGGL(mlz::regex_mark_runs_kernel, dim3(grid), dim3(mlz::kRegexThreads), lds, sm, scratch, gr.used, size, D, rd->index_k, bounds[g],
                               reinterpret_cast<const uint4*>(d_image), image_bytes, pr.C, pr.start, pr.end_hi, static_cast<const mlz::RegexCarry*>(d_carry + (g & 1)), d_carry + ((g + 1) & 1),
                               w.sel, W, reinterpret_cast<const uint64_t*>(d_runs + gr.r0), n_runs, gr.head_first, gr.tail_end);
            return 0;
        });
        if (r < 0) return r;   // (nothing has been written to the caller's arrays)
    }
    return grep_select_compact(rd, sm, call, (flags & MLZ_GREP_INVERT) != 0, before, after, out, w, totals);
}

}  // namespace

extern "C" {

int mlz_regex_literals(const mlz_regex* re, uint8_t* buf, size_t buf_cap, uint32_t* lens, size_t lens_cap, uint64_t* info) {
    if (!re || (buf_cap && !buf) || (lens_cap && !lens)) return -MLZ_ERR_ARG;
    const std::vector<std::string>& L = re->prog.literals;
    size_t at = 0, bytes = 0, shortest = 0;
    bool room = true;
    for (size_t i = 0; i < L.size(); i++) {
        if (i < lens_cap) lens[i] = uint32_t(L[i].size());
        room = room && L[i].size() <= buf_cap - at;   // whole strings only, and none behind one that did not fit
        if (room) { std::memcpy(buf + at, L[i].data(), L[i].size()); at += L[i].size(); }
        bytes += L[i].size();
        shortest = i == 0 || L[i].size() < shortest ? L[i].size() : shortest;
    }
    if (info) { info[0] = L.size(); info[1] = bytes; info[2] = shortest; info[3] = (re->prog.flags & mlz::kRegexIgnoreCase) ? 1 : 0; }
    return int(L.size());
}

int64_t mlz_dev_reader_grep_regex_pruned(mlz_dev_reader* rd, void* stream, uint32_t flags, const mlz_regex* re, uint64_t before, uint64_t after, uint64_t* d_rec_no, uint8_t* d_rec_kind,
                                         size_t rec_cap, uint64_t* totals, uint64_t* stats) {
    if (!rd || !re || (flags & ~uint32_t(MLZ_STREAM_IGNORE_CRC | MLZ_GREP_INVERT | MLZ_SEARCH_NO_TABLES)) || (rec_cap && !d_rec_no)) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    GrepOut out;
    if (const int e = grep_enter(rd, [] { return true; }, d_rec_no, d_rec_kind, rec_cap, &out)) return e;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_grep_regex_pruned_locked(rd, sm, flags, re->prog, before, after, out, totals, stats));
}

}  // extern "C"
