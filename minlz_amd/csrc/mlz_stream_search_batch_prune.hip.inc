// mlz_stream_search_batch_prune.hip.inc — mlz_stream_search_batch_device_pruned: the search over a batch of streams in HBM, pruned by the
// streams' inline block search tables (included behind mlz_stream_search_batch.hip.inc, whose walk, passes and argument checks it shares).
//
// What the single-stream search does once per handle and once per call is done here for the whole batch in a few launches, and the result is
// one byte per data chunk: the job list of stream_search_batch_pass.  Everything behind that list — the virtual positions, the layout, the
// scratch decode, search_many_kernel, the mark-streams mode, search_batch_finish_kernel, the second pass — runs as it does without the plan.
//   search_batch_info_kernel    a lane per stream hops to the stream's info chunk (0x44) and leaves a key of 16 bytes (mlz::BatchInfoKey) and,
//                               on the device, where the payload lies.  The host numbers the distinct keys in descriptor order
//                               (mlz::batch_assign_classes); the first kSidecarMaxConfigs classes prune, and search_batch_rep_kernel
//                               gathers their first streams' info payloads, which come home once per class.
//   search_batch_class_kernel   a lane per stream compares its info payload with its class's configuration byte for byte: the key holds a
//                               hash of the prefix field, and a collision must never prune.
//   search_batch_locate_kernel  a lane per data chunk of the batch: search_locate_kernel's hop with the stream's class configuration; the first
//                               chunk of a stream hops from the stream's first byte.  0x46 chunks are stepped over: the call owns no handle that
//                               could keep their expansion, which costs more than the decode it would save (DESIGN.md §4).
//   the CRC rounds              stay on the device: search_batch_crc_desc_kernel turns the located tables into the CRC pass's block
//                               records and tile map, the pass (crc_device_described, the launching half of crc_device_locked) checks the
//                               tables of all streams in one launch per round, and search_batch_crc_settle_kernel compares: a stale table is
//                               passed over (skip[k]++) for the next fitting one in the round that follows, which locates and checks only
//                               the chunks that changed.  One word per round comes home: the tiles to check, 0 when the rounds are over.
//   search_batch_plan_kernel    a lane per (data chunk, pattern): the probes and the rule of mlz_stream_search.h inside the chunk's own stream
//                               (mlz::batch_plan_mark); a stream that is decoded whole is marked without probing.
//   search_batch_pack_kernel    a lane per data chunk: bit 0 = taken, bit 1 = has a usable table; the one byte per chunk that comes home.
// A class serves the call when its configuration gives every pattern a window (mlz::batch_class_patterns, as dev_reader_search_plan decides
// for one stream); the streams of a class that does not are decoded whole, as are streams without a usable info chunk.

#include "mlz_stream_search_batch_prune.h"

namespace mlz {

__global__ __launch_bounds__(64) void search_batch_info_kernel(const uint8_t* __restrict__ src, const BatchPlanStream* __restrict__ st, uint32_t n, BatchInfoKey* __restrict__ keys,
                                                               uint64_t* __restrict__ at) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint64_t a = 0;
    keys[i] = st[i].mode == kBatchPlanSkip ? BatchInfoKey{0, 0, 0, 0, 0, 0, 0} : batch_info_key(src, st[i].start, st[i].limit, &a);
    at[i] = a;
}

// A workgroup per class: the info payload of the class's first stream into the class's slot of kBatchPayloadSlot bytes
struct BatchReps { uint32_t stream[kSidecarMaxConfigs]; };
__global__ __launch_bounds__(64) void search_batch_rep_kernel(const uint8_t* __restrict__ src, const BatchInfoKey* __restrict__ keys, const uint64_t* __restrict__ at, BatchReps reps,
                                                              uint8_t* __restrict__ payload) {
    const uint32_t i = reps.stream[blockIdx.x], bytes = 3u + keys[i].flen;
    for (uint32_t j = threadIdx.x; j < kBatchPayloadSlot; j += 64) payload[blockIdx.x * kBatchPayloadSlot + j] = j < bytes ? src[at[i] + j] : 0;
}

// same[i] = 1: stream i's info payload is its class's configuration, byte for byte
__global__ __launch_bounds__(64) void search_batch_class_kernel(const uint8_t* __restrict__ src, const BatchInfoKey* __restrict__ keys, const uint64_t* __restrict__ at,
                                                                const uint8_t* __restrict__ cls, const SearchConfig* __restrict__ cfg, uint32_t n, uint8_t* __restrict__ same) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint8_t c = cls[i];
    same[i] = c != kBatchNoClass && keys[i].ok && batch_class_same(src + at[i], keys[i].flen, cfg[c]) ? 1 : 0;
}

// redo[k] != 0: chunk k is located in this round (the first round: every chunk; later: those whose table the round before found stale)
__global__ __launch_bounds__(64) void search_batch_locate_kernel(const uint8_t* __restrict__ src, const SearchHop* __restrict__ hop, const uint32_t* __restrict__ skip,
                                                                 const uint8_t* __restrict__ redo, const uint32_t* __restrict__ chunk_stream, const BatchPlanStream* __restrict__ st,
                                                                 const SearchConfig* __restrict__ cfg, uint32_t nck, SearchTab* __restrict__ tabs) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nck || !redo[k]) return;
    const BatchPlanStream s = st[chunk_stream[k]];
    tabs[k] = s.mode == kBatchPlanPrune ? batch_locate(src, hop[k].from, hop[k].limit, skip[k], cfg[s.cls]) : SearchTab{0, 0, kSearchNoTable, 0, 0};
}

// One workgroup: the tables this round checks (redo[k] and a table in front of chunk k) as the CRC pass's blocks — blocks[k] for every chunk,
// of no bytes and no tiles where there is nothing to check —, the tile map, and *total = the tiles of all of them.  A table has at most
// 2^20 bytes: 32 tiles.
__global__ __launch_bounds__(1024) void search_batch_crc_desc_kernel(const SearchTab* __restrict__ tabs, const uint8_t* __restrict__ redo, uint32_t nck, BlockInfo* __restrict__ blocks,
                                                                     uint32_t* __restrict__ tile_block, uint32_t tile_room, uint32_t* __restrict__ total) {
    __shared__ uint32_t lds[1024];
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nck; base += 1024) {
        const uint32_t k = base + tid;
        SearchTab t{0, 0, kSearchNoTable, 0, 0};
        uint32_t nt = 0;
        if (k < nck && redo[k]) {
            t = tabs[k];
            if (t.R != kSearchNoTable) nt = (t.bytes + kTile - 1) >> kTileLog;
        }
        uint32_t sum = 0;
        const uint32_t first = carry + wg_scan<1024>(nt, lds, tid, [](uint32_t x, uint32_t y) { return x + y; }, &sum);
        if (first + nt > tile_room) nt = 0;   // (never: the room is the host's bound over the spans the tables lie in)
        if (k < nck) {
            blocks[k] = BlockInfo{nt ? t.off : 0, nt ? t.bytes : 0, 0, 0, first, nt, 0, 0, 0};
            for (uint32_t j = 0; j < nt; j++) tile_block[first + j] = k;
        }
        carry += sum;
    }
    if (tid == 0) *total = carry < tile_room ? carry : tile_room;
}

// A lane per chunk: the CRC the pass computed against the one the table's chunk states.  A stale table is passed over in the next round
// (skip[k]++, redo[k] stays set); in the last round the traffic bound pays for (last != 0) it counts as no table.  Every other chunk is settled.
__global__ __launch_bounds__(256) void search_batch_crc_settle_kernel(SearchTab* __restrict__ tabs, const uint32_t* __restrict__ crc, const BlockInfo* __restrict__ blocks,
                                                                      uint8_t* __restrict__ redo, uint32_t* __restrict__ skip, uint32_t nck, uint32_t last) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nck || !redo[k]) return;
    const bool bad = blocks[k].n_tiles && crc[k] != tabs[k].crc;
    redo[k] = bad && !last ? 1 : 0;
    if (bad && !last) skip[k]++;
    if (bad && last) tabs[k].R = kSearchNoTable;
}

// pats[c * np + p]: pattern p as class c sees it; its hashes lie in the call's one array (under kFold: its offsets in voff).  bits[c]: B of class c.
struct BatchPlanBits { uint32_t B[kSidecarMaxConfigs]; };
template <bool kFold>
__global__ __launch_bounds__(256) void search_batch_plan_kernel(const uint8_t* __restrict__ src, const SearchTab* __restrict__ tabs, const uint64_t* __restrict__ n_of,
                                                                const uint32_t* __restrict__ chunk_stream, const BatchPlanStream* __restrict__ st, uint32_t nck, BatchPlanBits bits,
                                                                const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ voff, const SearchManyPat* __restrict__ pats,
                                                                uint32_t np, uint8_t* __restrict__ take) {
    const uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= uint64_t(nck) * np) return;
    const uint32_t k = uint32_t(idx % nck), p = uint32_t(idx / nck);
    const BatchPlanStream s = st[chunk_stream[k]];
    auto sizes = [&](size_t j) { return n_of[j]; };
    if (s.mode != kBatchPlanPrune) {   // decoded whole (one lane per chunk says so), or not searched
        if (p == 0) batch_plan_mark(k, s, SearchManyPat{0, 0, 1, 1, 1, 0}, [](size_t, bool) { return 0u; }, sizes, take);
        return;
    }
    const SearchManyPat pt = pats[size_t(s.cls) * np + p];
    const uint32_t B = bits.B[s.cls];
    auto probe = [&](size_t j, bool lead) {
        const SearchTab t = tabs[j];
        uint32_t a = pt.nw, sv = pt.nw;
        if (t.R != kSearchNoTable) {
            if (kFold) search_probe_fold(src + t.off, B - t.R, voff + pt.h_off, hashes, pt.nw, &a, &sv, pt.gsize);
            else search_probe(src + t.off, B - t.R, hashes + pt.h_off, pt.nw, &a, &sv, pt.gsize);
        }
        return lead ? a : sv;
    };
    batch_plan_mark(k, s, pt, probe, sizes, take);
}

__global__ __launch_bounds__(256) void search_batch_pack_kernel(const uint8_t* __restrict__ take, const SearchTab* __restrict__ tabs, uint32_t nck, uint8_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < nck) out[k] = uint8_t(take[k] | (tabs[k].R != kSearchNoTable ? 2 : 0));
}

}  // namespace mlz

namespace {

// The plan of the pruned call: take[k] per chunk of the walk, and the call's stats 4 .. 7
struct SearchBatchPlan {
    std::vector<uint8_t> take;
    uint64_t tabbed = 0, skipped = 0, classes = 0, whole = 0;
    uint64_t home = 0;   // bytes the plan brought to the host, the classes' configurations apart (mlz_get_counter 16)
};

int64_t stream_search_batch_plan(mlz_ctx* c, hipStream_t sm, bool ignore_crc, const uint8_t* d_src, const mlz_block_desc* streams, const BatchWalk& bw, size_t n,
                                 const SearchManyScan& scan, SearchBatchPlan* plan) {
    const size_t nck = bw.chunks.size(), np = scan.n;
    plan->take.assign(nck, 0);
    auto n_of = [&](size_t k) { return uint64_t(bw.chunks[k].n); };
    std::vector<mlz::BatchPlanStream> st(n);
    std::vector<uint8_t> part(n), tabbed(nck, 0);
    for (size_t i = 0; i < n; i++) {
        part[i] = bw.parsed[i] >= 0 ? 1 : 0;
        const uint64_t start = streams[i].src_off;
        st[i] = mlz::BatchPlanStream{start, bw.c1[i] > bw.c0[i] ? uint64_t(bw.chunks[bw.c0[i]].body_off) : start + streams[i].src_len, uint32_t(bw.c0[i]), uint32_t(bw.c1[i]),
                                     part[i] ? mlz::kBatchPlanWhole : mlz::kBatchPlanSkip, 0};
    }
    auto finish = [&]() {
        mlz::batch_prune_stats(st.data(), n, plan->take.data(), tabbed.data(), n_of, &plan->tabbed, &plan->skipped, &plan->whole);
        return 0;
    };
    auto all_whole = [&]() {   // no stream prunes: the unpruned call's job list, and no launch
        for (size_t i = 0; i < n; i++)
            for (size_t k = bw.c0[i]; part[i] && k < bw.c1[i]; k++) plan->take[k] = bw.chunks[k].n ? 1 : 0;
        return finish();
    };
    if (nck == 0) return finish();
    if ((uint64_t(nck) * np + 255) / 256 > 0x7fffffffull) return all_whole();   // (more lanes than one launch has workgroups for: no plan)

    // ---- the keys, the classes and their configurations ----
    const uint32_t nwg = uint32_t((n + 63) / 64);
    Carve ca;
    const auto a_st = ca.take<mlz::BatchPlanStream>(n);
    const auto a_keys = ca.take<mlz::BatchInfoKey>(n);
    const auto a_at = ca.take<uint64_t>(n);
    const auto a_cfg = ca.take<mlz::SearchConfig>(mlz::kSidecarMaxConfigs);
    const auto a_pay = ca.take<uint8_t>(mlz::kSidecarMaxConfigs * mlz::kBatchPayloadSlot);
    const auto a_cls = ca.take<uint8_t>(n), a_same = ca.take<uint8_t>(n);
    HIPCHK(c, c->d_rplan.ensure(ca.bytes));
    int e = ensure_stream_objects(c, 0, std::max<size_t>(n * sizeof(mlz::BatchInfoKey), mlz::kSidecarMaxConfigs * mlz::kBatchPayloadSlot));
    if (e) return e;
    void* ws = c->d_rplan.p;
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(a_st.at(ws), st.data(), n * sizeof(mlz::BatchPlanStream), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_batch_info_kernel, dim3(nwg), dim3(64), 0, sm, d_src, a_st.at(ws), uint32_t(n), a_keys.at(ws), a_at.at(ws));
    if ((e = fetch(c, sm, c->pinned2, a_keys.at(ws), n * sizeof(mlz::BatchInfoKey)))) return e;
    plan->home += n * sizeof(mlz::BatchInfoKey);
    const std::vector<mlz::BatchInfoKey> keys(static_cast<const mlz::BatchInfoKey*>(c->pinned2), static_cast<const mlz::BatchInfoKey*>(c->pinned2) + n);
    std::vector<uint8_t> cls(n);
    size_t rep[mlz::kSidecarMaxConfigs] = {};
    plan->classes = mlz::batch_assign_classes(keys.data(), part.data(), n, cls.data(), rep);
    const uint32_t ncls = uint32_t(std::min<uint64_t>(plan->classes, mlz::kSidecarMaxConfigs));
    if (!ncls) return all_whole();
    // a class's full configuration: gathered on the device, fetched once per class (one copy for all of them)
    mlz::BatchReps reps{};
    for (uint32_t k = 0; k < ncls; k++) reps.stream[k] = uint32_t(rep[k]);
    hipLaunchKernelGGL(mlz::search_batch_rep_kernel, dim3(ncls), dim3(64), 0, sm, d_src, a_keys.at(ws), a_at.at(ws), reps, a_pay.at(ws));
    if ((e = fetch(c, sm, c->pinned2, a_pay.at(ws), size_t(ncls) * mlz::kBatchPayloadSlot))) return e;
    std::vector<mlz::SearchConfig> cfg(mlz::kSidecarMaxConfigs);
    for (uint32_t k = 0; k < ncls; k++) {
        std::memset(&cfg[k], 0, sizeof(mlz::SearchConfig));
        cfg[k].ok = mlz::search_info(static_cast<const uint8_t*>(c->pinned2) + k * mlz::kBatchPayloadSlot, 3u + keys[rep[k]].flen, &cfg[k].T, &cfg[k].M, &cfg[k].B, cfg[k].field) ? 1 : 0;
    }
    HIPCHK(c, hipMemcpyAsync(a_cfg.at(ws), cfg.data(), cfg.size() * sizeof(mlz::SearchConfig), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(a_cls.at(ws), cls.data(), n, hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_batch_class_kernel, dim3(nwg), dim3(64), 0, sm, d_src, a_keys.at(ws), a_at.at(ws), a_cls.at(ws), a_cfg.at(ws), uint32_t(n), a_same.at(ws));
    if ((e = fetch(c, sm, c->pinned2, a_same.at(ws), n))) return e;
    plan->home += n;
    const std::vector<uint8_t> same(static_cast<const uint8_t*>(c->pinned2), static_cast<const uint8_t*>(c->pinned2) + n);

    // ---- every class's view of the patterns ----
    std::vector<uint32_t> hs, voff;
    std::vector<mlz::SearchManyPat> pats(size_t(ncls) * np);
    bool served[mlz::kSidecarMaxConfigs] = {};
    for (uint32_t k = 0; k < ncls; k++)
        served[k] = cfg[k].ok && mlz::batch_class_patterns(cfg[k], scan.patterns, scan.index.off.data(), np, scan.fold, pats.data() + size_t(k) * np, &hs, &voff);
    bool any = false;
    for (size_t i = 0; i < n; i++)
        if (part[i] && cls[i] != mlz::kBatchNoClass && same[i] && served[cls[i]]) { st[i].mode = mlz::kBatchPlanPrune; st[i].cls = cls[i]; any = true; }
    if (!any) return all_whole();

    // ---- the tables of every data chunk, the CRC rounds, the plan ----
    std::vector<mlz::SearchHop> hop(nck, mlz::SearchHop{0, 0});
    std::vector<uint32_t> chunk_stream(nck, 0);
    uint64_t tile_room = 0;   // the most tiles the tables can have: a table lies between its chunk's `from` and `limit`
    std::vector<uint64_t> sizes(nck);
    for (size_t i = 0; i < n; i++)
        for (size_t k = bw.c0[i]; k < bw.c1[i]; k++) {
            chunk_stream[k] = uint32_t(i);
            hop[k] = mlz::SearchHop{k == bw.c0[i] ? st[i].start : uint64_t(bw.chunks[k - 1].body_off + bw.chunks[k - 1].body_len), uint64_t(bw.chunks[k].body_off)};
            if (st[i].mode == mlz::kBatchPlanPrune) tile_room += (hop[k].limit - hop[k].from + mlz::kTile - 1) >> mlz::kTileLog;
        }
    if (tile_room > 0x7fffffffull || nck > 0x7fffffffull) return all_whole();   // (the CRC pass counts tiles and blocks in 31 bits)
    for (size_t k = 0; k < nck; k++) sizes[k] = bw.chunks[k].n;
    // (plan streams | configurations | hops | chunk streams | sizes | hashes | offsets | pattern records go up as ONE block)
    Carve up;
    const auto b_st = up.take<mlz::BatchPlanStream>(n);
    const auto b_cfg = up.take<mlz::SearchConfig>(mlz::kSidecarMaxConfigs);
    const auto b_hop = up.take<mlz::SearchHop>(nck);
    const auto b_cs = up.take<uint32_t>(nck);
    const auto b_n = up.take<uint64_t>(nck);
    const auto b_hs = up.take<uint32_t>(hs.size() + 1), b_voff = up.take<uint32_t>(voff.size() + 1);
    const auto b_pats = up.take<mlz::SearchManyPat>(pats.size());
    std::vector<uint8_t> block(up.bytes, 0);
    std::memcpy(b_st.at(block.data()), st.data(), n * sizeof(mlz::BatchPlanStream));
    std::memcpy(b_cfg.at(block.data()), cfg.data(), cfg.size() * sizeof(mlz::SearchConfig));
    std::memcpy(b_hop.at(block.data()), hop.data(), nck * sizeof(mlz::SearchHop));
    std::memcpy(b_cs.at(block.data()), chunk_stream.data(), nck * 4);
    std::memcpy(b_n.at(block.data()), sizes.data(), nck * 8);
    if (!hs.empty()) std::memcpy(b_hs.at(block.data()), hs.data(), hs.size() * 4);
    if (!voff.empty()) std::memcpy(b_voff.at(block.data()), voff.data(), voff.size() * 4);
    std::memcpy(b_pats.at(block.data()), pats.data(), pats.size() * sizeof(mlz::SearchManyPat));
    Carve cb;
    const auto r_up = cb.take<uint8_t>(up.bytes);
    const auto b_skip = cb.take<uint32_t>(nck), b_crc = cb.take<uint32_t>(nck), b_tb = cb.take<uint32_t>(size_t(tile_room) + 1), b_total = cb.take<uint32_t>(4);
    const auto b_tabs = cb.take<mlz::SearchTab>(nck);
    const auto b_blocks = cb.take<mlz::BlockInfo>(nck);
    const auto b_take = cb.take<uint8_t>(nck), b_out = cb.take<uint8_t>(nck), b_redo = cb.take<uint8_t>(nck);
    HIPCHK(c, c->d_rplan.ensure(cb.bytes));   // (the first phase's regions are spent)
    if ((e = ensure_stream_objects(c, 0, nck + 64))) return e;
    void* const base = c->d_rplan.p;
    ws = r_up.at(base);   // the block's regions count from here
    mlz::SearchTab* d_tabs = b_tabs.at(base);
    HIPCHK(c, hipMemcpyAsync(ws, block.data(), up.bytes, hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemsetAsync(b_skip.at(base), 0, nck * 4, sm));
    HIPCHK(c, hipMemsetAsync(b_redo.at(base), 1, nck, sm));
    // the rounds: locate, describe, one word home (the tiles to check), check, settle; every round but the first over the chunks that changed
    const uint64_t rounds = std::max<uint64_t>(mlz::batch_crc_rounds(n), 1);
    for (uint64_t round = 1;; round++) {
        hipLaunchKernelGGL(mlz::search_batch_locate_kernel, dim3(uint32_t((nck + 63) / 64)), dim3(64), 0, sm, d_src, b_hop.at(ws), b_skip.at(base), b_redo.at(base), b_cs.at(ws),
                           b_st.at(ws), b_cfg.at(ws), uint32_t(nck), d_tabs);
        if (ignore_crc) break;
        hipLaunchKernelGGL(mlz::search_batch_crc_desc_kernel, dim3(1), dim3(1024), 0, sm, static_cast<const mlz::SearchTab*>(d_tabs), b_redo.at(base), uint32_t(nck), b_blocks.at(base),
                           b_tb.at(base), uint32_t(tile_room), b_total.at(base));
        if ((e = fetch(c, sm, c->pinned2, b_total.at(base), 4))) return e;
        plan->home += mlz::kBatchHomePerRound;
        const uint32_t tiles = *static_cast<const uint32_t*>(c->pinned2);
        if (!tiles) break;
        if ((e = crc_device_described(c, sm, d_src, b_blocks.at(base), b_tb.at(base), tiles, int(nck), b_crc.at(base)))) return e;
        hipLaunchKernelGGL(mlz::search_batch_crc_settle_kernel, dim3(uint32_t((nck + 255) / 256)), dim3(256), 0, sm, d_tabs, b_crc.at(base), b_blocks.at(base), b_redo.at(base),
                           b_skip.at(base), uint32_t(nck), round >= rounds ? 1u : 0u);
        if (round >= rounds) break;
    }
    mlz::BatchPlanBits bits{};
    for (uint32_t k = 0; k < ncls; k++) bits.B[k] = cfg[k].B;
    HIPCHK(c, hipMemsetAsync(b_take.at(base), 0, nck, sm));
    const uint64_t lanes = uint64_t(nck) * np;
    hipLaunchKernelGGL(scan.fold ? mlz::search_batch_plan_kernel<true> : mlz::search_batch_plan_kernel<false>, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, sm, d_src,
                       static_cast<const mlz::SearchTab*>(d_tabs), b_n.at(ws), b_cs.at(ws), b_st.at(ws), uint32_t(nck), bits, b_hs.at(ws), b_voff.at(ws), b_pats.at(ws), uint32_t(np),
                       b_take.at(base));
    hipLaunchKernelGGL(mlz::search_batch_pack_kernel, dim3(uint32_t((nck + 255) / 256)), dim3(256), 0, sm, b_take.at(base), static_cast<const mlz::SearchTab*>(d_tabs), uint32_t(nck), b_out.at(base));
    if ((e = fetch(c, sm, c->pinned2, b_out.at(base), nck))) return e;
    plan->home += nck;
    const uint8_t* h_out = static_cast<const uint8_t*>(c->pinned2);
    for (size_t k = 0; k < nck; k++) { plan->take[k] = h_out[k] & 1; tabbed[k] = (h_out[k] >> 1) & 1; }
    return finish();
}

// mlz_stream_search_batch_device_pruned behind its argument checks
int64_t stream_search_batch_pruned_locked(mlz_ctx* c, hipStream_t sm, uint32_t flags, const uint8_t* d_src, const mlz_block_desc* streams, size_t n, const uint8_t* patterns,
                                          const uint32_t* pattern_len, size_t np, int64_t* out_count, const SearchBatchOut& out, uint64_t* stats) {
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0;
    BatchWalk bw;
    int r = stream_batch_walk(c, sm, d_src, streams, n, &bw);
    if (r) return r;
    begin_decode_call(c);
    c->search_chunks = c->search_tables = c->search_compressed = c->search_plan_bytes = 0;
    SearchManyScan scan;
    scan.prepare(flags, patterns, pattern_len, np);
    SearchBatchPlan plan;
    const int64_t p = stream_search_batch_plan(c, sm, ignore_crc, d_src, streams, bw, n, scan, &plan);
    if (p < 0) return p;
    uint64_t four[4];
    const int64_t total = stream_search_batch_passes(c, sm, ignore_crc, d_src, bw, n, plan.take.data(), scan, out_count, out, four);
    if (total < 0) return total;
    c->search_tables = plan.tabbed;
    c->search_plan_bytes = plan.home;
    if (stats) {
        for (int i = 0; i < 4; i++) stats[i] = four[i];
        stats[4] = plan.tabbed; stats[5] = plan.skipped; stats[6] = plan.classes; stats[7] = plan.whole;
    }
    return total;
}

}  // namespace

extern "C" int64_t mlz_stream_search_batch_device_pruned(mlz_ctx* c, void* stream, uint32_t flags, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams,
                                                         const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns, int64_t* out_count, uint64_t* d_stream_counts,
                                                         uint64_t* d_pattern_counts, uint32_t* d_present, uint32_t* d_hit_stream, uint64_t* d_hit_pos, uint32_t* d_hit_which,
                                                         size_t cap, uint64_t* stats) {
    const int a = search_batch_args(c, flags, d_src, streams, n_streams, patterns, pattern_len, n_patterns, out_count, d_hit_stream, d_hit_pos, d_hit_which, cap, &c);
    if (a) {
        if (a > 0 && stats) for (int i = 0; i < 8; i++) stats[i] = 0;
        return a < 0 ? a : 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    const SearchBatchOut out{d_stream_counts, d_pattern_counts, d_present, d_hit_stream, d_hit_pos, d_hit_which, uint64_t(cap)};
    if (!search_batch_outputs_on_device(c, out)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    if (flags & MLZ_SEARCH_NO_TABLES) {   // the existing call, with the plan's stats at zero
        uint64_t four[4] = {0, 0, 0, 0};
        c->search_plan_bytes = 0;
        const int64_t r = settled(sm, stream_search_batch_locked(c, sm, flags, d_src, streams, size_t(n_streams), patterns, pattern_len, n_patterns, out_count, out, four));
        if (r >= 0 && stats) for (int i = 0; i < 8; i++) stats[i] = i < 4 ? four[i] : 0;
        return r;
    }
    return settled(sm, stream_search_batch_pruned_locked(c, sm, flags, d_src, streams, size_t(n_streams), patterns, pattern_len, n_patterns, out_count, out, stats));
}
