// mlz_stream_set_tables.hip.inc — mlz_stream_open_batch_device_tables: a set of streams (mlz_stream_set.hip.inc) whose searches use every
// stream's inline block search tables (included behind mlz_stream_set.hip.inc, whose open it shares, and behind the pruned batch search,
// whose per-stream discovery kernels it launches).  The rules are those of mlz_stream_set_tables.h, which the host check runs as plain loops.
//
// The open is the plain set's: nothing of the tables is touched.  The first search that does not carry MLZ_SEARCH_NO_TABLES finds them and
// keeps them on the handle (dev_reader_set_tables):
//   once per handle      search_batch_info_kernel (a lane per stream hops to its info chunk 0x44 and leaves a key), the host numbers the
//                        distinct configurations in descriptor order (batch_assign_classes), search_batch_rep_kernel brings one payload per
//                        class home and search_batch_class_kernel compares every stream's field with its class's byte for byte.
//   once per CRC mode    set_tables_locate_kernel, a lane per data chunk: the first fitting table chunk between the previous data chunk's
//                        end (the stream's first byte) and its own body, 0x45 or 0x46, with its stream's class configuration; the table
//                        records come home as the single handle's do (24 bytes per chunk and round, no table byte), cst_resolve expands the
//                        0x46 candidates of all streams into the handle's arena, and one CRC pass per round checks the 0x45 tables of all
//                        streams.  A table that is refused is passed over for the next fitting one (skip[]).
//   once per index       set_tables_cross_kernel, a lane per stream: the crossing flags of rule c, a byte per stream comes home.
// Per call (dev_reader_set_tables_plan, the branch of dev_reader_search_plan for such a handle): the host decides which classes serve every
// pattern (batch_class_patterns), set_tables_plan_kernel applies the rule per (data chunk, pattern), one byte per chunk comes home.
// No kernel waits for another workgroup.

namespace mlz {

// tabs[c * nck + k]: chunk k's table as class c sees it — located for the class of the chunk's stream when that stream may prune
// (st[].mode == kBatchPlanPrune), no table for every other class.  skip[k]: the fitting tables in front of chunk k that an earlier round
// found broken.  own[k] = the table of chunk k's own class, the one record per chunk that comes home.
__global__ __launch_bounds__(64) void set_tables_locate_kernel(const uint8_t* __restrict__ src, const SearchHop* __restrict__ hop, const uint32_t* __restrict__ skip,
                                                               const SetTabChunk* __restrict__ chunks, const BatchPlanStream* __restrict__ st, const SearchConfig* __restrict__ cfg,
                                                               uint32_t ncls, uint32_t nck, SearchTab* __restrict__ tabs, SearchTab* __restrict__ own) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nck) return;
    const BatchPlanStream s = st[chunks[k].stream];
    const bool prune = s.mode == kBatchPlanPrune && s.cls < ncls;
    SearchTab mine{0, 0, kSearchNoTable, 0, 0};
    if (prune) mine = set_tables_locate(src, hop[k].from, hop[k].limit, skip[k], cfg[s.cls]);
    own[k] = mine;
    for (uint32_t c = 0; c < ncls; c++) {   // (field by field: a choice between two records would go through scratch)
        const bool me = prune && s.cls == c;
        tabs[size_t(c) * nck + k] = SearchTab{me ? mine.off : 0, me ? mine.bytes : 0, me ? mine.R : kSearchNoTable, me ? mine.crc : 0, me ? mine.pad : 0};
    }
}

// cross[i] of rule c; records != 0: the record-bound form over the handle's record index D[0 .. k)
__global__ __launch_bounds__(64) void set_tables_cross_kernel(const uint64_t* __restrict__ D, uint64_t k, const uint64_t* __restrict__ bases, uint32_t ns, uint32_t records,
                                                              uint8_t* __restrict__ cross) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= ns) return;
    cross[i] = (records ? set_tables_cross_records([&](uint64_t j) { return D[j]; }, k, bases, ns, i) : set_tables_cross(bases, ns, i)) ? 1 : 0;
}

// A lane per (data chunk, pattern): set_tables_plan_mark.  pats[c * np + p]: pattern p as class c sees it (L is set in every record).
template <bool kFold>
__global__ __launch_bounds__(256) void set_tables_plan_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ arena, const SearchTab* __restrict__ tabs,
                                                              const SetTabChunk* __restrict__ chunks, uint32_t nck, const BatchPlanStream* __restrict__ st, BatchPlanBits bits,
                                                              const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ voff, const SearchManyPat* __restrict__ pats,
                                                              uint32_t np, const uint8_t* __restrict__ cross, uint8_t* __restrict__ take) {
    const uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= uint64_t(nck) * np) return;
    const uint32_t k = uint32_t(idx % nck), p = uint32_t(idx / nck);
    const BatchPlanStream s = st[chunks[k].stream];
    const bool prune = s.mode == kBatchPlanPrune;
    const SearchManyPat pt = prune ? pats[size_t(s.cls) * np + p] : SearchManyPat{0, 0, 1, 1, pats[p].L, 0};
    const uint32_t B = bits.B[prune ? s.cls : 0];
    auto probe = [&](size_t j, bool lead) {
        const SearchTab t = tabs[size_t(s.cls) * nck + j];
        uint32_t a = pt.nw, sv = pt.nw;
        if (t.R != kSearchNoTable) {
            const uint8_t* table = (t.pad ? arena : src) + t.off;
            if (kFold) search_probe_fold(table, B - t.R, voff + pt.h_off, hashes, pt.nw, &a, &sv, pt.gsize);
            else search_probe(table, B - t.R, hashes + pt.h_off, pt.nw, &a, &sv, pt.gsize);
        }
        return lead ? a : sv;
    };
    set_tables_plan_mark(k, nck, s, pt, probe, [&](size_t j) { return chunks[j]; }, [&](uint32_t i) { return cross[i] != 0; }, take);
}

}  // namespace mlz

namespace {

// The handle's chunk records where the kernels can read them, made by the first search
int dev_reader_set_tables_chunks(mlz_dev_reader* rd, hipStream_t sm) {
    mlz_ctx* c = rd->ctx;
    mlz_dev_reader::SetTabled& tb = rd->tabled;
    const size_t nck = rd->chunks.size();
    if (tb.d_chunks || nck == 0) return 0;
    std::vector<mlz::SetTabChunk> ck(nck);
    for (size_t i = 0; i < tb.st.size(); i++)
        for (size_t k = tb.st[i].c0; k < tb.st[i].c1; k++)
            ck[k] = mlz::SetTabChunk{uint64_t(rd->chunks[k].n), rd->bases[i + 1] - (uint64_t(rd->chunks[k].out_off) + rd->chunks[k].n), uint32_t(i), 0};
    HIPCHK(c, hipMalloc(&tb.d_chunks, nck * sizeof(mlz::SetTabChunk)));
    HIPCHK(c, hipMemcpyAsync(tb.d_chunks, ck.data(), nck * sizeof(mlz::SetTabChunk), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipStreamSynchronize(sm));   // (ck leaves the scope)
    return 0;
}

// Once per handle: the streams' keys, the classes and their configurations, and which streams a class may prune.  Caller holds c->mu.
int64_t dev_reader_set_tables_classes(mlz_dev_reader* rd, hipStream_t sm) {
    mlz_ctx* c = rd->ctx;
    mlz_dev_reader::SetTabled& tb = rd->tabled;
    if (tb.classed) return 0;
    const size_t n = tb.st.size();
    tb.prunable.assign(n, 0);
    tb.classes = tb.ncls = 0;
    std::vector<uint8_t> part(n);
    bool any = false;
    for (size_t i = 0; i < n; i++) any = (part[i] = tb.st[i].mode != mlz::kBatchPlanSkip ? 1 : 0) || any;
    if (!any) { tb.classed = true; return 0; }
    const uint32_t nwg = uint32_t((n + 63) / 64);
    Carve ca;
    const auto a_st = ca.take<mlz::BatchPlanStream>(n);
    const auto a_keys = ca.take<mlz::BatchInfoKey>(n);
    const auto a_at = ca.take<uint64_t>(n);
    const auto a_cfg = ca.take<mlz::SearchConfig>(mlz::kSidecarMaxConfigs);
    const auto a_pay = ca.take<uint8_t>(mlz::kSidecarMaxConfigs * mlz::kBatchPayloadSlot);
    const auto a_cls = ca.take<uint8_t>(n), a_same = ca.take<uint8_t>(n);
    HIPCHK(c, c->d_rplan.ensure(ca.bytes));
    int e = ensure_stream_objects(c, 0, 64);
    if (e) return e;
    void* ws = c->d_rplan.p;
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(a_st.at(ws), tb.st.data(), n * sizeof(mlz::BatchPlanStream), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_batch_info_kernel, dim3(nwg), dim3(64), 0, sm, rd->d_src, a_st.at(ws), uint32_t(n), a_keys.at(ws), a_at.at(ws));
    std::vector<mlz::BatchInfoKey> keys(n);
    if ((e = fetch(c, sm, keys.data(), a_keys.at(ws), n * sizeof(mlz::BatchInfoKey)))) return e;
    std::vector<uint8_t> cls(n);
    size_t rep[mlz::kSidecarMaxConfigs] = {};
    tb.classes = mlz::batch_assign_classes(keys.data(), part.data(), n, cls.data(), rep);
    const uint32_t ncls = uint32_t(std::min<uint64_t>(tb.classes, mlz::kSidecarMaxConfigs));
    if (!ncls) { tb.classed = true; return 0; }
    mlz::BatchReps reps{};
    for (uint32_t k = 0; k < ncls; k++) reps.stream[k] = uint32_t(rep[k]);
    hipLaunchKernelGGL(mlz::search_batch_rep_kernel, dim3(ncls), dim3(64), 0, sm, rd->d_src, a_keys.at(ws), a_at.at(ws), reps, a_pay.at(ws));
    std::vector<uint8_t> pay(size_t(ncls) * mlz::kBatchPayloadSlot);
    if ((e = fetch(c, sm, pay.data(), a_pay.at(ws), pay.size()))) return e;
    for (uint32_t k = 0; k < mlz::kSidecarMaxConfigs; k++) {
        std::memset(&tb.cfg[k], 0, sizeof(mlz::SearchConfig));
        if (k < ncls) tb.cfg[k].ok = mlz::search_info(pay.data() + k * mlz::kBatchPayloadSlot, 3u + keys[rep[k]].flen, &tb.cfg[k].T, &tb.cfg[k].M, &tb.cfg[k].B, tb.cfg[k].field) ? 1 : 0;
    }
    HIPCHK(c, hipMemcpyAsync(a_cfg.at(ws), tb.cfg, sizeof(tb.cfg), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(a_cls.at(ws), cls.data(), n, hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(mlz::search_batch_class_kernel, dim3(nwg), dim3(64), 0, sm, rd->d_src, a_keys.at(ws), a_at.at(ws), a_cls.at(ws), a_cfg.at(ws), uint32_t(n), a_same.at(ws));
    std::vector<uint8_t> same(n);
    if ((e = fetch(c, sm, same.data(), a_same.at(ws), n))) return e;
    for (size_t i = 0; i < n; i++)
        if (part[i] && cls[i] != mlz::kBatchNoClass && same[i] && tb.cfg[cls[i]].ok) { tb.prunable[i] = 1; tb.st[i].cls = cls[i]; }
    tb.ncls = ncls;
    tb.classed = true;
    return 0;
}

// Once per handle and CRC mode: every data chunk's table, as dev_reader_search_tables finds them for one stream.  Caller holds c->mu.
int64_t dev_reader_set_tables(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc) {
    mlz_dev_reader::SearchTables& st = rd->search[ignore_crc ? 1 : 0];
    if (st.ready) return 0;
    mlz_ctx* c = rd->ctx;
    mlz_dev_reader::SetTabled& tb = rd->tabled;
    const size_t nck = rd->chunks.size(), n = tb.st.size();
    int64_t r = dev_reader_set_tables_classes(rd, sm);
    if (r) return r;
    bool any = false;
    for (size_t i = 0; i < n; i++) any = any || (tb.prunable[i] && tb.st[i].c1 > tb.st[i].c0);
    st.ncfg = 0;
    st.base = rd->d_src;
    if (!any || nck == 0 || uint64_t(nck) * tb.ncls > 0x7fffffffull) { st.ready = true; return 0; }
    if ((r = dev_reader_set_tables_chunks(rd, sm))) return r;
    const uint32_t ncls = tb.ncls;
    const size_t nt = size_t(ncls) * nck;
    std::vector<mlz::BatchPlanStream> pst(tb.st);   // mode = prune: the stream's class may prune it
    for (size_t i = 0; i < n; i++) if (tb.prunable[i]) pst[i].mode = mlz::kBatchPlanPrune;
    std::vector<mlz::SearchHop> hop(nck, mlz::SearchHop{0, 0});
    for (size_t i = 0; i < n; i++)
        for (size_t k = tb.st[i].c0; k < tb.st[i].c1; k++)
            hop[k] = mlz::SearchHop{k == tb.st[i].c0 ? tb.st[i].start : uint64_t(rd->chunks[k - 1].body_off + rd->chunks[k - 1].body_len), uint64_t(rd->chunks[k].body_off)};
    // chunk k's own place among the table sets (none: its stream is not pruned); skip is laid out like the sets, as cst_resolve indexes it
    constexpr size_t kNone = ~size_t(0);
    std::vector<size_t> place(nck, kNone);
    for (size_t i = 0; i < n; i++)
        for (size_t k = tb.st[i].c0; tb.prunable[i] && k < tb.st[i].c1; k++) place[k] = size_t(tb.st[i].cls) * nck + k;
    std::vector<uint32_t> skip(nt, 0), own_skip(nck, 0), crc;
    std::vector<mlz::SearchTab> own(nck);
    Carve cv;   // workspace: hops | skips | plan streams | configurations | table CRCs | every chunk's own table
    const auto r_hop = cv.take<mlz::SearchHop>(nck);
    const auto r_skip = cv.take<uint32_t>(nck);
    const auto r_st = cv.take<mlz::BatchPlanStream>(n);
    const auto r_cfg = cv.take<mlz::SearchConfig>(mlz::kSidecarMaxConfigs);
    const auto r_crc = cv.take<uint32_t>(nck);
    const auto r_own = cv.take<mlz::SearchTab>(nck);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    if (!st.d_tabs) HIPCHK(c, hipMalloc(&st.d_tabs, nt * sizeof(mlz::SearchTab)));
    int e = ensure_stream_objects(c, 0, 64);
    if (e) return e;
    void* ws = c->d_rplan.p;
    mlz::SearchTab* d_tabs = static_cast<mlz::SearchTab*>(st.d_tabs);
    for (uint32_t k = 0; k < mlz::kSidecarMaxConfigs; k++) st.cfg[k] = tb.cfg[k];
    st.tabs.assign(nt, mlz::SearchTab{0, 0, mlz::kSearchNoTable, 0, 0});
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(r_hop.at(ws), hop.data(), nck * sizeof(mlz::SearchHop), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(r_st.at(ws), pst.data(), n * sizeof(mlz::BatchPlanStream), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(r_cfg.at(ws), tb.cfg, sizeof(tb.cfg), hipMemcpyHostToDevice, sm));
    for (;;) {
        for (size_t k = 0; k < nck; k++) own_skip[k] = place[k] == kNone ? 0 : skip[place[k]];
        HIPCHK(c, hipMemcpyAsync(r_skip.at(ws), own_skip.data(), nck * 4, hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(mlz::set_tables_locate_kernel, dim3(uint32_t((nck + 63) / 64)), dim3(64), 0, sm, rd->d_src, r_hop.at(ws), r_skip.at(ws),
                           static_cast<const mlz::SetTabChunk*>(tb.d_chunks), r_st.at(ws), r_cfg.at(ws), ncls, uint32_t(nck), d_tabs, r_own.at(ws));
        // one record per chunk comes home: every other class's entry is no table by construction
        if ((e = fetch(c, sm, own.data(), r_own.at(ws), nck * sizeof(mlz::SearchTab)))) return e;
        for (size_t k = 0; k < nck; k++) if (place[k] != kNone) st.tabs[place[k]] = own[k];
        bool again = false;
        st.ncfg = ncls;   // (cst_resolve reads the configurations by set)
        if ((e = cst_resolve(c, sm, rd->d_src, &st, &st.tabs, nck, ignore_crc, &skip, &again, st.d_tabs))) return e;   // the 0x46 candidates of all streams: expanded, or skipped
        if (again) continue;
        if (ignore_crc) break;
        std::vector<mlz_block_desc> desc;
        std::vector<size_t> who;
        for (size_t k = 0; k < nt; k++)
            if (st.tabs[k].R != mlz::kSearchNoTable && !st.tabs[k].pad) { desc.push_back(mlz_block_desc{st.tabs[k].off, st.tabs[k].bytes, 0, 0}); who.push_back(k); }
        if (desc.empty()) break;
        if ((e = crc_device_locked(c, sm, rd->d_src, desc.data(), int(desc.size()), r_crc.at(ws)))) return e;   // one pass over the tables of all streams
        crc.resize(desc.size());
        if ((e = fetch(c, sm, crc.data(), r_crc.at(ws), desc.size() * 4))) return e;
        for (size_t i = 0; i < who.size(); i++)
            if (crc[i] != st.tabs[who[i]].crc) { skip[who[i]]++; again = true; }   // a stale table: the next one that fits, if there is one
        if (!again) break;
    }
    // what stands expanded in this mode's arena now (cst_resolve settles a table there only when its parse, decode and CRC passed)
    for (const mlz::SearchTab& t : st.tabs) tb.expansions += st.d_arena && t.R != mlz::kSearchNoTable && t.pad == mlz::kSearchTabArena ? 1 : 0;
    st.ready = true;
    return 0;
}

// The crossing flags of rule c (form 0: a position call, 1: a record-bound call over the handle's record index), once per handle and index
int64_t dev_reader_set_tables_cross(mlz_dev_reader* rd, hipStream_t sm, int form) {
    mlz_ctx* c = rd->ctx;
    mlz_dev_reader::SetTabled& tb = rd->tabled;
    if (tb.cross_ready[form]) return 0;
    const size_t n = tb.st.size();
    if (form == 1 && !rd->index_ready) return -MLZ_ERR_ARG;
    const uint64_t* d_bases = nullptr;
    int64_t r = dev_reader_bases(rd, &d_bases);
    if (r) return r;
    if (!tb.d_cross[form]) HIPCHK(c, hipMalloc(&tb.d_cross[form], n));
    hipLaunchKernelGGL(mlz::set_tables_cross_kernel, dim3(uint32_t((n + 63) / 64)), dim3(64), 0, sm, static_cast<const uint64_t*>(rd->d_index), form ? rd->index_k : 0, d_bases,
                       uint32_t(n), uint32_t(form), static_cast<uint8_t*>(tb.d_cross[form]));
    tb.cross[form].assign(n, 0);
    if (const int e = fetch(c, sm, tb.cross[form].data(), tb.d_cross[form], n)) return e;
    tb.cross_ready[form] = true;
    return 0;
}

// dev_reader_search_plan on a tabled set.  *planned = false: no stream prunes in this call, and the caller takes every chunk with bytes
// (the plain set's plan; nothing was launched for it).  records: a record-bound call (rule c's joined form).
int64_t dev_reader_set_tables_plan(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const uint8_t* patterns, const std::vector<uint32_t>& off, size_t np, bool records,
                                   std::vector<uint8_t>* take, size_t* n_take, uint64_t* unserved, bool* planned) {
    mlz_ctx* c = rd->ctx;
    mlz_dev_reader::SetTabled& tb = rd->tabled;
    const size_t nck = rd->chunks.size(), n = tb.st.size();
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0, fold = (flags & MLZ_SEARCH_IGNORE_CASE) != 0;
    *planned = false;
    *unserved = np;
    int64_t r = dev_reader_set_tables(rd, sm, ignore_crc);
    if (r) return r;
    const mlz_dev_reader::SearchTables& st = rd->search[ignore_crc ? 1 : 0];
    const uint32_t ncls = st.ncfg;
    auto bytes_of = [&](size_t i) { return rd->bases[i + 1] > rd->bases[i]; };
    uint64_t whole = 0;
    for (size_t i = 0; i < n; i++) whole += bytes_of(i) ? 1 : 0;
    for (uint64_t& v : tb.info) v = 0;
    tb.info[0] = tb.classes; tb.info[2] = whole;
    if (!ncls || (uint64_t(nck) * np + 255) / 256 > 0x7fffffffull) return 0;

    // every class's view of the patterns; a class prunes when it serves them all
    std::vector<uint32_t> hs, voff, win(mlz::kSearchMaxWindows);
    std::vector<mlz::SearchManyPat> pats(size_t(ncls) * np);
    for (size_t i = 0; i < pats.size(); i++) pats[i] = mlz::SearchManyPat{0, 0, 1, 1, off[i % np + 1] - off[i % np], 0};   // (L stands in every record, served or not)
    bool served[mlz::kSidecarMaxConfigs] = {}, used[mlz::kSidecarMaxConfigs] = {};
    for (size_t i = 0; i < n; i++) if (tb.prunable[i]) used[tb.st[i].cls] = true;
    for (uint32_t k = 0; k < ncls; k++)
        served[k] = used[k] && mlz::batch_class_patterns(st.cfg[k], patterns, off.data(), np, fold, pats.data() + size_t(k) * np, &hs, &voff);
    uint64_t windowed = 0;   // patterns to which a pruning class gives a window
    for (size_t p = 0; p < np; p++) {
        bool any = false;
        for (uint32_t k = 0; k < ncls && !any; k++) {
            uint32_t t_min = 1;
            any = used[k] && mlz::search_windows(patterns + off[p], off[p + 1] - off[p], st.cfg[k].T, st.cfg[k].M, st.cfg[k].field, win.data(), &t_min, nullptr, fold) != 0;
        }
        windowed += any ? 1 : 0;
    }
    std::vector<mlz::BatchPlanStream> pst(tb.st);
    uint64_t pruned = 0, tabbed = 0, packed = 0;
    whole = 0;
    for (size_t i = 0; i < n; i++) {
        if (tb.prunable[i] && served[tb.st[i].cls]) {
            pst[i].mode = mlz::kBatchPlanPrune;
            pruned++;
            for (size_t k = pst[i].c0; k < pst[i].c1; k++) {
                const mlz::SearchTab& t = st.tabs[size_t(pst[i].cls) * nck + k];
                tabbed += t.R != mlz::kSearchNoTable ? 1 : 0;
                packed += t.R != mlz::kSearchNoTable && t.pad ? 1 : 0;
            }
        } else if (pst[i].mode == mlz::kBatchPlanWhole && bytes_of(i)) whole++;
    }
    tb.info[1] = pruned; tb.info[2] = whole;
    if (!pruned) return 0;
    *unserved = np - windowed;
    if ((r = dev_reader_set_tables_cross(rd, sm, records ? 1 : 0))) return r;
    uint64_t crossed = 0;
    for (uint8_t v : tb.cross[records ? 1 : 0]) crossed += v;
    tb.info[3] = tabbed; tb.info[4] = packed; tb.info[5] = crossed;
    c->search_tables = tabbed;
    c->search_compressed = packed;

    // plan streams | pattern records | hashes | offsets go up as one block; one byte per chunk comes back
    Carve up;
    const auto u_st = up.take<mlz::BatchPlanStream>(n);
    const auto u_pats = up.take<mlz::SearchManyPat>(pats.size());
    const auto u_hs = up.take<uint32_t>(hs.size() + 1), u_voff = up.take<uint32_t>(voff.size() + 1);
    Carve cv;
    const auto r_up = cv.take<uint8_t>(up.bytes);
    const auto r_take = cv.take<uint8_t>(nck);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    int e = ensure_stream_objects(c, 0, std::max<size_t>(up.bytes, nck) + 64);
    if (e) return e;
    uint8_t* block = static_cast<uint8_t*>(c->pinned2);   // staged in the pinned buffer, as dev_reader_search_plan stages its block
    std::memset(block, 0, up.bytes);
    std::memcpy(u_st.at(block), pst.data(), n * sizeof(mlz::BatchPlanStream));
    std::memcpy(u_pats.at(block), pats.data(), pats.size() * sizeof(mlz::SearchManyPat));
    if (!hs.empty()) std::memcpy(u_hs.at(block), hs.data(), hs.size() * 4);
    if (!voff.empty()) std::memcpy(u_voff.at(block), voff.data(), voff.size() * 4);
    void* ws = r_up.at(c->d_rplan.p);
    uint8_t* d_take = r_take.at(c->d_rplan.p);
    mlz::BatchPlanBits bits{};
    for (uint32_t k = 0; k < ncls; k++) bits.B[k] = st.cfg[k].B;
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(ws, block, up.bytes, hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemsetAsync(d_take, 0, nck, sm));
    const uint64_t lanes = uint64_t(nck) * np;
    hipLaunchKernelGGL(fold ? mlz::set_tables_plan_kernel<true> : mlz::set_tables_plan_kernel<false>, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, sm, st.base,
                       static_cast<const uint8_t*>(st.d_arena), static_cast<const mlz::SearchTab*>(st.d_tabs), static_cast<const mlz::SetTabChunk*>(tb.d_chunks), uint32_t(nck),
                       u_st.at(ws), bits, u_hs.at(ws), u_voff.at(ws), u_pats.at(ws), uint32_t(np), static_cast<const uint8_t*>(tb.d_cross[records ? 1 : 0]), d_take);
    if ((e = fetch(c, sm, c->pinned2, d_take, nck))) return e;   // (behind the upload on sm: the staged block has left the pinned buffer)
    std::memcpy(take->data(), c->pinned2, nck);
    *n_take = 0;
    for (size_t k = 0; k < nck; k++) *n_take += (*take)[k];
    *planned = true;
    return 0;
}

}  // namespace

extern "C" {

int64_t mlz_stream_open_batch_device_tables(mlz_ctx* c, void* stream, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, int64_t* out_len, mlz_dev_reader** out) {
    return stream_open_batch_handle(c, stream, d_src, streams, n_streams, out_len, out, true);
}

int64_t mlz_dev_reader_set_tables_info(const mlz_dev_reader* rd, uint64_t* out) {
    if (!rd || !out || !rd->tabled.on) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(rd->ctx->mu);
    for (uint32_t i = 0; i < mlz::kSetTabInfoValues; i++) out[i] = rd->tabled.info[i];
    return int64_t(rd->tabled.expansions);
}

}  // extern "C"
