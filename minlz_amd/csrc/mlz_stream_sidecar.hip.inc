// mlz_stream_sidecar.hip.inc — sidecar search indexes for a stream that lies in HBM (included at the end of mlz_hip.hip, behind the two
// searches, whose handle, table sets and plan it feeds).
//
// The reference's BuildSidecar and SidecarSearcher (SEARCH.md "Sidecar Streams", SPEC_SEARCH.md 1.1 and 2.3; sidecar.go, sidecar_search.go): a
// sidecar is a second, valid MinLZ stream that holds search tables for the blocks of a main stream and names each block with a remote block
// reference (0x47: the offset of the block's data chunk header in the main stream and its decoded size).  The main stream is never touched,
// so ANY stream can be searched by tables: those of other writers, stored blocks, streams whose tables are compressed (0x46).
//
// Build (mlz_dev_reader_build_sidecar): the handle's data chunks are decoded group by group into the ReadSeeker's scratch, side by side
// (ScratchDecode, mlz_stream_walk.hip.inc; the first chunk of the next group is a job of both groups and lies behind a group's last one, so
// that every chunk's overlap lies behind it).  Per group and configuration the block-list form of the table kernels (mlz_search_tables.hip.inc: StabBlock) builds and folds the
// tables; 8 bytes per (chunk, configuration) visit the host (table bytes or 0, R), the existing CRC pass runs over the kept tables (4 more
// bytes each), and sidecar_place_kernel writes the group's chunks — and, with the first and the last group, the identifier with the info
// chunks and the EOF — at offsets the host has summed up from those sizes.
// Attach (mlz_dev_reader_attach_sidecar): the sidecar is walked on the device with the form of the chunk walk that keeps its search chunks;
// sidecar_info_kernel reads the configurations from the head of the chunk table, sidecar_attach_kernel (a lane per 0x47) parses the
// references, finds each one's data chunk in the handle's chunk table by binary search, checks size and order, and takes the tables in
// front of it, one per configuration; the CRC pass checks them, broken ones are passed over in a further round as in the inline rule.

namespace mlz {

// One data chunk of the main stream as the attach kernel sees it
struct SideMain { uint64_t hdr_off, n; };
// One block's chunks in the sidecar: its table chunks (tb[c] bytes of table, 0 = none) start at dst_off, the reference follows them.
// R[c] with kSideSection set: the chunk is a compressed one (0x46), tb[c] bytes of huff0 section, which lie sec_off behind the table's slot
constexpr uint8_t kSideSection = 0x80;
struct SidePlace { uint64_t dst_off, hdr_off; uint32_t mma, tb[kSidecarMaxConfigs], crc[kSidecarMaxConfigs]; uint8_t R[kSidecarMaxConfigs]; };
static_assert(sizeof(SidePlace) == 56, "a record shared with the host");

struct SidePlaceArgs {
    uint8_t* dst;
    const uint8_t* tabs;       // set c's table of block b: tabs + (c * cnt + b) * slot
    const SidePlace* rec;
    const SearchConfig* cfg;
    const uint8_t* head;       // identifier and info chunks (head_n bytes, to dst[0 ...)); head_n = 0: not this launch
    uint64_t eof_at;           // where the EOF chunk goes; ~0: not this launch
    uint32_t cnt, ncfg, slot, pieces, head_n;
    uint64_t sec_off;          // the section area: set c's section of block b at tabs + sec_off + (c * cnt + b) * slot
};

// A workgroup per (block, configuration, 64 KiB piece of a table slot): the table chunk's `45 len24 | T M B | field | R | crc32le` (piece 0)
// and its piece of the table in 16-byte vectors (wg_copy); configuration 0's piece 0 also writes the block's `47 len24 | uvarint | uvarint`.
__global__ __launch_bounds__(256) void sidecar_place_kernel(const SidePlaceArgs a) {
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0) {
        for (uint32_t i = tid; i < a.head_n; i += 256) a.dst[i] = a.head[i];
        if (a.eof_at != ~uint64_t(0) && tid < 5) a.dst[a.eof_at + tid] = tid == 0 ? 0x20 : tid == 1 ? 1 : 0;   // `20 01 00 00 | 00`
    }
    const uint32_t piece = blockIdx.x % a.pieces, c = (blockIdx.x / a.pieces) % a.ncfg, b = blockIdx.x / (a.pieces * a.ncfg);
    if (b >= a.cnt) return;
    const SidePlace& r = a.rec[b];
    uint64_t o = r.dst_off, mine = 0;
    for (uint32_t cc = 0; cc < a.ncfg; cc++) {
        if (cc == c) mine = o;
        if (r.tb[cc]) o += 12 + search_field_len(a.cfg[cc].T, a.cfg[cc].field) + r.tb[cc];
    }
    if (c == 0 && piece == 0 && tid == 0) sidecar_put_ref(a.dst + o, r.hdr_off, r.mma);
    const uint32_t tb = r.tb[c];
    if (!tb) return;
    const SearchConfig& cf = a.cfg[c];
    const uint32_t f = search_field_len(cf.T, cf.field), clen = 8 + f + tb;
    const bool sect = (r.R[c] & kSideSection) != 0;
    if (piece == 0)
        for (uint32_t i = tid; i < 12 + f; i += 256) {
            uint8_t v;
            if (i == 0) v = sect ? kChunkSearchTableCompressed : kChunkSearchTable;
            else if (i < 4) v = uint8_t(clen >> (8 * (i - 1)));
            else if (i == 4) v = uint8_t(cf.T);
            else if (i == 5) v = uint8_t(cf.M);
            else if (i == 6) v = uint8_t(cf.B);
            else if (i < 7 + f) v = cf.field[i - 7];
            else if (i == 7 + f) v = r.R[c] & uint8_t(~kSideSection);
            else v = uint8_t(r.crc[c] >> (8 * (i - 8 - f)));
            a.dst[mine + i] = v;
        }
    const uint32_t p0 = piece * kPlacePiece;
    if (p0 >= tb) return;
    wg_copy(a.dst + mine + 12 + f + p0, a.tabs + (sect ? a.sec_off : 0) + (size_t(c) * a.cnt + b) * a.slot + p0, tb - p0 < kPlacePiece ? tb - p0 : kPlacePiece, int(tid), 256);
}

// The configurations of a sidecar: the first kSidecarMaxConfigs valid info chunks in front of the first table or reference chunk of its
// chunk table (one lane: the head of a sidecar is a handful of chunks).  out[c].ok = 1 for those found.
__global__ __launch_bounds__(64) void sidecar_info_kernel(const uint8_t* __restrict__ side, const WalkChunk* __restrict__ rec, uint32_t ns, SearchConfig* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    for (uint32_t c = 0; c < kSidecarMaxConfigs; c++) out[c].ok = 0;
    uint32_t n = 0;
    for (uint32_t i = 0; i < ns && n < kSidecarMaxConfigs; i++) {
        const uint8_t type = uint8_t(rec[i].tl >> 24);
        if (type == kChunkSearchTable || type == kChunkSearchTableCompressed || type == kChunkRemoteRef) break;
        if (type != kChunkSearchInfo || (rec[i].flags & (kWalkTrunc | kWalkStub))) continue;
        SearchConfig& o = out[n];   // (filled in place: the field is too large for registers)
        if (search_info(side + rec[i].off + 4, rec[i].tl & 0xffffffu, &o.T, &o.M, &o.B, o.field)) { o.ok = 1; n++; }
    }
}

__global__ __launch_bounds__(256) void sidecar_fill_kernel(SearchTab* __restrict__ tabs, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) tabs[i] = SearchTab{0, 0, kSearchNoTable, 0, 0};
}

// A lane per chunk of the sidecar's table; those of a 0x47 work.  The references are checked against the main stream's data chunks
// (sidecar_check_refs; `floor`: the last reference of the 0x47 before this one, which the lane parses again), and the chunk that the first
// reference names takes, per configuration, the first fitting 0x45 between the previous 0x47 and this one (skip: fitting tables that an
// earlier round found broken).  *err becomes 1 for a reference that does not hold; every lane stores the same value.
// Cost: a lane walks back over the chunks between its 0x47 and the one before it, once per configuration and per CRC round.  A built sidecar has
// at most kSidecarMaxConfigs chunks there; a hostile one may put all its chunks in front of a single 0x47, and that one lane then walks them
// all (a few passes over the chunk table, bounded by the sidecar's size: slow, never out of bounds).
__global__ __launch_bounds__(64) void sidecar_attach_kernel(const uint8_t* __restrict__ side, const WalkChunk* __restrict__ rec, uint32_t ns, const SideMain* __restrict__ mainck,
                                                            uint32_t nck, uint64_t max_block, const SearchConfig* __restrict__ cfg, uint32_t ncfg, const uint32_t* __restrict__ skip,
                                                            SearchTab* __restrict__ tabs, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= ns) return;
    auto is_ref = [&](uint32_t j) { return uint8_t(rec[j].tl >> 24) == kChunkRemoteRef && !(rec[j].flags & (kWalkTrunc | kWalkStub)); };
    if (!is_ref(i)) return;
    auto hdr_of = [&](size_t k) { return mainck[k].hdr_off; };
    auto n_of = [&](size_t k) { return mainck[k].n; };
    uint32_t j = i;   // the 0x47 before this one: rec[j - 1], or none (j = 0)
    while (j > 0 && !is_ref(j - 1)) j--;
    bool have_floor = false;
    uint64_t floor = 0, last = 0;
    if (j > 0) {
        // (a previous chunk that does not parse is its own lane's error)
        have_floor = sidecar_parse_refs(side + rec[j - 1].off + 4, rec[j - 1].tl & 0xffffffu, max_block, [&](uint64_t off, uint64_t) { floor = off; }) > 0;
    }
    const int64_t k = sidecar_check_refs(side + rec[i].off + 4, rec[i].tl & 0xffffffu, max_block, nck, hdr_of, n_of, have_floor, floor, &last);
    if (k < 0) { *err = 1; return; }
    for (uint32_t c = 0; c < ncfg; c++) {
        const SearchConfig& cf = cfg[c];
        uint32_t left = skip[size_t(c) * nck + size_t(k)];
        for (uint32_t t = j; t < i; t++) {
            const uint8_t type = uint8_t(rec[t].tl >> 24);
            if ((type != kChunkSearchTable && type != kChunkSearchTableCompressed) || (rec[t].flags & (kWalkTrunc | kWalkStub))) continue;
            const uint32_t clen = rec[t].tl & 0xffffffu;
            const uint8_t* p = side + rec[t].off + 4;
            if (type == kChunkSearchTableCompressed) {   // a candidate for cst_resolve, as search_locate_kernel takes it
                const int R = cst_fixed_fields(p, clen, cf.M, cf.B, cf.T, cf.field);
                if (R >= 0 && left-- == 0) {
                    const uint8_t* q = p + 4 + search_field_len(cf.T, cf.field);
                    tabs[size_t(c) * nck + size_t(k)] =
                        SearchTab{rec[t].off + 4, clen, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, kSearchTabArena};
                    break;
                }
                continue;
            }
            const int R = search_table_reductions(p, clen, cf.M, cf.B, cf.T, cf.field);
            if (R >= 0 && left-- == 0) {
                const uint32_t f = search_field_len(cf.T, cf.field);
                const uint8_t* q = p + 4 + f;
                tabs[size_t(c) * nck + size_t(k)] =
                    SearchTab{rec[t].off + 12 + f, clen - 8 - f, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, 0};
                break;
            }
        }
    }
}

}  // namespace mlz

namespace {

// An mlz_search_config -> the Writer's configuration of that type: the checks of the three Writer calls, said there
StreamTables sidecar_config(const mlz_search_config& q) {
    if (q.reserved || q.reserved2[0] || q.reserved2[1]) return no_stream_tables();
    if (q.table_type == 4) {
        mlz_search_long_prefix l{};
        l.match_len = q.match_len; l.extras = q.extras; l.prefix_len = q.prefix_len;
        std::memcpy(l.prefix, q.prefix, sizeof(l.prefix));
        return stream_long_prefix_config(0, &l);
    }
    if (q.extras || (q.table_type == 2 && q.prefix_len > 8)) return no_stream_tables();
    mlz_search_tables t{};
    t.table_type = q.table_type; t.match_len = q.match_len; t.n_prefix = q.table_type == 2 ? uint8_t(q.prefix_len) : 0;
    std::memcpy(t.prefix, q.prefix, sizeof(t.prefix));
    return stream_tables_config(0, &t);
}

// The configurations of a call, or false
bool sidecar_configs(const mlz_search_config* cfgs, int n_cfgs, std::vector<StreamTables>* out) {
    if (!cfgs || n_cfgs < 1 || n_cfgs > int(mlz::kSidecarMaxConfigs)) return false;
    for (int i = 0; i < n_cfgs; i++) {
        out->push_back(sidecar_config(cfgs[i]));
        if (!out->back().valid) return false;
    }
    return true;
}

uint32_t sidecar_max_block(const mlz_dev_reader* rd) { return 1u << ((rd->ident_byte & 15) + 10); }

uint64_t sidecar_head_bytes(const std::vector<StreamTables>& stb) {
    uint64_t h = 10;
    for (const StreamTables& s : stb) h += 7 + s.flen();
    return h;
}

int64_t sidecar_bound(const mlz_dev_reader* rd, const std::vector<StreamTables>& stb) {
    const uint32_t B = mlz::search_table_bits(sidecar_max_block(rd));
    uint64_t per = mlz::kSidecarRefBound;
    for (const StreamTables& s : stb) per += mlz::search_chunk_bound(B, s.flen());
    return int64_t(sidecar_head_bytes(stb) + uint64_t(rd->chunks.size()) * per + 5);
}

constexpr size_t kSidecarTableBytes = size_t(64) << 20;   // a group's table slots take this much of c->d_stab at the most (or one chunk's)

// One pass over the handle's stream: place = false only sums up the sidecar's size.  Returns the size or an error.
int64_t sidecar_build_pass(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const std::vector<StreamTables>& stb, uint8_t* d_dst, uint64_t dst_cap, bool place, bool compress) {
    mlz_ctx* c = rd->ctx;
    const uint32_t ncfg = uint32_t(stb.size()), max_block = sidecar_max_block(rd), B = mlz::search_table_bits(max_block);
    const size_t slot = size_t(1) << (B - 3);
    const std::vector<size_t> dc = mlz::chunks_with_bytes(rd->chunks.size(), [&](size_t k) { return rd->chunks[k].n; });
    const size_t nd = dc.size();
    // groups: about 64 MiB of chunk output (as range_group_ends) and table slots within kSidecarTableBytes
    const size_t group_chunks = std::max<size_t>(1, kSidecarTableBytes / (slot * ncfg));
    std::vector<size_t> gfirst{0};
    for (size_t i = 0; i < nd;) {
        uint64_t acc = 0;
        const size_t i0 = i;
        while (i < nd && acc < mlz::kRangeGroupBytes && i - i0 < group_chunks) acc += rd->chunks[dc[i++]].n;
        gfirst.push_back(i);
    }
    const size_t ng = gfirst.size() - 1;
    // the decode list: a group's chunks side by side from scratch[0] on, then the next group's first chunk (its first bytes are the last chunk's overlap)
    ScratchDecode dec;
    size_t cnt_max = 0;
    for (size_t g = 0; g < ng; g++) {
        const size_t i1 = gfirst[g + 1] < nd ? gfirst[g + 1] + 1 : nd;
        uint64_t o = 0;
        for (size_t i = gfirst[g]; i < i1; i++) {
            dec.jobs.push_back(ChunkJob{dc[i], nullptr}); dec.at.push_back(o);
            o += rd->chunks[dc[i]].n;
        }
        dec.gend.push_back(dec.jobs.size());
        cnt_max = std::max(cnt_max, gfirst[g + 1] - gfirst[g]);
    }
    // per configuration the block list of every group (a chunk's place in ITS group's scratch and the bytes of overlap behind it)
    std::vector<mlz::StabBlock> lists(size_t(ncfg) * nd);
    for (uint32_t s = 0; s < ncfg; s++)
        for (size_t g = 0; g < ng; g++) {
            uint64_t o = 0;
            for (size_t i = gfirst[g]; i < gfirst[g + 1]; i++) {
                const uint64_t n = rd->chunks[dc[i]].n;
                const uint64_t over = i + 1 < nd ? std::min<uint64_t>(rd->chunks[dc[i + 1]].n, stb[s].overlap()) : 0;
                lists[size_t(s) * nd + i] = mlz::StabBlock{o, uint32_t(n), uint32_t(over)};
                o += n;
            }
        }
    // the head: the main stream's identifier and an info chunk per configuration
    std::vector<uint8_t> head(size_t(sidecar_head_bytes(stb)));
    std::vector<mlz::SearchConfig> cfg(ncfg);
    {
        std::memcpy(head.data(), kMagicChunk, 9);
        head[9] = rd->ident_byte;
        size_t o = 10;
        for (uint32_t s = 0; s < ncfg; s++) {
            const uint32_t f = stb[s].flen(), ilen = 3 + f;
            const uint8_t info[7] = {mlz::kChunkSearchInfo, uint8_t(ilen), uint8_t(ilen >> 8), 0, uint8_t(stb[s].T), uint8_t(stb[s].M), uint8_t(B)};
            std::memcpy(head.data() + o, info, 7);
            std::memcpy(head.data() + o + 7, stb[s].field, f);
            o += 7 + f;
            cfg[s] = mlz::SearchConfig{stb[s].T, stb[s].M, B, 1, {}};
            std::memcpy(cfg[s].field, stb[s].field, f);
        }
    }
    if (head.size() + 5 > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;

    const size_t nrec = size_t(ncfg) * cnt_max;
    Carve cv, pin;   // workspace: configurations | head | block lists | table CRCs | block records; pinned: the decode's | (bytes, R) | table CRCs | block records | uploads
    const auto r_cfg = cv.take<mlz::SearchConfig>(ncfg);
    const auto r_head = cv.take<uint8_t>(head.size());
    const auto r_lists = cv.take<mlz::StabBlock>(lists.size());
    const auto r_tcrc = cv.take<uint32_t>(nrec + 16);
    const auto r_rec = cv.take<mlz::SidePlace>(cnt_max);
    int e = dec.take(c, rd->chunks, &pin);
    if (e) return e;
    const auto h_info_r = pin.take<uint2>(nrec);
    const auto h_tcrc_r = pin.take<uint32_t>(nrec);
    const auto h_seclen_r = pin.take<int64_t>(compress ? nrec : 0);
    const auto h_rec_r = pin.take<mlz::SidePlace>(cnt_max);
    const auto h_up_r = pin.take<uint8_t>(r_tcrc.off, 64);   // what goes up once, as one block: configurations | head | block lists, laid out as in the workspace
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    // compressed tables (MLZ_STREAM_SEARCH_COMPRESS): behind the slots and records a section area of as many slots, and the sections' lengths
    const size_t sec_off = (nrec * slot + nrec * sizeof(uint2) + 64 + 63) & ~size_t(63), seclen_off = sec_off + nrec * slot;
    HIPCHK(c, c->d_stab.ensure(compress ? seclen_off + nrec * sizeof(int64_t) + 64 : nrec * slot + nrec * sizeof(uint2) + 64));
    if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
    void* ws = c->d_rplan.p;
    uint8_t *scratch = c->d_range.as<uint8_t>(), *h_up = h_up_r.at(c->pinned2);
    const mlz::SearchConfig* d_cfg = r_cfg.at(ws);
    const mlz::StabBlock* d_lists = r_lists.at(ws);
    uint32_t *d_tcrc = r_tcrc.at(ws), *h_tcrc = h_tcrc_r.at(c->pinned2);
    mlz::SidePlace *d_rec = r_rec.at(ws), *h_rec = h_rec_r.at(c->pinned2);
    int64_t *h_seclen = h_seclen_r.at(c->pinned2), *d_seclen = reinterpret_cast<int64_t*>(c->d_stab.as<uint8_t>() + seclen_off);
    uint2 *h_info = h_info_r.at(c->pinned2), *d_info = reinterpret_cast<uint2*>(c->d_stab.as<uint8_t>() + nrec * slot);
    std::memcpy(r_cfg.at(h_up), cfg.data(), ncfg * sizeof(mlz::SearchConfig));
    std::memcpy(r_head.at(h_up), head.data(), head.size());
    if (!lists.empty()) std::memcpy(r_lists.at(h_up), lists.data(), lists.size() * sizeof(mlz::StabBlock));
    { WorkspaceOrder order(c, sm); }
    HIPCHK(c, hipMemcpyAsync(ws, h_up, r_tcrc.off, hipMemcpyHostToDevice, sm));

    uint64_t total = head.size(), wrote46 = 0;   // wrote46: table chunks placed as 0x46, counted once the whole sidecar is in place
    auto launch_place = [&](uint32_t cnt, bool first, bool last_one) {
        mlz::SidePlaceArgs a{};
        a.dst = d_dst; a.tabs = c->d_stab.as<uint8_t>(); a.rec = d_rec; a.cfg = d_cfg; a.head = r_head.at(ws);
        a.eof_at = last_one ? total : ~uint64_t(0);
        a.cnt = cnt; a.ncfg = ncfg; a.slot = uint32_t(slot); a.pieces = uint32_t(std::max<size_t>(1, slot / kPlacePiece)); a.head_n = first ? uint32_t(head.size()) : 0;
        a.sec_off = sec_off;
        hipLaunchKernelGGL(mlz::sidecar_place_kernel, dim3(std::max<uint32_t>(1, cnt * ncfg * a.pieces)), dim3(256), 0, sm, a);
    };
    // a group's bytes are in the scratch: its tables, their sizes and CRCs, its chunks' places, the placement
    auto tables_of_group = [&](size_t g) -> int {
        const size_t i0 = gfirst[g], cnt = gfirst[g + 1] - i0;
        for (uint32_t s = 0; s < ncfg; s++) {
            const int r = search_tables_build_list(c, sm, scratch, d_lists + size_t(s) * nd + i0, cnt, max_block, stb[s].T, stb[s].field, stb[s].M, B,
                                                   reinterpret_cast<uint32_t*>(c->d_stab.as<uint8_t>() + size_t(s) * cnt * slot), d_info + size_t(s) * cnt);
            if (r) return r;
        }
        int r = fetch(c, sm, h_info, d_info, ncfg * cnt * sizeof(uint2));
        if (r) return r;
        std::vector<mlz_block_desc> tdesc;   // the kept tables, in (configuration, block) order: slot t = s * cnt + b
        for (size_t t = 0; t < ncfg * cnt; t++)
            if (h_info[t].x) tdesc.push_back(mlz_block_desc{t * slot, h_info[t].x, 0, 0});
        if (!tdesc.empty() && compress) {
            // every kept table's section behind its slot's twin in the section area, with one byte less of room than the table has: a
            // section that is no shorter is that item's error, nothing is written for it and its chunk stays 0x45.  Both passes run
            // this: the sizing pass sums the real sizes.
            std::vector<mlz_block_desc> cdesc(tdesc.size());
            for (size_t q = 0; q < tdesc.size(); q++) cdesc[q] = mlz_block_desc{tdesc[q].src_off, tdesc[q].src_len, sec_off + tdesc[q].src_off, tdesc[q].src_len - 1};
            if ((r = search_bitmaps_compress_locked(c, sm, c->d_stab.as<uint8_t>(), c->d_stab.as<uint8_t>(), cdesc.data(), int(cdesc.size()), d_seclen))) return r;
            if ((r = fetch(c, sm, h_seclen, d_seclen, tdesc.size() * sizeof(int64_t)))) return r;
        }
        if (!tdesc.empty() && place) {
            if ((r = crc_device_locked(c, sm, c->d_stab.as<uint8_t>(), tdesc.data(), int(tdesc.size()), d_tcrc))) return r;
            if ((r = fetch(c, sm, h_tcrc, d_tcrc, tdesc.size() * 4))) return r;
        }
        std::vector<uint32_t> crc_at(ncfg * cnt, 0);
        for (size_t t = 0, q = 0; t < ncfg * cnt; t++) if (h_info[t].x) crc_at[t] = uint32_t(q++);
        for (size_t b = 0; b < cnt; b++) {
            const StreamChunk& ck = rd->chunks[dc[i0 + b]];
            mlz::SidePlace& p = h_rec[b];
            p = mlz::SidePlace{};
            p.dst_off = total; p.hdr_off = ck.hdr_off; p.mma = uint32_t(max_block - ck.n);
            for (uint32_t s = 0; s < ncfg; s++) {
                const size_t t = size_t(s) * cnt + b;
                p.tb[s] = h_info[t].x; p.R[s] = uint8_t(h_info[t].y);
                if (!p.tb[s]) continue;
                if (place) p.crc[s] = h_tcrc[crc_at[t]];
                if (compress && h_seclen[crc_at[t]] > 0 && h_seclen[crc_at[t]] < int64_t(p.tb[s])) {
                    p.tb[s] = uint32_t(h_seclen[crc_at[t]]);
                    p.R[s] |= mlz::kSideSection;
                    if (place) wrote46++;
                }
                total += 12 + stb[s].flen() + p.tb[s];
            }
            total += mlz::sidecar_ref_bytes(p.hdr_off, p.mma);
        }
        if (!place) return 0;
        if (total + 5 > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;   // (never with a capacity the caller took from the bound or that the sizing pass has passed)
        HIPCHK(c, hipMemcpyAsync(d_rec, h_rec, cnt * sizeof(mlz::SidePlace), hipMemcpyHostToDevice, sm));
        launch_place(uint32_t(cnt), g == 0, g + 1 == ng);
        HIPCHK(c, hipStreamSynchronize(sm));   // (the records' staging is reused by the next group)
        return 0;
    };
    if (ng == 0) {
        if (place) launch_place(0, true, true);
    } else {
        const int64_t r = dec.run(c, sm, ignore_crc, rd->d_src, rd->chunks, tables_of_group);
        if (r < 0) return r;
    }
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    if (place) c->tables_compressed = wrote46;
    return int64_t(total + 5);
}

int64_t dev_reader_build_sidecar_locked(mlz_dev_reader* rd, hipStream_t sm, uint32_t flags, const std::vector<StreamTables>& stb, uint8_t* d_dst, uint64_t dst_cap) {
    mlz_ctx* c = rd->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const bool ignore_crc = (flags & MLZ_STREAM_IGNORE_CRC) != 0, compress = (flags & MLZ_STREAM_SEARCH_COMPRESS) != 0;
    c->tables_compressed = 0;
    // a capacity below the bound may not hold the result: the sizes are found first, so that nothing is written when it does not
    if (dst_cap < uint64_t(sidecar_bound(rd, stb))) {
        const int64_t need = sidecar_build_pass(rd, sm, ignore_crc, stb, d_dst, dst_cap, false, compress);
        if (need < 0) return need;
        if (uint64_t(need) > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;
    }
    return sidecar_build_pass(rd, sm, ignore_crc, stb, d_dst, dst_cap, true, compress);
}

// The attach: the sidecar's table sets -> *out (device memory of its own).  Returns 0 or the error; nothing of the handle changes here.
int64_t dev_reader_attach_sidecar_locked(mlz_dev_reader* rd, hipStream_t sm, bool ignore_crc, const uint8_t* d_side, size_t n_side, mlz_dev_reader::SearchTables* out) {
    mlz_ctx* c = rd->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nck = rd->chunks.size();
    std::vector<StreamChunk> side_data;
    std::vector<mlz::WalkChunk> rec;
    int64_t parsed = 0;
    uint32_t n_ident = 0;
    uint8_t ident_byte = 0;
    int e = stream_walk_device(c, sm, d_side, n_side, &side_data, &parsed, &n_ident, &ident_byte, &rec);
    if (e) return e;
    if (!side_data.empty()) return -MLZ_ERR_CORRUPT;   // a data chunk inside a sidecar
    if (parsed < 0) return parsed;                     // a framing error, no EOF chunk
    if (n_ident > 1) return -MLZ_ERR_UNSUPPORTED;
    const size_t ns = rec.size();
    const uint64_t max_block = uint64_t(1) << ((ident_byte & 15) + 10);
    out->ready = true; out->ncfg = 0; out->base = d_side; out->tabs.clear();
    if (ns == 0 || n_ident == 0) return 0;
    constexpr uint32_t kMaxCfg = mlz::kSidecarMaxConfigs;
    const size_t ntab = std::max<size_t>(1, kMaxCfg * nck);
    Carve cv, pin;   // workspace: main chunks | skips | configurations | error | table CRCs; what comes back: tables | table CRCs | configurations | error
    const auto r_main = cv.take<mlz::SideMain>(nck);
    const auto r_skip = cv.take<uint32_t>(ntab);
    const auto r_cfg = cv.take<mlz::SearchConfig>(kMaxCfg);
    const auto r_err = cv.take<uint32_t>(4);
    const auto r_crc = cv.take<uint32_t>(ntab);
    const auto r_htabs = pin.take<mlz::SearchTab>(ntab);
    const auto r_hcrc = pin.take<uint32_t>(ntab, 4);
    const auto r_hcfg = pin.take<mlz::SearchConfig>(kMaxCfg + 1, 4);   // (the last one: room for the error word)
    const auto r_hmain = pin.take<mlz::SideMain>(nck, 8);
    const auto r_hskip = pin.take<uint32_t>(ntab, 4);
    HIPCHK(c, c->d_rplan.ensure(cv.bytes));
    HIPCHK(c, hipMalloc(&out->d_tabs, ntab * sizeof(mlz::SearchTab)));
    if ((e = ensure_stream_objects(c, 0, pin.bytes))) return e;
    void* ws = c->d_rplan.p;
    mlz::SideMain *d_main = r_main.at(ws), *h_main = r_hmain.at(c->pinned2);
    mlz::SearchConfig *d_cfg = r_cfg.at(ws), *h_cfg = r_hcfg.at(c->pinned2);
    uint32_t *d_skip = r_skip.at(ws), *h_skip = r_hskip.at(c->pinned2), *d_err = r_err.at(ws), *d_crc = r_crc.at(ws), *h_crc = r_hcrc.at(c->pinned2);
    mlz::SearchTab *d_tabs = static_cast<mlz::SearchTab*>(out->d_tabs), *h_tabs = r_htabs.at(c->pinned2);
    const mlz::WalkChunk* d_rec = c->d_walk_tab.as<mlz::WalkChunk>();   // (the walk's table, still where the walk left it: this call holds the lock)
    for (size_t k = 0; k < nck; k++) h_main[k] = mlz::SideMain{uint64_t(rd->chunks[k].hdr_off), uint64_t(rd->chunks[k].n)};
    std::vector<uint32_t> skip(ntab, 0);
    { WorkspaceOrder order(c, sm); }
    if (nck) HIPCHK(c, hipMemcpyAsync(d_main, h_main, nck * sizeof(mlz::SideMain), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemsetAsync(d_err, 0, 16, sm));
    hipLaunchKernelGGL(mlz::sidecar_info_kernel, dim3(1), dim3(64), 0, sm, d_side, d_rec, uint32_t(ns), d_cfg);
    if ((e = fetch(c, sm, h_cfg, d_cfg, kMaxCfg * sizeof(mlz::SearchConfig)))) return e;
    uint32_t ncfg = 0;
    while (ncfg < kMaxCfg && h_cfg[ncfg].ok) { out->cfg[ncfg] = h_cfg[ncfg]; ncfg++; }
    for (;;) {
        std::memcpy(h_skip, skip.data(), ntab * 4);
        HIPCHK(c, hipMemcpyAsync(d_skip, h_skip, ntab * 4, hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(mlz::sidecar_fill_kernel, dim3(uint32_t((ntab + 255) / 256)), dim3(256), 0, sm, d_tabs, uint32_t(ntab));
        hipLaunchKernelGGL(mlz::sidecar_attach_kernel, dim3(uint32_t((ns + 63) / 64)), dim3(64), 0, sm, d_side, d_rec, uint32_t(ns), d_main, uint32_t(nck), max_block, d_cfg, ncfg,
                           d_skip, d_tabs, d_err);
        HIPCHK(c, hipMemcpyAsync(h_tabs, d_tabs, ntab * sizeof(mlz::SearchTab), hipMemcpyDeviceToHost, sm));
        if ((e = fetch(c, sm, h_cfg + kMaxCfg, d_err, 4))) return e;
        if (*reinterpret_cast<const uint32_t*>(h_cfg + kMaxCfg)) return -MLZ_ERR_CORRUPT;
        out->tabs.assign(h_tabs, h_tabs + size_t(ncfg) * nck);
        if (!ncfg) break;
        bool again = false;
        if (nck) {   // the compressed tables: expanded, or skipped
            const int x = cst_resolve(c, sm, d_side, out, &out->tabs, nck, ignore_crc, &skip, &again, out->d_tabs);
            if (x) return x;
        }
        if (again) continue;
        if (ignore_crc) break;
        std::vector<mlz_block_desc> desc;
        std::vector<size_t> who;
        for (size_t t = 0; t < out->tabs.size(); t++)
            if (out->tabs[t].R != mlz::kSearchNoTable && !out->tabs[t].pad) { desc.push_back(mlz_block_desc{out->tabs[t].off, out->tabs[t].bytes, 0, 0}); who.push_back(t); }
        if (desc.empty()) break;
        int r = crc_device_locked(c, sm, d_side, desc.data(), int(desc.size()), d_crc);
        if (r) return r;
        if ((r = fetch(c, sm, h_crc, d_crc, desc.size() * 4))) return r;
        for (size_t i = 0; i < who.size(); i++)
            if (h_crc[i] != out->tabs[who[i]].crc) { skip[who[i]]++; again = true; }   // a broken table: the next one that fits, if there is one
        if (!again) break;
    }
    out->ncfg = ncfg;
    return 0;
}

}  // namespace

extern "C" {

int64_t mlz_dev_reader_sidecar_bound(const mlz_dev_reader* rd, const mlz_search_config* cfgs, int n_cfgs) {
    std::vector<StreamTables> stb;
    if (!rd || !sidecar_configs(cfgs, n_cfgs, &stb)) return -MLZ_ERR_ARG;
    return sidecar_bound(rd, stb);
}

int64_t mlz_dev_reader_build_sidecar(mlz_dev_reader* rd, void* stream, uint32_t flags, const mlz_search_config* cfgs, int n_cfgs, uint8_t* d_dst, size_t dst_cap) {
    std::vector<StreamTables> stb;
    if (!rd || !d_dst || !sidecar_configs(cfgs, n_cfgs, &stb)) return -MLZ_ERR_ARG;
    if (rd->set) return -MLZ_ERR_UNSUPPORTED;   // a set of streams (mlz_stream_open_batch_device): as concatenated streams
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!on_device(c, d_dst)) return -MLZ_ERR_ARG;
    if (rd->n_ident > 1) return -MLZ_ERR_UNSUPPORTED;
    if (rd->n_ident == 0) return -MLZ_ERR_CORRUPT;   // (an empty stream: no identifier to repeat)
    begin_decode_call(c);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    return settled(sm, dev_reader_build_sidecar_locked(rd, sm, flags, stb, d_dst, uint64_t(dst_cap)));
}

int64_t mlz_dev_reader_attach_sidecar(mlz_dev_reader* rd, void* stream, uint32_t flags, const uint8_t* d_side, size_t n_side) {
    if (!rd || (!d_side && n_side)) return -MLZ_ERR_ARG;
    if (rd->set) return -MLZ_ERR_UNSUPPORTED;
    mlz_ctx* c = rd->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (enter_device(c)) return -MLZ_ERR_HIP;
    if (!d_side) {   // detach: the handle searches by its inline tables again
        search_tables_release(&rd->side);
        rd->side = mlz_dev_reader::SearchTables{};
        rd->side_on = false;
        return 0;
    }
    if (n_side == 0 || uint64_t(n_side) > kWalkMaxStream || !on_device(c, d_side)) return -MLZ_ERR_ARG;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    mlz_dev_reader::SearchTables fresh;
    const int64_t r = settled(sm, dev_reader_attach_sidecar_locked(rd, sm, (flags & MLZ_STREAM_IGNORE_CRC) != 0, d_side, n_side, &fresh));
    if (r < 0) {   // nothing is attached: the handle keeps what it had
        search_tables_release(&fresh);
        return r;
    }
    search_tables_release(&rd->side);
    rd->side = std::move(fresh);
    rd->side_on = true;
    return 0;
}

}  // extern "C"
