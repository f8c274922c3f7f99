// mlz_stream.hip.inc — MinLZ stream framing on top of the block kernels (host code; included at the end
// of mlz_hip.hip).
//
// mlz_stream_encode = NewWriter(dst, WriterLevel, WriterBlockSize, WriterAddIndex).EncodeBuffer(src) + Close()
//   (writer.go:441-563, :854-965, :1051-1126): stream header, one chunk per block
//   `[0x02][len24][crc][uvarint N][tokens]` or `[0x01][len24][crc][raw]`, EOF chunk, optional seek index.
// mlz_stream_decode = NewReader(src).Read until EOF (reader.go:248-543) for MinLZ streams.
//
// Blocks are encoded / decoded / checksummed on the device in groups of ~256 MiB; the host-to-device
// copy of group g+1 and the device-to-host copy of group g-1 run on their own streams while group g
// is in the kernels (the reference overlaps I/O and compression with goroutines, writer.go:501-560).
//
// Both Writers (mlz_stream_encode over host memory, stream_encode_groups; the device-resident one, stream_gather_range under
// stream_encode_gather_device_with) frame with the same helpers: chunk_shape and put_chunk_header for a block's chunk, put_stream_head and
// stream_foot for what stands around the chunks, place_pieces + stream_place_kernel for chunk bodies that a kernel moves (stream_hdr_kernel and
// stream_tabhdr_kernel write the device-resident Writer's chunk headers).  StreamTables is the one configuration of the search tables,
// whichever call it came in by.

#include "mlz_stream_scratch.h"
#include "mlz_stream_walk.h"
#include "mlz_stream_batch.h"
#include "mlz_stream_ranges.h"

namespace {

constexpr uint8_t kChunkUncompressed = 0x01, kChunkMinLZ = 0x02, kChunkMinLZCompCRC = 0x03, kChunkEOF = 0x20, kChunkIndex = 0x40;  // minlz.go:108-131
constexpr uint32_t kMinStreamBlock = 4u << 10;                      // minlz.go:98
const uint8_t kMagicChunk[9] = {0xff, 0x06, 0x00, 0x00, 'M', 'i', 'n', 'L', 'z'};
constexpr size_t kStreamGroupBytes = 64u << 20;   // per group: copy-in, kernels and copy-out of different groups overlap

size_t put_uvarint64(uint8_t* d, uint64_t v) {
    size_t i = 0;
    while (v >= 0x80) { d[i++] = uint8_t(v) | 0x80; v >>= 7; }
    d[i++] = uint8_t(v);
    return i;
}
size_t put_varint64(uint8_t* d, int64_t v) { return put_uvarint64(d, (uint64_t(v) << 1) ^ uint64_t(v >> 63)); }  // binary.PutVarint

// Seek index, write side (Index.reset / add / reduce / reduceLight / appendTo, index.go:56-269).
struct SeekIndex {
    static constexpr size_t kMaxEntries = 1u << 16;
    static constexpr int64_t kMinDist = 1 << 20;
    int64_t est = 0;
    std::vector<std::pair<int64_t, int64_t>> off;  // (compressed offset, uncompressed offset)
    void reset(int64_t max_block) {
        while (max_block < kMinDist) max_block *= 2;
        est = max_block; off.clear();
    }
    void reduce_light() {
        est *= 2;
        size_t j = 0;
        for (size_t i = 0; i < off.size(); i++) {
            const auto base = off[i];
            off[j++] = base;
            while (i < off.size() && off[i].second - base.second < est) i++;
        }
        off.resize(j);
    }
    void add(int64_t c, int64_t u) {
        if (!off.empty() && u - off.back().second < est) return;
        off.emplace_back(c, u);
        if (off.size() > kMaxEntries) reduce_light();
    }
    void reduce() {
        if (off.size() < kMaxEntries) return;
        size_t remove_n = (off.size() + 1) / kMaxEntries;
        while (est * int64_t(remove_n + 1) < kMinDist && off.size() / (remove_n + 1) > 1000) remove_n++;
        size_t j = 0;
        for (size_t i = 0; i < off.size(); i += remove_n + 1) off[j++] = off[i];
        off.resize(j);
        est += est * int64_t(remove_n);
    }
    static size_t bound(size_t n_blocks) { return 64 + 20 * std::min(n_blocks, kMaxEntries + 1); }
    size_t append_to(uint8_t* b, int64_t total_u, int64_t total_c) {
        reduce();
        size_t o = 0;
        b[o++] = kChunkIndex; b[o++] = 0; b[o++] = 0; b[o++] = 0;
        std::memcpy(b + o, "s2idx\0", 6); o += 6;
        o += put_varint64(b + o, total_u);
        o += put_varint64(b + o, total_c);
        o += put_varint64(b + o, est);
        o += put_varint64(b + o, int64_t(off.size()));
        uint8_t has_u = 0;
        for (size_t i = 0; i < off.size(); i++) {
            if (i == 0 ? off[0].second != 0 : off[i].second != off[i - 1].second + est) { has_u = 1; break; }
        }
        b[o++] = has_u;
        if (has_u)
            for (size_t i = 0; i < off.size(); i++) o += put_varint64(b + o, i ? off[i].second - (off[i - 1].second + est) : off[i].second);
        int64_t predict = est / 2;
        for (size_t i = 0; i < off.size(); i++) {
            int64_t cv = off[i].first;
            if (i) { cv -= off[i - 1].first + predict; predict += cv / 2; }
            o += put_varint64(b + o, cv);
        }
        const uint32_t total = uint32_t(o + 4 + 6);
        std::memcpy(b + o, &total, 4); o += 4;
        std::memcpy(b + o, "\0xdi2s", 6); o += 6;
        const uint32_t chunk_len = uint32_t(o - 4);
        b[1] = uint8_t(chunk_len); b[2] = uint8_t(chunk_len >> 8); b[3] = uint8_t(chunk_len >> 16);
        return o;
    }
};

int ensure_stream_objects(mlz_ctx* c, size_t n_events, size_t pinned_bytes) {
    // The copy streams get the highest priority: the copy-out of a group runs as a shader copy on some ROCm builds, and on a
    // queue of the kernels' priority it was observed to wait for every kernel queued before it (rocprofv3 timeline).
    if (!c->s_in || !c->s_out) {
        int lo = 0, hi = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
        if (!c->s_in) HIPCHK(c, hipStreamCreateWithPriority(&c->s_in, hipStreamNonBlocking, hi));
        if (!c->s_out) HIPCHK(c, hipStreamCreateWithPriority(&c->s_out, hipStreamNonBlocking, hi));
    }
    while (c->evpool.size() < n_events) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->evpool.push_back(e);
    }
    if (pinned_bytes > c->pinned2_cap) {
        if (c->pinned2) HIPCHK(c, hipHostFree(c->pinned2));
        c->pinned2 = nullptr;
        c->pinned2_cap = pinned_bytes * 2 + 4096;
        HIPCHK(c, hipHostMalloc(&c->pinned2, c->pinned2_cap, hipHostMallocDefault));
    }
    return 0;
}

// MLZ_STREAM_SEARCH_TABLES in `flags`: the match length M (bits 8 .. 11, 0 = the reference's default), 0 when the flag is clear, -1 for 9 .. 15
int stream_search_match_len(uint32_t flags) {
    if (!(flags & MLZ_STREAM_SEARCH_TABLES)) return 0;
    const uint32_t m = (flags >> 8) & 15;
    return m == 0 ? int(mlz::kSearchDefaultMatchLen) : m <= 8 ? int(m) : -1;
}

// The Writer's search tables: T = 0 without them, else the table type, the match length and the prefix field as the chunks carry it.
// valid = false: what the caller handed in is no configuration (-MLZ_ERR_ARG, behind the checks of the call's other arguments)
struct StreamTables {
    bool valid = true;
    uint32_t T = 0, M = 0;
    uint8_t field[mlz::kSearchMaxField] = {};
    uint32_t flen() const { return mlz::search_field_len(T, field); }
    // bytes behind a block that its prefixes and windows reach
    uint32_t overlap() const { return mlz::search_overlap(T, M, field); }
    // the stream's head: magic chunk and, with tables, the info chunk
    uint32_t head_bytes() const { return T ? 17 + flen() : 10; }
};
StreamTables no_stream_tables() { StreamTables st; st.valid = false; return st; }
// flags and an mlz_search_tables (may be NULL) -> the configuration
StreamTables stream_tables_config(uint32_t flags, const mlz_search_tables* cfg) {
    StreamTables st;
    if (!cfg) {
        const int m = stream_search_match_len(flags);
        if (m < 0) return no_stream_tables();
        if (m) { st.T = 1; st.M = uint32_t(m); }
        return st;
    }
    if ((flags & (MLZ_STREAM_SEARCH_TABLES | MLZ_STREAM_SEARCH_MATCH_LEN(15))) || cfg->table_type < 1 || cfg->table_type > 3 || cfg->match_len > 8 || cfg->reserved) return no_stream_tables();
    st.T = cfg->table_type;
    st.M = cfg->match_len ? cfg->match_len : mlz::kSearchDefaultMatchLen;
    if (st.T == 2) {
        if (cfg->n_prefix < 1 || cfg->n_prefix > 8) return no_stream_tables();
        for (uint32_t i = 0; i < 8; i++) st.field[i] = cfg->prefix[i < cfg->n_prefix ? i : cfg->n_prefix - 1u];
    } else if (st.T == 3) std::memcpy(st.field, cfg->prefix, 32);
    return st;
}
// An mlz_search_long_prefix -> the configuration of table type 4
StreamTables stream_long_prefix_config(uint32_t flags, const mlz_search_long_prefix* cfg) {
    if (!cfg || (flags & (MLZ_STREAM_SEARCH_TABLES | MLZ_STREAM_SEARCH_MATCH_LEN(15)))) return no_stream_tables();
    if (cfg->prefix_len < 1 || cfg->prefix_len > mlz::kSearchMaxPrefix || cfg->match_len > 8 || cfg->extras > mlz::kSearchMaxExtras) return no_stream_tables();
    for (uint8_t r : cfg->reserved) if (r) return no_stream_tables();
    StreamTables st;
    st.T = 4;
    st.M = cfg->match_len ? cfg->match_len : mlz::kSearchDefaultMatchLen;
    if (st.M + cfg->extras > mlz::kSearchMaxGroupWindows) return no_stream_tables();
    st.field[0] = uint8_t(cfg->prefix_len - 1); st.field[1] = cfg->extras;
    std::memcpy(st.field + 2, cfg->prefix, cfg->prefix_len);
    return st;
}

size_t stream_bound(uint64_t n, uint32_t bs, bool add_index, const StreamTables& stb) {
    const uint64_t nblk = (n + bs - 1) / bs;
    // search tables: the info chunk and, per block, a table chunk with the unreduced table; both carry the type's prefix field
    const uint64_t tables = stb.T ? 7 + stb.flen() + nblk * mlz::search_chunk_bound(mlz::search_table_bits(bs), stb.flen()) : 0;
    return size_t(10 + nblk * (8 + 5) + n + 4 + 10 + (add_index ? SeekIndex::bound(size_t(nblk)) : 0) + tables);
}

// ---- framing, said once for mlz_stream_encode and the device-resident Writer ----
// A block as the encoder leaves it is `00 uvarint(N) tokens` or the stored form `00 00 raw` (encode.go:74-139, :223-228); only the stored form
// has length N + 2 (tokens are < N - N/32 - 5).  Its chunk's body is the block minus its leading 0x00, or the raw bytes.
struct ChunkShape { bool stored; size_t body; };
ChunkShape chunk_shape(int64_t elen, size_t src_len) {
    const bool stored = elen == int64_t(src_len) + 2;
    return ChunkShape{stored, stored ? src_len : size_t(elen) - 1};
}
// The 8 bytes in front of a chunk's body: type, len24 (the CRC's 4 bytes and the body), crc
void put_chunk_header(uint8_t* b, const ChunkShape& s, uint32_t crc) {
    const size_t chunk_len = 4 + s.body;
    b[0] = s.stored ? kChunkUncompressed : kChunkMinLZ;
    b[1] = uint8_t(chunk_len); b[2] = uint8_t(chunk_len >> 8); b[3] = uint8_t(chunk_len >> 16);
    std::memcpy(b + 4, &crc, 4);
}
// The stream's head (stb.head_bytes() bytes; it goes out with the first block, writer.go:463-467): the magic chunk and, with tables, the info
// chunk `44 len24 | T M B | prefix field`
void put_stream_head(uint8_t* b, uint32_t bs, const StreamTables& stb) {
    std::memcpy(b, kMagicChunk, 9);
    b[9] = uint8_t((32 - __builtin_clz(bs - 1)) - 10);  // log2(block size) - 10, writer.go:1553-1556
    if (!stb.T) return;
    const uint32_t ilen = 3 + stb.flen();
    const uint8_t info[7] = {mlz::kChunkSearchInfo, uint8_t(ilen), uint8_t(ilen >> 8), 0, uint8_t(stb.T), uint8_t(stb.M), uint8_t(mlz::search_table_bits(bs))};
    std::memcpy(b + 10, info, 7);
    std::memcpy(b + 17, stb.field, stb.flen());
}
// The stream's foot: the EOF chunk (writer.go:1063-1074), then the index (writer.go:1080-1122) over the blocks' chunks, whose bytes (a table
// chunk in front included) are `framed`.  *at: where the foot goes, behind `head` bytes and the chunks.
std::vector<uint8_t> stream_foot(size_t n, uint32_t bs, size_t head, const std::vector<uint32_t>& framed, bool add_index, size_t* at) {
    SeekIndex index;
    index.reset(bs);
    if (n > 0) index.add(0, 0);  // the stream header's own entry (writer.go:236-243): the first block's (head, 0) is then dropped (index.go:87-90)
    size_t o = n > 0 ? head : 0;
    for (size_t i = 0; i < framed.size(); i++) {
        index.add(int64_t(o), int64_t(i * size_t(bs)));  // writer.go:945
        o += framed[i];
    }
    *at = o;
    std::vector<uint8_t> foot(16 + (add_index ? SeekIndex::bound(framed.size()) : 0));
    const size_t vn = put_uvarint64(foot.data() + 4, n);
    foot[0] = kChunkEOF; foot[1] = uint8_t(vn); foot[2] = 0; foot[3] = 0;
    size_t t = 4 + vn;
    if (add_index) t += index.append_to(foot.data() + t, int64_t(n), int64_t(o + t));
    foot.resize(t);
    return foot;
}
// What a call over several workers returns: the first worker's own verdict (one that only stopped because another one failed says -MLZ_ERR_HIP)
int64_t first_own_verdict(const std::vector<int64_t>& rcs) {
    for (int64_t r : rcs) if (r && r != -MLZ_ERR_HIP) return r;
    for (int64_t r : rcs) if (r) return r;
    return 0;
}

// ---- kernels that lay chunks out ----
// Chunk bodies: one workgroup per 64 KiB piece copies from a source in HBM to the destination, a run of chunks in HBM or, through its device
// alias, the caller's page-locked buffer (the per-block copy-out of a pinned buffer runs as shader copies on this ROCm build and queues up
// behind every kernel of the stream: 22.6 GB/s against 31.3 into pageable memory for 100 MB).  desc.pad selects the source: for the Writer
// 0 = the encoder's output, 1 = the raw block (stored chunks), 2 = the block's search table; a caller with fewer sources passes nullptr.
using mlz::PlaceDesc; using mlz::kPlacePiece; using mlz::place_pieces;   // mlz_stream_scratch.h
__global__ __launch_bounds__(256) void stream_place_kernel(const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, const uint8_t* __restrict__ src2,
                                                           uint8_t* __restrict__ dst, const PlaceDesc* __restrict__ descs) {
    const PlaceDesc d = descs[blockIdx.x];
    mlz::wg_copy(dst + d.dst_off, (d.pad == 2 ? src2 : d.pad ? src1 : src0) + d.src_off, d.len, threadIdx.x, 256);
}
// Chunk headers of the device-resident Writer: eight literal bytes at a destination offset (a table chunk's: twelve and its prefix field, 20 or
// 44 with table type 2 or 3; type 4's field of 2 + K bytes is the same in every table chunk and travels once, in the kernel's arguments:
// TabHdrDesc::b then holds `45 len24 T M B` and `R crc32le`, and the field goes between the two).
struct HdrDesc { uint64_t dst_off; uint8_t b[8]; };
struct TabHdrDesc { uint64_t dst_off; uint8_t b[12 + 32]; uint32_t n; };
struct TabLongField { uint32_t n; uint8_t b[mlz::kSearchMaxField + 2]; };   // n = 0: table types 1 .. 3
__global__ __launch_bounds__(64) void stream_tabhdr_kernel(uint8_t* __restrict__ run, const TabHdrDesc* __restrict__ hd, uint32_t n, const TabLongField lf) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const TabHdrDesc& h = hd[i];
    if (lf.n == 0) {
        for (uint32_t k = 0; k < h.n; k++) run[h.dst_off + k] = h.b[k];
        return;
    }
    for (uint32_t k = 0; k < 7; k++) run[h.dst_off + k] = h.b[k];
    for (uint32_t k = 0; k < lf.n; k++) run[h.dst_off + 7 + k] = lf.b[k];
    for (uint32_t k = 0; k < 5; k++) run[h.dst_off + 7 + lf.n + k] = h.b[7 + k];
}
__global__ __launch_bounds__(64) void stream_hdr_kernel(uint8_t* __restrict__ run, const HdrDesc* __restrict__ hd, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const HdrDesc h = hd[i];
#pragma unroll
    for (int k = 0; k < 8; k++) run[h.dst_off + k] = h.b[k];
}

// What the workers of one stream-encode call share when the stream's blocks are dealt to several devices (mlz_init_devices): the framed size of every
// UNIT of the stream (a group of blocks of mlz_stream_encode, a range of mlz_stream_encode_gather_device), in stream order.  A chunk's place in the
// stream is known once the sizes of all chunks before it are: whoever frames unit u publishes its size first and then waits for the units before it —
// the in-order emit of the reference's Writer (writer.go:219-272) without its channel chain.  Waits only ever go to LOWER units and every worker takes
// its units in ascending order, publishing before waiting: no cycle.
struct StreamEncShared {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int64_t> unit_bytes;   // bytes of unit u's chunks; -1 = not known yet
    bool failed = false;               // a worker gave up: nobody waits for a size that will not come
    explicit StreamEncShared(size_t units) : unit_bytes(units, -1) {}
    void publish(size_t u, int64_t v) {
        { std::lock_guard<std::mutex> lk(mu); if (unit_bytes[u] < 0) unit_bytes[u] = v; }
        cv.notify_all();
    }
    void fail(size_t = 0) {
        { std::lock_guard<std::mutex> lk(mu); failed = true; }
        cv.notify_all();
    }
    // bytes of the units before u, or -1 when a worker failed
    int64_t base_of(size_t u) {
        std::unique_lock<std::mutex> lk(mu);
        int64_t sum = 0;
        for (size_t i = 0; i < u; i++) {
            cv.wait(lk, [&] { return failed || unit_bytes[i] >= 0; });
            if (failed) return -1;
            sum += unit_bytes[i];
        }
        return sum;
    }
};


// Worker j of k: the stream's GROUPS of blocks (kStreamGroupBytes of input each) j, j + k, j + 2k, ... — copy-in, encode, CRC, and the chunks
// `[type][len24][crc][body]` written to their FINAL place in dst.  Everything is enqueued up front; a group's chunks are placed as soon as its sizes
// and those of the groups before it are known (one device: its own earlier groups; several: the other devices' groups of the same pipeline step, which
// finish at the same time), while the worker's later groups are still in the kernels — the copy-out of step t rides under the kernels of step t + 1
// on every device.  (Round 6's first form gave every device one contiguous range: a device then knew its base only when ALL its kernels were done,
// and nothing of its copy-out overlapped them: 23 against 32 GB/s with two contexts on one GPU.)
// framed[i] receives the bytes of block i's chunk (header included) for the seek index.  Returns 0 or -MLZ_ERR_*.
int64_t stream_encode_groups(mlz_ctx* c, int level, uint32_t bs, const uint8_t* src, size_t n, uint8_t* dst, uint64_t mir_base, StreamEncShared* sh,
                             size_t j, size_t k, size_t pg /* blocks per group */, uint32_t* framed) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nblk = (n + bs - 1) / bs;
    const size_t G = (nblk + pg - 1) / pg;
    const size_t mine = j < G ? (G - j + k - 1) / k : 0;                    // my groups: j, j + k, ...
    if (mine == 0) return 0;
    const size_t ostride = (size_t(bs) + 16 + 63) & ~size_t(63);
    const size_t cap_blocks = mine * pg;
    HIPCHK(c, c->d_in.ensure(cap_blocks * size_t(bs) + 64));
    HIPCHK(c, c->d_out.ensure(cap_blocks * ostride + 64));
    HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * cap_blocks));
    HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * cap_blocks + 64));
    // (a page-locked destination: the chunk bodies are placed by a kernel, stream_place_kernel)
    const size_t max_pieces = mir_base ? cap_blocks * ((size_t(bs) + kPlacePiece - 1) / kPlacePiece + 1) : 0;
    Carve pin;
    const auto r_len = pin.take<int64_t>(cap_blocks);
    const auto r_crc = pin.take<uint32_t>(cap_blocks);
    const auto r_place = pin.take<PlaceDesc>(max_pieces, 64);
    int r = ensure_stream_objects(c, 3 * mine, pin.bytes);
    if (r) return r;
    int64_t* h_len = r_len.at(c->pinned2);
    uint32_t* h_crc = r_crc.at(c->pinned2);
    PlaceDesc* h_place = r_place.at(c->pinned2);
    size_t n_place = 0;
    if (mir_base) HIPCHK(c, c->d_place.ensure(max_pieces * sizeof(PlaceDesc)));
    // local slot li * pg + i <-> block (j + li * k) * pg + i of the stream; offsets inside this worker's d_in / d_out
    std::vector<mlz_block_desc> desc(cap_blocks);
    auto first_block = [&](size_t li) { return (j + li * k) * pg; };
    auto count_of = [&](size_t li) { return std::min(pg, nblk - first_block(li)); };
    for (size_t li = 0; li < mine; li++)
        for (size_t i = 0; i < count_of(li); i++) {
            mlz_block_desc& d = desc[li * pg + i];
            d.src_off = (li * pg + i) * size_t(bs); d.src_len = std::min<size_t>(bs, n - (first_block(li) + i) * size_t(bs));
            d.dst_off = (li * pg + i) * ostride; d.dst_cap = ostride;
        }
    uint8_t* d_in = c->d_in.as<uint8_t>();
    uint8_t* d_out = c->d_out.as<uint8_t>();
    hipStream_t sm = c->stream;
    // enqueue everything; nothing below blocks the host
    for (size_t li = 0; li < mine; li++) {
        const size_t l0 = li * pg, cnt = count_of(li);
        const size_t byte0 = first_block(li) * size_t(bs), bytes = std::min(n, (first_block(li) + cnt) * size_t(bs)) - byte0;
        hipEvent_t e_in = c->evpool[3 * li], e_k = c->evpool[3 * li + 1], e_len = c->evpool[3 * li + 2];
        HIPCHK(c, hipMemcpyAsync(d_in + l0 * size_t(bs), src + byte0, bytes, hipMemcpyHostToDevice, c->s_in));
        HIPCHK(c, hipEventRecord(e_in, c->s_in));
        HIPCHK(c, hipStreamWaitEvent(sm, e_in, 0));
        r = encode_device_locked(c, sm, level, d_in, d_out, desc.data() + l0, int(cnt), c->d_len.as<int64_t>() + l0, true);
        if (r) return r;
        r = crc_device_locked(c, sm, d_in, desc.data() + l0, int(cnt), c->d_crc.as<uint32_t>() + l0);
        if (r) return r;
        HIPCHK(c, hipEventRecord(e_k, sm));
        HIPCHK(c, hipStreamWaitEvent(c->s_out, e_k, 0));
        HIPCHK(c, hipMemcpyAsync(h_len + l0, c->d_len.as<int64_t>() + l0, sizeof(int64_t) * cnt, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipMemcpyAsync(h_crc + l0, c->d_crc.as<uint32_t>() + l0, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipEventRecord(e_len, c->s_out));
    }
    // collect, group by group: sizes -> the group's place -> chunk headers (host) and bodies (copy-out stream)
    size_t place_done = 0;
    for (size_t li = 0; li < mine; li++) {
        const size_t g = j + li * k, l0 = li * pg, cnt = count_of(li);
        HIPCHK(c, hipEventSynchronize(c->evpool[3 * li + 2]));
        int64_t gbytes = 0;
        for (size_t i = l0; i < l0 + cnt; i++) {
            if (h_len[i] < 0) return h_len[i];
            gbytes += int64_t(8 + chunk_shape(h_len[i], size_t(desc[i].src_len)).body);
        }
        sh->publish(g, gbytes);
        const int64_t before = sh->base_of(g);
        if (before < 0) return -MLZ_ERR_HIP;   // (the failing worker reports its own error; this one only stops)
        size_t o = (n > 0 ? 10 : 0) + size_t(before);   // (behind the stream header)
        for (size_t i = l0; i < l0 + cnt; i++) {
            const ChunkShape s = chunk_shape(h_len[i], size_t(desc[i].src_len));
            uint8_t* ob = dst + o;
            put_chunk_header(ob, s, h_crc[i]);
            if (s.stored) std::memcpy(ob + 8, src + (first_block(li) + (i - l0)) * size_t(bs), s.body);
            else if (!mir_base) HIPCHK(c, hipMemcpyAsync(ob + 8, d_out + desc[i].dst_off + 1, s.body, hipMemcpyDeviceToHost, c->s_out));
            else place_pieces(desc[i].dst_off + 1, o + 8, s.body, 0, [&](const PlaceDesc& d) { h_place[n_place++] = d; });
            framed[first_block(li) + (i - l0)] = uint32_t(8 + s.body);
            o += 8 + s.body;
        }
        if (mir_base && n_place > place_done) {   // this group's bodies: descriptors up, one launch
            PlaceDesc* d_place = c->d_place.as<PlaceDesc>();
            HIPCHK(c, hipMemcpyAsync(d_place + place_done, h_place + place_done, (n_place - place_done) * sizeof(PlaceDesc), hipMemcpyHostToDevice, c->s_out));
            hipLaunchKernelGGL(stream_place_kernel, dim3(uint32_t(n_place - place_done)), dim3(256), 0, c->s_out, d_out, nullptr, nullptr, reinterpret_cast<uint8_t*>(mir_base),
                               d_place + place_done);
            place_done = n_place;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Stream header, the chunks of every block (by the workers above), EOF chunk, seek index.  `workers`: the contexts the groups are dealt to
// (one context: this thread; more: a thread each, every one under its context's lock).
int64_t stream_encode_over(mlz_ctx* const* workers, size_t k, int level, uint32_t bs, bool add_index, const uint8_t* src, size_t n, uint8_t* dst,
                           size_t dst_cap) {
    mlz_ctx* c0 = workers[0];
    const size_t nblk = (n + bs - 1) / bs;
    const StreamTables plain;
    if (dst_cap < stream_bound(n, bs, add_index, plain)) return -MLZ_ERR_DST_TOO_SMALL;
    if (n > 0) put_stream_head(dst, bs, plain);
    std::vector<uint32_t> framed(nblk, 0);
    if (nblk) {
        // blocks per group: 64 MiB for one device; several devices want a few pipeline steps each (a device with ONE group has nothing to put its
        // copy-out under): at least two groups per device, of 16 MiB or more
        size_t gbytes = kStreamGroupBytes;
        if (k > 1) gbytes = std::min<size_t>(kStreamGroupBytes, std::max<size_t>(size_t(16) << 20, n / (2 * k)));
        const size_t pg = std::max<size_t>(1, gbytes / bs), G = (nblk + pg - 1) / pg;
        if (k > G) k = G;
        StreamEncShared sh(G);
        int64_t rc = 0;
        if (k <= 1) {
            std::lock_guard<std::mutex> lk(c0->mu);
            HIPCHK(c0, hipSetDevice(c0->device));
            rc = stream_encode_groups(c0, level, bs, src, n, dst, pinned_alias(dst, dst_cap), &sh, 0, 1, pg, framed.data());
        } else {
            HIPCHK(c0, hipSetDevice(c0->device));
            const uint64_t mir_base = pinned_alias(dst, dst_cap);
            std::vector<int64_t> rcs(k, 0);
            auto work = [&](size_t j) {
                mlz_ctx* c = workers[j];
                std::lock_guard<std::mutex> lk(c->mu);
                rcs[j] = stream_encode_groups(c, level, bs, src, n, dst, mir_base, &sh, j, k, pg, framed.data());
                if (rcs[j]) {
                    sh.fail();
                    (void)hipStreamSynchronize(c->s_in); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->s_out);   // nothing of this call is left in flight
                }
            };
            std::vector<std::thread> th;
            for (size_t j = 1; j < k; j++) th.emplace_back(work, j);
            work(0);
            for (std::thread& t : th) t.join();
            rc = first_own_verdict(rcs);
        }
        if (rc) return rc;
    }
    size_t o = 0;
    const std::vector<uint8_t> foot = stream_foot(n, bs, plain.head_bytes(), framed, add_index, &o);
    std::memcpy(dst + o, foot.data(), foot.size());
    return int64_t(o + foot.size());
}

// ---- the device-resident Writer over several devices: sources in each device's HBM, the framed stream gathered GPU to GPU ----
// Range j (blocks [b0, b0 + cnt) of the stream, its bytes at d_src on c's device): encode + CRC on the device, sizes and CRCs (12 bytes per
// block) to the host, the run of chunks framed on the device, then moved to its place in d_dst on device dst_dev (the same device: framed in
// place; another one: hipMemcpyPeerAsync, which rides xGMI between the GPUs of a node).  Payload never visits the host.
// stb: the search tables (T > 0), whose builder takes the tail_n bytes at `tail` (host memory) that follow the range in the stream.
int64_t stream_gather_range(mlz_ctx* c, int level, uint32_t bs, const uint8_t* d_src, size_t len, size_t b0, uint8_t* d_dst, int dst_dev, StreamEncShared* sh, size_t j,
                            uint32_t* framed, const StreamTables& stb, const uint8_t* tail, uint32_t tail_n, bool compress) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cnt = (len + bs - 1) / bs;
    if (cnt == 0) { sh->publish(j, 0); return 0; }
    const uint32_t search_m = stb.T ? stb.M : 0, flen = stb.flen(), thdr = 12 + flen;   // thdr: a table chunk's bytes in front of its table
    const uint32_t search_b = mlz::search_table_bits(bs);
    const size_t tab_slot = size_t(1) << (search_b - 3);
    const size_t ostride = (size_t(bs) + 16 + 63) & ~size_t(63);
    HIPCHK(c, c->d_out.ensure(cnt * ostride + 64));
    HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * cnt));
    HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * cnt + 64));
    const size_t max_pieces = cnt * ((size_t(bs) + kPlacePiece - 1) / kPlacePiece + 1 + (search_m ? (tab_slot + kPlacePiece - 1) / kPlacePiece : 0));
    const size_t tcnt = search_m ? cnt : 0;
    Carve pin;   // what comes back: sizes | CRCs | (table bytes or 0, R) | table CRCs; what goes up: pieces | chunk headers | table chunk headers
    const auto r_len = pin.take<int64_t>(cnt);
    const auto r_crc = pin.take<uint32_t>(cnt);
    const auto r_tabinfo = pin.take<uint2>(tcnt);
    const auto r_tabcrc = pin.take<uint32_t>(tcnt);
    const auto r_seclen = pin.take<int64_t>(compress ? tcnt : 0);
    const auto r_place = pin.take<PlaceDesc>(max_pieces, 64);
    const auto r_hdr = pin.take<HdrDesc>(cnt);
    const auto r_tabhdr = pin.take<TabHdrDesc>(tcnt);
    int r = ensure_stream_objects(c, 1, pin.bytes);
    if (r) return r;
    int64_t* h_len = r_len.at(c->pinned2);
    uint32_t* h_crc = r_crc.at(c->pinned2);
    uint2* h_tabinfo = r_tabinfo.at(c->pinned2);
    uint32_t* h_tabcrc = r_tabcrc.at(c->pinned2);
    int64_t* h_seclen = r_seclen.at(c->pinned2);
    PlaceDesc* h_place = r_place.at(c->pinned2);
    HdrDesc* h_hdr = r_hdr.at(c->pinned2);
    TabHdrDesc* h_tabhdr = r_tabhdr.at(c->pinned2);
    std::vector<mlz_block_desc> desc(cnt);
    for (size_t i = 0; i < cnt; i++) {
        desc[i].src_off = i * size_t(bs); desc[i].src_len = std::min<size_t>(bs, len - i * size_t(bs));
        desc[i].dst_off = i * ostride; desc[i].dst_cap = ostride;
    }
    hipStream_t sm = c->stream;
    uint8_t* d_out = c->d_out.as<uint8_t>();
    r = encode_device_locked(c, sm, level, d_src, d_out, desc.data(), int(cnt), c->d_len.as<int64_t>(), true);
    if (r) return r;
    r = crc_device_locked(c, sm, d_src, desc.data(), int(cnt), c->d_crc.as<uint32_t>());
    if (r) return r;
    // compressed tables (MLZ_STREAM_SEARCH_COMPRESS): behind the slots and records, a section area of a slot per table and their lengths
    const size_t sec_off = search_m ? search_tables_extra_off(cnt, search_b) : 0, seclen_off = sec_off + cnt * tab_slot;
    if (search_m) {
        size_t tabinfo_off = 0;
        r = search_tables_build(c, sm, d_src, len, bs, cnt, stb.T, stb.field, search_m, search_b, tail, tail_n, &tabinfo_off, compress ? cnt * tab_slot + cnt * sizeof(int64_t) : 0);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(h_tabinfo, c->d_stab.as<uint8_t>() + tabinfo_off, sizeof(uint2) * cnt, hipMemcpyDeviceToHost, sm));
    }
    HIPCHK(c, hipMemcpyAsync(h_len, c->d_len.p, sizeof(int64_t) * cnt, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(h_crc, c->d_crc.p, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipStreamSynchronize(sm));
    size_t n_tabs = 0;
    if (search_m) {
        // a table goes in front of a block that was stored compressed (writer.go:528-540); its CRC is the stream's, over the table's bytes
        HIPCHK(c, hipGetLastError());
        std::vector<mlz_block_desc> tdesc;
        for (size_t i = 0; i < cnt; i++) {
            if (h_len[i] < 0) return h_len[i];
            if (chunk_shape(h_len[i], size_t(desc[i].src_len)).stored) h_tabinfo[i].x = 0;
            if (h_tabinfo[i].x) tdesc.push_back(mlz_block_desc{i * tab_slot, h_tabinfo[i].x, 0, 0});
        }
        n_tabs = tdesc.size();
        if (n_tabs && compress) {
            // every table's section into its slot of the area, with one byte less of room than the table has: a section that is no shorter
            // is that item's error and nothing is written for it (the chunk then stays 0x45).  The lengths come home with the CRCs.
            std::vector<mlz_block_desc> cdesc(n_tabs);
            for (size_t t = 0; t < n_tabs; t++) cdesc[t] = mlz_block_desc{tdesc[t].src_off, tdesc[t].src_len, sec_off + t * tab_slot, tdesc[t].src_len - 1};
            int64_t* d_seclen = reinterpret_cast<int64_t*>(c->d_stab.as<uint8_t>() + seclen_off);
            r = search_bitmaps_compress_locked(c, sm, c->d_stab.as<uint8_t>(), c->d_stab.as<uint8_t>(), cdesc.data(), int(n_tabs), d_seclen);
            if (r) return r;
            HIPCHK(c, hipMemcpyAsync(h_seclen, d_seclen, sizeof(int64_t) * n_tabs, hipMemcpyDeviceToHost, sm));
        }
        if (n_tabs) {
            HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * (cnt + n_tabs) + 64));
            r = crc_device_locked(c, sm, c->d_stab.as<uint8_t>(), tdesc.data(), int(n_tabs), c->d_crc.as<uint32_t>());
            if (r) return r;
            HIPCHK(c, hipMemcpyAsync(h_tabcrc, c->d_crc.p, sizeof(uint32_t) * n_tabs, hipMemcpyDeviceToHost, sm));
            HIPCHK(c, hipStreamSynchronize(sm));
        }
    }
    // the run's layout: [type][len24][crc][body] per block, a block's table chunk in front of it
    size_t run = 0, n_place = 0, tab_at = 0, wrote46 = 0;   // wrote46: table chunks laid out as 0x46, counted once the run is in place
    auto put_piece = [&](const PlaceDesc& d) { h_place[n_place++] = d; };
    for (size_t i = 0; i < cnt; i++) {
        if (h_len[i] < 0) return h_len[i];
        const ChunkShape s = chunk_shape(h_len[i], size_t(desc[i].src_len));
        framed[b0 + i] = 0;
        if (search_m && h_tabinfo[i].x) {   // 45 len24 | T M B | prefix field | R | crc32le | table
            // (compressed: 46 len24 | the same fields | the section, where that is shorter than the table)
            const bool sect = compress && h_seclen[tab_at] > 0 && h_seclen[tab_at] < int64_t(h_tabinfo[i].x);
            const uint32_t tb = sect ? uint32_t(h_seclen[tab_at]) : h_tabinfo[i].x, tlen = thdr - 4 + tb;
            TabHdrDesc& th = h_tabhdr[tab_at];
            th.dst_off = run; th.n = thdr;
            th.b[0] = sect ? mlz::kChunkSearchTableCompressed : mlz::kChunkSearchTable; th.b[1] = uint8_t(tlen); th.b[2] = uint8_t(tlen >> 8); th.b[3] = uint8_t(tlen >> 16);
            th.b[4] = uint8_t(stb.T); th.b[5] = uint8_t(search_m); th.b[6] = uint8_t(search_b);
            const uint32_t inl = stb.T == 4 ? 0 : flen;   // the field's bytes inside the record
            std::memcpy(th.b + 7, stb.field, inl);
            th.b[7 + inl] = uint8_t(h_tabinfo[i].y);
            std::memcpy(th.b + 8 + inl, &h_tabcrc[tab_at], 4);
            place_pieces(sect ? sec_off + tab_at * tab_slot : i * tab_slot, run + thdr, tb, 2, put_piece);
            wrote46 += sect ? 1 : 0;
            tab_at++;
            framed[b0 + i] = thdr + tb;
            run += thdr + tb;
        }
        h_hdr[i].dst_off = run;
        put_chunk_header(h_hdr[i].b, s, h_crc[i]);
        place_pieces(s.stored ? desc[i].src_off : desc[i].dst_off + 1, run + 8, s.body, s.stored ? 1 : 0, put_piece);
        framed[b0 + i] += uint32_t(8 + s.body);
        run += 8 + s.body;
    }
    sh->publish(j, int64_t(run));
    const int64_t before = sh->base_of(j);
    if (before < 0) return -MLZ_ERR_HIP;
    const size_t base = stb.head_bytes() + size_t(before);   // (a range with a block in it: the stream has a head)
    // frame the run: in place when d_dst is on this device, else in a local buffer that then travels
    const bool local = c->device == dst_dev;
    uint8_t* d_run = d_dst + base;
    if (!local) { HIPCHK(c, c->d_in.ensure(run + 64)); d_run = c->d_in.as<uint8_t>(); }
    Carve up;
    const auto u_place = up.take<PlaceDesc>(n_place);
    const auto u_hdr = up.take<HdrDesc>(cnt);
    const auto u_tabhdr = up.take<TabHdrDesc>(n_tabs);
    HIPCHK(c, c->d_place.ensure(up.bytes));
    PlaceDesc* d_place = u_place.at(c->d_place.p);
    HdrDesc* d_hdr = u_hdr.at(c->d_place.p);
    TabHdrDesc* d_tabhdr = u_tabhdr.at(c->d_place.p);
    if (n_place) HIPCHK(c, hipMemcpyAsync(d_place, h_place, n_place * sizeof(PlaceDesc), hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(d_hdr, h_hdr, cnt * sizeof(HdrDesc), hipMemcpyHostToDevice, sm));
    if (n_tabs) HIPCHK(c, hipMemcpyAsync(d_tabhdr, h_tabhdr, n_tabs * sizeof(TabHdrDesc), hipMemcpyHostToDevice, sm));
    if (n_place) hipLaunchKernelGGL(stream_place_kernel, dim3(uint32_t(n_place)), dim3(256), 0, sm, d_out, d_src, search_m ? c->d_stab.as<uint8_t>() : nullptr, d_run, d_place);
    if (n_tabs) {
        TabLongField lf{};
        if (stb.T == 4) { lf.n = flen; std::memcpy(lf.b, stb.field, flen); }
        hipLaunchKernelGGL(stream_tabhdr_kernel, dim3(uint32_t((n_tabs + 63) / 64)), dim3(64), 0, sm, d_run, d_tabhdr, uint32_t(n_tabs), lf);
    }
    hipLaunchKernelGGL(stream_hdr_kernel, dim3(uint32_t((cnt + 63) / 64)), dim3(64), 0, sm, d_run, d_hdr, uint32_t(cnt));
    if (!local) HIPCHK(c, hipMemcpyPeerAsync(d_dst + base, dst_dev, d_run, c->device, run, sm));
    HIPCHK(c, hipStreamSynchronize(sm));
    HIPCHK(c, hipGetLastError());
    c->tables_compressed += wrote46;
    return 0;
}

// The device-resident Writer behind mlz_stream_encode_gather_device, _tables and _long_prefix, which hand in their configuration as stb
int64_t stream_encode_gather_device_with(mlz_ctx* c, int level, uint32_t block_size, uint32_t flags, const StreamTables& stb, const uint8_t* const* d_src,
                                         const size_t* src_len, int n_ranges, uint8_t* d_dst, size_t dst_cap) {
    if (!c || !d_src || !src_len || n_ranges <= 0 || !d_dst) return -MLZ_ERR_ARG;
    if (block_size < kMinStreamBlock || block_size > kMaxBlockSize) return -MLZ_ERR_ARG;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    if (!stb.valid) return -MLZ_ERR_ARG;
    const bool add_index = (flags & MLZ_STREAM_ADD_INDEX) != 0, compress = (flags & MLZ_STREAM_SEARCH_COMPRESS) != 0;
    if (compress && !stb.T) return -MLZ_ERR_ARG;   // nothing to compress
    Workers w(c);
    for (size_t q = 0; q < w.n; q++) { std::lock_guard<std::mutex> lk(w.list[q]->mu); w.list[q]->tables_compressed = 0; }
    const size_t k = size_t(n_ranges);
    // every range on the device that holds it; all but the last are whole blocks (a short block ends a stream)
    std::vector<mlz_ctx*> own(k, nullptr);
    std::vector<size_t> first(k + 1, 0);
    size_t n = 0;
    for (size_t j = 0; j < k; j++) {
        if (src_len[j] && !d_src[j]) return -MLZ_ERR_ARG;
        if (j + 1 < k && src_len[j] % block_size) return -MLZ_ERR_ARG;
        first[j + 1] = first[j] + (src_len[j] + block_size - 1) / block_size;
        n += src_len[j];
        if (!src_len[j]) { own[j] = w.list[0]; continue; }
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_src[j]) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); return -MLZ_ERR_ARG; }
        // the contexts on that device (one, unless the device was listed twice) take its ranges in turn
        size_t on_dev = 0, earlier = 0;
        for (size_t q = 0; q < w.n; q++) on_dev += w.list[q]->device == at.device ? 1 : 0;
        if (!on_dev) return -MLZ_ERR_ARG;
        for (size_t i = 0; i < j; i++) earlier += (src_len[i] && own[i]->device == at.device) ? 1 : 0;
        for (size_t q = 0, hit = 0; q < w.n; q++)
            if (w.list[q]->device == at.device && hit++ == earlier % on_dev) own[j] = w.list[q];
    }
    hipPointerAttribute_t dat;
    if (hipPointerGetAttributes(&dat, d_dst) != hipSuccess || dat.type != hipMemoryTypeDevice) { (void)hipGetLastError(); return -MLZ_ERR_ARG; }
    const int dst_dev = dat.device;
    if (dst_cap < stream_bound(n, block_size, add_index, stb)) return -MLZ_ERR_DST_TOO_SMALL;
    // search tables: a range's last block indexes prefixes and windows that run into the bytes behind it, stb.overlap() of them at the most, which
    // the host hands over.  They all lie in the first non-empty range that follows: every range but the last is a whole number of blocks of
    // at least 4 KiB, more than any overlap (K - 1 + M + E <= 271), and behind the last range the stream ends (zeros stand for what is missing)
    const size_t need = stb.T ? stb.overlap() : 0;
    std::vector<uint8_t> tails(k * need + 1, 0);
    std::vector<uint32_t> tail_n(k, 0);
    for (size_t j = 0; need && j + 1 < k; j++) {
        size_t q = j + 1;
        while (q < k && !src_len[q]) q++;
        if (q == k || !src_len[j]) continue;
        tail_n[j] = uint32_t(std::min(need, src_len[q]));
        if (hipSetDevice(own[q]->device) != hipSuccess || hipMemcpy(&tails[j * need], d_src[q], tail_n[j], hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -MLZ_ERR_HIP; }
    }
    std::vector<uint32_t> framed(first[k], 0);
    StreamEncShared sh(k);
    std::vector<int64_t> rcs(k, 0);
    // two ranges may share a context (more ranges than contexts on a device): they queue on its lock in range order — the base_of() hand-over
    // only ever waits for LOWER ranges, which hold or have held the lock first when threads start in order; to be safe against any start order a
    // context's ranges run on ONE thread, lowest first
    std::vector<std::vector<size_t>> by_ctx;
    std::vector<mlz_ctx*> ctxs;
    for (size_t j = 0; j < k; j++) {
        size_t q = 0;
        while (q < ctxs.size() && ctxs[q] != own[j]) q++;
        if (q == ctxs.size()) { ctxs.push_back(own[j]); by_ctx.emplace_back(); }
        by_ctx[q].push_back(j);
    }
    auto work = [&](size_t q) {
        mlz_ctx* kc = ctxs[q];
        std::lock_guard<std::mutex> lk(kc->mu);
        for (size_t j : by_ctx[q]) {
            rcs[j] = stream_gather_range(kc, level, block_size, d_src[j], src_len[j], first[j], d_dst, dst_dev, &sh, j, framed.data(), stb, &tails[j * need], tail_n[j], compress);
            if (rcs[j]) { sh.fail(); (void)hipStreamSynchronize(kc->stream); }
        }
    };
    std::vector<std::thread> th;
    for (size_t q = 1; q < ctxs.size(); q++) th.emplace_back(work, q);
    work(0);
    for (std::thread& t : th) t.join();
    const int64_t rc = first_own_verdict(rcs);
    if (rc) {   // a call that fails has written no stream: counter 15 says so, whatever ranges had come through
        for (size_t q = 0; q < w.n; q++) { std::lock_guard<std::mutex> lk(w.list[q]->mu); w.list[q]->tables_compressed = 0; }
        std::lock_guard<std::mutex> lk(c->mu);
        for (size_t j = 0; j < k; j++) if (rcs[j] == rc) { c->err = own[j]->err; break; }
        return rc;
    }
    // stream header, EOF chunk and index: a few bytes from the host (writer.go:463-467, :1063-1122)
    mlz_ctx* c0 = w.list[0];
    std::lock_guard<std::mutex> lk(c0->mu);
    HIPCHK(c0, hipSetDevice(dst_dev));
    if (n > 0) {
        uint8_t head[17 + mlz::kSearchMaxField];
        put_stream_head(head, block_size, stb);
        HIPCHK(c0, hipMemcpy(d_dst, head, stb.head_bytes(), hipMemcpyHostToDevice));
    }
    size_t o = 0;
    const std::vector<uint8_t> foot = stream_foot(n, block_size, stb.head_bytes(), framed, add_index, &o);
    HIPCHK(c0, hipMemcpy(d_dst + o, foot.data(), foot.size(), hipMemcpyHostToDevice));
    return int64_t(o + foot.size());
}

// mlz_stream_bound, _tables and _long_prefix
int64_t stream_bound_checked(uint64_t n, uint32_t block_size, uint32_t flags, const StreamTables& stb) {
    if (block_size < kMinStreamBlock || block_size > kMaxBlockSize || !stb.valid) return -MLZ_ERR_ARG;
    return int64_t(stream_bound(n, block_size, (flags & MLZ_STREAM_ADD_INDEX) != 0, stb));
}

struct StreamChunk {
    uint8_t type;
    uint32_t crc;
    size_t body_off, body_len;  // tokens (0x02 / 0x03) or raw bytes (0x01) inside the stream
    size_t n, out_off;
    size_t hdr_off;             // where the chunk's 4-byte header lies in the stream (a sidecar's references name it)
};

// WalkReader's `data`: the chunk appended to `chunks`, its body and header offsets counted from `base` bytes in front of the stream
auto stream_chunk_sink(std::vector<StreamChunk>* chunks, uint64_t base = 0) {
    return [chunks, base](uint8_t type, uint32_t crc, uint64_t body_off, uint64_t body_len, uint64_t n, uint64_t out_off, uint64_t hdr_off) {
        chunks->push_back(StreamChunk{type, crc, size_t(base + body_off), size_t(body_len), size_t(n), size_t(out_off), size_t(base + hdr_off)});
    };
}

// Reader.Read's chunk walk (reader.go:248-543) over a stream in host memory: the walk, the records and the running state of
// mlz_stream_walk.h, header by header, up to the first error and not a byte further.  Fills `chunks`, returns total decoded bytes or
// -MLZ_ERR_*; on an error `chunks` holds the chunks in front of it, which the Reader decodes (and may fail on) before it reaches the error.
int64_t stream_parse(const uint8_t* src, size_t slen, std::vector<StreamChunk>* chunks) {
    mlz::WalkReader rd(kMaxBlockSize);
    int err = 0;
    mlz::walk_headers(src, slen, 0, slen, false, mlz::kWalkNoCap, [&](uint64_t e) {
        err = rd.step(mlz::walk_classify(src, slen, e), stream_chunk_sink(chunks));
        return err == 0;
    });
    return err ? err : rd.finish();
}

// One chunk of a decode list: `at` is where a compressed chunk (0x02 / 0x03) is decoded to, and where the bytes of a stored one (0x01) lie
// for its CRC.  The targets of one list may lie in several allocations (the caller's destination, the context's scratch, the stream itself).
struct ChunkJob { size_t ck; const uint8_t* at; };

// The decode and CRC descriptors of one group, jobs [j0, j1) of a list.  A compressed chunk gets a decode descriptor; every chunk gets one
// CRC descriptor, a 0x03 chunk's over its token bytes (reader.go:341-344), the others' over the bytes at `at`.  The chunk at stream offset
// body_off has its tokens at tok + (body_off - tok_bias): the stream itself, or the part of it a worker copied in.  Each list has its
// lowest address as base and holds distances from it (the decode's sources: from tok).  res_idx[j]: job j's place among the decode
// results, which the group's come to from `res0` on.
struct ChunkGroupDescs { std::vector<mlz_block_desc> dec, crc; uintptr_t dbase, cbase; };
void chunk_group_descs(const uint8_t* tok, size_t tok_bias, const std::vector<StreamChunk>& chunks, const ChunkJob* jobs, size_t j0, size_t j1, size_t res0,
                       size_t* res_idx, ChunkGroupDescs* d) {
    auto crc_at = [&](size_t j) {
        const StreamChunk& ck = chunks[jobs[j].ck];
        return reinterpret_cast<uintptr_t>(ck.type == kChunkMinLZCompCRC ? tok + (ck.body_off - tok_bias) : jobs[j].at);
    };
    d->dbase = d->cbase = ~uintptr_t(0);
    for (size_t j = j0; j < j1; j++) {
        if (chunks[jobs[j].ck].type != kChunkUncompressed) d->dbase = std::min(d->dbase, reinterpret_cast<uintptr_t>(jobs[j].at));
        d->cbase = std::min(d->cbase, crc_at(j));
    }
    d->dec.clear(); d->crc.clear();
    for (size_t j = j0; j < j1; j++) {
        const StreamChunk& ck = chunks[jobs[j].ck];
        d->crc.push_back(mlz_block_desc{uint64_t(crc_at(j) - d->cbase), ck.type == kChunkMinLZCompCRC ? ck.body_len : ck.n, 0, 0});
        if (ck.type == kChunkUncompressed) continue;
        res_idx[j] = res0 + d->dec.size();
        d->dec.push_back(mlz_block_desc{ck.body_off - tok_bias, ck.body_len, uint64_t(reinterpret_cast<uintptr_t>(jobs[j].at) - d->dbase), ck.n});
    }
}

// Chunks [k0, k1) of a parsed stream: their bytes to the device, decode, CRC, output to its final place in dst (every chunk's output offset
// is known from the chunk walk, so ranges of one stream are independent: reader.go:830-859 hands blocks to goroutines the same way).
// The groups (range_group_ends), their descriptors (chunk_group_descs) and the verdict (chunk_job_verdict) are the device-resident Reader's;
// the pipeline is this function's own: copy-in on s_in, kernels on c->stream, results and output home on s_out, three events per group.
// Returns 0, or the error of the FIRST chunk of the range that fails (-MLZ_ERR_*).
int64_t stream_decode_range(mlz_ctx* c, bool ignore_crc, const uint8_t* src, const std::vector<StreamChunk>& chunks, size_t k0, size_t k1, uint8_t* dst,
                            uint64_t mir_total /* bytes of dst that may be written through a pinned alias; 0 = ask nothing */) {
    if (k1 <= k0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nck = k1 - k0;
    std::vector<size_t> gend;   // groups of chunks covering ~64 MiB of output; the range's part of the stream image goes to the device group by group
    mlz::range_group_ends(nck, [&](size_t i) { return uint64_t(chunks[k0 + i].n); }, &gend);
    // this worker's buffers hold its range only: stream bytes from s_base, output from o_base
    const size_t s_base = chunks[k0].body_off, s_end = chunks[k1 - 1].body_off + chunks[k1 - 1].body_len;
    const size_t o_base = chunks[k0].out_off, o_end = chunks[k1 - 1].out_off + chunks[k1 - 1].n;
    HIPCHK(c, c->d_in.ensure(s_end - s_base + 64));
    HIPCHK(c, c->d_out.ensure(o_end - o_base + 64));
    HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * nck));
    HIPCHK(c, c->d_crc.ensure(sizeof(uint32_t) * nck + 64));
    int r = ensure_stream_objects(c, 3 * gend.size(), nck * 12);
    if (r) return r;
    int64_t* h_len = static_cast<int64_t*>(c->pinned2);
    uint32_t* h_crc = reinterpret_cast<uint32_t*>(h_len + nck);
    uint8_t* d_in = c->d_in.as<uint8_t>();
    uint8_t* d_out = c->d_out.as<uint8_t>();
    hipStream_t sm = c->stream;
    std::vector<ChunkJob> jobs(nck);   // job i - k0: chunk i, in this worker's d_out
    for (size_t i = k0; i < k1; i++) jobs[i - k0] = ChunkJob{i, d_out + (chunks[i].out_off - o_base)};
    std::vector<size_t> res_idx(nck, 0);
    ChunkGroupDescs gd;
    // A page-locked destination is written by the decode kernels themselves, tile by tile as they finish (the copy-out of a pinned
    // buffer runs as shader copies on this ROCm build and queues up behind every kernel of the stream: 11.4 ms against 4.4 ms into
    // pageable memory for 100 MB); stored chunks are copied on the host, from the stream image the caller handed in.
    const uint64_t mir_base = (mir_total && c->decode_algo == 0 && c->general_algo == 0) ? pinned_alias(dst, size_t(mir_total)) : 0;
    std::vector<uint64_t> dmir;
    for (size_t g = 0, r0 = 0; g < gend.size(); r0 = gend[g++]) {   // r0, r1: the group's chunks, counted inside the range
        const size_t r1 = gend[g], c0 = k0 + r0, c1 = k0 + r1;
        hipEvent_t e_in = c->evpool[3 * g], e_k = c->evpool[3 * g + 1], e_out = c->evpool[3 * g + 2];
        // stream bytes of this group: from its first chunk's body to the end of its last chunk's body
        const size_t s0 = chunks[c0].body_off, s1 = chunks[c1 - 1].body_off + chunks[c1 - 1].body_len;
        HIPCHK(c, hipMemcpyAsync(d_in + (s0 - s_base), src + s0, s1 - s0, hipMemcpyHostToDevice, c->s_in));
        HIPCHK(c, hipEventRecord(e_in, c->s_in));
        HIPCHK(c, hipStreamWaitEvent(sm, e_in, 0));
        dmir.clear();
        for (size_t i = c0; i < c1; i++) {
            const StreamChunk& ck = chunks[i];
            if (ck.type != kChunkUncompressed) { dmir.push_back(mir_base + ck.out_off); continue; }
            HIPCHK(c, hipMemcpyAsync(d_out + (ck.out_off - o_base), d_in + (ck.body_off - s_base), ck.n, hipMemcpyDeviceToDevice, sm));
            if (mir_base) std::memcpy(dst + ck.out_off, src + ck.body_off, ck.n);
        }
        // the group's decode results come to h_len[r0 .. r0 + its compressed chunks), compacted; its CRCs to h_crc[r0 .. r1)
        chunk_group_descs(d_in, s_base, chunks, jobs.data(), r0, r1, r0, res_idx.data(), &gd);
        if (!gd.dec.empty()) {
            r = decode_device_locked(c, sm, d_in, reinterpret_cast<uint8_t*>(gd.dbase), gd.dec.data(), int(gd.dec.size()), c->d_len.as<int64_t>() + r0, true,
                                     mir_base ? dmir.data() : nullptr, false);
            if (r) return r;
        }
        if (!ignore_crc) {
            r = crc_device_locked(c, sm, reinterpret_cast<const uint8_t*>(gd.cbase), gd.crc.data(), int(r1 - r0), c->d_crc.as<uint32_t>() + r0);
            if (r) return r;
        }
        HIPCHK(c, hipEventRecord(e_k, sm));
        HIPCHK(c, hipStreamWaitEvent(c->s_out, e_k, 0));
        if (!gd.dec.empty())
            HIPCHK(c, hipMemcpyAsync(h_len + r0, c->d_len.as<int64_t>() + r0, sizeof(int64_t) * gd.dec.size(), hipMemcpyDeviceToHost, c->s_out));
        if (!ignore_crc)
            HIPCHK(c, hipMemcpyAsync(h_crc + r0, c->d_crc.as<uint32_t>() + r0, sizeof(uint32_t) * (r1 - r0), hipMemcpyDeviceToHost, c->s_out));
        const size_t o0 = chunks[c0].out_off, o1 = chunks[c1 - 1].out_off + chunks[c1 - 1].n;
        if (!mir_base) HIPCHK(c, hipMemcpyAsync(dst + o0, d_out + (o0 - o_base), o1 - o0, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipEventRecord(e_out, c->s_out));
    }
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    for (size_t j = 0; j < nck; j++) {
        const StreamChunk& ck = chunks[k0 + j];
        const bool compressed = ck.type != kChunkUncompressed;
        const int64_t v = mlz::chunk_job_verdict(compressed, compressed ? h_len[res_idx[j]] : 0, ck.n, !ignore_crc, ignore_crc ? 0 : h_crc[j], ck.crc);
        if (v) return v;
    }
    return 0;
}

// The parsed chunks (total: their decoded bytes) dealt to the workers; returns total or the first error in stream order.
int64_t stream_decode_chunks(mlz_ctx* const* workers, size_t k, bool ignore_crc, const uint8_t* src, std::vector<StreamChunk>& chunks, uint8_t* dst,
                             size_t total) {
    for (size_t j = 0; j < k; j++) { std::lock_guard<std::mutex> lk(workers[j]->mu); begin_decode_call(workers[j]); }   // (workers that get no chunk included)
    const size_t nck = chunks.size();
    if (nck == 0) return 0;
    if (k > nck) k = nck;
    if (k <= 1) {
        mlz_ctx* c = workers[0];
        std::lock_guard<std::mutex> lk(c->mu);
        const int64_t r = stream_decode_range(c, ignore_crc, src, chunks, 0, nck, dst, uint64_t(total));
        return r ? r : int64_t(total);
    }
    // range j ends where the output passes j + 1 k-ths of the total
    std::vector<size_t> cut(k + 1, nck);
    cut[0] = 0;
    {
        size_t j = 1;
        for (size_t i = 0; i < nck && j < k; i++) {
            const size_t end = chunks[i].out_off + chunks[i].n;
            while (j < k && end * k >= size_t(total) * j) cut[j++] = i + 1;
        }
    }
    std::vector<int64_t> rcs(k, 0);
    auto work = [&](size_t j) {
        mlz_ctx* c = workers[j];
        std::lock_guard<std::mutex> lk(c->mu);
        rcs[j] = stream_decode_range(c, ignore_crc, src, chunks, cut[j], cut[j + 1], dst, uint64_t(total));
        if (rcs[j]) { (void)hipStreamSynchronize(c->s_in); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->s_out); }
    };
    std::vector<std::thread> th;
    for (size_t j = 1; j < k; j++) th.emplace_back(work, j);
    work(0);
    for (std::thread& t : th) t.join();
    for (size_t j = 0; j < k; j++) if (rcs[j]) return rcs[j];
    return int64_t(total);
}

// The chunk walk, then the chunks dealt to `workers` in contiguous ranges of about equal output (one worker: this thread).
// The Reader reports the first error in stream order: the lowest failing range's.
// A framing error comes after the chunks in front of it: those are decoded and checked first, and their first error wins; the framing
// error is reported only when they all pass (and fit in dst: else -MLZ_ERR_DST_TOO_SMALL, where the Reader's write would fail).
int64_t stream_decode_over(mlz_ctx* const* workers, size_t k, bool ignore_crc, const uint8_t* src, size_t slen, uint8_t* dst, size_t dst_cap) {
    std::vector<StreamChunk> chunks;
    const int64_t parsed = stream_parse(src, slen, &chunks);
    if (parsed < 0) {
        const size_t prefix = chunks.empty() ? 0 : chunks.back().out_off + chunks.back().n;
        if (prefix > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;
        const int64_t r = prefix ? stream_decode_chunks(workers, k, ignore_crc, src, chunks, dst, prefix) : 0;
        return r < 0 ? r : parsed;
    }
    if (size_t(parsed) > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;
    return stream_decode_chunks(workers, k, ignore_crc, src, chunks, dst, size_t(parsed));
}

}  // namespace

extern "C" {

int64_t mlz_stream_bound(uint64_t n, uint32_t block_size, uint32_t flags) { return stream_bound_checked(n, block_size, flags, stream_tables_config(flags, nullptr)); }
int64_t mlz_stream_bound_tables(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_tables* cfg) { return stream_bound_checked(n, block_size, flags, stream_tables_config(flags, cfg)); }
int64_t mlz_stream_bound_long_prefix(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_long_prefix* cfg) { return stream_bound_checked(n, block_size, flags, stream_long_prefix_config(flags, cfg)); }

int64_t mlz_stream_encode(mlz_ctx* c, int level, uint32_t block_size, uint32_t flags, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
    if (!c || (!src && n) || !dst) return -MLZ_ERR_ARG;
    if (block_size < kMinStreamBlock || block_size > kMaxBlockSize) return -MLZ_ERR_ARG;  // writer.go:1238-1246
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    if (flags & MLZ_STREAM_SEARCH_TABLES) return -MLZ_ERR_ARG;   // search tables: the device-resident Writer only
    Workers w(c);
    return stream_encode_over(w.list, w.n, level, block_size, (flags & MLZ_STREAM_ADD_INDEX) != 0, src, n, dst, dst_cap);
}

// The device-resident Writer: each call converts its configuration; the arguments are checked in one place, stream_encode_gather_device_with
int64_t mlz_stream_encode_gather_device(mlz_ctx* c, int level, uint32_t block_size, uint32_t flags, const uint8_t* const* d_src, const size_t* src_len,
                                        int n_ranges, uint8_t* d_dst, size_t dst_cap) {
    return stream_encode_gather_device_with(c, level, block_size, flags, stream_tables_config(flags, nullptr), d_src, src_len, n_ranges, d_dst, dst_cap);
}
int64_t mlz_stream_encode_gather_device_tables(mlz_ctx* c, int level, uint32_t block_size, uint32_t flags, const mlz_search_tables* cfg, const uint8_t* const* d_src,
                                               const size_t* src_len, int n_ranges, uint8_t* d_dst, size_t dst_cap) {
    return stream_encode_gather_device_with(c, level, block_size, flags, stream_tables_config(flags, cfg), d_src, src_len, n_ranges, d_dst, dst_cap);
}
int64_t mlz_stream_encode_gather_device_long_prefix(mlz_ctx* c, int level, uint32_t block_size, uint32_t flags, const mlz_search_long_prefix* cfg,
                                                    const uint8_t* const* d_src, const size_t* src_len, int n_ranges, uint8_t* d_dst, size_t dst_cap) {
    return stream_encode_gather_device_with(c, level, block_size, flags, stream_long_prefix_config(flags, cfg), d_src, src_len, n_ranges, d_dst, dst_cap);
}

int64_t mlz_stream_decoded_len(const uint8_t* src, size_t n) {
    if (!src && n) return -MLZ_ERR_ARG;
    std::vector<StreamChunk> chunks;
    return stream_parse(src, n, &chunks);
}

int64_t mlz_stream_decoded_prefix_len(const uint8_t* src, size_t n) {
    if (!src && n) return -MLZ_ERR_ARG;
    std::vector<StreamChunk> chunks;
    const int64_t r = stream_parse(src, n, &chunks);
    if (r >= 0) return r;
    return chunks.empty() ? 0 : int64_t(chunks.back().out_off + chunks.back().n);
}

int64_t mlz_stream_decode(mlz_ctx* c, uint32_t flags, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
    if (!c || (!src && n) || (!dst && dst_cap)) return -MLZ_ERR_ARG;
    Workers w(c);
    return stream_decode_over(w.list, w.n, (flags & MLZ_STREAM_IGNORE_CRC) != 0, src, n, dst, dst_cap);
}

}  // extern "C"
