// mlz_hip.hip — C ABI (include/minlz_hip.h) + launch logic of the MI355X MinLZ block codec.
//
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC
// No CPU codec lives in this library: every encode/decode call runs the HIP kernels, and a HIP
// failure is reported as -MLZ_ERR_HIP (the Go wrapper then falls back to upstream's CPU path).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/minlz_hip.h"
#include "../../include/minlz_hip_search_batch.h"
#include "../../include/minlz_hip_search_batch_prune.h"
#include "../../include/minlz_hip_stream_set.h"
#include "../../include/minlz_hip_stream_set_tables.h"
#include "../../include/minlz_hip_search_compressed.h"
#include "../../include/minlz_hip_search_compress.h"
#include "../../include/minlz_hip_sidecar_extract.h"
#include "../../include/minlz_hip_record_index_store.h"
#include "../../include/minlz_hip_encode_batch_tables.h"
#include "mlz_format.h"
#include "mlz_kernels.h"

#include "mlz_encode.hip.inc"
#include "mlz_encode2.hip.inc"
#include "mlz_decode_serial.hip.inc"
#include "mlz_toktab.h"
#include "mlz_stream_search.h"
#include "mlz_search_compressed.h"
#include "mlz_stream_set_tables.h"
#include "mlz_decode.hip.inc"
#include "mlz_decode_index.hip.inc"
#include "mlz_decode_exec.hip.inc"
#include "mlz_decode_general.hip.inc"
#include "mlz_crc.hip.inc"

using namespace mlz;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = n + n / 4 + 4096;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() { return static_cast<T*>(p); }
};

// The layout of a workspace (a DevBuf, the pinned result buffer c->pinned2), region by region: a bump allocator over a byte count.  ensure()
// of either kind frees and reallocates a buffer that grows, so a pointer taken before it is stale.  Hence the order of every phase: take all
// of its regions, ensure the buffer ONCE with `bytes`, then turn regions into pointers — at(base) is the only way to one.
template <class T> struct Region {
    size_t off;
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off); }
};
struct Carve {
    size_t bytes = 0;
    template <class T> Region<T> take(size_t count, size_t align = 16) {
        const size_t off = (bytes + align - 1) & ~(align - 1);
        bytes = off + count * sizeof(T);
        return Region<T>{off};
    }
};

constexpr size_t kProfTiles = 4096;                      // debug timeline: tiles recorded by the exec pass
constexpr size_t kProfBytes = 256 + kProfTiles * 32;

// Levels served on the device (encode.go:25-43); LevelSmallest (3) stays on the host side of the boundary.
inline bool valid_level(int level) { return level >= MLZ_LEVEL_SUPERFAST && level <= MLZ_LEVEL_BALANCED; }

enum { T_FAR = 0, T_ENC_TILES, T_ENC_LAYOUT, T_ENC_GATHER, T_DEC_PARSE, T_DEC_CHAIN, T_DEC_INDEX, T_DEC_EXEC, T_DEC_SERIAL, T_CRC, T_ENC_SER, T_DEC_GENERAL, T_COUNT };
const char* kTimerNames[T_COUNT] = {"enc_far_build", "enc_tiles", "enc_layout", "enc_gather", "dec_parse", "dec_chain", "dec_index", "dec_exec", "dec_serial", "crc", "enc_serialize", "dec_general"};

}  // namespace

// One single-block host call waiting to be run (see submit_single below).
struct SingleReq {
    bool encode, with_header, has_dlen;
    int level;
    const uint8_t* src; size_t n;
    uint8_t* dst; size_t cap;
    size_t dlen;      // decode_block: exact decoded length
    int64_t out = 0;  // bytes produced (or a negative per-block error)
    int rc = 0;       // failure of the whole batch
    bool done = false;
    bool same_kind(const SingleReq& o) const { return encode == o.encode && with_header == o.with_header && has_dlen == o.has_dlen && level == o.level; }
};

constexpr size_t kHostGroupEncodeDefault = 32u << 20, kHostGroupDecodeDefault = 48u << 20;  // see host_batch

struct mlz_ctx {
    int device = 0;
    // mlz_init_devices: the per-device contexts this one deals blocks to.  Such a context owns no device state of its own: every entry point
    // either fans out over `kids` (batches, streams), hands a single-block call to one of them in turn, or routes a device-resident call to the
    // kid whose device holds the buffers.
    std::vector<mlz_ctx*> kids;
    std::atomic<uint32_t> rr{0};
    std::mutex mu;
    // combining queue of the single-block host calls
    std::mutex q_mu;
    std::condition_variable q_cv;
    std::vector<SingleReq*> q_pending;
    bool q_leader = false;
    uint64_t q_batches = 0, q_requests = 0;  // mlz_get_counter
    uint64_t acc_call = 0;                   // the decode call (dec_call) whose first group has reset d_gen_acc
    uint64_t dec_call = 0;                   // call_seq at the start of the last decode API call: its host groups, stream groups and internal groups share it
    std::string err;
    std::string dev_name;
    hipStream_t stream = nullptr;  // used by the host-pointer calls
    // descriptors
    // Block descriptors on the device, one set per kind of call (0 encode / crc, 1 decode): an encode and a decode that
    // alternate (a Writer next to a Reader, bench.py) each find their descriptors already uploaded.
    DevBuf d_blocks_k[2], d_tile_block_k[2], d_seg_block_k[2];
    DevBuf d_place;                          // mlz_stream_encode into pinned memory: placement descriptors
    std::vector<BlockInfo> h_blocks, h_blocks_prev_k[2];
    int dk = 0;  // kind of the call in progress
    DevBuf& d_blocks_cur() { return d_blocks_k[dk]; }
    DevBuf& d_tile_block_cur() { return d_tile_block_k[dk]; }
    DevBuf& d_seg_block_cur() { return d_seg_block_k[dk]; }
    std::vector<uint32_t> h_tile_block, h_seg_block;
    // descriptor staging: two page-locked buffers used in turn, so that the upload of one internal group (device_group below) does not make
    // the host wait for the kernels of the group before it
    void* pinned_k[2] = {nullptr, nullptr};
    size_t pinned_cap_k[2] = {0, 0};
    hipEvent_t upload_done_k[2] = {nullptr, nullptr};
    bool upload_pending_k[2] = {false, false};
    int up_slot = 0;
    // Device batches run in internal groups of about this many bytes of uncompressed data (option MLZ_OPT_DEVICE_GROUP): the workspace is then
    // bounded by the group, not by the batch (round 4: 42 GB of decode workspace for a 4 GiB batch).  Throughput is flat from 64 x 8 MiB blocks on.
    size_t device_group = size_t(512) << 20;
    // One workspace serves every call on this context: a call on another stream first waits (on the device) for the
    // previous call's last launch, so descriptors, scratch and flags are never shared by two calls in flight.
    hipEvent_t ws_done = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    bool ws_recorded = false;   // mlz_release_stream: ws_done already covers the last call (its stream may be gone by the next one)
    // encode workspace
    DevBuf d_scratch, d_tile_size, d_tile_out, d_flags, d_far, d_recs, d_piece_cnt, d_farbin;
    DevBuf d_stab;               // the device-resident Writer's block search tables: 2^(B - 3) bytes per block of a range, 8 bytes of verdict each
    // compressed search tables, the write side (mlz_search_tables_compress.hip.inc): the kernels' records, codes and descriptions, and the host's
    // item and job lists, which outlive the launches of a call that synchronises later
    DevBuf d_cstw;
    std::vector<mlz::CstwItem> h_cstw_items;
    std::vector<mlz::CstwJob> h_cstw_jobs;
    uint64_t tables_compressed = 0;   // table chunks the last device Writer or sidecar build call wrote as 0x46 (mlz_get_counter 15)
    // decode workspace
    DevBuf d_dec, d_idx;
    DevBuf d_walk, d_walk_tab;   // the device-resident Reader's chunk walk: exit tables (8 bytes per stream byte) and the chunk table
    DevBuf d_batch;              // the batch calls over many streams: counts and places of the batch walk (8 bytes per stream, a flag bit each); its table is d_walk_tab
    DevBuf d_batch_desc;         // ... and the streams' descriptors on the device (32 bytes per stream)
    uint64_t batch_long = 0;     // streams the last batch call sent through the region walk (mlz_get_counter 12)
    uint64_t table_slot_bytes = 0;   // bytes of table slots the last stream batch encode carved from d_stab (mlz_get_counter 17)
    DevBuf d_range;              // the device-resident ReadSeeker: where partly wanted chunks of a group are decoded (a group plus one block at the most)
    DevBuf d_rplan;              // mlz_dev_reader_read_device: the plan kernels' workspace (16 bytes per range, 28 per chunk of the stream)
    DevBuf d_records, d_rwin;    // mlz_dev_reader_search_records: what lives across its read phase (the occurrences, windows and records: about 100 bytes per occurrence), and the merged windows' bytes (at most the decoded size)
    uint64_t range_plan_host = 0;   // plan bytes that crossed between host and device in the last mlz_dev_reader_read_device (mlz_get_counter 9)
    uint64_t search_plan_bytes = 0;                 // the last mlz_stream_search_batch_device_pruned: bytes its plan brought to the host, the classes' configurations apart (mlz_get_counter 16)
    uint64_t search_compressed = 0;                 // of search_tables, the chunks whose usable table came from a compressed chunk, 0x46 (mlz_get_counter 14)
    uint64_t search_chunks = 0, search_tables = 0;  // the last mlz_dev_reader_search: chunks decoded or copied, chunks with a usable table (mlz_get_counter 10 / 11)
    uint64_t range_chunks = 0, range_scratch = 0;   // the last range read: chunks decoded or copied, decoded bytes that went through d_range (mlz_get_counter 7 / 8)
    DevBuf d_gen_acc;      // two words summed over a call's internal groups by the schedule code: general blocks, largest team (mlz_get_counter 2 / 6)
    uint64_t l0_launches = 0;   // internal groups of the last decode call whose level-0 candidates, verdicts and schedule went in dec_level0_kernel's launch (mlz_get_counter 13)
    int general_algo = 0;  // 0 = pointer-jumping pass for general blocks, 1 = tile chain in the exec pass
    size_t host_group_enc = kHostGroupEncodeDefault, host_group_dec = kHostGroupDecodeDefault;  // host-pointer batches: bytes per overlapped group
    int gen_grid = 0;      // workgroups of dec_general_kernel the device holds at once
    uint32_t gen_spin_limit = 1u << 24;  // role S's patience with a tile's ready flag, in polls (~0.3 us each): ~5 s
    int n_cus = 0;
    int far_slices_l2 = 0;     // debug option 18: 1 = LevelBalanced's far tables by far_build_kernel (slice workgroups, round 4) even without level sets
    int gen_settle_cap = 0;    // debug option 20: settling workgroups of dec_general_kernel at most (0 = a quarter of the device)
    int l2_gap = 4;            // option 19: LevelBalanced without levels: a far source lies at least this many tiles back (1 = anywhere; 4: the decoder settles four tiles of a block side by side)
    int l2_free = 1;           // option 14 (default on): LevelBalanced without the tile-level constraint (better ratio; its blocks decode through the general path)
    uint64_t gen_fallbacks = 0;  // decode calls whose general blocks took the tile chain because the general pass's buffers could not be allocated (mlz_get_counter 5)
    int gen_force_packed = 0;  // tests: every tile of a general block takes the byte-packed pool (the fallback path)
    int fold_layout = 1;       // option 24: the encode layout rides in the gather kernel when every block of the group has tiles and room (0: always encode_layout_kernel)
    int level0_by_e = 1;       // option 23: few level-0 candidates (tile 16 j of a block) are decoded by dec_level0_kernel before the exec pass, verdicts and schedule beside them (0: dec_viol_kernel, dec_schedule_kernel, every tile by the exec pass: rounds 2-5)
    int l0_grid_cap = 0;       // debug option 25: candidates dec_level0_kernel is launched for at most (0 = as many as the device has CUs)
    int fuse_ser = 1;          // option 21: the match kernel serializes its pieces itself (0: serialize_pieces_kernel, rounds 2-5; cross-checks)
    // host-pointer staging
    DevBuf d_in, d_out, d_len, d_crc, d_crc_tabs, d_crc_tiles;
    // stream calls: copy-in / copy-out streams, event pool, pinned result buffer
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> evpool;
    void* pinned2 = nullptr;
    size_t pinned2_cap = 0;
    // options
    int decode_algo = 0;
    int encode_far = 1;
    bool enc_attrs = false, far_attr = false, farbin_attr = false, stab_attr = false, dec_attrs = false, gen_attr = false, l0_attr = false, l0_attr_failed = false, regex_runs_attr = false;  // per device: dynamic-LDS limits raised (raise_lds_once)
    uint32_t timer_mask = 0xffffffffu;  // timers that record events (an event pair costs ~10 us of idle device per kernel boundary)
    int timing = 0;  // 0 off, 1 = the last call's kernel times, 2 = running mean over the calls since it was enabled (no sync per call)
    int debug_status = 0;
    bool prof_on = false;
    DevBuf d_prof;
    // Every DevBuf above, once, by side: 0 = what mlz_get_counter 3 sums (encode), 1 = counter 4 (decode), 2 = the rest; mlz_destroy frees all three.  A buffer added to the struct is added here.
    std::vector<DevBuf*> bufs(int side) {
        if (side == 0) return {&d_scratch, &d_tile_size, &d_tile_out, &d_flags, &d_far, &d_recs, &d_piece_cnt, &d_farbin, &d_stab, &d_cstw};
        if (side == 1) return {&d_dec, &d_idx, &d_walk, &d_walk_tab, &d_batch, &d_range, &d_rplan, &d_records, &d_rwin};
        return {&d_blocks_k[0], &d_blocks_k[1], &d_tile_block_k[0], &d_tile_block_k[1], &d_seg_block_k[0], &d_seg_block_k[1], &d_place, &d_batch_desc, &d_gen_acc, &d_in, &d_out, &d_len, &d_crc, &d_crc_tabs, &d_crc_tiles, &d_prof};
    }
    // A ring of event pairs per timer, resolved kTimerRing uses later (long complete by then), so reading the clock never stalls the caller and
    // launches can run ahead of the device.  A device batch runs as one or more internal groups, each firing the timers: acc_ms sums them and
    // ev_calls counts the API calls a timer fired in.  timing == 1 restarts a timer's sum at the first firing of a new call (the last call's
    // times), timing == 2 keeps the sum over all calls since it was enabled (get_timers divides by the calls).
    static constexpr int kTimerRing = 8;
    hipEvent_t evr[T_COUNT][kTimerRing][2] = {};
    uint64_t ev_cnt[T_COUNT] = {}, ev_res[T_COUNT] = {}, ev_calls[T_COUNT] = {}, ev_last_call[T_COUNT] = {};
    uint64_t call_seq = 0;
    double acc_ms[T_COUNT] = {};
    void resolve_one(int id) {
        const int slot = int(ev_res[id] % kTimerRing);
        float t = 0;
        if (hipEventSynchronize(evr[id][slot][1]) == hipSuccess && hipEventElapsedTime(&t, evr[id][slot][0], evr[id][slot][1]) == hipSuccess) acc_ms[id] += t;
        ev_res[id]++;
    }
};

namespace {

#define HIPCHK(ctx, call)                                                                 \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return -MLZ_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

struct Timer {
    mlz_ctx* c; int id; hipStream_t s;
    bool on;
    Timer(mlz_ctx* c_, int id_, hipStream_t s_) : c(c_), id(id_), s(s_), on(c_->timing != 0 && ((c_->timer_mask >> id_) & 1) != 0) {
        if (!on) return;
        if (c->ev_last_call[id] != c->call_seq) {   // first firing in this API call
            c->ev_last_call[id] = c->call_seq;
            if (c->timing == 1) {
                while (c->ev_res[id] < c->ev_cnt[id]) c->resolve_one(id);
                c->acc_ms[id] = 0; c->ev_calls[id] = 0;
            }
            c->ev_calls[id]++;
        }
        while (c->ev_cnt[id] - c->ev_res[id] >= uint64_t(mlz_ctx::kTimerRing)) c->resolve_one(id);
        (void)hipEventRecord(c->evr[id][c->ev_cnt[id] % mlz_ctx::kTimerRing][0], s);
    }
    ~Timer() {
        if (!on) return;
        (void)hipEventRecord(c->evr[id][c->ev_cnt[id] % mlz_ctx::kTimerRing][1], s);
        c->ev_cnt[id]++;
    }
};

// Orders the calls that share the context's workspace across streams (see mlz_ctx::ws_done).  The event is recorded LAZILY — by the next call
// that arrives on another stream, on the previous call's stream: it then covers everything that stream was given, the previous call included —
// because an event record after every call idles the device for ~5 us at each call boundary (rocprofv3 timeline: 11 us of a 1.41 ms
// encode + decode step), and calls on one stream need no event at all.
struct WorkspaceOrder {
    mlz_ctx* c; hipStream_t s;
    WorkspaceOrder(mlz_ctx* c_, hipStream_t s_) : c(c_), s(s_) {
        if (c->ws_used && (c->ws_recorded || c->ws_stream != s)) {
            if (c->ws_recorded) (void)hipStreamWaitEvent(s, c->ws_done, 0);   // recorded by mlz_release_stream while the stream was alive
            else if (hipEventRecord(c->ws_done, c->ws_stream) == hipSuccess) (void)hipStreamWaitEvent(s, c->ws_done, 0);
            else { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }   // (the caller destroyed that stream: whatever it held is waited for)
        }
    }
    ~WorkspaceOrder() {
        c->ws_stream = s;
        c->ws_used = true;
        c->ws_recorded = false;
    }
};

// Builds BlockInfo / tile map on the host and uploads them when they differ from the last call.
int upload_blocks(mlz_ctx* c, hipStream_t st, const mlz_block_desc* desc, int n, bool tiles_from_dst, uint32_t* total_tiles, uint32_t* total_segs = nullptr,
                  const uint64_t* mirror = nullptr, bool any_length = false /* the CRC pass: tiles for spans of any length */) {
    c->dk = tiles_from_dst ? 1 : 0;
    std::vector<BlockInfo>& prev = c->h_blocks_prev_k[c->dk];
    c->h_blocks.resize(n);
    uint32_t tiles = 0, segs = 0;
    for (int i = 0; i < n; i++) {
        BlockInfo& b = c->h_blocks[i];
        b.src_off = desc[i].src_off; b.src_len = desc[i].src_len; b.dst_off = desc[i].dst_off; b.dst_cap = desc[i].dst_cap;
        b.mirror = mirror ? mirror[i] : 0;
        uint64_t span = tiles_from_dst ? desc[i].dst_cap : desc[i].src_len;
        if (span > kMaxBlockSize && !any_length) span = tiles_from_dst ? kMaxBlockSize : 0;
        b.first_tile = tiles;
        b.n_tiles = uint32_t((span + kTile - 1) >> kTileLog);
        tiles += b.n_tiles;
        b.first_seg = segs;
        b.n_segs = 0;
        if (tiles_from_dst) {  // decode: segments of the token stream
            // a valid token stream is at most twice its output (dec_header_kernel rejects longer ones before any pass walks them)
            uint64_t cl = std::min<uint64_t>(desc[i].src_len, 2 * std::min<uint64_t>(desc[i].dst_cap, kMaxBlockSize) + 32);
            b.n_segs = uint32_t((cl + kSeg - 1) >> kSegLog);
            segs += b.n_segs;
        }
    }
    *total_tiles = tiles;
    if (total_segs) *total_segs = segs;
    const bool same = prev.size() == c->h_blocks.size() && std::memcmp(prev.data(), c->h_blocks.data(), sizeof(BlockInfo) * n) == 0;
    if (same) return 0;
    c->h_tile_block.resize(tiles);
    c->h_seg_block.resize(segs);
    for (int i = 0; i < n; i++) {
        for (uint32_t t = 0; t < c->h_blocks[i].n_tiles; t++) c->h_tile_block[c->h_blocks[i].first_tile + t] = uint32_t(i);
        for (uint32_t t = 0; t < c->h_blocks[i].n_segs; t++) c->h_seg_block[c->h_blocks[i].first_seg + t] = uint32_t(i);
    }
    const size_t nb = sizeof(BlockInfo) * n, nt = sizeof(uint32_t) * tiles, ns = sizeof(uint32_t) * segs;
    const int sl = (c->up_slot ^= 1);
    if (c->upload_pending_k[sl]) { HIPCHK(c, hipEventSynchronize(c->upload_done_k[sl])); c->upload_pending_k[sl] = false; }
    if (nb + nt + ns > c->pinned_cap_k[sl]) {
        if (c->pinned_k[sl]) HIPCHK(c, hipHostFree(c->pinned_k[sl]));
        c->pinned_k[sl] = nullptr;
        c->pinned_cap_k[sl] = (nb + nt + ns) * 2 + 4096;
        HIPCHK(c, hipHostMalloc(&c->pinned_k[sl], c->pinned_cap_k[sl], hipHostMallocDefault));
    }
    char* pin = static_cast<char*>(c->pinned_k[sl]);
    HIPCHK(c, c->d_blocks_cur().ensure(nb + 64));
    HIPCHK(c, c->d_tile_block_cur().ensure(nt + 64));
    HIPCHK(c, c->d_seg_block_cur().ensure(ns + 64));
    std::memcpy(pin, c->h_blocks.data(), nb);
    std::memcpy(pin + nb, c->h_tile_block.data(), nt);
    std::memcpy(pin + nb + nt, c->h_seg_block.data(), ns);
    if (nb) HIPCHK(c, hipMemcpyAsync(c->d_blocks_cur().p, pin, nb, hipMemcpyHostToDevice, st));
    if (nt) HIPCHK(c, hipMemcpyAsync(c->d_tile_block_cur().p, pin + nb, nt, hipMemcpyHostToDevice, st));
    if (ns) HIPCHK(c, hipMemcpyAsync(c->d_seg_block_cur().p, pin + nb + nt, ns, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->upload_done_k[sl], st));
    c->upload_pending_k[sl] = true;
    prev = c->h_blocks;
    return 0;
}

// Blocks [0, n) of a device batch cut into consecutive groups of about c->device_group bytes of uncompressed data (at least one block each):
// calls fn(first, count) per group.  The groups run one after the other on the call's stream and share the workspace.
template <class F> int for_each_group(mlz_ctx* c, const mlz_block_desc* desc, int n, bool by_dst, F fn) {
    int b0 = 0;
    while (b0 < n) {
        uint64_t bytes = 0;
        int b1 = b0;
        while (b1 < n) {
            const uint64_t span = std::min<uint64_t>(by_dst ? desc[b1].dst_cap : desc[b1].src_len, kMaxBlockSize);
            if (b1 > b0 && bytes + span > c->device_group) break;
            bytes += span;
            b1++;
        }
        const int r = fn(b0, b1 - b0);
        if (r) return r;
        b0 = b1;
    }
    return 0;
}

// Raises the dynamic-LDS limit of every kernel of `list` (entries with .fn and .lds) the first time a context, that is a device, comes by.
template <class List> int raise_lds_once(mlz_ctx* c, bool& raised, const List& list) {
    if (raised) return 0;
    for (const auto& k : list) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, int(k.lds)));
    raised = true;
    return 0;
}
template <class Fn> struct Kernel { Fn fn; uint32_t lds; };   // a kernel and the dynamic LDS it is launched with
struct AnyKernel : Kernel<const void*> { template <class F> AnyKernel(F* f, uint32_t l) : Kernel{reinterpret_cast<const void*>(f), l} {} };   // ... in a list of kernels that share no signature
using Kernels = std::initializer_list<AnyKernel>;

// ---- encode: every instantiation of the match kernel and of the far-table kernel, named once, with the dynamic LDS it is launched with.  A launch takes a
// row of these tables and the limits are raised for a whole table at once, so no instantiation runs without its limit.  Every level goes through the match +
// serialize kernels on 8 KiB pieces (mlz_encode2.hip.inc); LevelBalanced is their configuration with larger near tables, denser far tables and a second far probe (kL2*).
using MatchFn = void (*)(const uint8_t*, const BlockInfo*, const uint32_t*, uint2*, uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                         uint32_t, uint8_t*, uint32_t*);
enum MatchId { M_L1_BIG_FAR, M_L1_SMALL_FAR, M_L1_BIG, M_L1_SMALL, M_SUPERFAST, M_L2_BIG, M_L2_SMALL, M_L2_ONE_TILE, M_COUNT };
const Kernel<MatchFn> kMatch[M_COUNT] = {
    {match_tiles_kernel<true, MLZ_M2_NW, kM2HashBitsBig, kFarBits, false>, M2Cfg<kM2HashBitsBig>::kLds},
    {match_tiles_kernel<true, MLZ_M2_NW, kM2HashBitsSmall, 0, false>, M2Cfg<kM2HashBitsSmall>::kLds},                  // far tables of the block's own size
    {match_tiles_kernel<false, MLZ_M2_NW, kM2HashBitsBig, kFarBits, false>, M2Cfg<kM2HashBitsBig>::kLds},
    {match_tiles_kernel<false, MLZ_M2_NW, kM2HashBitsSmall, kFarBits, false>, M2Cfg<kM2HashBitsSmall>::kLds},
    {match_tiles_kernel<false, MLZ_M2_NW, kM2HashBitsSuperFast, kFarBits, false>, M2Cfg<kM2HashBitsSuperFast>::kLds},  // (MLZ_L1_HB = 12, the default: the function of M_L1_BIG)
    {match_tiles_kernel<true, MLZ_M2_NW, kM2HashBitsSmall, kL2FarBits, true>, M2Cfg<kM2HashBitsSmall>::kLds},          // LevelBalanced: one configuration for both block classes,
    {match_tiles_kernel<true, MLZ_M2_NW, kM2HashBitsSmall, 0, true>, M2Cfg<kM2HashBitsSmall>::kLds},                   // with far tables of the level's size or of the block's
    {match_tiles_kernel<false, MLZ_M2_NW, kM2HashBitsSmall, kL2FarBits, true>, M2Cfg<kM2HashBitsSmall>::kLds},         // no far tables, but the level's near-table seeding
};
using FarBuildFn = void (*)(const uint8_t*, const BlockInfo*, uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
const Kernel<FarBuildFn> kFarBuild[4] = {   // [2 * LevelBalanced + blocks of kBigBlock and more]; the smaller blocks' tables go with their length
    {far_build_kernel<0, kFarStride>, 4u << kFarSliceBits}, {far_build_kernel<kFarBits, kFarStride>, 4u << kFarSliceBits},
    {far_build_kernel<0, kL2FarStride>, 4u << kFarSliceBits}, {far_build_kernel<kL2FarBits, kL2FarStride>, 4u << kFarSliceBits},
};

// The match launches of a group: one per block class that occurs in it (usually one), each workgroup leaving at once when its block belongs
// to the other class.  cls: 2 = every block, 1 = those of kM2BigBlock and more, 0 = the smaller ones.
struct MatchPlan { int n; struct { MatchId id; uint32_t cls; } launch[2]; };
MatchPlan match_plan(int level, bool far, bool any_big, bool any_small) {
    if (level == MLZ_LEVEL_SUPERFAST) return {1, {{M_SUPERFAST, 2u}}};
    const bool l2 = level == MLZ_LEVEL_BALANCED;
    if (l2 && !far) return {1, {{M_L2_ONE_TILE, 2u}}};   // (the level forces far matching on: no block of the group exceeds a tile)
    MatchPlan p{};
    if (any_big) p.launch[p.n++] = {l2 ? M_L2_BIG : far ? M_L1_BIG_FAR : M_L1_BIG, any_small ? 1u : 2u};
    if (any_small) p.launch[p.n++] = {l2 ? M_L2_SMALL : far ? M_L1_SMALL_FAR : M_L1_SMALL, any_big ? 0u : 2u};
    return p;
}

// What the parts of a group's encode read; encode_device_group computes it once.
struct EncGroup {
    int level, n;
    const BlockInfo* blocks; const uint32_t* tile_block;   // the group's descriptors on the device
    uint32_t tiles, epochs, pattern, far_gap;
    size_t units;            // pieces
    bool far, any_big, any_small;   // far tables are built and probed; block classes that occur
    int fbits;               // far tables lie 2^fbits entries apart
};

int encode_far_tables(mlz_ctx* c, hipStream_t st, const EncGroup& g, const uint8_t* d_src, const mlz_block_desc* desc) {
    Timer t(c, T_FAR, st);
    const bool l2 = g.level == MLZ_LEVEL_BALANCED;
    HIPCHK(c, c->d_far.ensure(((size_t(g.n) * far_sets(g.pattern) * g.epochs) << g.fbits) * 4));
    if (int r = raise_lds_once(c, c->far_attr, kFarBuild)) return r;
    // one-dimensional grid: the 2^slice_log slice workgroups of a (block, epoch) on one XCD (far_place, mlz_encode.hip.inc)
    auto build = [&](const Kernel<FarBuildFn>& v, uint32_t slice_log, uint32_t grid_epochs, uint32_t lds, uint32_t cls) {
        const uint32_t groups = uint32_t(g.n) * grid_epochs;
        hipLaunchKernelGGL(v.fn, dim3(far_grid(groups, slice_log)), dim3(1024), lds, st, d_src, g.blocks, c->d_far.as<uint32_t>(), g.epochs, g.pattern, uint32_t(g.fbits), cls,
                           slice_log, grid_epochs, groups);
    };
    if (g.any_big) {
        if (l2 && g.pattern == kPatternFree && !c->far_slices_l2) {
            // no level sets: the windows sorted by slice once (far_bin_kernel), every slice workgroup reads its eighth (far_slice_kernel)
            using FBn = FarBin<kL2FarBits, kL2FarStride>;
            const size_t units2 = size_t(g.tiles) * 2;
            HIPCHK(c, c->d_farbin.ensure(units2 * FBn::kPerUnit * 4 + units2 * FBn::kOffs * 4 + 256));
            uint32_t* bins = c->d_farbin.as<uint32_t>();
            uint32_t* binoff = bins + units2 * FBn::kPerUnit;
            constexpr uint32_t kSliceLds = (4u << kBinSliceBits) + 256 * 4 + 132 * 4;
            if (int r = raise_lds_once(c, c->farbin_attr, Kernels{{far_bin_kernel<kL2FarBits, kL2FarStride>, FBn::kLds}, {far_slice_kernel<kL2FarBits, kL2FarStride>, kSliceLds}})) return r;
            hipLaunchKernelGGL((far_bin_kernel<kL2FarBits, kL2FarStride>), dim3(uint32_t(units2)), dim3(256), FBn::kLds, st, d_src, g.blocks, g.tile_block, bins, binoff);
            hipLaunchKernelGGL((far_slice_kernel<kL2FarBits, kL2FarStride>), dim3(FBn::kSlices, g.epochs, g.n), dim3(1024), kSliceLds, st, g.blocks, bins, binoff, c->d_far.as<uint32_t>(), g.epochs);
        } else
            build(kFarBuild[2 * l2 + 1], uint32_t((l2 ? kL2FarBits : kFarBits) - kFarSliceBits), g.epochs, kFarBuild[2 * l2 + 1].lds, g.any_small ? 1u : 2u);
    }
    if (g.any_small) {
        uint64_t max_small = 0;
        for (int i = 0; i < g.n; i++) if (desc[i].src_len < kBigBlock) max_small = std::max<uint64_t>(max_small, desc[i].src_len);
        const int sb = small_far_bits(max_small) + (l2 ? 1 : 0);
        const uint32_t lds = 4u << std::min<int>(sb, kFarSliceBits);   // small tables leave room for more workgroups per CU
        build(kFarBuild[2 * l2], uint32_t(std::max<int>(sb, kFarSliceBits) - kFarSliceBits), 1, lds, g.any_big ? 0u : 2u);
    }
    return 0;
}

// The match kernel on every tile of the group, and the serializer where the match kernel's waves do not serialize their pieces themselves.
int encode_match(mlz_ctx* c, hipStream_t st, const EncGroup& g, const uint8_t* d_src) {
    HIPCHK(c, c->d_recs.ensure(g.units * kRecPerPiece * sizeof(uint2)));
    HIPCHK(c, c->d_piece_cnt.ensure(g.units * sizeof(uint32_t)));
    if (int r = raise_lds_once(c, c->enc_attrs, kMatch)) return r;
    const uint32_t* ftab = g.far ? c->d_far.as<uint32_t>() : nullptr;
    uint8_t* fuse_scratch = c->fuse_ser ? c->d_scratch.as<uint8_t>() : nullptr;   // option 21, default on
    {
        Timer t(c, T_ENC_TILES, st);
        const uint32_t grid = ((g.tiles + 7) / 8) * 8;  // whole rounds of the eight XCDs (see the kernel's workgroup -> tile map)
        const MatchPlan plan = match_plan(g.level, g.far, g.any_big, g.any_small);
        for (int i = 0; i < plan.n; i++) {
            const Kernel<MatchFn>& v = kMatch[plan.launch[i].id];
            hipLaunchKernelGGL(v.fn, dim3(grid), dim3(256), v.lds, st, d_src, g.blocks, g.tile_block, c->d_recs.as<uint2>(), c->d_piece_cnt.as<uint32_t>(), ftab, g.epochs,
                               g.pattern, g.tiles, plan.launch[i].cls, uint32_t(g.fbits), g.far_gap, fuse_scratch, c->d_tile_size.as<uint32_t>());
        }
    }
    if (!fuse_scratch) {
        Timer t(c, T_ENC_SER, st);
        hipLaunchKernelGGL(serialize_pieces_kernel, dim3(g.tiles), dim3(256), kSerLds, st, d_src, g.blocks, g.tile_block, c->d_recs.as<uint2>(),
                           c->d_piece_cnt.as<uint32_t>(), c->d_scratch.as<uint8_t>(), c->d_tile_size.as<uint32_t>());
    }
    return 0;
}

// The layout (piece offsets, stored-or-not, header, length) rides in the gather when every block of the group has tiles and room — the common case;
// an empty, oversize or too tightly bounded block needs encode_layout_kernel's verdicts (option 24 = 0: always the separate kernel).
void encode_layout_gather(mlz_ctx* c, hipStream_t st, const EncGroup& g, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int64_t* d_out_len,
                          bool with_header) {
    bool fold = c->fold_layout && g.tiles > 0 && g.level != MLZ_LEVEL_UNCOMPRESSED;
    for (int i = 0; fold && i < g.n; i++) {
        const uint64_t len = desc[i].src_len;
        if (len == 0 || len > kMaxBlockSize || desc[i].dst_cap < (with_header ? len + 2 : len)) fold = false;
    }
    if (!fold) {
        Timer t(c, T_ENC_LAYOUT, st);
        hipLaunchKernelGGL(encode_layout_kernel, dim3(g.n), dim3(64), 0, st, g.blocks, c->d_tile_size.as<uint32_t>(), c->d_tile_out.as<uint32_t>(), d_dst, d_out_len,
                           c->d_flags.as<uint32_t>(), g.level, with_header ? 1 : 0, kSubLog);
    }
    if (g.tiles > 0) {
        Timer t(c, T_ENC_GATHER, st);
        const auto gather = fold ? encode_gather2_kernel<true> : encode_gather2_kernel<false>;
        hipLaunchKernelGGL(gather, dim3(g.tiles), dim3(256), 0, st, d_src, g.blocks, g.tile_block, c->d_scratch.as<uint8_t>(),
                           c->d_tile_size.as<uint32_t>(), c->d_tile_out.as<uint32_t>(), d_dst, c->d_flags.as<uint32_t>(), with_header ? 1 : 0, g.level, d_out_len);
    }
}

int encode_device_group(mlz_ctx* c, hipStream_t st, int level, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n,
                        int64_t* d_out_len, bool with_header, const uint64_t* mirror) {
    EncGroup g{level, n};
    int r = upload_blocks(c, st, desc, n, false, &g.tiles, nullptr, mirror);
    if (r) return r;
    g.blocks = c->d_blocks_cur().as<BlockInfo>(); g.tile_block = c->d_tile_block_cur().as<uint32_t>();
    g.units = size_t(g.tiles) << kSubLog;
    HIPCHK(c, c->d_tile_size.ensure(sizeof(uint32_t) * (g.units + 1)));
    HIPCHK(c, c->d_tile_out.ensure(sizeof(uint32_t) * (g.units + 1)));
    HIPCHK(c, c->d_flags.ensure(sizeof(uint32_t) * n));
    if (level != MLZ_LEVEL_UNCOMPRESSED && g.tiles > 0) {
        HIPCHK(c, c->d_scratch.ensure(g.units * kPieceScratch));
        const bool l2 = level == MLZ_LEVEL_BALANCED;
        uint64_t maxlen = 0;
        for (int i = 0; i < n; i++) {
            const uint64_t len = std::min<uint64_t>(desc[i].src_len, kMaxBlockSize);
            maxlen = std::max(maxlen, len);
            (len >= kM2BigBlock ? g.any_big : g.any_small) = true;
        }
        g.epochs = uint32_t((maxlen + (1u << kEpochLog) - 1) >> kEpochLog);
        // LevelBalanced: far matching forced on, both epochs probed and a cost-aware lazy parse (DESIGN.md "Levels").
        // LevelSuperFast: tile-local matches only (no far tables are built or probed).
        g.far = ((c->encode_far && level != MLZ_LEVEL_SUPERFAST) || l2) && maxlen > kTile;
        g.pattern = (l2 && c->l2_free) ? kPatternFree : level_pattern_of(level);   // LevelBalanced: dense (four levels); the faster levels: three (DESIGN.md "Tile levels"); the decoder knows both and round 1's kPatternFast
        // LevelFastest: blocks below 1 MiB have far tables that go with their length (small_far_bits); the tables of a batch
        // are as far apart as its largest block needs
        g.fbits = g.any_big ? (l2 ? kL2FarBits : kFarBits) : small_far_bits(maxlen) + (l2 ? 1 : 0);
        // LevelBalanced without levels: far sources at least l2_gap tiles back (MLZ_OPT_L2_GAP)
        g.far_gap = g.pattern == kPatternFree && l2 ? uint32_t(c->l2_gap - 1) << kTileLog : 0u;
        if (g.far) r = encode_far_tables(c, st, g, d_src, desc);
        if (!r) r = encode_match(c, st, g, d_src);
        if (r) return r;
    }
    encode_layout_gather(c, st, g, d_src, d_dst, desc, d_out_len, with_header);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// dec_general_kernel's role S workgroups: up to four per block (teams, GenCtl::team), at most a quarter of the device; a multiple of 4
uint32_t gen_settle_wgs(mlz_ctx* c, int n) {
    const uint32_t grid = c->gen_grid > 0 ? uint32_t(c->gen_grid) : uint32_t(c->n_cus);
    const uint32_t cap = c->gen_settle_cap > 0 ? uint32_t(c->gen_settle_cap) : grid / 4;
    return std::max<uint32_t>(4u, std::min<uint32_t>(4u * uint32_t(n), cap) & ~3u);
}

int decode_parallel(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n, int64_t* d_out_len,
                    bool raw_body, const uint64_t* mirror) {
    uint32_t tiles = 0, segs = 0;
    int r = upload_blocks(c, st, desc, n, true, &tiles, &segs, mirror);
    if (r) return r;
    // the workspace, every region on a 256-byte boundary
    constexpr size_t kAl = 256;
    Carve cv;
    const auto r_dec = cv.take<DecBlock>(size_t(n), kAl);
    const auto r_exit = cv.take<uint32_t>(size_t(segs) * kExitKeep, kAl);
    const auto r_rexit = cv.take<uint8_t>(size_t(segs) * kSeg, kAl);
    const auto r_entry = cv.take<uint32_t>(segs, kAl);
    const auto r_tstart = cv.take<TileStart>(tiles, kAl);
    const auto r_tpos = cv.take<uint32_t>(size_t(segs) * kSeg, kAl);              // token list: a token has at least one stream byte
    const auto r_rd = cv.take<uint32_t>(size_t(segs) * kSegThreads, kAl), r_rr = cv.take<uint32_t>(size_t(segs) * kSegThreads, kAl);   // (per 64 tokens: indexed like the 64-byte chunks)
    const auto r_order = cv.take<uint32_t>(tiles, kAl), r_glist = cv.take<uint32_t>(size_t(n), kAl);   // the tile schedule; the general blocks of the batch (D3d)
    const auto r_xcnt = cv.take<GenTile>(tiles, kAl);                             // per-tile records of dec_general_kernel
    // dec_header_kernel zeroes everything between the two marks as one span: the order of these five regions is the contract
    const size_t zero_begin = cv.take<uint32_t>(0, kAl).off;
    const auto r_done = cv.take<uint32_t>(tiles, kAl), r_ticket = cv.take<uint32_t>(kAl / 4, kAl);
    const auto r_gen = cv.take<GenCtl>(1, kAl);
    const auto r_sstate = cv.take<unsigned long long>(size_t(segs) * 4, kAl);     // per segment: aggregate words of the index pass (the segment's, then three prefixes over its quarters)
    const auto r_sviol = cv.take<uint8_t>(size_t(segs) * 4, kAl);                 // ... and which level patterns its quarters' copies break
    const size_t zero_end = cv.take<uint32_t>(0, kAl).off;
    const auto r_tok16 = cv.take<uint16_t>(size_t(segs) * kSeg, kAl);             // ... and its token positions inside the segment (16 bits per stream byte; not zeroed)
    HIPCHK(c, c->d_dec.ensure(cv.take<uint8_t>(0, kAl).off));
    void* ws = c->d_dec.p;
    DecBlock* dec = r_dec.at(ws);
    TileStart* tile_start = r_tstart.at(ws);
    uint8_t *rexit_tab = r_rexit.at(ws), *sviol = r_sviol.at(ws);
    uint32_t *exit_tab = r_exit.at(ws), *seg_entry = r_entry.at(ws), *tok_pos = r_tpos.at(ws), *round_d = r_rd.at(ws), *round_rep = r_rr.at(ws), *order = r_order.at(ws);
    uint32_t *tile_done = r_done.at(ws), *ticket = r_ticket.at(ws);
    GenCtl* gen = r_gen.at(ws);
    uint32_t* gen_words = reinterpret_cast<uint32_t*>(gen);   // the kernels outside the general pass read its words by index
    unsigned long long* sstate = r_sstate.at(ws);
    uint16_t* tok16 = r_tok16.at(ws);
    // General blocks (streams of other encoders) go through dec_general_kernel when its workspace — 2 B of map and 1 B of pool per
    // output byte, 8 B per possible token for the external entries — is affordable (<= 64 GiB) and the current exec pass is in use.
    Carve idx;
    const auto r_gmap = idx.take<uint16_t>(size_t(tiles) << kTileLog);
    const auto r_gpool = idx.take<uint8_t>(size_t(tiles) << kTileLog);
    const auto r_ext = idx.take<ExtEnt>((size_t(segs) << kSegLog) + size_t(tiles) * kExtPerTile + 64 * size_t(n));
    bool jump = c->general_algo == 0 && c->decode_algo == 0 && tiles > 0;
    if (jump && c->d_idx.ensure(idx.bytes + 256) != hipSuccess) {
        // The device cannot hold the pass's buffers (another tenant's memory, a small part): not a reason to fail the call — general blocks
        // then stay on the exec pass's tile chain, which needs none (slow, correct).  Counted, so that a caller can see it: mlz_get_counter(ctx, 5).
        (void)hipGetLastError();
        c->gen_fallbacks++;
        jump = false;
    }
    uint32_t* gen_list = jump ? r_glist.at(ws) : nullptr;   // null: general blocks stay on the tile path
    const BlockInfo* blocks = c->d_blocks_cur().as<BlockInfo>();
    const uint32_t* tile_block = c->d_tile_block_cur().as<uint32_t>();
    const uint32_t* seg_block = c->d_seg_block_cur().as<uint32_t>();
    if ((r = raise_lds_once(c, c->dec_attrs, Kernels{{dec_exit_kernel, kExitLds}, {dec_index1_kernel, kIdxLds}, {dec_exec2_kernel, kExecLds}}))) return r;
    // The hand-over from the index pass to the exec pass.  Few level-0 candidates (tile 16 j of a block: level 0 under every pattern; at most one per CU):
    // ONE launch decodes them and, in a workgroup of its own, gives the verdicts and makes the schedule (dec_level0_kernel).  Otherwise — many small
    // blocks, option 23 = 0, another decode_algo, a device that refuses the kernel its LDS — dec_viol_kernel and dec_schedule_kernel, and the exec pass
    // decodes every tile.
    L0Cands cands;
    uint32_t n_cand = 0;
    bool l0 = tiles && c->level0_by_e && c->decode_algo == 0 && uint64_t(n) < (1ull << kL0BlockBits);
    if (l0) {
        const uint32_t cap = std::min<uint32_t>(c->l0_grid_cap > 0 ? uint32_t(c->l0_grid_cap) : uint32_t(c->n_cus), kL0MaxCands);
        for (int i = 0; i < n && n_cand <= cap; i++)
            for (uint32_t j = 0; 16 * j < c->h_blocks[i].n_tiles && n_cand <= cap; j++, n_cand++)
                if (n_cand < cap) cands.e[n_cand] = uint32_t(i) | (j << kL0BlockBits);
        l0 = n_cand >= 1 && n_cand <= cap;
    }
    if (l0 && !c->l0_attr) {   // refused: not a reason to fail the call
        if (!c->l0_attr_failed && hipFuncSetAttribute(reinterpret_cast<const void*>(dec_level0_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(kGenLds)) == hipSuccess) c->l0_attr = true;
        else { (void)hipGetLastError(); c->l0_attr_failed = true; l0 = false; }
    }
    uint32_t* n_general = jump ? &gen->n_general : nullptr;
    // the call's counters (d_gen_acc) start from 0 in its first group, whether or not that group has tiles to schedule
    HIPCHK(c, c->d_gen_acc.ensure(64));
    const uint32_t acc_reset = c->acc_call != c->dec_call ? 1u : 0u;
    if (acc_reset) c->l0_launches = 0;
    c->acc_call = c->dec_call;
    {
        Timer t(c, T_DEC_PARSE, st);
        // the header pass also initialises the workspace words the later passes expect (two memsets = two more launches otherwise)
        const uint32_t n_ff = segs, n_zero = uint32_t((zero_end - zero_begin) / 4);
        const uint32_t hdr_grid = std::max<uint32_t>(uint32_t(n + 63) / 64, std::min<uint32_t>((std::max(n_ff, n_zero) + 255) / 256, 256u));
        hipLaunchKernelGGL(dec_header_kernel, dim3(hdr_grid), dim3(64), 0, st, d_src, blocks, dec, n, raw_body ? 1 : 0, seg_entry, n_ff,
                           tile_done, n_zero);
        if (segs)
            hipLaunchKernelGGL(dec_exit_kernel, dim3(segs), dim3(kExitThreads), kExitLds, st, d_src, blocks, seg_block, dec, exit_tab, rexit_tab);
    }
    {
        Timer t(c, T_DEC_CHAIN, st);
        hipLaunchKernelGGL(dec_chain_kernel, dim3(n), dim3(kChainThreads), 0, st, blocks, dec, exit_tab, seg_entry, n, d_src, rexit_tab);
    }
    {
        Timer t(c, T_DEC_INDEX, st);
        if (segs) {
            hipLaunchKernelGGL(dec_index1_kernel, dim3(segs), dim3(kIdxThreads), kIdxLds, st, d_src, blocks, seg_block, dec, seg_entry, rexit_tab, sstate, sstate + segs, tok16);
            hipLaunchKernelGGL(dec_index2_kernel, dim3(2 * segs), dim3(kIdx2Threads), 0, st, d_src, blocks, seg_block, dec, sstate, sstate + segs, tok16, tile_start, tok_pos,
                               round_d, round_rep, sviol);
        }
        if (jump && segs && !c->gen_attr) {
            if ((r = raise_lds_once(c, c->gen_attr, Kernels{{dec_general_kernel, kGenLds}}))) return r;
            // how many of its workgroups the device holds at once (1024 threads + 132 KiB of LDS: one per CU).  Not a correctness
            // requirement — role E never waits and role S only waits for role E, whose workgroups come first in the grid —: it
            // sizes the grid so that the settling workgroups start beside the explaining ones instead of behind them.
            int per_cu = 0;
            HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(dec_general_kernel), kGenThreads, kGenLds));
            c->gen_grid = per_cu >= 1 ? c->n_cus * per_cu : 0;
        }
        if (!l0 && segs)
            hipLaunchKernelGGL(dec_viol_kernel, dim3((segs + 255) / 256), dim3(256), 0, st, seg_block, sviol, dec, n_general, segs);
        if (!l0 && tiles)
            hipLaunchKernelGGL(dec_schedule_kernel, dim3(1), dim3(1024), 0, st, blocks, tile_block, dec, order, tiles, uint32_t(n),
                               gen_list, gen_words, gen_settle_wgs(c, n), c->d_gen_acc.as<uint32_t>(), acc_reset);
        if (!tiles && acc_reset) HIPCHK(c, hipMemsetAsync(c->d_gen_acc.p, 0, 8, st));   // (no schedule in this group: the call's counters still start from 0)
    }
    {
        Timer t(c, T_DEC_EXEC, st);
        unsigned long long* prof = c->prof_on ? c->d_prof.as<unsigned long long>() : nullptr;
        // the level-0 candidates first, by role E of the general pass, one per workgroup; the last workgroup gives the verdicts and makes the schedule
        if (l0) {
            const L0Sched sc{seg_block, tile_block, sviol, n_general, order, gen_list, gen_words, c->d_gen_acc.as<uint32_t>(), segs, tiles, uint32_t(n), gen_settle_wgs(c, n), acc_reset};
            hipLaunchKernelGGL(dec_level0_kernel, dim3(n_cand + 1), dim3(kGenThreads), kGenLds, st, d_src, d_dst, blocks, dec, tok_pos, round_d, round_rep, tile_start,
                               tile_done, cands, sc);
            c->l0_launches++;
        }
        if (tiles)
            hipLaunchKernelGGL(dec_exec2_kernel, dim3(tiles), dim3(kExecThreads), kExecLds, st, d_src, d_dst, blocks, tile_block, dec, tile_start, tok_pos,
                               round_d, round_rep, order, tile_done, ticket, tiles, prof, l0 ? 1u : 0u);
    }
    {
        Timer tg(c, T_DEC_GENERAL, st);   // (+ the result pass)
        if (jump && segs) {  // returns at once unless D3 flagged a general block
            if (c->gen_grid == 0) { c->err = "dec_general_kernel: the device cannot hold a workgroup"; return -MLZ_ERR_HIP; }
            // role S: one workgroup per general block, at most a quarter of the device (more blocks take turns); role E: the rest
            const uint32_t nS = gen_settle_wgs(c, n);
            const uint32_t nE = std::max<uint32_t>(1u, uint32_t(c->gen_grid) > nS ? uint32_t(c->gen_grid) - nS : 1u);
            uint16_t* gmap = r_gmap.at(c->d_idx.p);
            uint8_t* gpool = r_gpool.at(c->d_idx.p);
            ExtEnt* ext = r_ext.at(c->d_idx.p);
            GenTile* gen_tile = r_xcnt.at(ws);
            hipLaunchKernelGGL(dec_general_kernel, dim3(nE + nS), dim3(kGenThreads), kGenLds, st, d_src, d_dst, blocks, dec, tok_pos, round_d, round_rep, tile_start,
                               gen_list, gmap, gpool, ext, gen_tile, tile_done, gen, nE, nS, c->gen_spin_limit, uint32_t(c->gen_force_packed), d_out_len, n, c->debug_status);   // (+ the results: D5)
        } else
            hipLaunchKernelGGL(dec_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, dec, d_out_len, n, c->debug_status);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int encode_device_locked(mlz_ctx* c, hipStream_t st, int level, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n,
                         int64_t* d_out_len, bool with_header, const uint64_t* mirror = nullptr) {
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    if (n <= 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    WorkspaceOrder order(c, st);
    c->call_seq++;
    return for_each_group(c, desc, n, false, [&](int b0, int cnt) {
        return encode_device_group(c, st, level, d_src, d_dst, desc + b0, cnt, d_out_len + b0, with_header, mirror ? mirror + b0 : nullptr);
    });
}

int decode_device_group(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n, int64_t* d_out_len,
                        bool raw_body, const uint64_t* mirror) {
    if (c->decode_algo == 1) {
        uint32_t tiles = 0;
        int r = upload_blocks(c, st, desc, n, true, &tiles);
        if (r) return r;
        Timer t(c, T_DEC_SERIAL, st);
        hipLaunchKernelGGL(decode_serial_kernel, dim3(n), dim3(64), 0, st, d_src, d_dst, c->d_blocks_cur().as<BlockInfo>(), d_out_len, raw_body ? 1 : 0);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    return decode_parallel(c, st, d_src, d_dst, desc, n, d_out_len, raw_body, mirror);
}

// A decode API call starts: counters 2 and 6 (mlz_get_counter) describe it alone from here on.  Every decode_device_locked of the call
// (host groups, stream groups) adds to d_gen_acc, the call's first group resets it, and a call that runs none reports 0.
void begin_decode_call(mlz_ctx* c) { c->call_seq++; c->dec_call = c->call_seq; }

int decode_device_locked(mlz_ctx* c, hipStream_t st, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n, int64_t* d_out_len,
                         bool raw_body, const uint64_t* mirror = nullptr, bool new_call = true /* false: a part of a call begun by the caller */) {
    if (n <= 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    WorkspaceOrder order(c, st);
    c->call_seq++;
    if (new_call) c->dec_call = c->call_seq;
    return for_each_group(c, desc, n, true, [&](int b0, int cnt) {
        return decode_device_group(c, st, d_src, d_dst, desc + b0, cnt, d_out_len + b0, raw_body, mirror ? mirror + b0 : nullptr);
    });
}

// The CRC pass over blocks whose descriptors lie on the device: d_blocks[i] names block i's bytes at d_base (src_off, src_len) and its
// tiles [first_tile, first_tile + n_tiles) of the `tiles` tiles in all, d_tile_block[t] the block of tile t.  crc_device_locked makes the
// two from host descriptors; the pruned batch search makes them by a kernel from the tables it located (mlz_stream_search_batch_prune.hip.inc).
int crc_device_described(mlz_ctx* c, hipStream_t st, const uint8_t* d_base, const BlockInfo* d_blocks, const uint32_t* d_tile_block, uint32_t tiles, int n, uint32_t* d_out) {
    static CrcPow pw;
    static CrcTabs tabs;
    static std::once_flag once;
    std::call_once(once, [] {
        uint32_t p = 1u << 30;  // x^1
        pw.x2n[0] = p;
        for (int k = 1; k < 32; k++) pw.x2n[k] = p = crc_mulmod(p, p);
        for (uint32_t t = 0; t < 256; t++) {
            tabs.k128[t] = crc_x2n(pw, 128ull * (255 - t), 3);                 // x^(8 * 128 (255 - t))
            tabs.ktile[t] = crc_x2n(pw, uint64_t(t) << kTileLog, 3);           // x^(8 * 32768 t)
        }
    });
    if (!c->d_crc_tabs.p) {   // per context (= per device): the two tables of constants
        HIPCHK(c, c->d_crc_tabs.ensure(sizeof(CrcTabs)));
        HIPCHK(c, hipMemcpy(c->d_crc_tabs.p, &tabs, sizeof(CrcTabs), hipMemcpyHostToDevice));
    }
    HIPCHK(c, c->d_crc_tiles.ensure(sizeof(uint32_t) * (size_t(tiles) + 1)));
    Timer t(c, T_CRC, st);
    if (tiles)
        hipLaunchKernelGGL(crc_tile_kernel, dim3(tiles), dim3(256), 0, st, d_base, d_blocks, d_tile_block, c->d_crc_tabs.as<CrcTabs>(), pw, c->d_crc_tiles.as<uint32_t>());
    hipLaunchKernelGGL(crc_block_kernel, dim3(n), dim3(64), 0, st, d_blocks, c->d_crc_tiles.as<uint32_t>(), c->d_crc_tabs.as<CrcTabs>(), pw, d_out, n);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int crc_device_locked(mlz_ctx* c, hipStream_t st, const uint8_t* d_base, const mlz_block_desc* desc, int n, uint32_t* d_out) {
    if (n <= 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    WorkspaceOrder order(c, st);
    c->call_seq++;
    uint32_t tiles = 0;
    int r = upload_blocks(c, st, desc, n, false, &tiles, nullptr, nullptr, true);
    if (r) return r;
    return crc_device_described(c, st, d_base, c->d_blocks_cur().as<BlockInfo>(), c->d_tile_block_cur().as<uint32_t>(), tiles, n, d_out);
}

// Device-visible address of the host range [p, p + len) when ALL of it lies in one page-locked (pinned, registered) allocation, else 0:
// such a destination is written by the kernels themselves.  (Both ends must lie in the SAME allocation: a buffer that merely starts
// in one is not ours to write through.)
uint64_t pinned_alias(const void* p, size_t len) {
    hipPointerAttribute_t at, at_end;
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeHost) { (void)hipGetLastError(); return 0; }
    if (len > 1) {
        const uint8_t* last = static_cast<const uint8_t*>(p) + len - 1;
        if (hipPointerGetAttributes(&at_end, last) != hipSuccess || at_end.type != hipMemoryTypeHost ||
            (at.devicePointer && at_end.devicePointer &&
             static_cast<const uint8_t*>(at_end.devicePointer) - static_cast<const uint8_t*>(at.devicePointer) != ptrdiff_t(len - 1))) {
            (void)hipGetLastError(); return 0;
        }
    }
    return reinterpret_cast<uint64_t>(at.devicePointer ? at.devicePointer : const_cast<void*>(p));
}

// ---- host-pointer plumbing: pack blocks into one device buffer, run, copy back ----
int ensure_stream_objects(mlz_ctx* c, size_t n_events, size_t pinned_bytes);  // mlz_stream.hip.inc

// Host-pointer batch: the blocks are cut into groups, and copy-in (stream s_in), kernels (the context's
// stream) and copy-out (s_out) of different groups overlap — the PCIe crossings (63 GB/s spec each way) cost about as
// much as the kernels, so run one after the other they halve the rate a Go caller sees.  Every copy is enqueued up
// front; the host only waits for a group's sizes (a few bytes per block) before it enqueues that group's exact-size
// copy-out, while the next groups' kernels are already queued.
// Group sizes: encode is bound by the copy-in (the kernels of the last group are what is left over when it ends: small
// groups); decode is bound by the kernels' own PCIe writes (every group drains its tail before the next starts: few groups).

int host_batch(mlz_ctx* c, bool encode, int level, int n, const uint8_t* const* src, const size_t* src_len, uint8_t* const* dst, const size_t* dst_cap,
               int64_t* out_len, bool with_header, const size_t* decoded_len /* decode_block only */) {
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<mlz_block_desc> desc(n);
    std::vector<int> gstart{0};
    size_t in_total = 0, out_total = 0, acc = 0;
    for (int i = 0; i < n; i++) {
        desc[i].src_off = in_total; desc[i].src_len = src_len[i];
        in_total += (src_len[i] + 63) & ~size_t(63);
        size_t cap = dst_cap[i];
        if (encode) cap = std::min<size_t>(cap, size_t(kMaxBlockSize) + 16);
        else if (decoded_len) cap = decoded_len[i];
        else cap = std::min<size_t>(cap, kMaxBlockSize);
        desc[i].dst_off = out_total; desc[i].dst_cap = cap;
        out_total += (cap + 63) & ~size_t(63);
        acc += std::max<size_t>(src_len[i], cap);
        if (acc >= (encode ? c->host_group_enc : c->host_group_dec) && i + 1 < n) { gstart.push_back(i + 1); acc = 0; }
    }
    gstart.push_back(n);
    const size_t ngroups = gstart.size() - 1;
    // Pinned (page-locked, device-visible) destinations are written by the kernels themselves: the gather pass of the
    // encoder stores the block straight into the caller's buffer and the decoder's passes store every tile there as
    // well as in HBM, so the batch has no copy-out stage at all (on this ROCm build the copy-out ran as shader copies
    // that queued up behind every kernel of the batch).  Pageable destinations go through the copy-out below.
    std::vector<uint64_t> mirror(size_t(n), 0);
    bool use_mirror = encode || (c->decode_algo == 0 && c->general_algo == 0);
    for (int i = 0; use_mirror && i < n; i++) {
        mirror[size_t(i)] = pinned_alias(dst[i], dst_cap[i]);
        if (!mirror[size_t(i)]) use_mirror = false;
    }
    const uint64_t* mir = use_mirror ? mirror.data() : nullptr;
    if (!encode) begin_decode_call(c);   // (one call however many groups)
    HIPCHK(c, c->d_in.ensure(in_total + 64));
    HIPCHK(c, c->d_out.ensure(out_total + 64));
    HIPCHK(c, c->d_len.ensure(sizeof(int64_t) * n));
    int r = ensure_stream_objects(c, 3 * ngroups, sizeof(int64_t) * size_t(n));
    if (r) return r;
    int64_t* h_len = static_cast<int64_t*>(c->pinned2);
    hipStream_t st = c->stream;
    for (size_t g = 0; g < ngroups; g++) {  // every copy-in, back to back on the copy-in stream
        for (int i = gstart[g]; i < gstart[g + 1]; i++)
            if (src_len[i]) HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + desc[i].src_off, src[i], src_len[i], hipMemcpyHostToDevice, c->s_in));
        HIPCHK(c, hipEventRecord(c->evpool[3 * g], c->s_in));
    }
    for (size_t g = 0; g < ngroups; g++) {  // kernels of a group once its bytes are in; its sizes go out behind them
        const int b0 = gstart[g], cnt = gstart[g + 1] - gstart[g];
        HIPCHK(c, hipStreamWaitEvent(st, c->evpool[3 * g], 0));
        r = encode ? encode_device_locked(c, st, level, c->d_in.as<uint8_t>(), c->d_out.as<uint8_t>(), desc.data() + b0, cnt, c->d_len.as<int64_t>() + b0, with_header,
                                          mir ? mir + b0 : nullptr)
                   : decode_device_locked(c, st, c->d_in.as<uint8_t>(), c->d_out.as<uint8_t>(), desc.data() + b0, cnt, c->d_len.as<int64_t>() + b0, !with_header,
                                          mir ? mir + b0 : nullptr, false);
        if (r) { (void)hipStreamSynchronize(c->s_in); (void)hipStreamSynchronize(st); (void)hipStreamSynchronize(c->s_out); return r; }
        HIPCHK(c, hipEventRecord(c->evpool[3 * g + 1], st));
        HIPCHK(c, hipStreamWaitEvent(c->s_out, c->evpool[3 * g + 1], 0));
        HIPCHK(c, hipMemcpyAsync(h_len + b0, c->d_len.as<int64_t>() + b0, sizeof(int64_t) * size_t(cnt), hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipEventRecord(c->evpool[3 * g + 2], c->s_out));
    }
    for (size_t g = 0; g < ngroups; g++) {  // exact-size copy-out as soon as a group's sizes are known
        HIPCHK(c, hipEventSynchronize(c->evpool[3 * g + 2]));
        for (int i = gstart[g]; i < gstart[g + 1]; i++) {
            out_len[i] = h_len[i];
            if (out_len[i] > 0) {
                if (size_t(out_len[i]) > dst_cap[i]) { out_len[i] = -MLZ_ERR_DST_TOO_SMALL; continue; }
                if (!use_mirror) HIPCHK(c, hipMemcpyAsync(dst[i], c->d_out.as<uint8_t>() + desc[i].dst_off, size_t(out_len[i]), hipMemcpyDeviceToHost, c->s_out));
            }
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    HIPCHK(c, hipStreamSynchronize(st));
    return 0;
}

// Single-block calls (mlz_encode / mlz_encode_block / mlz_decode / mlz_decode_block) from concurrent threads are
// combined into batched launches: the reference's Writer and Reader call their block codec from one goroutine
// per block (writer.go:501-560, reader.go:830-859), and one 8 MiB block alone cannot fill the device (a tile is a
// serial chain: one block takes about as long as twelve).  Every caller queues its request; whoever finds no
// batch in flight becomes the leader, takes every queued request of the same kind (up to kCombineMax) and runs
// them as ONE host batch while later arrivals queue up behind it; the others sleep until their request is done.
// No timer, no helper thread: a lone caller runs at once, a busy queue batches itself.
constexpr size_t kCombineMax = 64;
void submit_single(mlz_ctx* c, SingleReq& rq) {
    std::unique_lock<std::mutex> lk(c->q_mu);
    c->q_pending.push_back(&rq);
    while (!rq.done) {
        if (c->q_leader) { c->q_cv.wait(lk); continue; }
        c->q_leader = true;
        std::vector<SingleReq*> group;
        {
            const SingleReq& head = *c->q_pending.front();
            std::vector<SingleReq*> rest;
            for (SingleReq* r : c->q_pending) {
                if (group.size() < kCombineMax && r->same_kind(head)) group.push_back(r); else rest.push_back(r);
            }
            c->q_pending.swap(rest);
        }
        lk.unlock();
        const int n = int(group.size());
        std::vector<const uint8_t*> src(n); std::vector<size_t> slen(n), cap(n), dlen(n);
        std::vector<uint8_t*> dst(n); std::vector<int64_t> out(n, 0);
        for (int i = 0; i < n; i++) { src[i] = group[i]->src; slen[i] = group[i]->n; dst[i] = group[i]->dst; cap[i] = group[i]->cap; dlen[i] = group[i]->dlen; }
        const SingleReq& k = *group[0];
        const int r = host_batch(c, k.encode, k.level, n, src.data(), slen.data(), dst.data(), cap.data(), out.data(), k.with_header,
                                 k.has_dlen ? dlen.data() : nullptr);
        lk.lock();
        for (int i = 0; i < n; i++) { group[i]->rc = r; group[i]->out = out[i]; group[i]->done = true; }
        c->q_batches++; c->q_requests += uint64_t(n);
        c->q_leader = false;
        c->q_cv.notify_all();
    }
}

// The contexts a host-pointer call is dealt to: the context itself, or the per-device contexts behind it (mlz_init_devices).
struct Workers {
    mlz_ctx* one;
    mlz_ctx* const* list;
    size_t n;
    explicit Workers(mlz_ctx* c) : one(c), list(&one), n(1) {
        if (!c->kids.empty()) { list = c->kids.data(); n = c->kids.size(); }
    }
    mlz_ctx* next() const { return n == 1 ? list[0] : list[one->rr.fetch_add(1, std::memory_order_relaxed) % n]; }   // single-block calls: the kids in turn
};

// How the four single-block entry points end: the request through the queue of one of the context's devices; what it produced, or the batch's failure.
int64_t run_single(mlz_ctx* c, SingleReq rq) { submit_single(Workers(c).next(), rq); return rq.rc ? rq.rc : rq.out; }

// The kid whose device holds `p` (a device-resident call on a several-device context), or the context itself.
mlz_ctx* owner_of(mlz_ctx* c, const void* p) {
    if (c->kids.empty()) return c;
    hipPointerAttribute_t at;
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice) {
        for (mlz_ctx* k : c->kids) if (k->device == at.device) return k;
        return nullptr;
    }
    (void)hipGetLastError();
    return nullptr;
}

// A host-pointer batch over several devices: contiguous block ranges of about equal weight, one thread and one PCIe link per device,
// every range through host_batch on its own context (the reference fans the blocks of a stream to goroutines, writer.go:501-560,
// reader.go:830-859; results land at the caller's dst[i] whatever device produced them, so there is nothing to gather).
int multi_host_batch(mlz_ctx* c, bool encode, int level, int n, const uint8_t* const* src, const size_t* src_len, uint8_t* const* dst, const size_t* dst_cap,
                     int64_t* out_len) {
    Workers w(c);
    if (w.n == 1) return host_batch(w.list[0], encode, level, n, src, src_len, dst, dst_cap, out_len, true, nullptr);
    if (!encode)   // a device that gets no block of this call has no general block in it either (counters 2 / 6 sum over the devices)
        for (size_t j = 0; j < w.n; j++) { std::lock_guard<std::mutex> lk(w.list[j]->mu); begin_decode_call(w.list[j]); }
    std::vector<uint64_t> pre(size_t(n) + 1, 0);
    for (int i = 0; i < n; i++) {
        uint64_t wt = src_len[i];
        if (!encode) { const int64_t dl = mlz_decoded_len(src[i], src_len[i]); if (dl > 0) wt += uint64_t(dl); }
        pre[size_t(i) + 1] = pre[size_t(i)] + wt + 4096;
    }
    const uint64_t total = pre[size_t(n)];
    size_t k = std::min<size_t>(w.n, size_t(n));
    if (total < (uint64_t(4) << 20)) k = 1;    // not worth a second device
    if (k == 1) return host_batch(w.next(), encode, level, n, src, src_len, dst, dst_cap, out_len, true, nullptr);
    std::vector<int> cut(k + 1, n);
    cut[0] = 0;
    {
        size_t j = 1;
        for (int i = 0; i < n && j < k; i++)
            while (j < k && pre[size_t(i) + 1] * k >= total * j) cut[j++] = i + 1;
    }
    std::vector<int> rcs(k, 0);
    auto work = [&](size_t j) {
        const int b0 = cut[j], cnt = cut[j + 1] - cut[j];
        if (cnt > 0) rcs[j] = host_batch(w.list[j], encode, level, cnt, src + b0, src_len + b0, dst + b0, dst_cap + b0, out_len + b0, true, nullptr);
    };
    std::vector<std::thread> th;
    for (size_t j = 1; j < k; j++) th.emplace_back(work, j);
    work(0);
    for (std::thread& t : th) t.join();
    for (size_t j = 0; j < k; j++)
        if (rcs[j]) { std::lock_guard<std::mutex> lk(c->mu); c->err = w.list[j]->err; return rcs[j]; }
    return 0;
}

}  // namespace

extern "C" {

int mlz_version(void) { return 2; }

int mlz_init(int device, mlz_ctx** out) {
    if (!out) return -MLZ_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return -MLZ_ERR_HIP;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return -MLZ_ERR_HIP; }
    if (device >= count) return -MLZ_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return -MLZ_ERR_HIP;
    mlz_ctx* c = new mlz_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->dev_name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
        c->n_cus = prop.multiProcessorCount;
    }
    if (c->n_cus <= 0) c->n_cus = 64;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return -MLZ_ERR_HIP; }
    for (int k = 0; k < 2; k++)
        if (hipEventCreateWithFlags(&c->upload_done_k[k], hipEventDisableTiming) != hipSuccess) { delete c; return -MLZ_ERR_HIP; }
    if (hipEventCreateWithFlags(&c->ws_done, hipEventDisableTiming) != hipSuccess) { delete c; return -MLZ_ERR_HIP; }
    *out = c;
    return 0;
}

int mlz_init_devices(const int* devices, int n_devices, mlz_ctx** out) {
    if (!out || (devices && n_devices <= 0)) return -MLZ_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return -MLZ_ERR_HIP;
    std::vector<int> devs;
    if (devices) devs.assign(devices, devices + n_devices);
    else for (int d = 0; d < count && (n_devices <= 0 || d < n_devices); d++) devs.push_back(d);   // every visible device (or the first n_devices)
    mlz_ctx* p = new mlz_ctx();
    for (int d : devs) {
        mlz_ctx* k = nullptr;
        const int r = (d < 0 || d >= count) ? -MLZ_ERR_ARG : mlz_init(d, &k);
        if (r) { for (mlz_ctx* q : p->kids) mlz_destroy(q); delete p; return r; }
        p->kids.push_back(k);
    }
    p->device = p->kids[0]->device;
    p->n_cus = p->kids[0]->n_cus;
    p->dev_name = std::to_string(p->kids.size()) + " x " + p->kids[0]->dev_name;
    *out = p;
    return 0;
}

int mlz_device_count(mlz_ctx* c) { return !c ? -MLZ_ERR_ARG : c->kids.empty() ? 1 : int(c->kids.size()); }

mlz_ctx* mlz_device_ctx(mlz_ctx* c, int i) {
    if (!c || i < 0) return nullptr;
    if (c->kids.empty()) return i == 0 ? c : nullptr;
    return size_t(i) < c->kids.size() ? c->kids[size_t(i)] : nullptr;
}

void mlz_destroy(mlz_ctx* c) {
    if (!c) return;
    if (!c->kids.empty()) {   // a several-device context: its kids hold everything
        for (mlz_ctx* k : c->kids) mlz_destroy(k);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (int side = 0; side < 3; side++) for (DevBuf* b : c->bufs(side)) b->release();
    for (int k = 0; k < 2; k++) if (c->pinned_k[k]) (void)hipHostFree(c->pinned_k[k]);
    if (c->pinned2) (void)hipHostFree(c->pinned2);
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
    for (int i = 0; i < T_COUNT; i++)
        for (int k = 0; k < mlz_ctx::kTimerRing; k++)
            for (int e = 0; e < 2; e++)
                if (c->evr[i][k][e]) (void)hipEventDestroy(c->evr[i][k][e]);
    for (int k = 0; k < 2; k++) if (c->upload_done_k[k]) (void)hipEventDestroy(c->upload_done_k[k]);
    if (c->ws_done) (void)hipEventDestroy(c->ws_done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* mlz_last_error(mlz_ctx* c) {
    if (!c) return "null context";
    if (c->err.empty()) for (mlz_ctx* k : c->kids) if (!k->err.empty()) return k->err.c_str();
    return c->err.c_str();
}

int mlz_device_name(mlz_ctx* c, char* buf, size_t cap) {
    if (!c || !buf || cap == 0) return -MLZ_ERR_ARG;
    std::snprintf(buf, cap, "%s", c->dev_name.c_str());
    return 0;
}

int64_t mlz_max_encoded_len(uint64_t n) {
    if (n > kMaxBlockSize) return -1;
    if (n == 0) return 1;
    return int64_t(n) + 2;
}

int64_t mlz_decoded_len(const uint8_t* src, size_t n) {
    uint64_t body, dlen; int lits;
    int e = parse_block_header(src, n, &body, &dlen, &lits);
    if (e == 3) {  // non-MinLZ block: DecodedLen still reports the Snappy varint (decode.go:132-136)
        uint64_t x = 0; uint32_t shift = 0;
        for (size_t i = 0; i < n && i < 10; i++) {
            uint8_t b = src[i];
            if (b < 0x80) { x |= uint64_t(b) << shift; return x > 0xffffffffull ? -MLZ_ERR_CORRUPT : int64_t(x); }
            x |= uint64_t(b & 0x7f) << shift; shift += 7;
        }
        return -MLZ_ERR_CORRUPT;
    }
    if (e) return -e;
    return int64_t(dlen);
}

int64_t mlz_encode(mlz_ctx* c, int level, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
    if (!c || (!src && n) || !dst) return -MLZ_ERR_ARG;
    if (n > kMaxBlockSize) return -MLZ_ERR_TOO_LARGE;
    if (int64_t(dst_cap) < mlz_max_encoded_len(n)) return -MLZ_ERR_DST_TOO_SMALL;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    return run_single(c, {true, true, false, level, src, n, dst, dst_cap, 0});
}

int64_t mlz_encode_block(mlz_ctx* c, int level, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
    if (!c || (!src && n) || !dst) return -MLZ_ERR_ARG;
    if (n > kMaxBlockSize) return -MLZ_ERR_TOO_LARGE;
    if (dst_cap < n) return -MLZ_ERR_DST_TOO_SMALL;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    return run_single(c, {true, false, false, level, src, n, dst, dst_cap, 0});
}

int64_t mlz_decode(mlz_ctx* c, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
    if (!c || !src || (!dst && dst_cap)) return -MLZ_ERR_ARG;
    uint64_t body, dlen; int lits;
    int e = parse_block_header(src, n, &body, &dlen, &lits);
    if (e) return -e;
    if (dlen > dst_cap) return -MLZ_ERR_DST_TOO_SMALL;
    if (dlen == 0) return 0;
    return run_single(c, {false, true, false, 0, src, n, dst, dst_cap, 0});
}

int mlz_decode_block(mlz_ctx* c, const uint8_t* src, size_t clen, uint8_t* dst, size_t n) {
    if (!c || (!src && clen) || (!dst && n)) return -MLZ_ERR_ARG;
    if (n > kMaxBlockSize) return -MLZ_ERR_TOO_LARGE;
    if (n == 0) return clen == 0 ? 0 : 1;
    const int64_t out = run_single(c, {false, false, true, 0, src, clen, dst, n, n});   // (a failed batch: -MLZ_ERR_HIP, the only code a decode batch fails with)
    if (out == int64_t(n)) return 0;
    // Only a DEVICE failure (-MLZ_ERR_HIP: a launch that failed, a bounded wait that gave up) is passed on as < 0, the shim's cue
    // to run its CPU decoder (go/minlz_hip.go: r < 0, counted in hipFallbacks).  Every other per-block code (corrupt, too large,
    // unsupported, destination too small) is a verdict on the INPUT: minLZDecode's contract has one value for those, 1 = corrupt
    // (decode.go:26), and a healthy device never makes the caller decode a block twice.
    if (out == -MLZ_ERR_HIP) return -MLZ_ERR_HIP;
    return 1;
}

int mlz_encode_batch(mlz_ctx* c, int level, int n, const uint8_t* const* src, const size_t* src_len, uint8_t* const* dst, const size_t* dst_cap,
                     int64_t* out_len) {
    if (!c || n < 0) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    if (!valid_level(level)) return -MLZ_ERR_INVALID_LEVEL;
    return multi_host_batch(c, true, level, n, src, src_len, dst, dst_cap, out_len);
}

int mlz_decode_batch(mlz_ctx* c, int n, const uint8_t* const* src, const size_t* src_len, uint8_t* const* dst, const size_t* dst_cap, int64_t* out_len) {
    if (!c || n < 0) return -MLZ_ERR_ARG;
    if (n == 0) return 0;
    return multi_host_batch(c, false, 0, n, src, src_len, dst, dst_cap, out_len);
}

int mlz_encode_batch_device(mlz_ctx* c, void* stream, int level, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n,
                            int64_t* d_out_len) {
    if (!c || !desc || n < 0 || !d_out_len) return -MLZ_ERR_ARG;
    if (!(c = owner_of(c, d_src))) return -MLZ_ERR_ARG;   // (several devices: the one that holds the buffers)
    std::lock_guard<std::mutex> lk(c->mu);
    return encode_device_locked(c, static_cast<hipStream_t>(stream), level, d_src, d_dst, desc, n, d_out_len, true);
}

int mlz_decode_batch_device(mlz_ctx* c, void* stream, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* desc, int n, int64_t* d_out_len) {
    if (!c || !desc || n < 0 || !d_out_len) return -MLZ_ERR_ARG;
    if (!(c = owner_of(c, d_src))) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return decode_device_locked(c, static_cast<hipStream_t>(stream), d_src, d_dst, desc, n, d_out_len, false);
}

int mlz_set_option(mlz_ctx* c, int opt, int64_t value) {
    if (!c) return -MLZ_ERR_ARG;
    if (!c->kids.empty()) {   // every device alike (the debug read-backs 5 / 7: the first device's)
        if (opt == MLZ_OPT_PROFILE_READ || opt == MLZ_OPT_TILE_TIMELINE_READ) return mlz_set_option(c->kids[0], opt, value);
        for (mlz_ctx* k : c->kids) { const int r = mlz_set_option(k, opt, value); if (r) return r; }
        return 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    switch (opt) {
    case MLZ_OPT_DECODE_ALGO: c->decode_algo = int(value); return 0;
    case MLZ_OPT_ENCODE_FAR: c->encode_far = int(value); return 0;
    case MLZ_OPT_GENERAL_ALGO: c->general_algo = int(value); return 0;  // 0 = pointer-jumping pass for general blocks (default), 1 = tile chain
    case MLZ_OPT_TIMER_MASK: c->timer_mask = uint32_t(value); return 0;  // which timers record events (bit = index of mlz_timer_name)
    case MLZ_OPT_HOST_GROUP_ENC: c->host_group_enc = size_t(value > 0 ? value : 1) << 20; return 0;  // tuning: MiB per group of a host-pointer encode batch
    case MLZ_OPT_HOST_GROUP_DEC: c->host_group_dec = size_t(value > 0 ? value : 1) << 20; return 0;  // ... of a decode batch
    case MLZ_OPT_DEVICE_GROUP: c->device_group = size_t(value > 0 ? value : 1) << 20; return 0;  // MiB of uncompressed data per internal group of a device batch
    case MLZ_OPT_FAR_SLICES_L2: c->far_slices_l2 = int(value); return 0;  // debug / cross-check: LevelBalanced's far tables by the slice kernel of round 4
    case MLZ_OPT_L2_GAP: if (value < 1 || value > 16) return -MLZ_ERR_ARG; c->l2_gap = int(value); return 0;
    case MLZ_OPT_FOLD_LAYOUT: c->fold_layout = int(value); return 0;  // encode: 1 (default) = layout inside the gather kernel where possible, 0 = always the separate layout kernel (cross-checks)
    case MLZ_OPT_LEVEL0_KERNEL: c->level0_by_e = int(value); return 0;  // decode: 1 (default) = level-0 tiles, when no more than CUs, by dec_level0_kernel before the exec pass; 0 = by the exec pass
    case MLZ_OPT_FUSED_SERIALIZER: c->fuse_ser = int(value); return 0;  // encode: 1 (default) = the match kernel serializes its pieces itself, 0 = the separate serializer kernel of rounds 2-5 (cross-checks)
    case MLZ_OPT_GEN_SETTLE_CAP: c->gen_settle_cap = int(value); return 0;  // tuning: role S workgroups of the general pass at most
    case 25 /* debug, unnamed in the header */: c->l0_grid_cap = int(value); return 0;  // debug: level-0 candidates dec_level0_kernel is launched for at most (0 = the CU count)
    case MLZ_OPT_L2_FREE: c->l2_free = int(value); return 0;  // LevelBalanced: 1 = no tile levels (ratio of the reference's L2 and better; blocks decode as general blocks)
    case MLZ_OPT_GEN_PACKED: c->gen_force_packed = int(value); return 0;  // tests: general blocks settle through the byte-packed pool (fallback path of dec_general_kernel)
    case MLZ_OPT_GEN_SPIN: c->gen_spin_limit = value > 0 ? uint32_t(value) : 1u; return 0;  // grid-barrier patience of the general-block pass, in polls (tests)
    case MLZ_OPT_DEBUG_STATUS: c->debug_status = int(value); return 0;  // debug: report failure sites in the error code
    case MLZ_OPT_PROFILE: {  // debug: per-phase cycle counters (16 x u64: 0-7 encode, 8-15 decode)
        c->prof_on = value != 0;
        if (c->prof_on) { if (c->d_prof.ensure(kProfBytes) != hipSuccess) return -MLZ_ERR_HIP; if (hipMemset(c->d_prof.p, 0, kProfBytes) != hipSuccess) return -MLZ_ERR_HIP; }
        return 0;
    }
    case MLZ_OPT_PROFILE_READ: {  // debug: read the counters back into a host buffer whose address is `value`
        if (!c->d_prof.p) return -MLZ_ERR_ARG;
        if (hipDeviceSynchronize() != hipSuccess) return -MLZ_ERR_HIP;
        if (hipMemcpy(reinterpret_cast<void*>(value), c->d_prof.p, 128, hipMemcpyDeviceToHost) != hipSuccess) return -MLZ_ERR_HIP;
        return 0;
    }
    case MLZ_OPT_TILE_TIMELINE_READ: {  // debug: read the exec pass's per-tile timeline (kProfTiles x 4 u64, 100 MHz clock) into a host buffer
        if (!c->d_prof.p) return -MLZ_ERR_ARG;
        if (hipDeviceSynchronize() != hipSuccess) return -MLZ_ERR_HIP;
        if (hipMemcpy(reinterpret_cast<void*>(value), c->d_prof.as<uint8_t>() + 256, kProfBytes - 256, hipMemcpyDeviceToHost) != hipSuccess) return -MLZ_ERR_HIP;
        return 0;
    }
    case MLZ_TIMER_ENABLE:
        if (value < 0 || value > 2) return -MLZ_ERR_ARG;
        if (value != 0) {
            for (int i = 0; i < T_COUNT; i++)
                for (int k = 0; k < mlz_ctx::kTimerRing; k++)
                    for (int e = 0; e < 2; e++)
                        if (!c->evr[i][k][e]) HIPCHK(c, hipEventCreate(&c->evr[i][k][e]));
        }
        c->timing = int(value);
        for (int i = 0; i < T_COUNT; i++) {   // (events recorded under the old setting are dropped unread)
            c->ev_cnt[i] = c->ev_res[i] = 0; c->ev_calls[i] = 0; c->ev_last_call[i] = ~uint64_t(0); c->acc_ms[i] = 0;
        }
        return 0;
    default: return -MLZ_ERR_ARG;
    }
}

int mlz_release_stream(mlz_ctx* c, void* stream) {
    if (!c) return -MLZ_ERR_ARG;
    if (!c->kids.empty()) {
        for (mlz_ctx* k : c->kids) { const int r = mlz_release_stream(k, stream); if (r) return r; }
        return 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ws_used && !c->ws_recorded && c->ws_stream == static_cast<hipStream_t>(stream)) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventRecord(c->ws_done, c->ws_stream));   // covers everything the context put on that stream
        c->ws_recorded = true;
    }
    return 0;
}

int64_t mlz_get_counter(mlz_ctx* c, int which) {
    if (!c) return -MLZ_ERR_ARG;
    if (!c->kids.empty()) {   // sums over the devices (6, a team size: the largest)
        int64_t acc = 0;
        for (mlz_ctx* k : c->kids) {
            const int64_t v = mlz_get_counter(k, which);
            if (v < 0) return v;
            acc = which == 6 ? std::max(acc, v) : acc + v;
        }
        return acc;
    }
    if (which == 2 || which == 6) {
        // 2: blocks of the last decode call that fit no level pattern; 6: workgroups per block (1, 2 or 4) its general pass settled with (0 = no general block).
        // Both over ALL internal groups of the call (sum / maximum, kept by dec_schedule_kernel); waits for the device.
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->d_gen_acc.p || c->acc_call != c->dec_call) return 0;   // (the last decode call ran no group of the parallel decoder: nothing reset the words)
        uint32_t v[2] = {0, 0};
        if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(v, c->d_gen_acc.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -MLZ_ERR_HIP;
        return int64_t(which == 2 ? v[0] : (v[0] ? v[1] : 0));
    }
    if (which == 3 || which == 4) {  // device workspace this context holds: 3 = encode side, 4 = decode side (grow-only buffers: the high-water mark of the calls so far)
        std::lock_guard<std::mutex> lk(c->mu);
        size_t sum = 0;
        for (const DevBuf* b : c->bufs(which - 3)) sum += b->cap;
        return int64_t(sum);
    }
    if (which == 5) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->gen_fallbacks); }
    if (which == 7 || which == 8) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(which == 7 ? c->range_chunks : c->range_scratch); }
    if (which == 9) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->range_plan_host); }
    if (which == 12) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->batch_long); }
    if (which == 13) { std::lock_guard<std::mutex> lk(c->mu); return c->acc_call == c->dec_call ? int64_t(c->l0_launches) : 0; }   // groups of the last decode call that took dec_level0_kernel's launch
    if (which == 14) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->search_compressed); }
    if (which == 16) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->search_plan_bytes); }
    if (which == 15) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->tables_compressed); }
    if (which == 17) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(c->table_slot_bytes); }
    if (which == 10 || which == 11) { std::lock_guard<std::mutex> lk(c->mu); return int64_t(which == 10 ? c->search_chunks : c->search_tables); }
    std::lock_guard<std::mutex> lk(c->q_mu);
    return which == 0 ? int64_t(c->q_batches) : which == 1 ? int64_t(c->q_requests) : -MLZ_ERR_ARG;
}

int mlz_get_timers(mlz_ctx* c, float* ms, int cap) {
    if (!c || !ms) return -MLZ_ERR_ARG;
    if (!c->kids.empty()) {   // the devices work side by side: the slowest one's time per kernel family
        int n = 0;
        std::vector<float> t(size_t(std::max(cap, 0)));
        for (int i = 0; i < cap; i++) ms[i] = -1.f;
        for (mlz_ctx* k : c->kids) {
            n = mlz_get_timers(k, t.data(), cap);
            if (n < 0) return n;
            for (int i = 0; i < n; i++) ms[i] = std::max(ms[i], t[size_t(i)]);
        }
        return n;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    int n = std::min<int>(cap, T_COUNT);
    for (int i = 0; i < n; i++) {
        ms[i] = -1.f;
        while (c->ev_res[i] < c->ev_cnt[i]) c->resolve_one(i);
        if (c->ev_calls[i]) ms[i] = float(c->acc_ms[i] / double(c->ev_calls[i]));
    }
    return n;
}

const char* mlz_timer_name(int idx) { return idx >= 0 && idx < T_COUNT ? kTimerNames[idx] : ""; }

int mlz_crc_batch_device(mlz_ctx* c, void* stream, const uint8_t* d_base, const mlz_block_desc* desc, int n, uint32_t* d_out) {
    if (!c || !desc || n < 0 || !d_out) return -MLZ_ERR_ARG;
    if (!(c = owner_of(c, d_base))) return -MLZ_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return crc_device_locked(c, static_cast<hipStream_t>(stream), d_base, desc, n, d_out);
}

int64_t mlz_crc(mlz_ctx* c, const uint8_t* src, size_t n) {
    if (!c || (!src && n)) return -MLZ_ERR_ARG;
    c = Workers(c).next();
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->d_in.ensure(n + 64));
    HIPCHK(c, c->d_crc.ensure(64));
    if (n) HIPCHK(c, hipMemcpyAsync(c->d_in.p, src, n, hipMemcpyHostToDevice, c->stream));
    mlz_block_desc d{0, n, 0, 0};
    int r = crc_device_locked(c, c->stream, c->d_in.as<uint8_t>(), &d, 1, c->d_crc.as<uint32_t>());
    if (r) return r;
    uint32_t v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->d_crc.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return int64_t(v);
}

#ifdef MLZ_M2_PROF
// debug build only (tools/m2prof.py): per-phase cycle sums of match_tiles_kernel; reset after reading
int mlz_debug_m2prof(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return -MLZ_ERR_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mlz::g_m2prof), sizeof(unsigned long long) * 16) != hipSuccess) return -MLZ_ERR_HIP;
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mlz::g_m2prof), z, sizeof(z)) != hipSuccess) return -MLZ_ERR_HIP;
    return 0;
}
#endif

#ifdef MLZ_IDX_PROF
// debug build only (tools/idxprof.py): per-phase time sums of dec_index_kernel; reset after reading
int mlz_debug_idxprof(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return -MLZ_ERR_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mlz::g_idxprof), sizeof(unsigned long long) * 16) != hipSuccess) return -MLZ_ERR_HIP;
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mlz::g_idxprof), z, sizeof(z)) != hipSuccess) return -MLZ_ERR_HIP;
    return 0;
}
#endif

}  // extern "C"

#include "mlz_search_tables.hip.inc"
#include "mlz_search_tables_compress.hip.inc"
#include "mlz_stream.hip.inc"
#include "mlz_stream_walk.hip.inc"
#include "mlz_stream_ranges.hip.inc"
#include "mlz_stream_batch.hip.inc"
#include "mlz_stream_ranges_dev.hip.inc"
#include "mlz_stream_search_compressed.hip.inc"
#include "mlz_stream_search.hip.inc"
#include "mlz_stream_search_many.hip.inc"
#include "mlz_stream_search_batch.hip.inc"
#include "mlz_stream_search_batch_prune.hip.inc"
#include "mlz_stream_sidecar.hip.inc"
#include "mlz_stream_sidecar_extract.h"
#include "mlz_stream_sidecar_extract.hip.inc"
#include "mlz_stream_records.hip.inc"
#include "mlz_stream_record_index.hip.inc"
#include "mlz_stream_record_index_store.hip.inc"
#include "mlz_stream_grep.hip.inc"
#include "mlz_stream_set.hip.inc"
#include "mlz_stream_set_tables.hip.inc"
#include "mlz_stream_regex.hip.inc"
#include "mlz_stream_regex_prune.hip.inc"
