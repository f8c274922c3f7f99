// mlz_encode.hip.inc — what the encoder's kernels share (included by mlz_hip.hip before mlz_encode2.hip.inc): hashes, tile
// levels, the far tables (far_build_kernel), wave scans, the token sink, the per-block layout pass.
//
// Round 1's encoder lived here: one 64-lane wavefront per 32 KiB tile, 64 consecutive positions probed per step, a scalar
// selection walk and batched token emission — replaced in round 2 by the match + serialize kernels of mlz_encode2.hip.inc
// (first for LevelFastest / LevelSuperFast, at the end of the round for LevelBalanced as well).  What stayed is below.

namespace mlz {

constexpr uint32_t kLaneCap = 32;       // per-lane match extension cap; longer = cooperative
#ifndef MLZ_FAR_BITS
#define MLZ_FAR_BITS 17
#endif
#ifndef MLZ_EPOCH_LOG
#define MLZ_EPOCH_LOG 21
#endif
// 2^17 entries per (2 MiB epoch, level set): one per four sampled windows.  2^18 compressed 1 % better (enwik-like 0.4627 vs
// 0.4675) but the tables of the 1.5 epochs an XCD works on at a time then overflow its 4 MiB L2, and every sampled window is
// hashed by one workgroup per 2^15-bucket slice of its epoch's table: with half the slices far_build takes half the time
// (0.159 -> 0.081 ms per 100 MB) and the match kernel 6 % less (0.874 -> 0.824 ms).
constexpr int kFarBits = MLZ_FAR_BITS;    // far table entries per (epoch, level)
constexpr int kEpochLog = MLZ_EPOCH_LOG;  // far epoch size (log2 bytes)
// (the far probe of a position's own epoch does not test the offset: an epoch must fit the longest copy3 offset, encode.go:58)
static_assert((1u << kEpochLog) <= kMaxCopy3Offset, "a position's own epoch lies within one copy3 offset");
constexpr int kFarStride = 4;           // far tables index every 4th position (probes are dense)
// Blocks below 1 MiB get smaller far tables: a table of 2^17 entries for each of the three level sets is 1.5 MiB to fill
// and write per block — 24 times a 64 KiB block, the far build of 4096 such blocks wrote 6 GiB (1.44 ms of a 4.8 ms
// encode) and the match kernel's probes missed every cache.  A quarter of an entry per byte of the block, between 2^14
// and 2^17 (LevelBalanced, whose tables hold twice the windows: one bit more): costs 0.5 - 1 % in size on 64 - 256 KiB
// blocks (CPU model; 64 KiB text blocks 0.4337 -> 0.4367) for 1.5x the encode speed (4096 x 64 KiB: 56 -> 85 GB/s).
#ifndef MLZ_SMALL_FB_SHIFT
#define MLZ_SMALL_FB_SHIFT 2
#endif
__host__ __device__ __forceinline__ constexpr int small_far_bits(uint64_t block_len) {
    int lg = 14 + MLZ_SMALL_FB_SHIFT;   // ceil(log2(len))
    while (lg < 17 + MLZ_SMALL_FB_SHIFT && (1ull << lg) < block_len) lg++;
    return lg - MLZ_SMALL_FB_SHIFT;
}
constexpr uint32_t kFarMin = 8;         // minimum far match
constexpr int kLevels = 4;              // tile levels (far sources live in lower-level tiles)

__device__ __forceinline__ uint64_t ld64u(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
// Far-table entries are (position << 9) | tag: 9 further bits of the same product let a probe reject
// a foreign window without fetching the candidate's bytes (a 64-byte HBM line per probe otherwise).
constexpr int kFarTagBits = 9;
constexpr uint32_t kFarTagMask = (1u << kFarTagBits) - 1;
struct FarHash { uint32_t idx, tag; };
// (tagmask: which of the 9 tag bits a table uses — all of them, or far_tag_mask(FB) below)
__device__ __forceinline__ FarHash far_hash(uint64_t v, int bits, uint32_t tagmask = kFarTagMask) {
    // Round 3: two 32-bit multiplies and an add.  On gfx950 v_mul_lo_u32 issues in the same 4 cycles as v_mul_u32_u24 / v_mad_u32_u24
    // (profiles/r03_valu_rate.txt: the "quarter rate" of older parts does not apply), so four 24-bit multiply-adds bought
    // nothing over this; the model's ratio is a hair better (enwik-like 0.4687 -> 0.4685).
    const uint32_t a = (uint32_t(v) * 0x9E3779B1u + uint32_t(v >> 32)) * 0x85EBCA77u;
    return {a >> (32 - bits), (a >> (32 - bits - kFarTagBits)) & tagmask};
}
__device__ __forceinline__ uint32_t ctz64(uint64_t v) { return __builtin_ctzll(v); }
__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint32_t rdfirst(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Level of a tile.  A tile may copy from its own bytes and from tiles of strictly lower level, so the pattern
// trades how much of the window each level sees against how many tiles sit at the blind bottom (level-0 tiles
// can only match inside themselves and compress ~40 % worse) — and against the DECODER's critical path: its exec pass runs
// the tiles of a block level by level, a round of ~100 us per level whatever the batch (DESIGN.md section 6).  Three
// patterns, 2 bits per tile, tile 0 in the low bits, period 16:
//   fast  (round 1):                      0 1 2 3 0 1 2 3 ...                one tile in four does no far probing
//   dense (LevelBalanced; rounds 1-2 all): 0 1 2 3 1 2 3 2 3 1 2 3 2 3 2 3   (1 / 3 / 6 / 6 tiles of level 0 / 1 / 2 / 3)
//   three (LevelFastest, LevelSuperFast since round 3): 0 1 1 2 1 2 2 2 1 2 2 2 1 2 2 2   (1 / 5 / 10: THREE levels)
// dense is 7 % smaller than fast on text (CPU model: 0.3379 -> 0.3097).  three gives up 1.5 % (enwik-like) / 2.7 % (text) / 0.8 % (JSON)
// of dense's size for a decode round less and a far-table level set less: exec pass 0.525 -> 0.473 ms, far build 0.082 -> 0.052,
// match kernel 0.704 -> 0.688 ms per 100 MB (encode + decode 57.2 -> 61.1 GB/s); the other three-level patterns tried are within
// 0.5 % of it either way (DESIGN.md section 3).  The decoder recognises all three (mlz_decode.hip.inc, D3) and falls back to the
// position-order path for anything else.
constexpr uint32_t kPatternFast = 0xE4E4E4E4u;
#ifndef MLZ_PATTERN_DENSE
#define MLZ_PATTERN_DENSE 0xEEE7B9E4u
#endif
constexpr uint32_t kPatternDense = MLZ_PATTERN_DENSE;
#ifndef MLZ_PATTERN_THREE
#define MLZ_PATTERN_THREE 0xA9A9A994u
#endif
constexpr uint32_t kPatternThree = MLZ_PATTERN_THREE;
// No levels at all (round 4, LevelBalanced on request — option MLZ_OPT_L2_FREE): every tile may read every earlier tile of its window, one far
// table of ALL sampled positions per epoch.  That is what the level constraint costs LevelBalanced — 8-9 % of its output (CPU model, DESIGN.md
// section 3: 1.08-1.09 x the oracle's L2 with the dense pattern, 0.99 / 0.93 / 1.05 x without) — but the decoder then has no level schedule for
// the block: it is a GENERAL block like one of the reference's encoders (mlz_decode_general.hip.inc).
constexpr uint32_t kPatternFree = 0u;
__host__ __device__ __forceinline__ int tile_level_p(uint32_t tile_in_block, uint32_t pattern) { return int((pattern >> (2 * (tile_in_block & 15))) & 3); }
__host__ __device__ __forceinline__ int tile_level(uint32_t tile_in_block) { return tile_level_p(tile_in_block, kPatternFast); }
// the pattern the encoder writes at a compression level
__host__ __device__ __forceinline__ uint32_t level_pattern_of(int level) { return level >= 2 ? kPatternDense : kPatternThree; }

// far tables per (block, epoch): one per level set that somebody probes; without levels ONE
__host__ __device__ __forceinline__ uint32_t far_sets(uint32_t pattern) { return pattern == kPatternFree ? 1u : uint32_t(kLevels - 1); }

// common prefix of a[0..max) and b[0..max), 8 bytes at a time; both readable for max bytes.
__device__ __forceinline__ uint32_t match_len(const uint8_t* a, const uint8_t* b, uint32_t max) {
    uint32_t n = 0;
    while (n + 8 <= max) {
        uint64_t d = ld64u(a + n) ^ ld64u(b + n);
        if (d) return n + (ctz64(d) >> 3);
        n += 8;
    }
    while (n < max && a[n] == b[n]) n++;
    return n;
}

// ---- far tables: first occurrence per (level-set, epoch) of every kFarStride-th 8-byte window ----
// table[(lv * n_epochs + epoch) << kFarBits | hash8] = min position q (block-relative) over the
// sampled positions of that epoch whose tile level is <= lv.  "min" makes the result independent
// of scheduling.  Each workgroup owns a 32 Ki-bucket slice of one table in LDS (128 KiB), scans the
// epoch's sampled windows (16-byte coalesced reads; the slices of an epoch share an L2, "Placement" below), keeps
// the minima with LDS atomics and writes its slice out once — no global atomics, no memset.
constexpr int kFarSliceBits = 15;
// LevelBalanced's tables of 2^18 entries (blocks of kBigBlock and more) carry the top FOUR of the nine tag bits: the words far_bin_kernel sorts have
// room for four (14 bits of window index + 14 of bucket + 4), and the tag only decides which candidates are FETCHED — a foreign window that passes
// is rejected by the byte compare, so the output does not depend on the tag's width (1 false fetch in 16 foreign probes instead of 1 in 512).
constexpr int kL2FarBitsBig = 18;
__host__ __device__ constexpr uint32_t far_tag_mask(int FB) { return FB == kL2FarBitsBig ? 0x1E0u : kFarTagMask; }
// A workgroup builds its slice for the level sets in turn, lowest first: it scans only the epoch's tiles of
// level == lset and keeps accumulating minima in the same LDS slice, so level set L (levels <= L) is complete
// after pass L and is written out then — each sampled window is hashed once per slice instead of once per
// (slice, level set that contains it), and there is no merge with the previous set's table.
// FB: table entries per (epoch, level set), log2; ST: every ST-th 8-byte window is entered (LevelFastest 17 / 4, LevelBalanced 18 / 2).
// FB = 0: the blocks below kBigBlock of a batch, each with small_far_bits(its length) — tables are tab_log apart then
// (FB otherwise).  cls as in the match kernel: 0 = blocks below kBigBlock only, 1 = the others only, 2 = all.
//
// Placement.  The S = 2^slice_log slice workgroups of one (block, epoch) read the same sampled tiles, so they belong behind ONE L2.  Workgroups
// are dispatched in linear order and workgroup L runs on XCD L % 8 (observed, not promised: the match kernel's tile map leans on the same
// observation), and on a (slice, epoch, block) grid the four slices of an epoch sat on four XCDs: every source byte crossed the fabric four
// times.  The grid is one-dimensional instead and far_place() reads it as
//     x = L & 7, r = L >> 3, slice = r % S, j = r / S, group q = 8 j + x          (q = block * grid_epochs + epoch, n_groups of them)
// so the slices of a group are 8 apart in L — one XCD, neighbouring dispatch slots, the second to the S-th reader of a tile hit in L2 — and
// eight groups at a time take the eight XCDs.  The grid is 8 S ceil(n_groups / 8) workgroups; those with q >= n_groups leave at once.  A
// placement for speed only: no workgroup waits for another, every workgroup writes its own slice whatever XCD it lands on.  grid_epochs is
// the launch's count of epochs per block (1 for the class below kBigBlock, whose blocks have one), epochs_per_block the tables' layout.
constexpr uint64_t kBigBlock = 1u << 20;
struct FarPlace { uint32_t slice, group; };
__host__ __device__ __forceinline__ FarPlace far_place(uint32_t wg, uint32_t slice_log) {
    const uint32_t r = wg >> 3;
    return {r & ((1u << slice_log) - 1), ((r >> slice_log) << 3) | (wg & 7)};
}
__host__ __device__ __forceinline__ uint32_t far_grid(uint32_t n_groups, uint32_t slice_log) { return ((n_groups + 7) / 8 * 8) << slice_log; }
template <int FB, int ST>
__global__ __launch_bounds__(1024) void far_build_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                         uint32_t* __restrict__ far_tab, uint32_t epochs_per_block, uint32_t pattern,
                                                         uint32_t tab_log, uint32_t cls, uint32_t slice_log, uint32_t grid_epochs,
                                                         uint32_t n_groups) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* slot = reinterpret_cast<uint32_t*>(smem);
    const FarPlace at = far_place(blockIdx.x, slice_log);
    if (at.group >= n_groups) return;    // the padding of the last eight groups
    const uint32_t slice = at.slice;                 // which 32 Ki buckets
    const uint32_t blk = at.group / grid_epochs;     // block of the launch
    const uint32_t ep = at.group % grid_epochs;      // epoch
    const BlockInfo b = blocks[blk];
    if (cls != 2 && uint32_t(b.src_len >= kBigBlock) != cls) return;
    if (b.src_len > kMaxBlockSize) return;   // reported as too large by the layout pass; it has no tiles, nobody probes a table of it
    const int fb = FB ? FB : small_far_bits(b.src_len) + (ST == 2 ? 1 : 0);
    const uint32_t tlog = FB ? uint32_t(FB) : tab_log;
    const int sbits = fb < kFarSliceBits ? fb : kFarSliceBits;   // buckets of this workgroup's slice, log2
    if (slice >= (1u << (fb - sbits))) return;
    const uint8_t* s = src_base + b.src_off;
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < (1u << sbits) / 4; i += 1024) reinterpret_cast<uint4*>(slot)[i] = uint4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    __syncthreads();
    const uint64_t e0 = uint64_t(ep) << kEpochLog;
    const uint64_t e1 = e0 + (1ull << kEpochLog) < b.src_len ? e0 + (1ull << kEpochLog) : b.src_len;
    // Every thread takes kPerTile of a tile's sampled windows; two tiles of the level are in flight at a time (all their
    // loads are issued before the first hash), so the scan costs a memory round trip per 16 windows instead of one per tile.
    // (Four tiles in flight, measured with the 16-byte loads below: 36.8 us against 35.5.)
    constexpr uint32_t kPerTile = kTile / ST / 1024;   // windows of one tile per thread (8 or 16)
    constexpr int kFbTiles = ST >= 4 ? 2 : 1;          // tiles in flight at a time: 16 windows either way
    constexpr uint32_t kBatch = kFbTiles * kPerTile;
    const uint32_t tiles_in_epoch = e1 > e0 && b.src_len >= 8 ? uint32_t((e1 - e0 + kTile - 1) >> kTileLog) : 0;  // short blocks of a mixed batch have no such epoch
    constexpr uint32_t kEpochTiles = 1u << (kEpochLog - kTileLog);
    static_assert(kEpochTiles % 64 == 0, "an epoch is a whole number of 64-tile groups (4 periods of the level pattern each)");
    // level sets somebody probes: those below the highest level among the block's tiles (a 64 KiB block — tiles of level
    // 0 and 1 — needs the first only)
    uint32_t need = 0;
    const bool free_levels = pattern == kPatternFree;   // one set of all tiles
    {
        const uint64_t nt = (b.src_len + kTile - 1) >> kTileLog;
        for (uint32_t k = 1; k < 16 && k < nt; k++) need = need > uint32_t(tile_level_p(k, pattern)) ? need : uint32_t(tile_level_p(k, pattern));
        if (free_levels) need = nt > 1 ? 1 : 0;
    }
    for (uint32_t lset = 0; lset < need; lset++) {
      for (uint32_t g64 = 0; g64 < kEpochTiles; g64 += 64) {
        const uint32_t left = tiles_in_epoch > g64 ? tiles_in_epoch - g64 : 0;
        const uint64_t in_epoch = left >= 64 ? ~0ull : ((1ull << left) - 1);
        uint64_t todo = 0;  // the group's tiles of this level
        for (uint32_t k = 0; k < 16; k++)
            if (free_levels || uint32_t(tile_level_p(k, pattern)) == lset) todo |= 0x0001000100010001ull << k;
        todo &= in_epoch;
        while (todo) {
            uint32_t kk[kFbTiles];
#pragma unroll
            for (int t = 0; t < kFbTiles; t++) { kk[t] = todo ? g64 + uint32_t(ctz64(todo)) : tiles_in_epoch; todo &= todo - 1; }
            // Whole tiles: when every tile of the batch lies inside the block with 8 bytes to spare — all but a block's last tile — every
            // lane has its windows, the same answer for the whole workgroup, decided here once (as the match kernel's deep_tile).
            bool whole = true;
#pragma unroll
            for (int t = 0; t < kFbTiles; t++) whole = whole && kk[t] < tiles_in_epoch && e0 + (uint64_t(kk[t] + 1) << kTileLog) + 8 <= b.src_len;
            if (whole) {
                // A thread takes the 16 / ST windows that START in one 16-byte group: one 16-byte load per group and the 4 (ST = 2: 8)
                // bytes behind it that its last windows reach into — 20 bytes and two load instructions per four windows where an 8-byte
                // load per window at a stride of ST bytes took 32 and four.  The kernel was bound by its CU's load path, not by the
                // fabric or the hashing: the workgroup placement above cut the fabric fetch fourfold for 1 us, the 32-bit positions and
                // the missing predicate of this path took 40 % of the vector instructions for 1 us, these loads took 15 us of 50
                // (profiles/far_build_placement_time.txt).  Which thread enters a window does not matter to the minimum.  Positions are
                // 32-bit: a block has at most kMaxBlockSize bytes.  No merge of in-flight registers with the edge path: each path has
                // its own loads AND its own hashes, behind a branch that is uniform for the workgroup.
                constexpr uint32_t kWin = 16 / ST;               // windows of a group
                constexpr uint32_t kGroups = kPerTile / kWin;    // groups of a tile per thread
                constexpr uint32_t kG = kFbTiles * kGroups;      // groups in flight
                constexpr uint32_t kX = ST == 4 ? 1 : 2;         // dwords behind the group
                static_assert(ST == 2 || ST == 4, "windows start on even bytes of a group");
                static_assert((kWin - 1) * ST + 8 <= 16 + 4 * kX && 4 * kX <= 8, "the last window ends inside the loaded bytes, those inside the tile's 8 spare bytes");
                uint32_t at[kG];
                uint32_t d[kG][4 + kX];
#pragma unroll
                for (uint32_t g = 0; g < kG; g++) at[g] = uint32_t(e0) + (kk[g / kGroups] << kTileLog) + ((g % kGroups) * 1024 + uint32_t(tid)) * 16;
#pragma unroll
                for (uint32_t g = 0; g < kG; g++) __builtin_memcpy(d[g], s + at[g], 16 + 4 * kX);
#pragma unroll
                for (uint32_t g = 0; g < kG; g++) {
#pragma unroll
                    for (uint32_t j = 0; j < kWin; j++) {
                        const uint32_t o = j * ST;   // the window's first byte in the group
                        const auto dword_at = [&](uint32_t i) {   // the loaded bytes [i, i + 4), i even
                            if constexpr (ST == 4) return d[g][i / 4];
                            else return i % 4 ? (d[g][i / 4] >> 16) | (d[g][i / 4 + 1] << 16) : d[g][i / 4];
                        };
                        const FarHash fh = far_hash(uint64_t(dword_at(o + 4)) << 32 | dword_at(o), fb, far_tag_mask(FB));
                        if ((fh.idx >> sbits) == slice) atomicMin(&slot[fh.idx & ((1u << sbits) - 1)], ((at[g] + o) << kFarTagBits) | fh.tag);
                    }
                }
            } else {
                // the block's last tile (and a batch's missing second tile): a window per load, a predicate per lane
                uint64_t w[kBatch];
                uint64_t qq[kBatch];
                bool ok[kBatch];
#pragma unroll
                for (uint32_t u = 0; u < kBatch; u++) {
                    const uint32_t k = kk[u / kPerTile];                // tile of this level
                    const uint64_t q = e0 + (uint64_t(k) << kTileLog) + (uint64_t(u % kPerTile) * 1024 + tid) * ST;
                    qq[u] = q;
                    ok[u] = k < tiles_in_epoch && q + 8 <= b.src_len && q < e1;
                    // unconditional (lanes without a window read the block's first bytes): a load under a divergent branch is
                    // followed by a wait for it, which turned these 16 loads into 16 round trips
                    w[u] = ld64u(s + (ok[u] ? q : 0));
                }
#pragma unroll
                for (uint32_t u = 0; u < kBatch; u++) {
                    const FarHash fh = far_hash(w[u], fb, far_tag_mask(FB));
                    if (ok[u] && (fh.idx >> sbits) == slice)
                        atomicMin(&slot[fh.idx & ((1u << sbits) - 1)], (uint32_t(qq[u]) << kFarTagBits) | fh.tag);
                }
            }
        }
      }
        __syncthreads();
        const size_t tab = ((size_t(blk) * far_sets(pattern) + lset) * epochs_per_block + ep) << tlog;
        uint32_t* out = far_tab + tab + (size_t(slice) << sbits);
        for (uint32_t i = tid; i < (1u << sbits) / 4; i += 1024) reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(slot)[i];
        __syncthreads();  // the copy-out is complete before the next pass lowers entries
    }
}

// ---- far table WITHOUT level sets (LevelBalanced, kPatternFree), blocks of kBigBlock and more: every sampled window hashed once per pass, read once ----
// far_build_kernel gives every 32 Ki-bucket slice of an epoch's table a workgroup that scans ALL of the epoch's sampled windows: with
// LevelBalanced's 2^18 entries and every second window that is 8 workgroups loading and hashing the same million windows each — 0.54 ms
// per 100 MB, 17 of the 75 ms of a 4 GiB encode (round 4).  Round 5 splits the work at the only place where it must meet, the slice:
//   far_bin_kernel     one workgroup per half tile (16 KiB): hashes its sampled windows and writes them out SORTED BY SLICE (a counting
//                      sort through LDS; a 4-byte word per window: window index in the tile << 14 | bucket inside the slice) plus the
//                      seventeen segment offsets of the tile;
//   far_slice_kernel   one workgroup per (epoch, slice): reads only ITS segment of each of the epoch's 128 half tiles (a sixteenth of the
//                      words), keeps the minimum entry per bucket in LDS (64 KiB) and writes the slice out.
// No global atomics, no memset, "min" keeps the result independent of scheduling, the table is bit for bit the one far_build_kernel makes.
// (Built first and measured, 12 x 8 MiB of the JSON stream: the table filled in place with atomicMin, every window hashed once, an LDS bit
// per bucket filtering what a workgroup has sent before — 0.11 ms for the scan, 0.55 ms with the atomics: 12.5 M device-scope atomics at
// ~28 G/s; looking at the entry before sending does not help — 0.58 ms, 0.95 with non-temporal loads.  Not kept.)
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v);   // (below)
// The slices of the two-kernel form are 2^14 buckets (64 KiB of LDS: two workgroups per CU), sixteen per table of 2^18; the unit of the sort
// is HALF a tile (8192 windows: 32 KiB of sorted words + 16 KiB of counters = three workgroups per CU — with whole tiles a CU held one
// workgroup and the pass was all load latency: 117 of its 204 us in pass 1).
constexpr int kBinSliceBits = 14;
template <int FB, int ST> struct FarBin {
    static_assert(FB == kL2FarBitsBig, "the sorted word: 4 tag bits << 28 | window << 14 | bucket");
    static constexpr uint32_t kPerUnit = kTile / 2 / ST;                 // sampled windows of half a tile
    static constexpr uint32_t kSlices = 1u << (FB - kBinSliceBits);      // 16
    static constexpr uint32_t kOffs = kSlices + 1;                       // segment offsets per unit
    static constexpr uint32_t kCounters = 4 * kSlices * 64;              // [slice][wave][lane]
    static constexpr uint32_t kLds = kPerUnit * 4 + kCounters * 4 + kOffs * 4 + 64;
};
// far_bin_kernel: a lane keeps PRIVATE counters, one per slice, in LDS (no ballots, no shared cursors): pass 1 hashes the wave's quarter of
// the unit's windows — 64 consecutive windows per round, coalesced, sixteen rounds requested at a time —, keeps the words in registers and
// counts; an exclusive scan over the 4096 counters in (slice, wave, lane) order turns them into cursors; pass 2 places every word with one
// returning LDS add.  The order inside a segment is (wave, lane, round): irrelevant to a minimum.
template <int FB, int ST>
__global__ __launch_bounds__(256) void far_bin_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                      const uint32_t* __restrict__ tile_block, uint32_t* __restrict__ bins,
                                                      uint32_t* __restrict__ binoff) {
    using C = FarBin<FB, ST>;
    constexpr uint32_t kPerUnit = C::kPerUnit, kPerWave = kPerUnit / 4, kRounds = kPerWave / 64, kS = C::kSlices;
    static_assert(kPerUnit <= (1u << 14) && kRounds <= 64 && kRounds % 16 == 0, "window index in 14 bits; a lane's words in registers");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* B = reinterpret_cast<uint32_t*>(smem);                       // the sorted words
    uint32_t* cnt = B + kPerUnit;                                          // [slice][wave][lane]
    uint32_t* segoff = cnt + C::kCounters;                                 // [kS + 1]
    uint32_t* wsum = segoff + C::kOffs;                                    // [4] scan carry between waves
    const uint32_t unit = blockIdx.x, gt = unit >> 1;
    const BlockInfo b = blocks[tile_block[gt]];
    if (b.src_len < kBigBlock) return;   // (the smaller blocks of a mixed batch: far_build_kernel<0, ST>, tables sized by the block)
    const uint32_t tib = gt - b.first_tile;
    const uint64_t base = (uint64_t(tib) << kTileLog) + (unit & 1) * (kTile / 2);
    const uint8_t* s = src_base + b.src_off;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = rdfirst(uint32_t(tid) >> 6);
    for (uint32_t i = tid; i < C::kCounters / 4; i += 256) reinterpret_cast<uint4*>(cnt)[i] = uint4{0, 0, 0, 0};
    __syncthreads();
    // pass 1: word = slice << 28 | window index << 14 | bucket inside the slice, the tag kept beside it; 0xffffffff = no window (the block ends before it does)
    uint32_t word[kRounds];
    uint8_t tag4[kRounds];
    uint32_t* mine = cnt + wv * 64 + lane;                                  // my counter of slice k: mine[k * 256]
#pragma unroll
    for (uint32_t r0 = 0; r0 < kRounds; r0 += 16) {
        uint64_t w[16];
        bool ok[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const uint64_t q = base + uint64_t(wv * kPerWave + (r0 + u) * 64 + lane) * ST;
            ok[u] = q + 8 <= b.src_len;
            w[u] = ld64u(s + (ok[u] ? q : 0));      // unconditional: a load under a branch is followed by a wait for it
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const FarHash fh = far_hash(w[u], FB, far_tag_mask(FB));
            const uint32_t j = wv * kPerWave + (r0 + u) * 64 + lane;
            word[r0 + u] = ok[u] ? (fh.idx >> kBinSliceBits) << 28 | j << kBinSliceBits | (fh.idx & ((1u << kBinSliceBits) - 1)) : 0xffffffffu;
            tag4[r0 + u] = uint8_t(fh.tag >> 5);
            if (ok[u]) atomicAdd(&mine[(fh.idx >> kBinSliceBits) * 256], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the counters in place: thread t takes 16 consecutive ones
    {
        uint32_t v[16], sum = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { v[i] = cnt[tid * 16 + i]; sum += v[i]; }
        const uint32_t incl = wave_incl_scan_u32(sum);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t carry = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) carry += k < wv ? wsum[k] : 0;
        uint32_t run = carry + incl - sum;
#pragma unroll
        for (int i = 0; i < 16; i++) { cnt[tid * 16 + i] = run; run += v[i]; }
        if (tid == 255) segoff[kS] = run;
        __syncthreads();
        if (tid < int(kS)) segoff[tid] = cnt[tid * 256];
    }
    // pass 2: every word to its place: tag << 28 | window << 14 | bucket
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++)
        if (word[r] != 0xffffffffu) B[atomicAdd(&mine[(word[r] >> 28) * 256], 1u)] = (word[r] & 0x0fffffffu) | uint32_t(tag4[r]) << 28;
    __syncthreads();
    const uint32_t total = segoff[kS];
    uint32_t* out = bins + size_t(unit) * kPerUnit;
    for (uint32_t i = tid * 4; i < total; i += 1024) reinterpret_cast<uint4*>(out + i)[0] = reinterpret_cast<const uint4*>(B + i)[0];   // (the tail runs into unused words of the unit's space)
    if (tid < int(C::kOffs)) binoff[size_t(unit) * C::kOffs + tid] = segoff[tid];
}

// far_slice_kernel: the minimum position per bucket of ONE slice of one epoch's table, from that slice's segments of the epoch's 128 half tiles.
template <int FB, int ST>
__global__ __launch_bounds__(1024) void far_slice_kernel(const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ bins,
                                                         const uint32_t* __restrict__ binoff, uint32_t* __restrict__ far_tab, uint32_t epochs_per_block) {
    using C = FarBin<FB, ST>;
    constexpr uint32_t kPerUnit = C::kPerUnit, kSlice = 1u << kBinSliceBits;
    constexpr uint32_t kEpochUnits = 2u << (kEpochLog - kTileLog);
    static_assert(kEpochUnits == 128, "128 half tiles per epoch: a thread pair per unit for the segment offsets");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* slot = reinterpret_cast<uint32_t*>(smem);
    uint32_t* so = slot + kSlice;                                         // [128][2]: my segment's offsets in each unit
    const uint32_t slice = blockIdx.x, ep = blockIdx.y;
    const BlockInfo b = blocks[blockIdx.z];
    // (a block above MaxBlockSize has no tiles — upload_blocks — and so no units in bins / binoff: the batch reports it as too large, nothing is built for it)
    if (b.src_len < kBigBlock || b.n_tiles == 0) return;
    const uint32_t units_len = uint32_t((b.src_len + kTile / 2 - 1) / (kTile / 2));
    const uint32_t units = units_len < 2 * b.n_tiles ? units_len : 2 * b.n_tiles;   // never beyond the block's own units
    const uint32_t u0 = ep * kEpochUnits, u1 = u0 + kEpochUnits < units ? u0 + kEpochUnits : units;
    if (u0 >= u1) return;                  // (an epoch this block does not have: nobody probes its table)
    const uint32_t nu = u1 - u0;
    const size_t unit0 = size_t(b.first_tile) * 2 + u0;
    const int tid = threadIdx.x;
    if (tid < 256) {
        const uint32_t u = uint32_t(tid) >> 1;
        so[tid] = u < nu ? binoff[(unit0 + u) * C::kOffs + slice + (tid & 1)] : 0u;
    }
    for (uint32_t i = tid; i < kSlice / 4; i += 1024) reinterpret_cast<uint4*>(slot)[i] = uint4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    __syncthreads();
    // The slice's words of all units as ONE run, dealt to the threads 1024 apart (segments are 512 words on average but pile up on repetitive
    // data: a thread per segment position left some threads with a dozen dependent loads): pre[u] = words before unit u; a word's unit by
    // binary search (7 LDS reads); sixteen words per thread are requested before the first one is used.
    uint32_t* pre = so + 256;                                             // [129]
    if (tid < 64) {
        const uint32_t a0 = so[4 * tid + 1] - so[4 * tid], a1 = so[4 * tid + 3] - so[4 * tid + 2];
        const uint32_t incl = wave_incl_scan_u32(a0 + a1);
        pre[2 * tid] = incl - a0 - a1; pre[2 * tid + 1] = incl - a1;
        if (tid == 63) pre[128] = incl;
    }
    __syncthreads();
    const uint32_t total = pre[128];
    for (uint32_t e0 = 0; e0 < total; e0 += 16 * 1024) {
        uint32_t w[16], ub[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t e = e0 + 1024 * k + uint32_t(tid);
            const uint32_t ee = e < total ? e : total - 1;
            uint32_t u = 0;
#pragma unroll
            for (uint32_t step = 64; step; step >>= 1) u += pre[u + step] <= ee ? step : 0;     // the last unit whose words start at or before ee
            ub[k] = e < total ? (u0 + u) * (kTile / 2) : 0xffffffffu;
            w[k] = bins[(unit0 + u) * kPerUnit + so[2 * u] + (ee - pre[u])];
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            // LDS value = position << 9 | tag (the table's entry): the minimum is the lowest position
            if (ub[k] != 0xffffffffu)
                atomicMin(&slot[w[k] & (kSlice - 1)], (ub[k] + ((w[k] >> kBinSliceBits) & (kSlice - 1)) * ST) << kFarTagBits | (w[k] >> 28) << 5);
    }
    __syncthreads();
    uint32_t* tab = far_tab + ((size_t(blockIdx.z) * far_sets(kPatternFree) * epochs_per_block + ep) << FB) + (size_t(slice) << kBinSliceBits);
    for (uint32_t i = tid; i < kSlice / 4; i += 1024) reinterpret_cast<uint4*>(tab)[i] = reinterpret_cast<const uint4*>(slot)[i];
}

// ---- LDS helpers: the tile's source bytes live in LDS as dwords ----
// 8 bytes at byte offset p (any alignment): three aligned dword reads + two funnel shifts.
// Adjacent lanes share dwords (broadcast), so a wave reading 64 consecutive positions is
// conflict-free.
__device__ __forceinline__ uint64_t lds_ld64(const uint32_t* w, uint32_t p) {
    const uint32_t i = p >> 2, sh = p & 3;
    const uint32_t a = w[i], b = w[i + 1], c = w[i + 2];
    const uint32_t lo = __builtin_amdgcn_alignbyte(b, a, sh);
    const uint32_t hi = __builtin_amdgcn_alignbyte(c, b, sh);
    return lo | (uint64_t(hi) << 32);
}
__device__ __forceinline__ uint8_t lds_ld8(const uint32_t* w, uint32_t p) { return reinterpret_cast<const uint8_t*>(w)[p]; }

// Tile bytes: either staged in LDS (STAGED) or read in place from global memory through L1/L2.
// STAGED costs 32 KiB of LDS per wave (3 waves/CU); in-place costs none (8 waves/CU) but every
// access is a vector-memory round trip.
template <bool STAGED>
struct TileBytes {
    const uint32_t* w;  // LDS copy (STAGED)
    const uint8_t* g;   // global pointer to the tile's first byte
    __device__ __forceinline__ uint64_t ld64(uint32_t p) const { return STAGED ? lds_ld64(w, p) : ld64u(g + p); }
    __device__ __forceinline__ uint8_t ld8(uint32_t p) const { return STAGED ? lds_ld8(w, p) : g[p]; }
};

// common prefix (up to max) of tile bytes at a and either tile bytes at b (GLOBAL_B = false) or
// global bytes gb (GLOBAL_B = true)
template <bool GLOBAL_B, class TB>
__device__ __forceinline__ uint32_t match_len_lds(const TB& w, uint32_t a, uint32_t b, const uint8_t* gb, uint32_t max) {
    uint32_t n = 0;
    while (n + 8 <= max) {
        const uint64_t x = w.ld64(a + n);
        const uint64_t y = GLOBAL_B ? ld64u(gb + n) : w.ld64(b + n);
        const uint64_t d = x ^ y;
        if (d) return n + (ctz64(d) >> 3);
        n += 8;
    }
    while (n < max && w.ld8(a + n) == (GLOBAL_B ? gb[n] : w.ld8(b + n))) n++;
    return n;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add_u32(uint32_t v) {
    return v + uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROW_MASK, 0xf, false));
}
// inclusive wave64 prefix sum: DPP row shifts + row broadcasts (VALU speed, no LDS crossbar)
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
    v = dpp_add_u32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add_u32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add_u32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add_u32<0x118, 0xf>(v);  // row_shr:8
    v = dpp_add_u32<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
    v = dpp_add_u32<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
    return v;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v) {
    const uint32_t o = uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROW_MASK, 0xf, false));
    return v > o ? v : o;
}
// inclusive wave64 prefix maximum (same DPP pattern as the prefix sum)
__device__ __forceinline__ uint32_t wave_incl_max_u32(uint32_t v) {
    v = dpp_max_u32<0x111, 0xf>(v);
    v = dpp_max_u32<0x112, 0xf>(v);
    v = dpp_max_u32<0x114, 0xf>(v);
    v = dpp_max_u32<0x118, 0xf>(v);
    v = dpp_max_u32<0x142, 0xa>(v);
    v = dpp_max_u32<0x143, 0xc>(v);
    return v;
}

// RING bytes of LDS staging, written out FLUSH bytes at a time (16 B per lane, FLUSH/16 lanes)
template <uint32_t RING, uint32_t FLUSH>
struct TokenSinkT {
    uint8_t* ring;   // LDS
    uint8_t* out;    // global scratch for this tile (16-byte aligned)
    uint32_t o;      // bytes produced
    uint32_t flushed;  // bytes already written to global (multiple of FLUSH)
    int lane;
    __device__ __forceinline__ void flush_ready() {
        while (o - flushed >= FLUSH) {
            if (FLUSH == 1024 || uint32_t(lane) < FLUSH / 16) {
                const uint4 x = *reinterpret_cast<const uint4*>(ring + (flushed & (RING - 1)) + lane * 16);
                *reinterpret_cast<uint4*>(out + flushed + lane * 16) = x;
            }
            flushed += FLUSH;
        }
    }
    __device__ __forceinline__ void put_hdr(Hdr h) {
        if (uint32_t(lane) < h.n) ring[(o + lane) & (RING - 1)] = uint8_t(h.bits >> (8 * lane));
        o += h.n;
    }
    // literal bytes [from .. from+n) of the tile
    template <class TB>
    __device__ __forceinline__ void put_lits(const TB& w, uint32_t from, uint32_t n) {
        while (n) {
            const uint32_t room = RING - (o - flushed) - 64;
            const uint32_t piece = n < room ? n : room;
            for (uint32_t q = lane; q < piece; q += 64) ring[(o + q) & (RING - 1)] = w.ld8(from + q);
            o += piece; from += piece; n -= piece;
            flush_ready();
        }
    }
    __device__ __forceinline__ void finish() {  // whole 16-byte units; the scratch stride leaves room
        for (uint32_t f = flushed + lane * 16; f < o; f += 1024) {
            const uint4 x = *reinterpret_cast<const uint4*>(ring + (f & (RING - 1)));
            *reinterpret_cast<uint4*>(out + f) = x;
        }
    }
};

// ---- per-block layout: prefix sums of tile sizes, stored-block decision, header ----
// One wave per block.  Writes tile_out[] (offset of each tile's tokens in the block's dst),
// the block header, and out_len; flags[bi] = 1 when the block is stored uncompressed.
__global__ __launch_bounds__(64) void encode_layout_kernel(const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ tile_size,
                                                           uint32_t* __restrict__ tile_out, uint8_t* __restrict__ dst_base,
                                                           int64_t* __restrict__ out_len, uint32_t* __restrict__ flags, int level,
                                                           int with_header, uint32_t sub_log) {
    const int lane = threadIdx.x;
    const uint32_t bi = blockIdx.x;
    const BlockInfo b = blocks[bi];
    uint8_t* dst = b.mirror ? reinterpret_cast<uint8_t*>(b.mirror) : dst_base + b.dst_off;
    const uint64_t n = b.src_len;
    if (n > kMaxBlockSize) { if (lane == 0) { out_len[bi] = -2; flags[bi] = 2; } return; }
    const uint64_t need = with_header ? (n == 0 ? 1 : n + 2) : n;
    if (b.dst_cap < need) { if (lane == 0) { out_len[bi] = -6; flags[bi] = 2; } return; }
    uint32_t hdr = 0;
    uint8_t hb[8];
    if (with_header) { hb[0] = 0; hdr = 1 + put_uvarint(hb + 1, n); }
    // exclusive scan of the unit sizes (units = the pieces of mlz_encode2.hip.inc, 2^sub_log per tile): every lane takes 16
    // consecutive units — sixteen independent loads, a local sum, one wave scan of the lane totals — 1024 units per round
    // (a round per load was sixteen dependent memory round trips for an 8 MiB block)
    uint32_t running = 0;
    const uint32_t n_units = b.n_tiles << sub_log;
    const size_t first = size_t(b.first_tile) << sub_log;
    for (uint32_t t0 = 0; t0 < n_units; t0 += 1024) {
        uint32_t sz[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t t = t0 + uint32_t(lane) * 16 + j;
            sz[j] = tile_size[first + (t < n_units ? t : 0)] & 0x7fffffffu;
            if (t >= n_units) sz[j] = 0;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) mine += sz[j];
        const uint32_t incl = wave_incl_scan_u32(mine);
        uint32_t at = hdr + running + incl - mine;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t t = t0 + uint32_t(lane) * 16 + j;
            if (t < n_units) tile_out[first + t] = at;
            at += sz[j];
        }
        running += rdlane(incl, 63);
    }
    const int64_t limit = int64_t(n) - int64_t(n >> 5) - 6;  // dstLimit, encode_l1.go:60
    const bool stored = level == 0 || n < kMinNonLiteralBlock || int64_t(running) > limit;
    if (lane == 0) {
        flags[bi] = stored ? 1 : 0;
        if (!with_header) {
            out_len[bi] = stored ? 0 : int64_t(running);  // encodeBlock contract: 0 = incompressible
        } else if (stored) {
            if (n == 0) { dst[0] = 0; out_len[bi] = 1; }      // encodeUncompressed, encode.go:223-228
            else { dst[0] = 0; dst[1] = 0; out_len[bi] = int64_t(n) + 2; }
        } else {
            for (uint32_t k = 0; k < hdr; k++) dst[k] = hb[k];
            out_len[bi] = int64_t(hdr) + running;
        }
    }
}

// ---- gather tile token streams (or raw bytes for stored blocks) into the final block ----
// One 256-thread workgroup per tile; 16-byte vector copies where alignment allows.
__device__ __forceinline__ void wg_copy(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint32_t n, int tid, int nthreads) {
    // head bytes until d is 16-byte aligned
    uint32_t head = uint32_t((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (head > n) head = n;
    if (uint32_t(tid) < head) d[tid] = s[tid];
    d += head; s += head; n -= head;
    uint32_t nv = n >> 4;
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const uint4* sv = reinterpret_cast<const uint4*>(s);
        uint4* dv = reinterpret_cast<uint4*>(d);
        for (uint32_t k = tid; k < nv; k += nthreads) dv[k] = sv[k];
    } else {
        uint4* dv = reinterpret_cast<uint4*>(d);
        for (uint32_t k = tid; k < nv; k += nthreads) {
            uint4 x;
            __builtin_memcpy(&x, s + 16 * size_t(k), 16);
            dv[k] = x;
        }
    }
    uint32_t done = nv << 4;
    if (uint32_t(tid) < n - done) d[done + tid] = s[done + tid];
}

// Exclusive prefix of v over the N lanes of the workgroup (Hillis-Steele in lds[N]; *total, when wanted: the sum); op is associative
template <uint32_t N, class T, class Op> __device__ __forceinline__ T wg_scan(T v, T* lds, uint32_t tid, Op op, T* total = nullptr) {
    __syncthreads();   // (lds may still be read from the scan before)
    lds[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < N; d <<= 1) {
        const T a = tid >= d ? lds[tid - d] : T{};
        __syncthreads();
        if (tid >= d) lds[tid] = op(a, lds[tid]);
        __syncthreads();
    }
    if (total) *total = lds[N - 1];
    return tid ? lds[tid - 1] : T{};
}

}  // namespace mlz
