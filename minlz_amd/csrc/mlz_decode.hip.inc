// mlz_decode.hip.inc — parallel MinLZ block decoder for gfx950 (included by mlz_hip.hip).
//
// Replaces minLZDecodeGo / decodeBlockAsm (decode.go:178-622, _generate/gen.go:3599-4507),
// which walk one token stream serially.  A MinLZ block carries no index, so intra-block
// parallelism has to be recovered from the bytes:
//
//   D0 header    one thread per block: isMinLZ header parse (decode.go:120-156); also initialises the workspace words.
//   D1 exits     the token stream is cut into 8 KiB segments (kSeg), 512 threads each, 16 byte offsets per thread; for EVERY
//                offset i the position next(i) "if a token started here" is computed, and exits are finished from the
//                right (thread, 64-byte region, wave's group of regions): kept are a region exit per stream byte (one byte:
//                the distance from the region's end) and the segment exits of a segment's first 256 offsets (followed through
//                the groups, a hop each).
//   D2 chain     one workgroup per block: the true entry offset of every segment by guess + pointer jumping over the
//                exit table (a serial walk only when six rounds of repair do not settle it).
//   D3 index     mlz_decode_index.hip.inc (round 4): per segment, from its true entry — the regions chained through D1's region
//                exits, token starts found by a lane per region, then a lane per token: the block's TOKEN LIST (stream position
//                of every token, per 64 tokens {output position, repeat offset}), per 32 KiB output tile the token covering its
//                first byte, the level conformance of every copy; dec_viol_kernel and the tile schedule (D3d) are here.
//   D4 exec      mlz_decode_exec.hip.inc: one 3-wave workgroup per 32 KiB output tile, a lane per TOKEN (64 consecutive
//                entries of the token list D3 made), literals and copies from earlier tiles unordered, copies inside
//                the tile in dependency passes, tile image in LDS flushed with 16-byte write-through stores; a tile
//                waits once for its lower-level source tiles (workgroup i takes the i-th tile of the level-ordered schedule: no deadlock).
//   general      mlz_decode_general.hip.inc: blocks without a level structure (other encoders', and this library's LevelBalanced):
//                tile-local terminal maps built in parallel, then a run-granular in-order settle per block.
//
// Output is bit-exact with the reference for valid input; invalid input is reported as corrupt
// exactly when the reference's decoder does (length/offset/stream-end checks).

namespace mlz {

#ifndef MLZ_SEG_LOG
#define MLZ_SEG_LOG 13
#endif
constexpr int kSegLog = MLZ_SEG_LOG;
constexpr uint32_t kSeg = 1u << kSegLog;  // bytes of token stream per segment
constexpr uint32_t kSegThreads = kSeg / 64;  // one thread per 64-byte region
constexpr uint32_t kNone = 0xffffffffu;

struct DecBlock {
    uint32_t body_off;  // start of the token stream inside the block's src
    uint32_t clen;      // token stream bytes
    uint32_t dlen;      // decoded bytes
    int32_t status;     // 0 ok, else MLZ_ERR_*
    uint32_t literals;  // 1 = stored block: body is copied verbatim
    uint32_t total_out; // filled by D3
    uint32_t general;   // set by D3 when the block fits neither level pattern (bit 0); bit 1: the block is
                        // decoded by the pointer-jumping pass (mlz_decode_general.hip.inc) instead of tile by tile
    uint32_t viol;      // D3: bit 0 = some copy breaks the fast level pattern, bit 1 = ... the dense one, bit 2 = ... the three-level one
    uint32_t ntok;      // D3: tokens in the stream (the exec pass deals them out 64 at a time)
};
__device__ __forceinline__ int lane_of(int tid) { return tid & 63; }
constexpr uint32_t kViolAll = 7;   // a block that breaks every pattern (bits 0-2) is a general block
// bits 3-5 (round 5): some copy reads the tile 1 / 2 / 3 in front of its own — the dependency distance of a general block (team_of)
constexpr uint32_t kViolNear1 = 8, kViolNear2 = 16, kViolNear3 = 32, kViolNearAll = 56;
__device__ __forceinline__ uint32_t team_of(uint32_t viol) { return (viol & kViolNear1) ? 1u : (viol & (kViolNear2 | kViolNear3)) ? 2u : 4u; }   // tiles of a block that never read each other: 1, 2 or 4
// The level pattern a block is scheduled with (meaningful when !general): the first one it conforms to — the three-level
// pattern first (a block without cross-tile copies, e.g. LevelSuperFast's, conforms to all and takes the shortest schedule).
__device__ __forceinline__ uint32_t block_pattern(const DecBlock& d) { return !(d.viol & 4) ? kPatternThree : !(d.viol & 2) ? kPatternDense : kPatternFast; }

struct TileStart {
    uint32_t cpos;  // token-stream offset of the token covering the tile's first byte
    uint32_t d;     // output position where that token starts
    uint32_t rep;   // repeat offset in force before that token
    uint32_t rank;  // its index in the block's token list
};

// (Tok / decode_tok: mlz_toktab.h)
static_assert(kTokMinCopy2Offset == kMinCopy2Offset && kTokMinCopy3Offset == kMinCopy3Offset, "mlz_toktab.h restates the format's constants");

// hdr + lit of decode_tok (how far the token stream advances past a token starting here), from the token's first four bytes:
// the exit pass evaluates this at every byte offset of the stream and is bound by VALU issue.
__device__ __forceinline__ uint32_t tok_advance(uint32_t lo) {
    const uint32_t tag = lo & 3;
    const uint32_t x = (lo >> 3) & 31;
    const uint32_t e0 = x > 28 ? x - 28 : 0;                                   // literal / repeat: 0..3 length bytes
    const uint32_t v0 = __builtin_amdgcn_ubfe(lo, 8, 8 * e0);                  // their value (width 0 -> 0)
    const uint32_t lit0 = (lo & 4) ? 0 : x + 1 + v0 - (e0 > 1 ? e0 - 1 : 0);   // e0 ? 30 + v0 : x + 1   (x = 28 + e0 then)
    const uint32_t a0 = 1 + e0 + lit0;
    const uint32_t a1 = 2 + (((lo >> 2) & 15) == 15 ? 1u : 0u);
    const uint32_t l2 = (lo >> 2) & 63;
    const uint32_t a2 = 3 + (l2 > 60 ? l2 - 60 : 0);
    const uint32_t lits = (lo >> 3) & 3, l3 = (lo >> 5) & 63;
    const uint32_t a3 = 4 + lits + ((lo & 4) && l3 > 60 ? l3 - 60 : 0);        // copy3: 4 + ext + lits; fused copy2: 3 + (lits + 1)
    return tag == 0 ? a0 : tag == 1 ? a1 : tag == 2 ? a2 : a3;
}

// The same from a 256-entry table indexed by the token's first byte (the exit pass keeps it in LDS: 1 KiB).  The first byte fixes the
// advance except for the length bytes of a long literal (their count is in the entry: bits 8..12 = 8 x count) and of a long copy3
// (possible when the next byte's low three bits are set; the entry's bits 16..17 hold the 1..3 bytes that then follow) — about 13
// instructions and one LDS read against 28 instructions, checked against tok_advance for all 2^32 inputs (tools/tok_advance_check.cpp).
__device__ __forceinline__ uint32_t tok_advance_entry(uint32_t b) {
    const uint32_t tag = b & 3;
    uint32_t adv, e8 = 0, c = 0;
    if (tag == 0) {
        const uint32_t x = b >> 3;
        const bool rep = (b & 4) != 0;
        if (x <= 28) adv = 1 + (rep ? 0 : x + 1);
        else { const uint32_t e0 = x - 28; adv = 1 + e0 + (rep ? 0 : 30); e8 = rep ? 0 : 8 * e0; }
    } else if (tag == 1) {
        adv = 2 + (((b >> 2) & 15) == 15 ? 1u : 0u);
    } else if (tag == 2) {
        const uint32_t l2 = b >> 2;
        adv = 3 + (l2 > 60 ? l2 - 60 : 0);
    } else {
        adv = 4 + ((b >> 3) & 3);
        if ((b & 4) && (b >> 5) >= 5) c = (b >> 5) - 4;
    }
    return adv | (e8 << 8) | (c << 16);
}
__device__ __forceinline__ uint32_t tok_advance_tab(uint32_t lo, const uint32_t* tab /* LDS, 256 entries */) {
    const uint32_t t = tab[lo & 0xff];
    uint32_t adv = t & 63;
    adv += __builtin_amdgcn_ubfe(lo, 8, __builtin_amdgcn_ubfe(t, 8, 5));
    adv += ((lo >> 8) & 7) == 7 ? __builtin_amdgcn_ubfe(t, 16, 2) : 0;
    return adv;
}

// 8 bytes at p[i..i+8) with bytes at or beyond `n` read as zero (never touches memory >= p+n).
__device__ __forceinline__ uint64_t ld64_clamped(const uint8_t* p, uint32_t i, uint32_t n) {
    if (n >= 8) {   // (uniform per block) ONE load at min(i, n - 8), shifted down: no per-lane branch, no byte loop in the callers' token walks
        const uint32_t a0 = i < n - 8 ? i : n - 8;
        const uint32_t sh = 8 * (i - a0);
        const uint64_t w = ld64u(p + a0);
        return sh < 64 ? w >> sh : 0;
    }
    uint64_t w = 0;
    for (uint32_t k = 0; k < 8 && i + k < n; k++) w |= uint64_t(p[i + k]) << (8 * k);
    return w;
}

// LDS index swizzles for "thread t sweeps its own 64 consecutive entries": one dword of padding per
// 64 entries makes the 64 lanes of a wave hit 32 distinct banks instead of one (PMC showed 90 % of
// the exit kernel's LDS cycles were bank conflicts without it).
__device__ __forceinline__ uint32_t pj(uint32_t i) { return i + (i >> 6); }        // u32 entries
__device__ __forceinline__ uint32_t pr(uint32_t i) { return i + 2 * (i >> 6); }    // u16 entries
__device__ __forceinline__ uint32_t pb(uint32_t i) { return i + 4 * (i >> 6); }    // bytes
constexpr uint32_t kSegBufBytes = kSeg + 16 + 4 * ((kSeg + 16) >> 6) + 16;
__device__ __forceinline__ uint64_t lds_bytes8(const uint8_t* buf, uint32_t p) {
    uint64_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) w |= uint64_t(buf[pb(p + k)]) << (8 * k);
    return w;
}

// Stage kSeg + 16 bytes of the token stream (zero beyond the stream's end) into the swizzled LDS image:
// 16 bytes per thread per step; a 16-byte piece never straddles a 64-byte group, so it lands contiguously.
template <uint32_t THREADS = kSegThreads>
__device__ __forceinline__ void load_segment(uint8_t* buf, const uint8_t* src, uint32_t avail, int tid) {
    // All of a thread's 16-byte pieces are requested before the first is stored (a load under a branch is waited
    // for at once: with 128 threads that was four round trips in a row); pieces that are not whole — the end of
    // the stream — are read again byte by byte afterwards.
    constexpr uint32_t kPieces = (kSeg + 16) / 16;
    constexpr uint32_t kPer = (kPieces + THREADS - 1) / THREADS;
    uint4 w[kPer];
    const bool any16 = avail >= 16;
#pragma unroll
    for (uint32_t q = 0; q < kPer; q++) {
        const uint32_t i = 16 * (q * THREADS + uint32_t(tid));
        const bool whole = i + 16 <= avail;
        w[q] = uint4{0, 0, 0, 0};
        if (any16) __builtin_memcpy(&w[q], src + (whole ? i : 0), 16);   // wave-uniform test; the address is always readable
        if (!whole) w[q] = uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (uint32_t q = 0; q < kPer; q++) {
        const uint32_t j = q * THREADS + uint32_t(tid);
        const uint32_t i = 16 * j;
        if (j >= kPieces) continue;
        if (i < avail && i + 16 > avail) {  // ragged piece
            uint8_t t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t k = 0; k < avail - i; k++) t[k] = src[i + k];
            __builtin_memcpy(&w[q], t, 16);
        }
        uint32_t* d = reinterpret_cast<uint32_t*>(buf + pb(i));
        d[0] = w[q].x; d[1] = w[q].y; d[2] = w[q].z; d[3] = w[q].w;
    }
}

// ---------------- D0: headers ----------------
__global__ void dec_header_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks, DecBlock* __restrict__ dec, int n,
                                  int raw_body, uint32_t* __restrict__ fill_ff, uint32_t n_ff, uint32_t* __restrict__ fill_zero, uint32_t n_zero) {
    // workspace initialisation: segment entries = "unknown" (all ones), done flags / ticket / general-block control = 0
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_ff; i += gridDim.x * blockDim.x) fill_ff[i] = 0xffffffffu;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_zero; i += gridDim.x * blockDim.x) fill_zero[i] = 0;
    int bi = blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= n) return;
    const BlockInfo b = blocks[bi];
    DecBlock d;
    d.body_off = 0; d.clen = 0; d.dlen = 0; d.status = 0; d.literals = 0; d.total_out = 0; d.general = 0; d.viol = 0; d.ntok = 0;
    // Every token produces at least one output byte per two stream bytes (a 1-byte literal: tag + byte), so a token
    // stream longer than 2 x dlen must run past dst — the reference walks it and returns "corrupt" (decode.go:615).
    // Deciding that here keeps clen inside the segment budget the workspace was sized for (upload_blocks) and inside
    // 32 bits whatever length the caller passes.
    if (raw_body) {  // minLZDecode(dst[:n], src): tokens only, decoded length = dst_cap
        d.clen = uint32_t(b.src_len); d.dlen = uint32_t(b.dst_cap);
        if (b.dst_cap > kMaxBlockSize) d.status = 2;
        else if (b.src_len > 2 * b.dst_cap + 8) { d.status = 1 | (10 << 8); d.clen = 0; }
    } else {
        uint64_t body, dlen; int lits;
        int e = parse_block_header(src_base + b.src_off, b.src_len, &body, &dlen, &lits);
        d.status = e;
        if (!e) {
            d.body_off = uint32_t(body); d.dlen = uint32_t(dlen); d.literals = uint32_t(lits);
            d.clen = uint32_t(b.src_len - body);
            if (dlen > b.dst_cap) d.status = 6;
            else if (!lits && b.src_len - body > 2 * dlen + 8) { d.status = 1 | (10 << 8); d.clen = 0; }
        }
    }
    // an empty token stream decodes to nothing (the index pass has no segment to say so: decode.go:615, d != len(dst))
    if (d.status == 0 && !d.literals && d.clen == 0 && d.dlen != 0) d.status = 1 | (2 << 8);
    dec[bi] = d;
}

constexpr uint32_t kExitLds = (kSeg + (kSeg >> 6)) * 4 + kSegBufBytes + 64 + 1024;   // + the token-advance table
constexpr uint32_t kExitKeep = 256;   // exits kept per segment (offsets 0 .. kExitKeep-1; one thread each at the end of dec_exit_kernel)
// ---------------- D1: exit tables ----------------
// LDS: buf[kSeg + 16] bytes, jmp[kSeg] u32.  256 threads, 64 positions each.
// kExitSplit x 128 threads per segment: the per-offset decode and the jumping rounds use all of them, the
// right-to-left sweep that produces the 64-byte region exits uses the first 128 (one region each).
#ifndef MLZ_EXIT_SPLIT
#define MLZ_EXIT_SPLIT 4
#endif
constexpr uint32_t kExitSplit = MLZ_EXIT_SPLIT;               // threads per 64-byte region in the parallel phases
constexpr uint32_t kExitThreads = kExitSplit * kSegThreads;
constexpr uint32_t kExitSpan = 64 / kExitSplit;               // offsets per thread there
__global__ __launch_bounds__(kExitThreads) void dec_exit_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                       const uint32_t* __restrict__ seg_block, const DecBlock* __restrict__ dec,
                                                       uint32_t* __restrict__ exit_tab, uint8_t* __restrict__ rexit_tab) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* jmp = reinterpret_cast<uint32_t*>(smem);
    uint8_t* buf = smem + (kSeg + (kSeg >> 6)) * 4;
    const uint32_t seg = blockIdx.x;
    const uint32_t bi = seg_block[seg];
    const BlockInfo b = blocks[bi];
    const DecBlock d = dec[bi];
    if (d.status != 0 || d.literals) return;
    const uint32_t s0 = (seg - b.first_seg) << kSegLog;
    if (s0 >= d.clen) return;
    const uint8_t* src = src_base + b.src_off + d.body_off;
    const uint32_t avail = d.clen - s0;  // bytes of stream from s0
    const int tid = threadIdx.x;
    uint32_t* adv_tab = reinterpret_cast<uint32_t*>(smem + (kSeg + (kSeg >> 6)) * 4 + kSegBufBytes + 64);
    if (tid < 256) adv_tab[tid] = tok_advance_entry(uint32_t(tid));
    load_segment<kExitThreads>(buf, src + s0, avail, tid);
    __syncthreads();
    const uint32_t h0 = uint32_t(tid) * kExitSpan;  // my offsets for the decode and the jumping rounds
    {
        // 12-byte window (3 dwords) sliding over my 64 positions, 4 positions per step; the dword for
        // the next step is requested before the current one is decoded.  Word 16+ lives in the next
        // region's row of the swizzled image (one pad dword further).
        // (word index w of the 64-byte row that holds h0; rows are 68 bytes apart in the swizzled image)
        const uint32_t* bw = reinterpret_cast<const uint32_t*>(buf + pb(h0 & ~63u));
        const uint32_t w0 = (h0 & 63) >> 2;
        auto word = [&](uint32_t k) { return bw[k + (k >= 16 ? 1 : 0)]; };
        uint32_t a = word(w0), b2 = word(w0 + 1);
        for (uint32_t g = 0; g < kExitSpan / 4; g++) {
            const uint32_t nb = word(w0 + g + 2);
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                const uint32_t i = h0 + 4 * g + e;
                const uint32_t lo = e == 0 ? a : __builtin_amdgcn_alignbyte(b2, a, e);   // the four bytes at offset i
                // Values < kSeg are interior pointers; anything else is final.  Bit 31 marks "the path
                // ended inside this segment": exactly at the end of the stream (the only legal way) or on
                // padding beyond it (reported as a position far past clen, i.e. corrupt).
                uint32_t nx = i == avail ? (0x80000000u | avail) : 0xC0000000u;
                if (i < avail) nx = i + tok_advance_tab(lo, adv_tab);   // (< 2^25: no clamp needed)
                jmp[pj(i)] = nx;
            }
            a = b2; b2 = nb;
        }
    }
    __syncthreads();
    // Region exits: after this every entry points beyond its 64-byte region (exact: the first position on the
    // path at or beyond the end of the region).  Right to left in two levels, like the segment exits below: every
    // thread finishes its own kExitSpan offsets (each step reads only entries it finished before), then the
    // kExitSplit threads of a region — neighbouring lanes of one wave, whose LDS operations are ordered — finish
    // the region's sub-ranges from the right.
    {
        const uint32_t sub_end = h0 + kExitSpan;
        for (int i = int(sub_end) - 1; i >= int(h0); i--) {
            const uint32_t v = jmp[pj(i)];
            if (v < sub_end) jmp[pj(i)] = jmp[pj(v)];
        }
        if (kExitSplit > 1) {
            static_assert(64 % kExitSplit == 0 && kExitSpan % kExitSplit == 0, "a region's threads share a wave and split a sub-range evenly");
            const uint32_t rbase = h0 & ~63u, rend = rbase + 64;
            const uint32_t me = uint32_t(tid) % kExitSplit;              // my place among the region's threads
            for (int sub = int(kExitSplit) - 2; sub >= 0; sub--) {       // the last sub-range is finished already
                const uint32_t b0 = rbase + uint32_t(sub) * kExitSpan + me * (kExitSpan / kExitSplit);
                uint32_t v[kExitSpan / kExitSplit], u[kExitSpan / kExitSplit];
#pragma unroll
                for (uint32_t q = 0; q < kExitSpan / kExitSplit; q++) v[q] = jmp[pj(b0 + q)];
#pragma unroll
                for (uint32_t q = 0; q < kExitSpan / kExitSplit; q++) u[q] = v[q] < rend ? jmp[pj(v[q])] : v[q];
#pragma unroll
                for (uint32_t q = 0; q < kExitSpan / kExitSplit; q++) if (v[q] < rend) jmp[pj(b0 + q)] = u[q];
            }
        }
    }
    __syncthreads();
    const uint32_t r0 = uint32_t(tid) * 64;
    if (tid < int(kSegThreads)) {
    // These "region exits" are what the index pass (D3) chains through once the true entry of the segment is known.  Kept
    // as ONE BYTE per stream byte: the distance of the exit from the end of the region, 255 = further than 254 bytes (a long
    // literal) or the path ends — whoever needs that exit decodes the token at the offset itself (round 2 kept 16-bit
    // positions: twice the traffic here and a conversion of 64 values per lane in D3).
    {
        uint8_t* rx = rexit_tab + (size_t(seg) << kSegLog) + r0;
        const uint32_t rend = r0 + 64;
        for (uint32_t q = 0; q < 64; q += 16) {
            uint32_t w4[4];
#pragma unroll
            for (uint32_t e = 0; e < 16; e++) {
                const uint32_t v = jmp[pj(r0 + q + e)];            // (beyond the region, or a flag in the top bits: both far above rend)
                const uint32_t x = min(v - rend, 255u);
                if (e & 3) w4[e >> 2] |= x << (8 * (e & 3)); else w4[e >> 2] = x;
            }
            uint4 o; o.x = w4[0]; o.y = w4[1]; o.z = w4[2]; o.w = w4[3];
            *reinterpret_cast<uint4*>(rx + q) = o;
        }
    }
    }
    // Segment exits.  After the sweep every entry points beyond its own region, so the regions can be finished
    // from the right: an entry of region r that points into a later region takes that (already final) entry's
    // value.  Two levels keep it parallel: each wave finishes its own group of consecutive regions right to left
    // (one LDS round trip per region), then the groups are finished right to left by the whole workgroup.
    // (Plain pointer doubling over all 8192 entries took seven rounds and half of this kernel's time.)
    constexpr uint32_t kWaves = kExitThreads / 64;
    constexpr uint32_t kGroupRegions = (kSeg / 64) / kWaves;      // regions per wave
    constexpr uint32_t kGroup = kGroupRegions * 64;               // offsets per group
    static_assert(kGroupRegions * kWaves * 64 == kSeg, "whole regions per wave");
    const uint32_t lane = uint32_t(tid) & 63, wv = uint32_t(tid) >> 6;
    __syncthreads();
    {
        const uint32_t g0 = wv * kGroup, g1 = g0 + kGroup;
        for (int r = int(kGroupRegions) - 2; r >= 0; r--) {  // (the group's last region points beyond the group already)
            const uint32_t i = g0 + uint32_t(r) * 64 + lane;
            const uint32_t v = jmp[pj(i)];
            if (v < g1) jmp[pj(i)] = jmp[pj(v)];              // v lies in a later region of my group: final within the group
        }
    }
    __syncthreads();
    // Every entry now points beyond its GROUP.  Only the first kExitKeep offsets' exits are kept (a segment is entered where a token of the
    // previous one ends, i.e. a few bytes in — further in only behind a long literal run, and dec_chain_kernel then follows the region exits:
    // exit_slow), so they alone are followed to the segment's end: at most one hop per group (rounds 2-3 finished all 8192 entries group by
    // group, 7 barriers and 14 updates per thread, to keep 256 of them; keeping all 8192 was 4 bytes of workspace traffic per stream byte).
    static_assert(kExitKeep <= kExitThreads, "a thread per kept exit");
    if (tid < int(kExitKeep)) {
        uint32_t v = jmp[pj(uint32_t(tid))];
        while (v < kSeg) v = jmp[pj(v)];
        exit_tab[size_t(seg) * kExitKeep + tid] = s0 + (v & 0x7fffffffu);
    }
}

// exit of a parse that enters its segment at body offset pos, from the region exits (D1) — the slow way, for entries
// beyond the kExitKeep offsets whose exits are tabulated: at most kSeg / 64 dependent loads, then a few tokens
__device__ inline uint32_t exit_slow(const uint8_t* __restrict__ src, uint32_t clen, uint32_t pos, const uint8_t* __restrict__ rexit_blk) {
    const uint32_t s0 = pos & ~(kSeg - 1);
    const uint32_t avail = clen - s0;
    const uint8_t* rx = rexit_blk + s0;
    uint64_t p = pos - s0;
    while (p < kSeg) {                       // same verdicts as the exit table: see next(i) in dec_exit_kernel
        if (p == avail) return clen;         // ended exactly at the end of the stream
        if (p > avail) return s0 + 0x40000000u;   // on the padding behind it: corrupt
        const uint64_t rend = ((p >> 6) + 1) * 64;
        const uint32_t dlt = rx[p];
        if (dlt != 255) { p = rend + dlt; continue; }
        // the exit lies further out or the path ends in this region: token by token until the region is left
        while (p < rend) {
            if (p == avail) return clen;
            if (p > avail) return s0 + 0x40000000u;
            const Tok t = decode_tok(ld64_clamped(src, s0 + uint32_t(p), clen));
            p += uint64_t(t.hdr) + t.lit;
        }
    }
    return p > 0x7fffffffull ? 0x7fffffffu : s0 + uint32_t(p);
}

// ---------------- D2: chain ----------------
// The entry offset of every segment: pos_0 = 0, pos_{i+1} = exit(pos_i).  Followed through exit_tab alone
// this is one dependent HBM/L2 load per segment (≈ 350 per 8 MiB block, 0.13 ms).  Token streams
// re-synchronise within a few tokens whatever offset a parse starts from, so the exit of a segment
// entered at its first byte is almost always its true exit as well: two parallel gathers — exit(first
// byte of k) for every k, then exit(that guess for k) — give a (guess, exit) pair per segment.  If along
// the list 0 -> segment of exit(0) -> ... every exit equals the guess of the segment it lands in, the
// guesses ARE the chain (induction from the true entry 0); the list is marked by pointer jumping in LDS
// (log2 rounds).  Any mismatch on the list falls back to the serial walk.  One workgroup per block.
constexpr uint32_t kChainThreads = 256;
constexpr uint32_t kChainMaxSegs = kMaxBlockSize >> kSegLog;
constexpr uint32_t kChainPer = (kChainMaxSegs + kChainThreads - 1) / kChainThreads;
__global__ __launch_bounds__(kChainThreads) void dec_chain_kernel(const BlockInfo* __restrict__ blocks, DecBlock* __restrict__ dec,
                                                                   const uint32_t* __restrict__ exit_tab, uint32_t* __restrict__ seg_entry, int n,
                                                                   const uint8_t* __restrict__ src_base, const uint8_t* __restrict__ rexit_tab) {
    __shared__ uint32_t guess[kChainMaxSegs + 1], gexit[kChainMaxSegs + 1];
    __shared__ uint16_t jump[kChainMaxSegs + 1];
    __shared__ uint8_t marked[kChainMaxSegs + 1];
    const int bi = blockIdx.x;
    const int tid = threadIdx.x;
    const BlockInfo b = blocks[bi];
    const DecBlock d = dec[bi];
    if (d.status != 0 || d.literals) return;
    const uint32_t* et_blk = exit_tab + size_t(b.first_seg) * kExitKeep;
    const uint8_t* src = src_base + b.src_off + d.body_off;
    const uint8_t* rexit_blk = rexit_tab + (size_t(b.first_seg) << kSegLog);
    auto et = [&](uint32_t pos) -> uint32_t {  // exit of a parse starting at body offset pos
        const uint32_t off = pos & (kSeg - 1);
        if (off < kExitKeep) return et_blk[size_t(pos >> kSegLog) * kExitKeep + off];
        return exit_slow(src, d.clen, pos, rexit_blk);
    };
    const uint32_t nseg = (d.clen + kSeg - 1) >> kSegLog;
    bool serial = nseg > kChainMaxSegs;
    if (!serial) {
        for (uint32_t k = tid; k < nseg; k += kChainThreads) gexit[k] = et_blk[size_t(k) * kExitKeep];
        __syncthreads();
        for (uint32_t k = tid; k < nseg; k += kChainThreads) {
            // guess for segment k: where a parse of segment k-1 that started at its first byte leaves it.  Such a parse reads
            // garbage until it falls in step with the real tokens, and a garbage "long literal" can carry it far into
            // segment k, beyond the tabulated offsets — then the parses from the next few bytes are tried instead.
            uint32_t g = k == 0 ? 0 : gexit[k - 1];
            if (k != 0 && ((g >> kSegLog) != k || g >= d.clen || (g & (kSeg - 1)) >= kExitKeep)) {
                for (uint32_t j = 1; j < 8; j++) {
                    const uint32_t e = et_blk[size_t(k - 1) * kExitKeep + j];
                    if ((e >> kSegLog) == k && e < d.clen && (e & (kSeg - 1)) < kExitKeep) { g = e; break; }
                }
            }
            if ((g >> kSegLog) != k || g >= d.clen) g = k << kSegLog;
            guess[k] = g;
        }
        __syncthreads();
        // A wrong guess on the list (typically the segment after a literal run longer than a segment) is
        // replaced by the exit that lands there and the list is rebuilt; every pass makes at least the
        // first wrong link right.  After kChainPasses the serial walk takes over.
        constexpr int kChainPasses = 6;
        serial = true;
        uint32_t ex[kChainPer], ex_of[kChainPer];   // exit of my segments' guesses, and the guess it was computed for
#pragma unroll
        for (uint32_t q = 0; q < kChainPer; q++) { ex[q] = 0; ex_of[q] = 0xffffffffu; }
        for (int pass = 0; pass < kChainPasses; pass++) {
            // table look-ups first, all in flight together (no branch around a load); the rare entries beyond the tabulated
            // offsets afterwards, and only when the guess has changed since the last pass
            bool slow[kChainPer];
            uint32_t fast[kChainPer];
#pragma unroll
            for (uint32_t q = 0; q < kChainPer; q++) {
                const uint32_t k = tid + q * kChainThreads;
                const uint32_t pos = k < nseg ? guess[k] : 0;
                const uint32_t off = pos & (kSeg - 1);
                slow[q] = k < nseg && off >= kExitKeep;
                fast[q] = et_blk[size_t(pos >> kSegLog) * kExitKeep + (off < kExitKeep ? off : 0)];
            }
#pragma unroll
            for (uint32_t q = 0; q < kChainPer; q++) {
                const uint32_t k = tid + q * kChainThreads;
                const uint32_t pos = k < nseg ? guess[k] : 0;
                if (k >= nseg) ex[q] = 0;
                else if (!slow[q]) ex[q] = fast[q];
                else if (ex_of[q] != pos) ex[q] = exit_slow(src, d.clen, pos, rexit_blk);
                ex_of[q] = pos;
            }
#pragma unroll
            for (uint32_t q = 0; q < kChainPer; q++) {
                const uint32_t k = tid + q * kChainThreads;
                if (k < nseg) {
                    const uint32_t e = ex[q];
                    gexit[k] = e;
                    jump[k] = uint16_t(e < d.clen ? e >> kSegLog : nseg);
                    marked[k] = k == 0;
                }
            }
            if (tid == 0) { jump[nseg] = uint16_t(nseg); marked[nseg] = 0; }
            __syncthreads();
            // The usual case needs no marking: every segment's exit lands in the NEXT segment, on that segment's guess — then
            // every segment is on the path and the guesses are the chain.
            {
                bool plain = true;
#pragma unroll
                for (uint32_t q = 0; q < kChainPer; q++) {
                    const uint32_t k = tid + q * kChainThreads;
                    if (k + 1 < nseg) plain = plain && jump[k] == k + 1 && guess[k + 1] == ex[q];
                    else if (k < nseg) plain = plain && jump[k] == nseg;
                }
                if (!__syncthreads_or(!plain)) {
#pragma unroll
                    for (uint32_t q = 0; q < kChainPer; q++) {
                        const uint32_t k = tid + q * kChainThreads;
                        if (k < nseg) marked[k] = 1;
                    }
                    __syncthreads();
                    serial = false;
                    break;
                }
            }
            // mark the list that starts at segment 0
            for (uint32_t span = 1; span < nseg; span <<= 1) {
                uint16_t j2[kChainPer];
#pragma unroll
                for (uint32_t q = 0; q < kChainPer; q++) {
                    const uint32_t k = tid + q * kChainThreads;
                    j2[q] = 0;
                    if (k < nseg) {
                        const uint32_t j = jump[k];
                        if (marked[k]) marked[j] = 1;
                        j2[q] = jump[j];
                    }
                }
                __syncthreads();
#pragma unroll
                for (uint32_t q = 0; q < kChainPer; q++) {
                    const uint32_t k = tid + q * kChainThreads;
                    if (k < nseg) jump[k] = j2[q];
                }
                __syncthreads();
            }
            bool on_bad = false;
#pragma unroll
            for (uint32_t q = 0; q < kChainPer; q++) {
                const uint32_t k = tid + q * kChainThreads;
                if (k < nseg && marked[k]) {
                    const uint32_t e = ex[q];
                    const uint32_t j = e < d.clen ? e >> kSegLog : nseg;
                    if (j < nseg && guess[j] != e) { on_bad = true; guess[j] = e; }  // one writer: the marked segments form a path
                }
            }
            if (!__syncthreads_or(on_bad)) { serial = false; break; }
        }
        if (!serial) {
            bool overrun = false;
#pragma unroll
            for (uint32_t q = 0; q < kChainPer; q++) {
                const uint32_t k = tid + q * kChainThreads;
                if (k < nseg && marked[k]) {
                    seg_entry[b.first_seg + k] = guess[k];
                    overrun = overrun || gexit[k] > d.clen;
                }
            }
            if (overrun) dec[bi].status = 1 | (1 << 8);  // a token runs past the end of the stream
            return;
        }
    }
    if (tid != 0) return;
    uint32_t pos = 0;
    while (pos < d.clen) {
        seg_entry[b.first_seg + (pos >> kSegLog)] = pos;
        pos = et(pos);
    }
    if (pos != d.clen) dec[bi].status = 1 | (1 << 8);
}

// ---------------- D3 / 3: verdicts ----------------
// The pattern verdicts and dependency-distance bits of a block = the or of its segments' verdict bytes (dec_index2_kernel), a thread per
// segment; runs of segments of one block inside a wavefront are combined first, so a block gets an atomic per 64 segments.  Whoever sets
// the last of the three pattern bits flags the block as general: it fits no level pattern.  (Round 5 tried this at the head of the
// one-workgroup schedule kernel, a launch less: 18.5 us against 4.9 + 9.1 — the fences between the atomics and the schedule's reads cost
// more than the launch.  Since the level-0 hand-over both run in ONE workgroup of dec_level0_kernel's launch, beside the level-0 candidates: a barrier
// between the two parts is enough there.  The kernels of their own serve the groups that do not take that launch.)
// (a device function: dec_viol_kernel runs it a thread per segment, the verdict workgroup of dec_level0_kernel in steps of its 1024 threads)
__device__ __forceinline__ void dec_viol_gather(const uint32_t* __restrict__ seg_block, const uint8_t* __restrict__ seg_viol, DecBlock* __restrict__ dec,
                                                uint32_t* __restrict__ n_general /* null: general blocks stay on the tile path */, uint32_t segs, uint32_t i /* my segment; whole wavefronts call */) {
    const int lane = threadIdx.x & 63;
    uint32_t v = 0, bi = 0xffffffffu;
    if (i < segs) {
        const uint32_t v4 = reinterpret_cast<const uint32_t*>(seg_viol)[i];
        v = (v4 | (v4 >> 8) | (v4 >> 16) | (v4 >> 24)) & (kViolAll | kViolNearAll);
        bi = seg_block[i];
    }
    const uint32_t prev = uint32_t(__builtin_amdgcn_update_dpp(-1, int(bi), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
    const bool head = lane == 0 || bi != prev;
    const uint64_t H = ballot64(head);
    const uint64_t m0 = ballot64(v & 1), m1 = ballot64(v & 2), m2 = ballot64(v & 4);
    const uint64_t m3 = ballot64(v & kViolNear1), m4 = ballot64(v & kViolNear2), m5 = ballot64(v & kViolNear3);
    if (head && bi != 0xffffffffu) {
        const uint64_t rest = lane == 63 ? 0ull : H & ~((2ull << lane) - 1);
        const uint64_t upto = rest ? (1ull << ctz64(rest)) - 1 : ~0ull;        // lanes before the next run's head
        const uint64_t run = upto & ~((1ull << lane) - 1);
        const uint32_t bits = ((m0 & run) ? 1u : 0u) | ((m1 & run) ? 2u : 0u) | ((m2 & run) ? 4u : 0u) |
                              ((m3 & run) ? kViolNear1 : 0u) | ((m4 & run) ? kViolNear2 : 0u) | ((m5 & run) ? kViolNear3 : 0u);
        if (bits) {
            const uint32_t old = atomicOr(&dec[bi].viol, bits) & kViolAll, lv3 = bits & kViolAll;
            if ((old | lv3) == kViolAll && old != kViolAll && atomicOr(&dec[bi].general, n_general ? 3u : 1u) == 0 && n_general) atomicAdd(n_general, 1u);
        }
    }
}
__global__ __launch_bounds__(256) void dec_viol_kernel(const uint32_t* __restrict__ seg_block, const uint8_t* __restrict__ seg_viol, DecBlock* __restrict__ dec,
                                                        uint32_t* __restrict__ n_general, uint32_t segs) {
    dec_viol_gather(seg_block, seg_viol, dec, n_general, segs, blockIdx.x * 256 + threadIdx.x);
}

// ---------------- D3d: schedule ----------------
// order[ticket] = global tile index.  Tiles of "general" blocks come first in position order
// (a tile may wait on any earlier tile of its block); then the tiles of level-conformant blocks,
// level 0 first: a tile only ever waits on tiles with a smaller ticket, so the exec pass cannot
// deadlock however few wavefronts are resident.  One 1024-thread workgroup, two passes.
__device__ __forceinline__ void dec_schedule_body(const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ tile_block,
                                                     DecBlock* __restrict__ dec, uint32_t* __restrict__ order, uint32_t total_tiles,
                                                     uint32_t n_blocks, uint32_t* __restrict__ gen_list /* null: no general pass */,
                                                     uint32_t* __restrict__ gen_ctl /* GenCtl: [0] blocks on the list, [2] their largest tile count */,
                                                     uint32_t n_settle /* role S workgroups of dec_general_kernel */,
                                                     uint32_t* __restrict__ call_acc /* per API call, over its internal groups: [0] general blocks, [1] largest team */,
                                                     uint32_t acc_reset /* first group of the call */) {
    // buckets: 0 = general blocks that stay on the tile path (position order matters: a tile there may wait for any earlier tile
    // of its block), 1 .. kLevels = levels of conformant blocks, kLevels + 1 = general blocks decoded by dec_general_kernel
    // (the exec pass returns at once for their tiles: last, any order)
    constexpr uint32_t kBuckets = kLevels + 2;
    __shared__ uint32_t cnt[kBuckets];
    __shared__ uint32_t base[kBuckets];
    const int tid = threadIdx.x;
    if (tid < int(kBuckets)) cnt[tid] = 0;
    __syncthreads();
    auto verdict_of = [&](uint32_t bi) -> DecBlock { return dec[bi]; };
    auto bucket_of = [&](uint32_t gt) -> uint32_t {
        const uint32_t bi = tile_block[gt];
        const DecBlock d = verdict_of(bi);
        if (d.general) return (d.general & 2) ? kBuckets - 1 : 0u;
        return 1u + uint32_t(tile_level_p(gt - blocks[bi].first_tile, block_pattern(d)));
    };
    // pass 1: bucket sizes (one LDS atomic per wavefront and bucket)
    for (uint32_t g0 = 0; g0 < total_tiles; g0 += 1024) {
        const uint32_t gt = g0 + tid;
        const uint32_t bk = gt < total_tiles ? bucket_of(gt) : 0xffffffffu;
        for (uint32_t b = 0; b < kBuckets; b++) {
            const uint64_t m = ballot64(bk == b);
            if (m && (tid & 63) == 0) atomicAdd(&cnt[b], uint32_t(__builtin_popcountll(m)));
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t b = 0; b < kBuckets; b++) { base[b] = run; run += cnt[b]; }
    }
    __syncthreads();
    // pass 2: placement.  Inside a level (and in the last bucket) the order is free — tiles of one level never wait for each
    // other —: a wavefront takes a run of slots with one atomic, its lanes keep their order.  Bucket 0 is placed by one thread
    // at the end; it is empty unless a foreign block stays on the tile path (a debug option).
    for (uint32_t g0 = 0; g0 < total_tiles; g0 += 1024) {
        const uint32_t gt = g0 + tid;
        const uint32_t bk = gt < total_tiles ? bucket_of(gt) : 0xffffffffu;
        for (uint32_t b = 1; b < kBuckets; b++) {
            const uint64_t m = ballot64(bk == b);
            if (!m) continue;
            uint32_t at = 0;
            if ((tid & 63) == 0) at = atomicAdd(&base[b], uint32_t(__builtin_popcountll(m)));
            at = rdfirst(at);
            if (bk == b) order[at + uint32_t(__builtin_popcountll(m & ((1ull << (tid & 63)) - 1)))] = gt;
        }
    }
    if (tid == 0 && cnt[0]) {
        uint32_t at = 0;
        for (uint32_t gt = 0; gt < total_tiles; gt++)
            if (bucket_of(gt) == 0) order[at++] = gt;
    }
    // The blocks dec_general_kernel decodes, in batch order, and the largest tile count among them (its role E deals tiles
    // position-major over this list; role S takes one block of it per workgroup).
    if (gen_list) {
        __shared__ uint32_t wcnt[16], gbase, gmax, gteam;
        if (tid == 0) { gbase = 0; gmax = 0; gteam = 4; }
        __syncthreads();
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024) {
            const uint32_t bi = b0 + tid;
            uint32_t nt = 0;
            bool is = false;
            if (bi < n_blocks) {
                const DecBlock d = verdict_of(bi);
                is = (d.general & 2) && d.status == 0 && !d.literals && d.dlen != 0;
                nt = (d.dlen + kTile - 1) >> kTileLog;
            }
            const uint64_t m = ballot64(is);
            if ((tid & 63) == 0) wcnt[tid >> 6] = uint32_t(__builtin_popcountll(m));
            __syncthreads();
            uint32_t at = gbase;
            for (int w = 0; w < (tid >> 6); w++) at += wcnt[w];
            if (is) { gen_list[at + uint32_t(__builtin_popcountll(m & ((1ull << (tid & 63)) - 1)))] = bi; atomicMax(&gmax, nt); atomicMin(&gteam, team_of(verdict_of(bi).viol)); }
            __syncthreads();
            if (tid == 0) { uint32_t s = 0; for (int w = 0; w < 16; w++) s += wcnt[w]; gbase += s; }
            __syncthreads();
        }
        // [5]: the batch's team size — tiles of a block that role S settles side by side: the smallest dependency distance among the batch's general blocks
        // — but no more than there are settling workgroups to go round: with many blocks one workgroup per block settles more tiles per
        // microsecond than teams do (a team's step takes 9 us, a single workgroup's 5.3: 512 blocks decoded at 156 instead of 180 GB/s)
        if (tid == 0) {
            const uint32_t per = gbase ? n_settle / gbase : 4u;
            const uint32_t team = gteam < (per >= 4 ? 4u : per >= 2 ? 2u : 1u) ? gteam : (per >= 4 ? 4u : per >= 2 ? 2u : 1u);
            gen_ctl[0] = gbase; gen_ctl[2] = gmax; gen_ctl[5] = team;
            // the call's totals (mlz_get_counter 2 / 6): the groups of a call run one after the other on one stream, so plain words do
            if (call_acc) {
                const uint32_t t = gbase ? team : 0u;
                if (acc_reset) { call_acc[0] = gbase; call_acc[1] = t; }
                else { call_acc[0] += gbase; call_acc[1] = call_acc[1] > t ? call_acc[1] : t; }
            }
        }
    } else if (tid == 0 && call_acc && acc_reset) { call_acc[0] = 0; call_acc[1] = 0; }
}
__global__ __launch_bounds__(1024) void dec_schedule_kernel(const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ tile_block, DecBlock* __restrict__ dec,
                                                           uint32_t* __restrict__ order, uint32_t total_tiles, uint32_t n_blocks, uint32_t* __restrict__ gen_list,
                                                           uint32_t* __restrict__ gen_ctl, uint32_t n_settle, uint32_t* __restrict__ call_acc, uint32_t acc_reset) {
    dec_schedule_body(blocks, tile_block, dec, order, total_tiles, n_blocks, gen_list, gen_ctl, n_settle, call_acc, acc_reset);
}

// ---------------- D4: exec ----------------
// (mlz_decode_exec.hip.inc; the wave scan it and the general pass use lives here)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROW_MASK, 0xf, false));
}
// inclusive wave64 prefix sum with DPP row shifts + row broadcasts (VALU speed, no LDS crossbar)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
    return v;
}

// ---------------- D5: results ----------------
__global__ void dec_finish_kernel(const DecBlock* __restrict__ dec, int64_t* __restrict__ out_len, int n, int debug) {
    int bi = blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= n) return;
    const DecBlock d = dec[bi];
    // status bits 8.. carry the failure site for debugging; callers see the plain error code
    out_len[bi] = d.status ? -int64_t(debug ? d.status : (d.status & 0xff)) : int64_t(d.dlen);
}

}  // namespace mlz
