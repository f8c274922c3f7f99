// mlz_decode_index.hip.inc — D3, the index pass of the parallel decoder: dec_index1_kernel (per segment) and dec_index2_kernel (per token)
// (round 4; dec_viol_kernel, in mlz_decode.hip.inc, gathers their verdict bytes per block; included by mlz_hip.hip after mlz_decode.hip.inc).
//
// Input: the true entry offset of every 8 KiB segment of the token stream (D2) and D1's region exits.  Output: what the exec pass
// (mlz_decode_exec.hip.inc) and the general-block pass work from — the block's TOKEN LIST (stream position of every token), per 64
// tokens {output position, repeat offset in force}, per 32 KiB output tile the token covering its first byte, the level conformance
// of every copy, the block's totals (decode.go:615: d != len(dst) is corrupt).
//
// The three-kernel form walked every 64-byte region's tokens TWICE with a lane per region, every step a dependent global load and a
// full token decode (selects over all four token kinds, ~65 instructions): once to count (a), once more (c) after a per-block scan
// (b) had told the segment where its output starts.  Here:
//   * the segment's bytes are staged in LDS and the decode is table-driven (mlz_toktab.h: one LDS word per first byte, ~10
//     instructions for the advance, ~12 for the output bytes);
//   * the chain of the segment's regions from its true entry — 128 dependent LDS reads of one thread — is walked by 15 lanes
//     from guessed starts that fall in step with the real tokens (see below);
//   * the lane-per-region walk finds the token starts (a 64-bit mask in registers) and sums output bytes / notes the last explicit
//     offset on the way; the starts are laid out in LDS in stream order;
//   * phase 1 ends with every segment writing its aggregate as one 64-bit word (bit 63 = written);
//   * phase 2 is a launch of its own, so every word is there when it starts: a workgroup adds up the words of ALL earlier segments
//     of its block (at most 2047, 128 x 4 at a time) instead of kernel b's scan — a look-back that never WAITS (the one-kernel form
//     with a spinning look-back was built and measured: 40 us of waiting per workgroup, DESIGN.md section 4 D3); a word without
//     bit 63 can only mean that phase 1 did not run for that segment: the block fails with status 7 | (12 << 8) = -MLZ_ERR_HIP;
//   * phase 2 then handles a TOKEN per lane — no divergence, no dependent loads —: output positions and repeat offsets by wave
//     scans, the lists, the tile starts, the level conformance of every copy (a verdict BYTE per quarter segment, gathered per
//     block by dec_viol_kernel: an atomic per wave on the block's word cost 80 us).
// Nothing in these kernels waits for another workgroup: liveness does not depend on dispatch order.
//
// Reference: decode.go:178-622 is a sequential loop that knows all of this implicitly.

namespace mlz {

constexpr uint32_t kIdxThreads = kSegThreads;                 // 128: a lane per 64-byte region in the walk
constexpr uint32_t kIdxStage = kSeg / 2;                      // 4096 token positions (16 bits each) per pass through the buffer
constexpr uint32_t kRex8Bytes = kSegThreads * 68;             // region exits: one byte per offset, rows of 64 + 4
constexpr uint32_t kIdxSegBytes = kSeg + 32;                  // the segment, 16 bytes behind it, padding
constexpr uint32_t kIdxBuf = kRex8Bytes > kIdxSegBytes ? kRex8Bytes : kIdxSegBytes;   // ONE buffer: the region exits, then the segment's bytes, then the token list
constexpr uint32_t kIdxLds = kIdxBuf + kSegThreads * 2 + 1024 + 256 + 512;   // ... + region entries, token table, scratch, the chain's group walks (phase 1)

#ifdef MLZ_IDX_PROF
__device__ unsigned long long g_idxprof[16];   // debug build only: per-phase time sums (10 ns units) over all workgroups (tools/idxprof.py)
#define IDXP(i) do { if (tid == 0) { const unsigned long long t_now = __builtin_amdgcn_s_memrealtime(); atomicAdd(&g_idxprof[i], t_now - idx_t); idx_t = t_now; } } while (0)
#else
#define IDXP(i) do { } while (0)
#endif

struct IdxAgg { uint32_t out, ntok, last; };                  // out saturates at 2^31 - 1 (corrupt streams can claim anything)
__device__ __forceinline__ uint32_t sat31(uint64_t v) { return v > 0x7fffffffull ? 0x7fffffffu : uint32_t(v); }
__device__ __forceinline__ IdxAgg idx_join(const IdxAgg& a, const IdxAgg& b) {   // a, then b
    IdxAgg r;
    r.out = sat31(uint64_t(a.out) + b.out); r.ntok = a.ntok + b.ntok; r.last = b.last ? b.last : a.last;
    return r;
}
// The look-back word of a segment: bit 63 = published, out (25 bits, saturating at 2^24: a block has at most 2^23 bytes, so a
// saturated segment makes the block's total wrong = corrupt, as it must) | ntok (14 bits: <= 8192) << 25 | last offset (22 bits) << 39.
constexpr uint32_t kIdxOutSat = 1u << 24;
__device__ __forceinline__ unsigned long long idx_word(const IdxAgg& a) {
    return (1ull << 63) | (unsigned long long)(a.out < kIdxOutSat ? a.out : kIdxOutSat) | ((unsigned long long)a.ntok << 25) | ((unsigned long long)a.last << 39);
}
__device__ __forceinline__ IdxAgg idx_unword(unsigned long long w) {
    IdxAgg a; a.out = uint32_t(w) & 0x1ffffffu; a.ntok = uint32_t(w >> 25) & 0x3fffu; a.last = uint32_t(w >> 39) & 0x3fffffu;
    return a;
}
#ifndef MLZ_IDX_GRP
#define MLZ_IDX_GRP 8
#endif
constexpr uint32_t kIdxGrp = MLZ_IDX_GRP, kIdxGroups = (kSeg / 64) / kIdxGrp;   // the region chain: 15 lanes, each walking two groups of 8 regions

__device__ const TokTable g_toktab = make_toktab();

// D3 / 1: token starts and aggregates of every segment
__global__ __launch_bounds__(kIdxThreads) void dec_index1_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                                  const uint32_t* __restrict__ seg_block, const DecBlock* __restrict__ dec,
                                                                  const uint32_t* __restrict__ seg_entry, const uint8_t* __restrict__ rexit_tab,
                                                                  unsigned long long* __restrict__ seg_state, unsigned long long* __restrict__ seg_part /* [3] per segment */,
                                                                  uint16_t* __restrict__ tok16) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // One 8.5 KiB buffer, three tenants in turn: D1's region exits (for the chain), then the segment's bytes (for the walk; they wait in
    // registers while the chain runs), then the token list on its way out.  (Both at once were 17 KiB: 8 workgroups per CU, and this
    // kernel waits for memory more than anything else.)
    uint32_t* segw = reinterpret_cast<uint32_t*>(smem);
    uint8_t* rex8 = smem;
    uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
    uint16_t* rentry = reinterpret_cast<uint16_t*>(smem + kIdxBuf);
    uint32_t* toktab = reinterpret_cast<uint32_t*>(smem + kIdxBuf + kSegThreads * 2);
    uint32_t* red = toktab + 256;                               // 64 words
    uint16_t* entg = reinterpret_cast<uint16_t*>(red + 64);     // [kIdxGroups][2 * kIdxGrp]: where group walk g enters the regions 8 g .. 8 g + 15
    const uint32_t seg = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = rdfirst(uint32_t(tid) >> 6);
    const uint32_t r0 = uint32_t(tid) * 64;
    // (what depends on the segment index alone is requested first: the descriptors below are two dependent round trips)
    uint4 xs[4];   // the segment's region exits, 16-byte piece q * 128 + tid (consecutive lanes read consecutive pieces: a thread reading its
    {              // own region's 64 bytes made every load instruction touch 32 lines for a quarter of each)
        const uint4* g = reinterpret_cast<const uint4*>(rexit_tab + (size_t(seg) << kSegLog));
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) xs[q] = g[q * kIdxThreads + uint32_t(tid)];
    }
    const uint32_t e = seg_entry[seg];
    const uint32_t bi = seg_block[seg];
    const BlockInfo b = blocks[bi];
    const DecBlock d = dec[bi];
    if (d.status != 0 || d.literals) return;
    const uint32_t s0 = (seg - b.first_seg) << kSegLog;
    if (s0 >= d.clen) return;
    const uint32_t avail = d.clen - s0;
    const uint8_t* srcb = src_base + b.src_off + d.body_off;
#ifdef MLZ_IDX_PROF
    unsigned long long idx_t = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) atomicAdd(&g_idxprof[15], 1ull);
#endif

    uint64_t mask = 0;      // token starts in my region
    uint32_t rank0 = 0;     // segment-relative rank of the first of them
    uint32_t ntok_seg = 0;
    IdxAgg* qagg = reinterpret_cast<IdxAgg*>(red + 8);   // [4]: what the regions of each quarter of the segment (32 regions, half a wave) add up to
    if (e != kNone) {   // (uniform: a segment no token starts in lies inside one long literal)
        for (uint32_t i = tid; i < 256; i += kIdxThreads) toktab[i] = g_toktab.e[i];
        // the segment's bytes (zero beyond the end of the stream) are requested now and stored after the chain; the region exits go to LDS
        constexpr uint32_t kPieces = (kSeg + 16) / 16, kPer = (kPieces + kIdxThreads - 1) / kIdxThreads;
        uint4 w[kPer];
        {
            const bool any16 = avail >= 16;
#pragma unroll
            for (uint32_t q = 0; q < kPer; q++) {
                const uint32_t i = 16 * (q * kIdxThreads + uint32_t(tid));
                const bool whole = i + 16 <= avail;
                w[q] = uint4{0, 0, 0, 0};
                if (any16) __builtin_memcpy(&w[q], srcb + s0 + (whole ? i : 0), 16);
                if (!whole) w[q] = uint4{0, 0, 0, 0};
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {   // piece j holds bytes 16 j .. 16 j + 15 = region j / 4, offset 16 (j % 4); rows of 64 + 4 bytes
                const uint32_t j = q * kIdxThreads + uint32_t(tid);
                uint32_t* row = reinterpret_cast<uint32_t*>(rex8 + (j >> 2) * 68 + (j & 3) * 16);
                row[0] = xs[q].x; row[1] = xs[q].y; row[2] = xs[q].z; row[3] = xs[q].w;
            }
            rentry[tid] = 0xffff;
            entg[tid] = 0xffff; entg[tid + kIdxThreads] = 0xffff;
        }
        __syncthreads();
        IDXP(0);
        auto lds4 = [&](uint32_t p) -> uint32_t { const uint32_t i = p >> 2; return __builtin_amdgcn_alignbyte(segw[i + 1], segw[i], p); };
        // One step of the region chain (the same verdicts as D1): from path position p to the first one beyond p's region.
        auto hop = [&](uint32_t p) -> uint32_t {
            const uint32_t rend = ((p >> 6) + 1) * 64;
            const uint32_t dlt = rex8[(p >> 6) * 68 + (p & 63)];
            if (dlt != 255) return rend + dlt;
            uint64_t q = p;   // a long token (or the end of the path): token by token until the region is left
            while (q < rend && q < avail) q += tok_advance(uint32_t(ld64_clamped(srcb, s0 + uint32_t(q), d.clen)));   // (the bytes are not in LDS yet)
            return q > 0x7fffffffull ? 0x7fffffffu : uint32_t(q);
        };
        // The chain from the true entry is 128 dependent LDS reads for one thread (14 us).  Fifteen lanes instead: lane g starts at
        // the first byte of region group g (8 regions; the groups at or before the entry start AT the entry) and walks two groups,
        // noting where it enters each region.  A parse from a wrong start falls in step with the real tokens within a few of them:
        // when walk g meets walk g - 1 somewhere in group g, it IS the true path from there on, i.e. in all of group g + 1.  Group k's
        // entries are taken from walk k - 1 (group 0: walk 0); if some walk did not meet its predecessor (a literal longer than a
        // group, the end of the stream, hostile input), one thread chains the segment as before.
        const uint32_t e_rel = e - s0;
        if (wv == 0) {
            bool ok = true;
            if (lane < int(kIdxGroups) - 1) {   // (walk g serves group g + 1: the last group needs none of its own)
                const uint32_t g = uint32_t(lane), gstart = 64 * kIdxGrp * g, gend = gstart + 2 * 64 * kIdxGrp;
                uint32_t p = gstart > e_rel ? gstart : e_rel;
                while (p < gend && p < kSeg && p < avail) {
                    entg[2 * kIdxGrp * g + ((p >> 6) - kIdxGrp * g)] = uint16_t(p);
                    p = hop(p);
                }
            }
            // (the walks are writes and reads of ONE wavefront: ordered)
            if (lane >= 1 && lane < int(kIdxGroups) - 1) {
                const uint32_t g = uint32_t(lane), gstart = 64 * kIdxGrp * g;
                if (gstart > e_rel && gstart < avail) {
                    bool met = false;
                    for (uint32_t k = 0; k < kIdxGrp; k++) {
                        const uint32_t a = entg[2 * kIdxGrp * g + k], c = entg[2 * kIdxGrp * (g - 1) + kIdxGrp + k];
                        met = met || (a != 0xffff && a == c);
                    }
                    ok = met;
                }
            }
            const bool all_ok = ballot64(!ok) == 0;
            if (lane == 0) red[2] = all_ok ? 1u : 0u;
        }
        __syncthreads();
        if (red[2] != 0) {
            const uint32_t k = uint32_t(tid) / kIdxGrp, from = k ? k - 1 : 0;
            rentry[tid] = entg[2 * kIdxGrp * from + (uint32_t(tid) - kIdxGrp * from)];
        } else if (tid == 0) {
            uint32_t p = e_rel;
            while (p < kSeg && p < avail) {
                rentry[p >> 6] = uint16_t(p);
                p = hop(p);
            }
        }
        __syncthreads();
        // the chain is done with the region exits: the segment's bytes take their place
#pragma unroll
        for (uint32_t q = 0; q < kPer; q++) {
            const uint32_t j = q * kIdxThreads + uint32_t(tid);
            if (j < kPieces) reinterpret_cast<uint4*>(segw)[j] = w[q];
        }
        if (tid < 4) segw[(kSeg + 16) / 4 + tid] = 0;
        __syncthreads();
        if (avail < kSeg + 16 && (avail & 15)) {   // (uniform) the ragged piece at the end of the stream, byte by byte over its zeros
            const uint32_t i0 = avail & ~15u;
            if (uint32_t(tid) < (avail & 15)) reinterpret_cast<uint8_t*>(segw)[i0 + tid] = srcb[s0 + i0 + tid];
            __syncthreads();
        }
        IDXP(1);
        // ---- the walk: token starts of my region, their output bytes, the last token with an offset of its own ----
        uint32_t rout = 0, plast = 0xffffffffu;   // (a region has at most 64 tokens of less than 2^25 bytes each)
        {
            uint32_t p = rentry[tid];
            const uint32_t lim = r0 + 64 < avail ? r0 + 64 : avail;
            if (p != 0xffff) {
                while (p < lim) {
                    const uint64_t w = lds_ld64(segw, p);
                    const uint32_t tt = toktab[uint32_t(w) & 0xff];
                    mask |= 1ull << (p - r0);
                    rout += tok_olen(w, tt);
                    if (tt >> 27) plast = p;
                    p += tok_adv(uint32_t(w), tt);   // (< 2^25 per step)
                }
            }
        }
        uint32_t rlast = 0;
        if (plast != 0xffffffffu) { const uint32_t lo = lds4(plast); rlast = tok_off(lo, toktab[lo & 0xff]); }
        const uint32_t cnt = uint32_t(__builtin_popcountll(mask));
        const uint32_t incl = wave_incl_scan_u32(cnt);
        const uint32_t sc_lo = wave_incl_scan_u32(rout & 0xffffffu), sc_hi = wave_incl_scan_u32(rout >> 24);
        const uint64_t has = ballot64(rlast != 0);
        {   // the two quarters of my wave: lanes 0..31 and 32..63 (an inclusive scan holds the first half's sum in lane 31)
            const uint32_t has0 = uint32_t(has), has1 = uint32_t(has >> 32);
            const uint32_t l0 = has0 ? rdlane(rlast, 31 - int(__builtin_clz(has0))) : 0, l1 = has1 ? rdlane(rlast, 63 - int(__builtin_clz(has1))) : 0;
            const uint32_t a_lo = rdlane(sc_lo, 31), a_hi = rdlane(sc_hi, 31), a_n = rdlane(incl, 31);
            const uint32_t t_lo = rdlane(sc_lo, 63), t_hi = rdlane(sc_hi, 63), t_n = rdlane(incl, 63);
            if (lane == 0) {
                IdxAgg a; a.out = sat31(uint64_t(a_lo) + (uint64_t(a_hi) << 24)); a.ntok = a_n; a.last = l0;
                IdxAgg c; c.out = sat31(uint64_t(t_lo - a_lo) + (uint64_t(t_hi - a_hi) << 24)); c.ntok = t_n - a_n; c.last = l1;
                qagg[2 * wv] = a; qagg[2 * wv + 1] = c;
            }
        }
        __syncthreads();   // (also: nobody reads the segment's bytes any more — the token list may be written over them)
        const uint32_t n_w0 = qagg[0].ntok + qagg[1].ntok;
        rank0 = incl - cnt + (wv ? n_w0 : 0);
        ntok_seg = n_w0 + qagg[2].ntok + qagg[3].ntok;
        IDXP(2);
    }
    // ---- the token list of the segment (16-bit positions, stream order) and its aggregates ----
    uint16_t* tl = tok16 + (size_t(seg) << kSegLog);
    const uint32_t nchunk = (ntok_seg + kIdxStage - 1) / kIdxStage;   // 1 unless tokens average less than two bytes
    for (uint32_t c = 0; c < nchunk; c++) {
        if (c) __syncthreads();
        {   // token positions of chunk c, in stream order
            const uint32_t lo = c * kIdxStage;
            uint64_t m = mask;
            uint32_t r = rank0 - lo;
            while (m) {
                const uint32_t bit = ctz64(m);
                m &= m - 1;
                if (r < kIdxStage) stage[r] = uint16_t(r0 + bit);
                r++;
            }
        }
        __syncthreads();
        const uint32_t n = ntok_seg - c * kIdxStage < kIdxStage ? ntok_seg - c * kIdxStage : kIdxStage;
        uint4* dst = reinterpret_cast<uint4*>(tl + c * kIdxStage);   // (kIdxStage is a multiple of 8; the copy may run up to 7 entries past n, inside the segment's slot)
        const uint4* sv = reinterpret_cast<const uint4*>(stage);
        for (uint32_t q = uint32_t(tid); q < (n + 7) / 8; q += kIdxThreads) dst[q] = sv[q];
    }
    if (tid == 0) {   // prefixes over the quarters: what precedes quarter 1, 2, 3 inside the segment, and the segment's total
        IdxAgg run{0, 0, 0};
        for (uint32_t k = 0; k < 4; k++) {
            if (e != kNone) run = idx_join(run, qagg[k]);
            if (k < 3) seg_part[3 * size_t(seg) + k] = idx_word(run); else seg_state[seg] = idx_word(run);
        }
    }
    IDXP(3);
}

// Per destination tile (mod 16, the period of the level patterns): which source tiles (mod 16) a copy must NOT read — those whose level
// is not strictly lower — for the three patterns, 16 bits each (fast: bits 0..15, dense: 16..31, three-level: 32..47).
struct IdxBadTab { uint64_t m[16]; };
__host__ __device__ constexpr IdxBadTab make_badtab() {
    IdxBadTab t{};
    const uint32_t pats[3] = {kPatternFast, kPatternDense, kPatternThree};
    for (uint32_t kq = 0; kq < 16; kq++) {
        uint64_t m = 0;
        for (uint32_t p = 0; p < 3; p++)
            for (uint32_t s = 0; s < 16; s++)
                if (((pats[p] >> (2 * s)) & 3) >= ((pats[p] >> (2 * kq)) & 3)) m |= 1ull << (16 * p + s);
        t.m[kq] = m;
    }
    return t;
}
__device__ const IdxBadTab g_badtab = make_badtab();

// D3 / 2: the lists.  No LDS staging: a lane's token position comes from phase 1's list (coalesced), its bytes from the stream
// (64 consecutive tokens are ~400 consecutive bytes), both requested a round ahead.
constexpr uint32_t kIdx2Threads = 128;   // two waves, a quarter of the segment's regions each: two workgroups per segment
__global__ __launch_bounds__(kIdx2Threads) void dec_index2_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                                  const uint32_t* __restrict__ seg_block, DecBlock* __restrict__ dec,
                                                                  const unsigned long long* __restrict__ seg_state, const unsigned long long* __restrict__ seg_part,
                                                                  const uint16_t* __restrict__ tok16, TileStart* __restrict__ tile_start,
                                                                  uint32_t* __restrict__ tok_pos, uint32_t* __restrict__ round_d, uint32_t* __restrict__ round_rep,
                                                                  uint8_t* __restrict__ seg_viol /* [4] per segment, zeroed: which level patterns each quarter's copies break */) {
    __shared__ uint32_t toktab[256];
    __shared__ uint32_t red[12];
    const uint32_t seg = blockIdx.x >> 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wvl = rdfirst(uint32_t(tid) >> 6);                 // wave inside the workgroup
    const uint32_t wv = 2 * (blockIdx.x & 1) + wvl;                  // quarter of the segment
#ifdef MLZ_IDX_PROF
    unsigned long long idx_t = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) atomicAdd(&g_idxprof[14], 1ull);
#endif
    const unsigned long long my_word = seg_state[seg];
    const unsigned long long w_before = wv ? seg_part[3 * size_t(seg) + wv - 1] : (1ull << 63), w_upto = wv < 3 ? seg_part[3 * size_t(seg) + wv] : my_word;
    const uint32_t bi = seg_block[seg];
    const BlockInfo b = blocks[bi];
    const DecBlock d = dec[bi];
    if (d.status != 0 || d.literals) return;
    const uint32_t s0 = (seg - b.first_seg) << kSegLog;
    if (s0 >= d.clen) return;
    const uint32_t avail = d.clen - s0;
    const bool last_seg = avail <= kSeg;
    const uint8_t* srcb = src_base + b.src_off + d.body_off;
    toktab[tid] = g_toktab.e[tid]; toktab[tid + 128] = g_toktab.e[tid + 128];
    // my wave's tokens: those of regions 32 w .. 32 w + 31 (phase 1 left what the quarters before mine add up to).  Their positions and the
    // first round's bytes are requested before the look-back below, which is a round trip of its own.
    const IdxAgg mine = idx_unword(my_word), before = idx_unword(w_before);
    const uint32_t ntok_seg = mine.ntok;
    const uint32_t lo = before.ntok, hi = idx_unword(w_upto).ntok;
    const uint16_t* tl = tok16 + (size_t(seg) << kSegLog);
    const bool whole = uint64_t(s0) + kSeg + 8 <= d.clen;   // every 8-byte read of this segment stays inside the stream
    const uint8_t* sp = srcb + s0;
    auto bytes_at = [&](uint32_t pos) -> uint64_t { return whole ? ld64u(sp + pos) : ld64_clamped(srcb, s0 + pos, d.clen); };
    auto pos_of = [&](uint32_t q) -> uint32_t { return tl[q < hi ? q : (hi ? hi - 1 : 0)]; };
    uint32_t pos_c = 0, pos_n = 0;
    uint64_t w_c = 0;
    if (lo < hi) {
        pos_c = pos_of(lo + uint32_t(lane)); pos_n = pos_of(lo + 64 + uint32_t(lane));
        w_c = bytes_at(pos_c);
    }
    // ---- what precedes the segment in its block: every thread reads the words of predecessors seg - 1 - tid - 256 j (at most 2047) ----
    {
        const uint32_t npred = seg - b.first_seg;
        uint32_t so = 0, sn = 0, near_key = 0, near_last = 0;   // (at most 16 words of at most 2^24 per thread)
        bool missing = !(my_word >> 63) || !(w_before >> 63) || !(w_upto >> 63);
        for (uint32_t j0 = 0; j0 < npred; j0 += 4 * kIdx2Threads) {
            unsigned long long w[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t j = j0 + u * kIdx2Threads + uint32_t(tid);
                w[u] = j < npred ? seg_state[seg - 1 - j] : (1ull << 63);
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t j = j0 + u * kIdx2Threads + uint32_t(tid);
                missing = missing || !(w[u] >> 63);
                so += uint32_t(w[u]) & 0x1ffffffu; sn += uint32_t(w[u] >> 25) & 0x3fffu;
                const uint32_t la = uint32_t(w[u] >> 39) & 0x3fffffu;
                if (la && !near_key) { near_key = 0xffffffffu - j; near_last = la; }   // (j ascends: the first one found is this thread's nearest)
            }
        }
        const uint32_t s_lo = rdlane(wave_incl_scan_u32(so & 0xffffffu), 63), s_hi = rdlane(wave_incl_scan_u32(so >> 24), 63);
        const uint32_t s_n = rdlane(wave_incl_scan_u32(sn), 63);
        const uint32_t kmax = rdlane(wave_incl_max_u32(near_key), 63);
        const uint64_t who = ballot64(near_key == kmax);
        const uint32_t nl = kmax ? rdlane(near_last, int(ctz64(who))) : 0;
        uint32_t* xr = red + 6 * wvl;
        if (lane == 0) { xr[0] = s_lo; xr[1] = s_hi; xr[2] = s_n; xr[3] = kmax; xr[4] = nl; xr[5] = ballot64(missing) ? 1u : 0u; }
    }
    IDXP(8);
    __syncthreads();
    IDXP(9);
    IdxAgg base;
    {
        uint64_t o_lo = 0, o_hi = 0;
        uint32_t nt = 0, key = 0, la = 0, miss = 0;
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t* x = red + 6 * k;
            o_lo += x[0]; o_hi += x[1]; nt += x[2]; miss |= x[5];
            if (x[3] > key) { key = x[3]; la = x[4]; }
        }
        base.out = sat31(o_lo + (o_hi << 24)); base.ntok = nt; base.last = key ? la : 0;
        if (miss) {   // a word phase 1 did not write: cannot happen (same early exits) — fail the block rather than index garbage
            if (tid == 0) dec[bi].status = 7 | (12 << 8);
            return;
        }
    }
    if (last_seg && tid == 0 && (blockIdx.x & 1) == 0) {   // the block's totals
        const IdxAgg incl = idx_join(base, mine);
        dec[bi].total_out = incl.out;
        dec[bi].ntok = incl.ntok;
        if (incl.out != d.dlen) dec[bi].status = 1 | (2 << 8);   // d != len(dst), decode.go:615
    }
    if (ntok_seg == 0) return;
    // ---- the lists ----
    const IdxAgg pre = wv ? idx_join(base, before) : base;
    if (lo >= hi) return;
    uint32_t carry_d = pre.out, carry_rep = pre.last ? pre.last : 1u;   // initial repeat offset is 1 (decode.go:185)
    const uint32_t rank_lo = pre.ntok;
    uint32_t* tpos = tok_pos + (size_t(b.first_seg) << kSegLog);
    uint32_t* rd = round_d + (size_t(b.first_seg) << (kSegLog - 6));
    uint32_t* rr = round_rep + (size_t(b.first_seg) << (kSegLog - 6));
    TileStart* ts = tile_start + b.first_tile;
    uint32_t acc_lo = 0, acc_hi = 0;        // forbidden source tiles hit, per pattern (IdxBadTab layout)
    uint32_t viol = 0;                      // ... and what the slow path found
    uint32_t near = 0;                      // dependency-distance bits
    auto lv = [](uint32_t pattern, uint32_t t) -> uint32_t { return (pattern >> (2 * (t & 15))) & 3; };
    IDXP(10);
    for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
        carry_d = rdfirst(carry_d); carry_rep = rdfirst(carry_rep);
        const uint32_t q = q0 + uint32_t(lane);
        const bool have = q < hi;
        const uint32_t pos = pos_c;
        // Everything requested a round ago is taken out of flight HERE, before this round's requests go out: the stores below sit under
        // branches, so wherever the compiler first meets a loaded value after them it waits for ALL outstanding accesses — with the
        // new requests already issued that was a full memory round trip per round.  (The asm is that first use.)
        uint32_t w_lo = uint32_t(w_c), w_hi = uint32_t(w_c >> 32);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(w_lo), "+v"(w_hi), "+v"(pos_n));
        const uint64_t w = w_lo | (uint64_t(w_hi) << 32);
        // the next round's bytes and the positions of the round after it
        w_c = bytes_at(pos_n);
        pos_c = pos_n;
        pos_n = pos_of(q + 128);
        const uint32_t tt = toktab[uint32_t(w) & 0xff];
        const uint32_t olen = have ? tok_olen(w, tt) : 0;           // (< 2^25: 64 of them fit 32 bits)
        const uint32_t lit = have ? tok_lit(olen, tt) : 0, cp = olen - lit;
        const uint32_t toff = have ? tok_off(uint32_t(w), tt) : 0;
        const uint32_t incl = wave_incl_scan_u32(olen);
        const uint32_t dpos = sat31(uint64_t(carry_d) + (incl - olen));
        const uint32_t tag = toff ? uint32_t(lane) + 1 : 0;
        const uint32_t t_incl = wave_incl_max_u32(tag);
        const uint32_t t_excl = uint32_t(__builtin_amdgcn_update_dpp(0, int(t_incl), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
        const uint32_t l_from = __shfl(toff, int(t_excl ? t_excl - 1 : 0));
        const uint32_t rep = t_excl ? l_from : carry_rep;
        const uint32_t rank = rank_lo + (q - lo);
        if (have) tpos[rank] = s0 + pos;
        if (have && (rank & 63) == 0) { rd[rank >> 6] = dpos; rr[rank >> 6] = rep; }
        {
            // Level conformance (DESIGN.md "Tile levels"): every tile a copy writes to reads, for its part of the copy, only itself or
            // tiles of a strictly lower level.  The usual copy lands in one tile kd and reads one or two tiles: their bits (mod 16, once
            // per pattern) are and-ed with kd's forbidden set and or-ed into an accumulator that is looked at once, at the end.
            const uint32_t off = toff ? toff : rep;
            const uint32_t dc = dpos + lit;
            const bool valid = cp != 0 && off != 0 && off <= dc && uint64_t(dc) + cp <= d.dlen;
            const uint32_t kd = dc >> kTileLog, kend = (dc + cp - 1) >> kTileLog;
            const uint32_t sw0 = dc - off;
            const uint32_t s0t = sw0 >> kTileLog;
            const uint32_t s1t = ((off >= cp ? sw0 + cp : dc) - 1) >> kTileLog;
            const bool fast = kend == kd && s1t <= s0t + 1;
            const bool far = valid && s0t != kd;
            const uint32_t s1c = s1t < kd ? s1t : s0t;   // (the part of the source inside tile kd itself needs no check)
            const uint32_t bits = (1u << (s0t & 15)) | (1u << (s1c & 15));
            const uint64_t bad = g_badtab.m[kd & 15];
            const bool take = far && fast;
            acc_lo |= take ? (bits | (bits << 16)) & uint32_t(bad) : 0u;
            acc_hi |= take ? bits & uint32_t(bad >> 32) : 0u;
            // Dependency distance (round 5, kViolNear*): how close below its own tile a copy reads — 1, 2 or 3 tiles.  A general block
            // none of whose copies reads the K - 1 tiles in front of its own (LevelBalanced's far_gap) has K tiles that never read each
            // other: dec_general_kernel settles them side by side.  Copies over tile boundaries (other encoders only) count as distance 1.
            {
                const uint32_t dist = kd - s1c;
                near |= take ? (dist == 1 ? kViolNear1 : dist == 2 ? kViolNear2 : dist == 3 ? kViolNear3 : 0u) : 0u;
                near |= valid && !fast ? kViolNearAll : 0u;
            }
            if (valid && !fast && viol != kViolAll) {   // a copy over a tile boundary (other encoders only)
                auto check = [&](uint32_t kq, uint32_t a0, uint32_t a1) {  // tile kq reads tiles a0..a1 (below kq)
                    for (uint32_t tsrc = a0; tsrc <= a1 && tsrc < kq; tsrc++) {
                        if (lv(kPatternFast, tsrc) >= lv(kPatternFast, kq)) viol |= 1;
                        if (lv(kPatternDense, tsrc) >= lv(kPatternDense, kq)) viol |= 2;
                        if (lv(kPatternThree, tsrc) >= lv(kPatternThree, kq)) viol |= 4;
                    }
                };
                for (uint32_t kq = kd; kq <= kend && viol != kViolAll; kq++) {
                    uint32_t a0, a1;  // source tiles of the part of the copy that lands in tile kq
                    if (off >= cp) {
                        const uint32_t p0 = kq == kd ? dc : kq << kTileLog;
                        const uint32_t p1 = kq == kend ? dc + cp : (kq + 1) << kTileLog;
                        a0 = (p0 - off) >> kTileLog; a1 = (p1 - 1 - off) >> kTileLog;
                    } else {  // overlapping copy: every byte comes from the window [dc - off, dc)
                        a0 = s0t; a1 = (dc - 1) >> kTileLog;
                    }
                    if (a0 < kq) check(kq, a0, a1);
                }
            }
        }
        {   // tiles whose first byte lies in [dpos, dpos + olen)
            const uint32_t k0 = (dpos + kTile - 1) >> kTileLog;
            const uint64_t endp = uint64_t(dpos) + olen;
            if (have && (uint64_t(k0) << kTileLog) < endp && k0 < b.n_tiles) {
                for (uint64_t k = k0; (k << kTileLog) < endp && k < b.n_tiles; k++) {
                    TileStart v; v.cpos = s0 + pos; v.d = dpos; v.rep = rep; v.rank = rank;
                    ts[k] = v;
                }
            }
        }
        carry_d = sat31(uint64_t(carry_d) + rdlane(incl, 63));
        const uint32_t t_all = rdlane(t_incl, 63);
        if (t_all) carry_rep = rdlane(toff, int(t_all - 1));
    }
    IDXP(11);
    // What my quarter found goes into a byte of its own; dec_viol_kernel gathers the bytes per block.  (Rounds 2-4a or-ed them into the
    // block's word with an atomic per wave — every wave of a block finds the same bits, and tens of thousands of device-scope atomics
    // and re-checking loads on a dozen addresses cost this kernel 80 of its 130 us.)
    viol |= ((acc_lo & 0xffffu) ? 1u : 0u) | ((acc_lo >> 16) ? 2u : 0u) | (acc_hi ? 4u : 0u) | near;
    viol = (ballot64(viol & 1) ? 1u : 0u) | (ballot64(viol & 2) ? 2u : 0u) | (ballot64(viol & 4) ? 4u : 0u) |
           (ballot64(viol & kViolNear1) ? kViolNear1 : 0u) | (ballot64(viol & kViolNear2) ? kViolNear2 : 0u) | (ballot64(viol & kViolNear3) ? kViolNear3 : 0u);
    if (viol && lane == int(ctz64(ballot64(true)))) seg_viol[4 * size_t(seg) + wv] = uint8_t(viol);
}

}  // namespace mlz
