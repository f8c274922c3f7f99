// mlz_encode2.hip.inc — LevelFastest / LevelSuperFast encoder for gfx950, round-2 design (included by mlz_hip.hip).
//
// Replaces the reference's L1 match-finder encodeBlockGo / encodeBlockAsm* (encode_l1.go:39-283,
// _generate/gen.go:257-1155) and its emit calls (encode_l1.go:190-206) by TWO kernels:
//
//   match_tiles_kernel      one 256-thread workgroup per 32 KiB tile.  The tile's bytes are staged in LDS once
//                           (coalesced 16-byte loads) and every later byte access of the match finder is an LDS
//                           read.  Each of the four wavefronts owns one 8 KiB PIECE of the tile and its own
//                           2^12-entry near table, which it first fills with the positions of the tile's earlier
//                           pieces (a hash and a 2-byte LDS store per position), so a piece finds the same near
//                           candidates a single pass over the tile would — but the serial chain of a tile is four
//                           times shorter.  Per iteration a wave probes 4 x 64 consecutive positions: 4-byte hash ->
//                           table look-up (all look-ups of a window before its inserts), 8-byte verify, straight-
//                           line extension to 32 bytes, one far probe into the block-wide first-occurrence tables
//                           (far_build_kernel, mlz_encode.hip.inc), three-position lazy matching.  Match finding
//                           does not depend on the parse (there is no repeat-offset probe: on the CPU model of this
//                           design, tools/encmodel2, it changes the output by < 0.01 %), so its loads are never
//                           behind a parse decision.  A wave-uniform scalar walk over the candidate mask does the
//                           reference's greedy "take the first hit, jump past it" parse and the selected lanes
//                           write 8-byte token RECORDS {match start, length, offset}.
//   serialize_pieces_kernel one wavefront per piece, one LANE per token (64 tokens per step instead of the ~6
//                           that start inside one 64-byte window): backward extension (encode_l1.go:169-172),
//                           pending literals, repeat detection, the reference's choice of token form
//                           (encode_l1.go:190-206), a prefix sum for the output offsets, header and literal bytes
//                           staged in an LDS ring and flushed with 16-byte stores.
//
// The per-block layout and the gather into the final block (encode_layout_kernel / encode_gather2_kernel) work
// on pieces: every piece is an independent token sub-stream (it never starts with a repeat).

namespace mlz {

constexpr uint32_t kSubLog = 2;
constexpr uint32_t kSub = 1u << kSubLog;                 // pieces (= wavefronts) per tile
constexpr uint32_t kPieceLog = kTileLog - kSubLog;
constexpr uint32_t kPiece = 1u << kPieceLog;             // 8 KiB
constexpr uint32_t kRecPerPiece = kPiece / 4;            // a match is at least 4 bytes
constexpr uint32_t kM2Pad = 256;                         // zero bytes behind the tile (windows and 36-byte reads run past it)
// Near tables: piece k of a tile indexes (k + 1) x 8 KiB of positions (the earlier pieces are seeded into it) and gets
// (k + 1) x kM2Unit entries — the same positions per entry for every piece.  Two workgroups of 32 KiB + 4 tables fit a
// CU's 160 KiB either way; graded tables of 2048 / 4096 / 6144 / 8192 entries (40 KiB) use what four 4096-entry tables
// (32 KiB) left idle and compress ~1 % better (CPU model: text 0.3416 -> 0.3385).
template <int HB> struct M2Cfg {                                                      // HB = hash bits of the near tables
    static constexpr uint32_t kUnit = (1u << HB) / kSub;                               // entries per 8 KiB of indexed positions
    static constexpr uint32_t kEntries = kUnit * (kSub * (kSub + 1) / 2);              // all four tables
    static constexpr uint32_t kLds = kTile + kM2Pad + 2 * kEntries;
};
// Near-table sizes.  13 hash bits: 40 KiB of tables, 72 KiB per workgroup, two workgroups per CU.  12 bits: 20 KiB of tables,
// 52 KiB per workgroup, THREE per CU — the kernel is bound by VALU issue with two waves per SIMD covering each other's waits
// badly (59 % VALU busy), and the third workgroup is worth 17 %.  The smaller tables cost ~4 % of output, which blocks of
// 1 MiB and more get back (and more) from the dense level pattern (one tile in 16 without far matching instead of one in 4:
// enwik-like 0.4647 -> 0.4627, text 0.3385 -> 0.3252, JSON 0.4395 -> 0.4405 on the CPU model); smaller blocks have too few
// tiles for that and keep the 13-bit tables.  LevelSuperFast (no far matching at all) always runs the 12-bit configuration.
// The class is a property of the BLOCK, so a block's bytes do not depend on what else is in the batch: a batch with both
// classes is two launches, each workgroup leaving at once when its block belongs to the other one.
#ifndef MLZ_L1_HB
#define MLZ_L1_HB 12
#endif
constexpr int kM2HashBitsSmall = 13, kM2HashBitsBig = MLZ_L1_HB, kM2HashBitsSuperFast = 12;
constexpr uint64_t kM2BigBlock = kBigBlock;   // blocks of at least this many bytes take the three-per-CU configuration
// LevelBalanced on the same kernels: 13-bit near tables seeded with every earlier position, far tables of 2^18 entries holding
// every second window (twice as dense, twice as large), and the previous epoch's table probed as well as the position's own.
constexpr int kL2FarBits = kL2FarBitsBig, kL2FarStride = 2;
constexpr uint32_t kPieceScratch = kPiece + 64;          // a piece that does not beat one literal run is stored raw
constexpr uint32_t kSkipShift = 10;
#ifndef MLZ_M2_SEEDSTRIDE
#define MLZ_M2_SEEDSTRIDE 2
#endif
constexpr uint32_t kSeedStride = MLZ_M2_SEEDSTRIDE;    // which positions of the earlier pieces a piece's near table is seeded with                      // growing skip over incompressible data
#ifndef MLZ_M2_NW
#define MLZ_M2_NW 4
#endif

__device__ __forceinline__ uint32_t albyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
__device__ __forceinline__ uint32_t common8(uint64_t a, uint64_t b) { const uint64_t d = a ^ b; return d ? ctz64(d) >> 3 : 8; }
// common prefix of two 24-byte strings given as three xor words
__device__ __forceinline__ uint32_t prefix24(uint64_t x1, uint64_t x2, uint64_t x3) {
    const uint32_t n3 = x3 ? ctz64(x3) >> 3 : 8;
    const uint32_t n2 = x2 ? ctz64(x2) >> 3 : 8 + n3;
    return x1 ? ctz64(x1) >> 3 : 8 + n2;
}
__device__ __forceinline__ uint64_t u64of(uint32_t lo, uint32_t hi) { return lo | (uint64_t(hi) << 32); }
// Near tables (round 3): the bucket of a 4-byte window is mul_hi(hash32, table entries) — the whole 32-bit hash scaled into the (graded,
// not a power of two) table in ONE instruction; as a byte offset: mul_hi(hash32, 2 * entries) & ~1.  The 16th bit of an entry is the
// hash bit just below the HB index bits.
__device__ __forceinline__ uint16_t* near_slot(uint16_t* table, uint32_t h32, uint32_t tsize) {
    return reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(table) + (__umulhi(h32, 2 * tsize) & ~1u));
}
template <int HB> __device__ __forceinline__ uint32_t near_tag(uint32_t h32) { return (h32 >> (16 - HB)) & 0x8000u; }
// Match lengths without 64-bit ctz chains.  v_ffbl_b32 returns 0xffffffff for 0, and OR-ing a dword's bit offset 32 * j into it
// keeps that "no difference" value, so the first differing BIT of N xor words is one unsigned minimum over (ffbl(x_j) | 32 j)
// — N ffbl, N - 1 or, (N - 1) / 2 min3 — instead of a ctz64 + compare + select per 8 bytes.  (On gfx950 v_or / v_and / v_add /
// v_lshrrev issue in 2 cycles per wave, everything else — ffbl, min, cmp, alignbyte, every VOP3 — in 4: profiles/r03_valu_rate.txt.)
__device__ __forceinline__ uint32_t ffbl_raw(uint32_t x) { uint32_t r; asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }
template <int N>
__device__ __forceinline__ uint32_t first_diff_bit(const uint32_t (&x)[N]) {   // 0xffffffff when all N words are zero
    uint32_t r = ffbl_raw(x[0]);
#pragma unroll
    for (int j = 1; j < N; j++) r = min(r, ffbl_raw(x[j]) | uint32_t(32 * j));
    return r;
}
__device__ __forceinline__ uint32_t usub_sat(uint32_t a, uint32_t b) { return __builtin_elementwise_sub_sat(a, b); }   // v_sub_u32 ... clamp

#ifdef MLZ_M2_PROF
__device__ unsigned long long g_m2prof[16];   // debug build only: per-phase cycle sums over all waves (tools/m2prof.py)
#define M2P(i) do { const unsigned long long t_now = __builtin_readcyclecounter(); m2pc[i] += t_now - m2t; m2t = t_now; } while (0)
#else
#define M2P(i) do { } while (0)
#endif

constexpr uint32_t kSerRing = 4096;
constexpr uint32_t kSerLds = kSub * kSerRing;
template <uint32_t RING, bool LDSSRC>
__device__ __forceinline__ uint32_t serialize_piece(const uint8_t* __restrict__ sblk, const uint8_t* __restrict__ s, const uint32_t* ldata, const BlockInfo& b,
                                                    const uint32_t base, const uint32_t ps, const uint32_t tl, const uint32_t cnt, const uint2* __restrict__ rp,
                                                    uint8_t* ring, uint8_t* __restrict__ out, const int lane);

// FB: far-table entries per (epoch, level set), log2.  FP: the previous epoch's table is probed as well (LevelBalanced, which
// also seeds its near tables with every earlier position).
#ifndef MLZ_M2_MINW
#define MLZ_M2_MINW 1   // minimum waves per SIMD the register allocation must allow (asking for 4 = 128 registers: +2 % on the round-2 loop, -7 % on the round-3 one)
#endif
template <bool FAR, int NW, int HB, int FB = kFarBits, bool FP = false>
__global__ __launch_bounds__(256, FP ? 1 : MLZ_M2_MINW) void match_tiles_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                          const uint32_t* __restrict__ tile_block, uint2* __restrict__ recs,
                                                          uint32_t* __restrict__ piece_cnt, const uint32_t* __restrict__ far_tab,
                                                          uint32_t epochs_per_block, uint32_t pattern, uint32_t n_tiles, uint32_t cls,
                                                          uint32_t tab_log /* FB = 0: the far tables are 2^tab_log entries apart */,
                                                          uint32_t far_gap /* bytes: a far source ends at least this far in front of the position's tile (MLZ_OPT_L2_GAP; 0 = anywhere) */,
                                                          uint8_t* __restrict__ scratch /* not null: the piece is serialized here too (token bytes to scratch, size word to piece_size) */,
                                                          uint32_t* __restrict__ piece_size) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* ldata = reinterpret_cast<uint32_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = rdfirst(uint32_t(tid) >> 6);
    constexpr uint32_t kM2Unit = M2Cfg<HB>::kUnit, kM2Lds = M2Cfg<HB>::kLds;
    constexpr int kM2HashBits = HB;
    uint16_t* table = reinterpret_cast<uint16_t*>(smem + kTile + kM2Pad) + kM2Unit * (wv * (wv + 1) / 2);   // tables of 1, 2, 3, 4 units
    const uint32_t tsize = (wv + 1) * kM2Unit;
    // Workgroup -> tile: consecutive tiles go to the SAME XCD (workgroup b is observed to run on XCD b % 8; a placement
    // for speed only).  An XCD then works its way through one 2 MiB epoch of one block at a time (32 CUs x 2 tiles), so the
    // epoch's far tables — probed at random, a 64-byte line per 4-byte probe — are served by that XCD's 4 MiB L2 instead
    // of by the fabric.
    const uint32_t per_xcd = (n_tiles + 7) >> 3;
    const uint32_t gt = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (gt >= n_tiles) return;
    const uint32_t bi = tile_block[gt];
    const BlockInfo b = blocks[bi];
    if (cls != 2 && uint32_t(b.src_len >= kM2BigBlock) != cls) return;   // cls: 0 = blocks below kM2BigBlock only, 1 = the others only, 2 = all
    const uint32_t tib = gt - b.first_tile;
    const uint32_t base = tib << kTileLog;
    const uint8_t* sblk = src_base + b.src_off;
    const uint8_t* s = sblk + base;
    const uint32_t tl = uint32_t(b.src_len - base < kTile ? b.src_len - base : kTile);

    // ---- stage the tile (16-byte loads), zero everything behind it, zero the four near tables ----
    {
        const uint32_t nv = tl >> 4;
        uint4* dv = reinterpret_cast<uint4*>(ldata);
        uint4 x[8];  // a full tile is 8 x 16 bytes per thread: all eight loads are issued before the first LDS store
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t q = tid + 256 * k;
            __builtin_memcpy(&x[k], s + 16 * size_t(q < nv ? q : 0), 16);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t q = tid + 256 * k;
            if (q < nv) dv[q] = x[k];
        }
        if (tid < 16) {
            const uint32_t q = (nv << 4) + tid;
            reinterpret_cast<uint8_t*>(ldata)[q] = q < tl ? s[q] : uint8_t(0);
        }
        constexpr uint32_t kAllV = kM2Lds >> 4;  // data + pad + tables, in 16-byte units
        for (uint32_t q = nv + 1 + tid; q < kAllV; q += 256) dv[q] = uint4{0, 0, 0, 0};
    }
    __syncthreads();
    const uint32_t ps = wv << kPieceLog;
    const size_t pid = size_t(gt) * kSub + wv;
    if (ps >= tl) {
        if (lane == 0) { piece_cnt[pid] = 0; if (scratch) piece_size[pid] = 0; }
        return;
    }
    const uint32_t pe = ps + kPiece < tl ? ps + kPiece : tl;

    // ---- near table := every kSeedStride-th position of the tile's earlier pieces, in order (highest position wins) ----
    // (every position: 10 % of the kernel's VALU instructions, the last piece seeding three times what it matches; every
    // second one costs 0.3 % of output on the CPU model)
    {
        constexpr uint32_t kSS = FP ? 1u : kSeedStride;
        for (uint32_t q0 = 0; q0 < ps; q0 += 256 * kSS) {
            uint32_t v4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t p = q0 + kSS * (64 * u + lane);
                const uint32_t A = p >> 2;
                v4[u] = albyte(ldata[A + 1], ldata[A], p);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t p = q0 + kSS * (64 * u + lane);
                const uint32_t h32 = v4[u] * 2654435761u;
                *near_slot(table, h32, tsize) = uint16_t(p | near_tag<kM2HashBits>(h32));
            }
        }
    }

    const int mylv = pattern == kPatternFree ? (tib > 0 ? 1 : 0) : tile_level_p(tib, pattern);   // (free: every tile but the first probes the one table of all positions)
    const uint32_t* ftab = nullptr;
    // FB = 0 (the class of blocks below 1 MiB): the table size goes with the block's length (small_far_bits)
    const int fb = FB ? FB : small_far_bits(b.src_len) + (FP ? 1 : 0);
    const uint32_t tlog = FB ? uint32_t(FB) : tab_log;
    if (FAR && mylv > 0) ftab = far_tab + ((size_t(bi) * far_sets(pattern) + (mylv - 1)) * epochs_per_block << tlog);
    uint2* rp = recs + pid * kRecPerPiece;

    // ---- the far pipeline ----
    // The table probe and the candidate fetch are the two accesses of this kernel that leave the CU, and with 8
    // wavefronts per CU nothing hides them but distance: right after iteration n's far compare, the candidates of
    // iteration n+1 (tag test of the entries requested an iteration earlier, then their 32 bytes) and the table
    // entries of iteration n+2 are requested — match finding does not depend on the parse, so the next windows are
    // known unless the parse skips ahead, in which case the next two iterations simply run without far candidates.
    // Each request has ONE site in the loop: a second definition of the destination registers makes the
    // compiler copy them at the join, and a copy of a register with a load in flight is a wait for that load.
    uint32_t pf_e[NW], pf_tag[NW];   // table entries (+ expected tags) of the windows at pf_cur
    uint32_t pf_e2[FP ? NW : 1];     // FP: the previous epoch's entries
    uint4 gx[FP ? NW : 1], gy[FP ? NW : 1];   // FP: their candidates' bytes
    uint32_t gq[FP ? NW : 1];
    uint32_t pf_cur = 0xffffffffu;
    uint4 fx[NW], fy[NW];            // 32 candidate bytes of the windows at cand_cur
    uint32_t fq[NW];                 // ... and where they are (block-relative); kNoFar = the lane has no far candidate
    constexpr uint32_t kNoFar = 0xffffffffu;
    uint32_t cand_cur = 0xffffffffu;
    const bool has_far = FAR && ftab != nullptr;
    uint32_t warm = has_far ? 2 : 0;  // two start-up trips fill the pipeline for the piece's first windows

#ifdef MLZ_M2_PROF
    unsigned long long m2pc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long m2t = __builtin_readcyclecounter();
#endif
    // A candidate needs 32 readable bytes on both sides: none is looked at in the last 40 bytes of a block.  Only the block's last
    // tile can come that close, so the per-lane test is compiled into the loop but skipped (wave-uniform) everywhere else.
    const bool deep_tile = uint64_t(base) + tl + 40 <= b.src_len;
    const uint32_t far_lim = base > far_gap ? base - far_gap : 0u;   // far sources lie below this position (the tile's start; LevelBalanced without levels: far_gap in front of it)
    uint32_t cur = ps, pos = ps, cnt = 0;
    while (cur + 4 <= pe) {
        cur = rdfirst(cur); pos = rdfirst(pos); cnt = rdfirst(cnt); warm = rdfirst(warm);
        pf_cur = rdfirst(pf_cur); cand_cur = rdfirst(cand_cur);
        M2P(9);
        const bool run = warm == 0;
        uint32_t best[NW], boff[NW];
        uint32_t m[NW][8];
        uint32_t maxl[NW], lim[NW];
        if (run) {
            // ---- phase A: my 36 bytes per window: nine aligned dwords (four lanes share them: broadcast reads) + funnel shifts ----
            // (v_alignbyte_b32 looks at the low two bits of its shift operand only: the position itself is the shift)
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t p = cur + 64 * w + lane;
                // Bytes left in the piece, 0 behind its end (a saturating subtract).  There is no separate "valid" flag: a position
                // with fewer than 4 bytes left ends with best < 4 = no candidate through the clamp below, and what it inserts into
                // the near table is never looked up (the piece ends with this iteration).
                maxl[w] = usub_sat(pe, p);
                lim[w] = maxl[w] < kLaneCap ? maxl[w] : kLaneCap;
                const uint32_t A = p >> 2;
                uint32_t d[9];
#pragma unroll
                for (int j = 0; j < 9; j++) d[j] = ldata[A + j];
#pragma unroll
                for (int j = 0; j < 8; j++) m[w][j] = albyte(d[j + 1], d[j], p);
            }
            M2P(0);  // mine
            // ---- phase B: near table: look-up, then insert (one instruction each: all look-ups of a window precede its inserts) ----
            uint32_t e[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t p = cur + 64 * w + lane;
                const uint32_t h32 = m[w][0] * 2654435761u;
                const uint32_t ntag = near_tag<kM2HashBits>(h32);
                uint16_t* slot = near_slot(table, h32, tsize);
                e[w] = *slot ^ ntag;                         // bit 15 clear <=> the stored hash bit agrees
                *slot = uint16_t(p | ntag);
            }
            M2P(1);  // table
            // ---- phase C: candidate bytes, 8-byte verify ----
            uint32_t c2[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t p = cur + 64 * w + lane;
                // positions are below 2^15 and a disagreeing hash bit sets bit 15 of e: "an earlier position whose stored bit agrees" is ONE compare
                const bool near_ok = e[w] < p;
                const uint32_t cand = e[w] & 0x7fffu;
                const uint32_t NA = cand >> 2;
                const uint32_t c0 = ldata[NA], c1 = ldata[NA + 1];
                c2[w] = ldata[NA + 2];
                const uint32_t x[2] = {m[w][0] ^ albyte(c1, c0, cand), m[w][1] ^ albyte(c2[w], c1, cand)};
                const uint32_t l8 = min(first_diff_bit(x) >> 3, 8u);
                best[w] = near_ok && l8 >= 4 ? l8 : 0;
                boff[w] = p - cand;
            }
            M2P(2);  // verify
            // ---- phase D: straight-line extension to 32 bytes (LDS, short latency: plain branches) ----
#pragma unroll
            for (int w = 0; w < NW; w++) {
                if (best[w] == 8 && lim[w] > 8) {
                    const uint32_t cand = e[w] & 0x7fffu;
                    const uint32_t NA = cand >> 2;
                    uint32_t c[7];
                    c[0] = c2[w];
#pragma unroll
                    for (int j = 1; j < 7; j++) c[j] = ldata[NA + 2 + j];
                    uint32_t x[6];
#pragma unroll
                    for (int j = 0; j < 6; j++) x[j] = m[w][2 + j] ^ albyte(c[j + 1], c[j], cand);
                    best[w] = min(8 + (first_diff_bit(x) >> 3), lim[w]);
                }
                if (best[w] > maxl[w]) best[w] = maxl[w];
            }
            M2P(3);  // extension
            // ---- phase E: far candidates (requested an iteration ago) ----
            if (has_far && cand_cur == cur) {
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const uint32_t pa = base + cur + 64 * w + lane;
                    auto far_cmp = [&](uint32_t q, const uint4& cx, const uint4& cy) {
                        const uint32_t x[8] = {m[w][0] ^ cx.x, m[w][1] ^ cx.y, m[w][2] ^ cx.z, m[w][3] ^ cx.w, m[w][4] ^ cy.x, m[w][5] ^ cy.y, m[w][6] ^ cy.z, m[w][7] ^ cy.w};
                        const uint32_t cleft = kTile - (q & (kTile - 1));     // the source must not leave its tile
                        const uint32_t lf = min(first_diff_bit(x) >> 3, min(cleft, lim[w]));
                        if (q != kNoFar && lf >= kFarMin && lf > best[w] + 2) { best[w] = lf; boff[w] = pa - q; }
                    };
                    far_cmp(fq[w], fx[w], fy[w]);
                    if constexpr (FP) far_cmp(gq[w], gx[w], gy[w]);   // the previous epoch's candidate after this epoch's
                }
            }
            M2P(4);  // far compare
        }
        if (has_far) {
            const uint32_t nx = run ? cur + 64 * NW : cur;   // the next trip's windows unless the parse skips
            if (pf_cur == nx) {
                // tag test of the entries in pf_e, then the candidates' 32 bytes.  (All tag tests come before the first
                // load: the loads sit under a branch, and after such a load the compiler waits for everything
                // outstanding at the next use of ANY loaded value.)
                // A hit = the 9 tag bits agree AND the entry's position lies before this tile: with the agreeing tag xor-ed away
                // and the word rotated right by 9, that is ONE unsigned compare (positions are below 2^23).
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const uint32_t pa = base + nx + 64 * w + lane;
                    auto hit = [&](uint32_t entry, bool extra) -> uint32_t {
                        const uint32_t k = __builtin_amdgcn_alignbit(entry ^ pf_tag[w], entry ^ pf_tag[w], kFarTagBits);   // ror 9: tag difference on top, position below
                        bool ok = k < far_lim && extra;
                        if (!deep_tile) ok = ok && uint64_t(pa) + 40 <= b.src_len;
                        if constexpr (FP) ok = ok && pa - k <= kMaxCopy3Offset;   // (the position's own epoch is never further than 2 MiB away)
                        return ok ? k : kNoFar;
                    };
                    fq[w] = hit(pf_e[w], true);
                    if constexpr (FP) gq[w] = hit(pf_e2[w], (pa >> kEpochLog) > 0);
                }
                // Only the lanes that have a candidate load: the texture-address unit works through a vector-memory
                // instruction lane by lane, so 64 lanes reading one shared dummy address cost what 64 scattered reads do.
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (fq[w] != kNoFar) {
                        const uint8_t* cptr = sblk + fq[w];
                        __builtin_memcpy(&fx[w], cptr, 16);
                        __builtin_memcpy(&fy[w], cptr + 16, 16);
                    }
                }
                if constexpr (FP) {
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        if (gq[w] != kNoFar) {
                            const uint8_t* cptr = sblk + gq[w];
                            __builtin_memcpy(&gx[w], cptr, 16);
                            __builtin_memcpy(&gy[w], cptr + 16, 16);
                        }
                    }
                }
                cand_cur = nx;
            }
            M2P(8);  // next candidates
            // table entries two trips ahead (the first start-up trip: of the piece's first windows)
            const uint32_t tgt = warm == 2 ? nx : nx + 64 * NW;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t p = tgt + 64 * w + lane;
                const bool vld = p + 4 <= pe;
                const uint32_t A = p >> 2;
                const uint32_t d0 = ldata[vld ? A : 0u], d1 = ldata[vld ? A + 1 : 1u], d2 = ldata[vld ? A + 2 : 2u];
                const FarHash fh = far_hash(u64of(albyte(d1, d0, p), albyte(d2, d1, p)), fb, far_tag_mask(FB));
                const uint32_t ep = (base + p) >> kEpochLog;
                pf_tag[w] = fh.tag;
                pf_e[w] = ftab[vld ? (ep << tlog) + fh.idx : 0u];
                if constexpr (FP) {
                    pf_e2[w] = ftab[vld && ep > 0 ? ((ep - 1) << tlog) + fh.idx : 0u];   // (the first epoch has none: tested where the entry is used)
                }
            }
            pf_cur = tgt;
            M2P(3);  // next table entries (counted with the extension)
        }
        if (!run) { warm--; continue; }
#pragma unroll
        for (int w = 0; w < NW; w++) if (best[w] < 4) best[w] = 0;
        // ---- lazy matching: a position is dropped when one of the next three starts a match that is longer by
        //      more than its distance minus one (the idea of encode_l2.go:232-254); compared: length less token size ----
        uint64_t mask[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) {
            // g = gain + 2 (0 candidates -> 2), so that g - 1 and g - 2 cannot wrap.  skip <=> max(g[i+1], g[i+2] - 1, g[i+3] - 2) > g[i],
            // evaluated right to left with one lane shift per step (the shifts fold into the max / compare as DPP operands);
            // the look-ahead does not cross into the next window (0.01 % of output on the CPU model).
            const uint32_t cost = boff[w] > kMaxCopy2Offset ? 2u : boff[w] > kMaxCopy1Offset ? 1u : 0u;   // token size - 2
            const uint32_t g = best[w] >= 4 ? best[w] - cost : best[w] + 2;
            const uint32_t g1 = g - 1, g2 = g - 2;
            const uint32_t u = max(g1, uint32_t(__builtin_amdgcn_update_dpp(0, int(g2), 0x130 /* wave_shl:1 */, 0xf, 0xf, true)));
            const uint32_t v2 = max(g, uint32_t(__builtin_amdgcn_update_dpp(0, int(u), 0x130, 0xf, 0xf, true)));
            const uint32_t mx = uint32_t(__builtin_amdgcn_update_dpp(0, int(v2), 0x130, 0xf, 0xf, true));
            mask[w] = ballot64(best[w] >= 4 && mx <= g);
        }
        M2P(5);  // lazy
        uint64_t startmask[NW];
        uint32_t lenx[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) {
            lenx[w] = best[w];
            const uint32_t w0 = cur + 64 * w;
            uint64_t mm = mask[w];
            if (pos > w0) mm = pos - w0 >= 64 ? 0 : mm & (~0ull << (pos - w0));
            const uint32_t nxt = uint32_t(lane) + best[w];  // window-relative end of my candidate
            uint64_t sm = 0;
            uint32_t endrel = 0;
            if ((mm & ballot64(best[w] >= kLaneCap)) == 0) {
                // no candidate needs extending (most windows): every lane holds the mask of the positions that stay
                // selectable once its match is taken, and a selection step is find-first, two readlanes, and, bit-set
                const uint32_t r = (nxt < 64 ? nxt : 64u) - 1;            // candidates: nxt >= 4
                const uint64_t keep = (~1ull) << (r & 63);
                const uint32_t klo = uint32_t(keep), khi = uint32_t(keep >> 32);
                while (mm) {
                    const int i = int(ctz64(mm));
                    sm |= 1ull << i;
                    mm &= u64of(rdlane(klo, i), rdlane(khi, i));
                }
                if (sm) endrel = rdlane(nxt, 63 - int(__builtin_clzll(sm)));
            } else
            while (mm) {  // per selected match: find-first, one readlane, three mask operations
                const int i = int(ctz64(mm));
                uint32_t rel = rdlane(nxt, i);
                if (__builtin_expect(rel - uint32_t(i) >= kLaneCap, 0)) {  // cooperative forward extension, 512 bytes per round (long matches only)
                    uint32_t L = rel - uint32_t(i);
                    const uint32_t off = rdlane(boff[w], i);
                    const uint32_t mp = w0 + uint32_t(i);
                    const bool is_far = off > mp;
                    const uint32_t q_abs = base + mp - off;
                    uint32_t end = pe;
                    if (is_far) {
                        const uint32_t srcleft = kTile - (q_abs & (kTile - 1));
                        if (mp + srcleft < end) end = mp + srcleft;
                    }
                    if (is_far) {
#ifndef MLZ_M2_COOPK
#define MLZ_M2_COOPK 4
#endif
                        // the source is in global memory: four rounds' bytes (2 KiB) are requested at once — one round trip per 512 bytes made
                        // LevelBalanced without tile levels crawl on text whose phrases repeat at a distance (19.6 GB/s)
                        for (bool done = false; !done;) {
                            uint64_t theirs[MLZ_M2_COOPK];
#pragma unroll
                            for (uint32_t k = 0; k < MLZ_M2_COOPK; k++) {
                                const uint32_t rel8 = L + 512 * k + 8 * uint32_t(lane);
                                theirs[k] = ld64u(sblk + q_abs + (mp + rel8 < end ? rel8 : 0u));
                            }
#pragma unroll
                            for (uint32_t k = 0; k < MLZ_M2_COOPK && !done; k++) {
                                const uint32_t at = mp + L + 512 * k + 8 * uint32_t(lane);
                                uint32_t n = 0;
                                if (at < end) {
                                    n = common8(lds_ld64(ldata, at), theirs[k]);
                                    if (n > end - at) n = end - at;
                                }
                                const uint64_t stop = ballot64(n < 8);
                                if (stop) {
                                    const int j = int(ctz64(stop));
                                    L += 512 * k + 8 * uint32_t(j) + rdlane(n, j);
                                    done = true;
                                }
                            }
                            if (!done) L += 512 * MLZ_M2_COOPK;
                        }
                    } else
                    while (true) {
                        const uint32_t at = mp + L + 8 * uint32_t(lane);
                        uint32_t n = 0;
                        if (at < end) {
                            n = common8(lds_ld64(ldata, at), lds_ld64(ldata, at - off));
                            if (n > end - at) n = end - at;
                        }
                        const uint64_t stop = ballot64(n < 8);
                        if (stop) {
                            const int j = int(ctz64(stop));
                            L += 8 * uint32_t(j) + rdlane(n, j);
                            break;
                        }
                        L += 512;
                    }
                    lenx[w] = lane == i ? L : lenx[w];
                    rel = uint32_t(i) + L;
                }
                sm |= 1ull << i;
                endrel = rel;
                const uint32_t r64 = rel < 64 ? rel : 64;
                mm &= (~1ull) << (r64 - 1);
            }
            startmask[w] = sm;
            if (sm) pos = w0 + endrel;
        }
        M2P(6);  // walk
        // ---- token records ----
        bool any = false;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const uint64_t sm = startmask[w];
            if (sm) {
                any = true;
                const bool sel = (sm >> lane) & 1;
                const uint32_t idx = cnt + __builtin_amdgcn_mbcnt_hi(uint32_t(sm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(sm), 0));
                if (sel) rp[idx] = uint2{(cur + 64 * w + lane) | (lenx[w] << 16), boff[w]};
                cnt += uint32_t(__builtin_popcountll(sm));
            }
        }
        uint32_t next = cur + 64 * NW;
        if (pos > next) next = pos & ~63u;
        else if (!any) {
            uint32_t extra = (next - pos) >> kSkipShift;
            if (extra > 7) extra = 7;
            next += 64 * NW * extra;
        }
        cur = next;
        M2P(7);  // records
    }
    if (lane == 0) piece_cnt[pid] = cnt;
#ifdef MLZ_M2_PROF
    if (lane == 0) for (int i = 0; i < 10; i++) atomicAdd(&g_m2prof[i], m2pc[i]);
#endif
    if (scratch) {
        // The piece's tokens, by the wave that found them (serialize_piece): records read back through the L2 (my stores have completed, and what
        // this CU's L1 may hold of those lines is dropped), literals and the bytes in front of the matches from the tile's LDS copy — the other
        // waves only READ it —, the output ring in my own near table: nobody looks a position up in it any more.  Wave 0's table is 2 KiB with
        // 12-bit tables: a ring of half the size (more of its long literal runs take the token-by-token path).
        cnt = rdfirst(cnt);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("buffer_inv sc0" ::: "memory");
        uint8_t* ring = reinterpret_cast<uint8_t*>(table);
#ifndef MLZ_M2_SER_RING
#define MLZ_M2_SER_RING 4096   // (timing experiments: 2048 = one instantiation for all four waves)
#endif
        constexpr uint32_t kRingN = MLZ_M2_SER_RING;
        constexpr uint32_t kRing0 = 2 * kM2Unit >= kRingN ? kRingN : 2048u;
        static_assert(2 * kM2Unit >= 2048 && 4 * kM2Unit >= kRingN, "a wave's near table holds its serializer ring");
        uint32_t sz;
        if (kRing0 != kRingN && wv == 0) sz = serialize_piece<kRing0, true>(sblk, s, ldata, b, base, ps, tl, cnt, rp, ring, scratch + pid * kPieceScratch, lane);
        else sz = serialize_piece<kRingN, true>(sblk, s, ldata, b, base, ps, tl, cnt, rp, ring, scratch + pid * kPieceScratch, lane);
        if (lane == 0) piece_size[pid] = sz;
    }
}

// ---- serialize: token records -> token bytes of the piece (in the piece's scratch), piece_size ----
// serialize_piece: ONE wavefront turns the records of ONE piece into its token bytes.  Called at the end of match_tiles_kernel by the wave
// that made the records (round 6, option 21: the tile's bytes are still in LDS — literals and the bytes in front of a match come from
// there —, the records and the far sources' lines are still in this XCD's L2, the ring lives in the wave's own near table, which nobody needs
// any more; the kernel is bound by VALU issue with a quarter of its issue slots idle, and this pass is mostly waiting for loads), or by
// serialize_pieces_kernel (rounds 2-5: a kernel of its own that read source, records and a line per far token again: 518 MB of traffic).
// Returns the piece's size word (bit 31: stored raw).
template <uint32_t RING, bool LDSSRC>
__device__ __forceinline__ uint32_t serialize_piece(const uint8_t* __restrict__ sblk, const uint8_t* __restrict__ s, const uint32_t* ldata, const BlockInfo& b,
                                                    const uint32_t base, const uint32_t ps, const uint32_t tl, const uint32_t cnt, const uint2* __restrict__ rp,
                                                    uint8_t* ring, uint8_t* __restrict__ out, const int lane) {
    const uint32_t pe = ps + kPiece < tl ? ps + kPiece : tl;
    const uint32_t plen = pe - ps;
    const uint32_t raw = lit_header(plen).n + plen;
    const TileBytes<LDSSRC> data{ldata, s};
    TokenSinkT<RING, 1024> sink{ring, out, 0, 0, lane};
    uint32_t carry_end = ps, carry_off = 0;
    bool overflow = false;
    // The records of a round are requested a round ahead: what a token needs from the source (the bytes before the match and before its
    // copy, its literals) hangs on them, and two dependent round trips per round were half of this kernel's time.
    uint2 r_next = cnt ? rp[uint32_t(lane) < cnt ? uint32_t(lane) : 0u] : uint2{0, 0};
    for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
        sink.o = rdfirst(sink.o); sink.flushed = rdfirst(sink.flushed);
        carry_end = rdfirst(carry_end); carry_off = rdfirst(carry_off);
        const uint32_t nhere = cnt - c0 < 64 ? cnt - c0 : 64;
        const bool have = uint32_t(lane) < nhere;
        uint2 r = r_next;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(r.x), "+v"(r.y));   // (the first use of the loaded value: the compiler's own wait lands here, before the next request)
        {
            const uint32_t qn = c0 + 64 + uint32_t(lane);
            r_next = rp[qn < cnt ? qn : c0];   // (c0 < cnt: always a record of this piece)
        }
        const uint32_t mp = r.x & 0xffffu, len0 = r.x >> 16, off = r.y;
        const uint32_t end_me = mp + len0;
        uint32_t prev_end = uint32_t(__builtin_amdgcn_update_dpp(0, int(end_me), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
        uint32_t prev_off = uint32_t(__builtin_amdgcn_update_dpp(0, int(off), 0x138, 0xf, 0xf, true));
        if (lane == 0) { prev_end = carry_end; prev_off = carry_off; }
        // backward extension: how many of the (at most 8) pending literal bytes before the match also agree
        const uint32_t pa = base + mp, qa = pa - off;
        uint32_t room = mp - prev_end;
        if (room > 8) room = 8;
        const uint32_t sroom = off <= mp ? mp - off : (qa & (kTile - 1));
        if (room > sroom) room = sroom;
        const bool bk_ok = have && room > 0 && qa >= 8;
        uint64_t xb;
        if constexpr (LDSSRC) {
            // the 8 bytes in front of the match come from the tile's LDS copy (mp >= room > 0; a match in the tile's first 8 bytes reads what lies
            // in front of the tile from memory), those in front of its source from LDS as well when the source lies in the tile
            const bool mine_lds = mp >= 8, src_lds = off <= mp && mp - off >= 8;
            const uint64_t a8 = lds_ld64(ldata, bk_ok && mine_lds ? mp - 8 : 0u), c8 = lds_ld64(ldata, bk_ok && src_lds ? mp - off - 8 : 0u);
            const bool ga = bk_ok && !mine_lds, gc = bk_ok && !src_lds;
            uint64_t ag = 0, cg = 0;
            if (ga) ag = ld64u(sblk + (pa - 8));
            if (gc) cg = ld64u(sblk + (qa - 8));
            xb = (mine_lds ? a8 : ag) ^ (src_lds ? c8 : cg);
        } else
            xb = ld64u(sblk + (bk_ok ? pa - 8 : 0u)) ^ ld64u(sblk + (bk_ok ? qa - 8 : 0u));
        uint32_t bk = xb ? uint32_t(__builtin_clzll(xb)) >> 3 : 8;
        if (bk > room) bk = room;
        if (!bk_ok) bk = 0;
        const uint32_t ms = mp - bk, len = len0 + bk;
        const uint32_t lits = have ? ms - prev_end : 0;
        const bool is_rep = have && off == prev_off;
        Emit e{{0, 0}, {0, 0}};
        if (ballot64(have && !plan_emit_is_short(lits, len, is_rep)) == 0) {
            if (have) e = plan_emit_short(lits, off, len, is_rep);
        } else {
            if (have) e = plan_emit(lits, off, len, is_rep);
        }
        const uint32_t pre_n = have ? e.pre.n : 0, post_n = have ? e.post.n : 0;
        const uint32_t sz = pre_n + lits + post_n;
        const uint32_t incl = wave_incl_scan_u32(sz);
        const uint32_t total = rdlane(incl, 63);
        if (sink.o + total > raw) { overflow = true; break; }
        if ((sink.o - sink.flushed) + total <= RING - 64) {
            // ---- parallel layout: every lane places its token ----
            const uint32_t toff = sink.o + incl - sz;
            const uint32_t pbase = toff + pre_n + lits;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if (q < pre_n) ring[(toff + q) & (RING - 1)] = uint8_t(e.pre.bits >> (8 * q));
                if (q < post_n) ring[(pbase + q) & (RING - 1)] = uint8_t(e.post.bits >> (8 * q));
            }
            if (ballot64(pre_n > 4 || post_n > 4)) {
                for (uint32_t q = 4; q < 8; q++) {
                    if (q < pre_n) ring[(toff + q) & (RING - 1)] = uint8_t(e.pre.bits >> (8 * q));
                    if (q < post_n) ring[(pbase + q) & (RING - 1)] = uint8_t(e.post.bits >> (8 * q));
                }
            }
            // literals: up to 16 per token from two 8-byte loads, longer runs by the whole wave
            const bool fast = lits > 0 && lits <= 16 && uint64_t(base) + prev_end + 16 <= b.src_len;
            const uint8_t* lp = s + (fast ? prev_end : ps);
            const bool can16 = uint64_t(base) + ps + 16 <= b.src_len;
            uint64_t la = 0, lb = 0;
            if constexpr (LDSSRC) { const uint32_t lo = fast ? prev_end : ps; la = lds_ld64(ldata, lo); lb = lds_ld64(ldata, lo + 8); }   // (the LDS copy is zero-padded behind the tile)
            else if (can16) { la = ld64u(lp); lb = ld64u(lp + 8); }
            const uint32_t lbase = toff + pre_n;
            // exact-size stores (8 + 8, or 4 / 2 / 1 for what is left): at most five per token — a byte per lane and iteration
            // was 16 iterations whenever one lane of the wave had 16 literals, a quarter of this kernel's time.  The few runs
            // that wrap around the end of the ring go byte by byte.
            const uint32_t lpos = lbase & (RING - 1);
            const bool wraps = fast && lpos + lits > RING;
            if (fast && !wraps) {
                uint8_t* lp8 = ring + lpos;
                uint64_t cur = la;
                uint32_t left = lits;
                if (left >= 8) { __builtin_memcpy(lp8, &la, 8); lp8 += 8; cur = lb; left -= 8; }
                if (left == 8) {
                    __builtin_memcpy(lp8, &lb, 8);
                } else {
                    if (left & 4) { const uint32_t x = uint32_t(cur); __builtin_memcpy(lp8, &x, 4); lp8 += 4; cur >>= 32; }
                    if (left & 2) { const uint16_t x = uint16_t(cur); __builtin_memcpy(lp8, &x, 2); lp8 += 2; cur >>= 16; }
                    if (left & 1) *lp8 = uint8_t(cur);
                }
            }
            for (uint32_t q = 0; ballot64(wraps && q < lits); q++) {
                const uint64_t wsel = q < 8 ? la : lb;
                if (wraps && q < lits) ring[(lbase + q) & (RING - 1)] = uint8_t(wsel >> (8 * (q & 7)));
            }
            uint64_t lm = ballot64(lits > 0 && !fast);
            while (lm) {
                const int i = int(ctz64(lm));
                lm &= lm - 1;
                const uint32_t n = rdlane(lits, i), from = rdlane(prev_end, i), at = rdlane(lbase, i);
                for (uint32_t q = lane; q < n; q += 64) ring[(at + q) & (RING - 1)] = data.ld8(from + q);
            }
            sink.o += total;
            sink.flush_ready();
        } else {
            // ---- a literal run too long for the ring: token by token, the wave cooperating on each ----
            for (uint32_t t = 0; t < nhere; t++) {
                Hdr hp, hq;
                hp.bits = (uint64_t(rdlane(uint32_t(e.pre.bits >> 32), int(t))) << 32) | rdlane(uint32_t(e.pre.bits), int(t));
                hp.n = rdlane(pre_n, int(t));
                hq.bits = (uint64_t(rdlane(uint32_t(e.post.bits >> 32), int(t))) << 32) | rdlane(uint32_t(e.post.bits), int(t));
                hq.n = rdlane(post_n, int(t));
                const uint32_t n = rdlane(lits, int(t)), from = rdlane(prev_end, int(t));
                sink.put_hdr(hp);
                if (n) sink.put_lits(data, from, n);
                sink.put_hdr(hq);
                sink.flush_ready();
            }
        }
        carry_end = rdlane(end_me, int(nhere - 1));
        carry_off = rdlane(off, int(nhere - 1));
    }
    if (!overflow && carry_end < pe) {
        const uint32_t lits = pe - carry_end;
        const Hdr hdr = lit_header(lits);
        // (>=: a piece that would only EQUAL its raw form is stored raw as well — without first copying its bytes to the scratch,
        //  which is all this kernel did for incompressible input: a piece without a single match is exactly that case)
        if (sink.o + hdr.n + lits >= raw) overflow = true;
        else { sink.put_hdr(hdr); sink.put_lits(data, carry_end, lits); }
    }
    if (!overflow) sink.finish();
    return (overflow || sink.o >= raw) ? (raw | 0x80000000u) : sink.o;
}

__global__ __launch_bounds__(256) void serialize_pieces_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                               const uint32_t* __restrict__ tile_block, const uint2* __restrict__ recs,
                                                               const uint32_t* __restrict__ piece_cnt, uint8_t* __restrict__ scratch,
                                                               uint32_t* __restrict__ piece_size) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = rdfirst(uint32_t(tid) >> 6);
    uint8_t* ring = smem + wv * kSerRing;
    const uint32_t gt = blockIdx.x;
    const uint32_t bi = tile_block[gt];
    const BlockInfo b = blocks[bi];
    const uint32_t tib = gt - b.first_tile;
    const uint32_t base = tib << kTileLog;
    const uint8_t* sblk = src_base + b.src_off;
    const uint8_t* s = sblk + base;
    const uint32_t tl = uint32_t(b.src_len - base < kTile ? b.src_len - base : kTile);
    const uint32_t ps = wv << kPieceLog;
    const size_t pid = size_t(gt) * kSub + wv;
    if (ps >= tl) {
        if (lane == 0) piece_size[pid] = 0;
        return;
    }
    const uint32_t sz = serialize_piece<kSerRing, false>(sblk, s, nullptr, b, base, ps, tl, piece_cnt[pid], recs + pid * kRecPerPiece, ring,
                                                         scratch + pid * kPieceScratch, lane);
    if (lane == 0) piece_size[pid] = sz;
}

// ---- gather the pieces' token streams (or raw bytes) into the final block: one workgroup per tile, one wave per piece ----
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint32_t n, int lane) {
    uint32_t head = uint32_t((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (head > n) head = n;
    if (uint32_t(lane) < head) d[lane] = s[lane];
    d += head; s += head; n -= head;
    const uint32_t nv = n >> 4;
    uint4* dv = reinterpret_cast<uint4*>(d);
    for (uint32_t k = lane; k < nv; k += 64) {
        uint4 x;
        __builtin_memcpy(&x, s + 16 * size_t(k), 16);
        dv[k] = x;
    }
    const uint32_t done = nv << 4;
    if (uint32_t(lane) < n - done) d[done + lane] = s[done + lane];
}

// LAYOUT = true (round 6): the kernel also does encode_layout_kernel's work — every tile's workgroup adds up the piece sizes of ITS block (at most 1024 words
// out of the L2: what dec_index2 does with its segments' words), which gives it the block's total (stored or not, encode_l1.go:60) and the offset of its own
// pieces; the block's first tile writes the header and the length.  One launch (7 us) less per encode call.  Only for batches whose every block has tiles and
// room (the host knows): an empty, oversize or too tightly bounded block still goes through encode_layout_kernel.
template <bool LAYOUT>
__global__ __launch_bounds__(256) void encode_gather2_kernel(const uint8_t* __restrict__ src_base, const BlockInfo* __restrict__ blocks,
                                                             const uint32_t* __restrict__ tile_block, const uint8_t* __restrict__ scratch,
                                                             const uint32_t* __restrict__ piece_size, const uint32_t* __restrict__ piece_out,
                                                             uint8_t* __restrict__ dst_base, const uint32_t* __restrict__ flags, int with_header,
                                                             int level, int64_t* __restrict__ out_len) {
    const uint32_t gt = blockIdx.x;
    const uint32_t bi = tile_block[gt];
    const BlockInfo b = blocks[bi];
    const uint32_t tib = gt - b.first_tile;
    uint32_t f, my_out = 0;
    if constexpr (LAYOUT) {
        __shared__ uint32_t red[8];
        const uint32_t n_units = b.n_tiles << kSubLog, mine0 = tib << kSubLog;
        const uint32_t* ps_ = piece_size + (size_t(b.first_tile) << kSubLog);
        uint32_t all = 0, before = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {   // (at most 256 tiles x 4 pieces = 1024 units per block)
            const uint32_t u = threadIdx.x + 256 * q;
            const uint32_t v = u < n_units ? ps_[u] & 0x7fffffffu : 0u;
            all += v; before += u < mine0 ? v : 0u;
        }
        const uint32_t a_incl = wave_incl_scan_u32(all), b_incl = wave_incl_scan_u32(before);
        if ((threadIdx.x & 63) == 63) { red[threadIdx.x >> 6] = a_incl; red[4 + (threadIdx.x >> 6)] = b_incl; }
        __syncthreads();
        const uint32_t total = red[0] + red[1] + red[2] + red[3];
        my_out = red[4] + red[5] + red[6] + red[7];
        const uint64_t n = b.src_len;
        uint32_t hdr = 0;
        uint8_t hb[8];
        if (with_header) { hb[0] = 0; hdr = 1 + put_uvarint(hb + 1, n); }
        const int64_t limit = int64_t(n) - int64_t(n >> 5) - 6;  // dstLimit, encode_l1.go:60
        const bool stored = level == 0 || n < kMinNonLiteralBlock || int64_t(total) > limit;
        f = stored ? 1u : 0u;
        my_out += hdr;
        if (tib == 0 && threadIdx.x == 0) {   // the block's header and length (encode_layout_kernel's tail)
            uint8_t* dst0 = b.mirror ? reinterpret_cast<uint8_t*>(b.mirror) : dst_base + b.dst_off;
            if (!with_header) out_len[bi] = stored ? 0 : int64_t(total);
            else if (stored) { dst0[0] = 0; dst0[1] = 0; out_len[bi] = int64_t(n) + 2; }
            else { for (uint32_t k = 0; k < hdr; k++) dst0[k] = hb[k]; out_len[bi] = int64_t(hdr) + total; }
        }
    } else {
        f = flags[bi];
        if (f == 2) return;
    }
    const uint32_t base = tib << kTileLog;
    const uint32_t tl = uint32_t(b.src_len - base < kTile ? b.src_len - base : kTile);
    uint8_t* dst = b.mirror ? reinterpret_cast<uint8_t*>(b.mirror) : dst_base + b.dst_off;  // pinned caller memory: written in place
    const uint8_t* s = src_base + b.src_off + base;
    if (f == 1) {  // stored block: 00 00 raw
        if (with_header && tl) wg_copy(dst + 2 + base, s, tl, threadIdx.x, 256);
        return;
    }
    const int lane = threadIdx.x & 63;
    const uint32_t wv = rdfirst(uint32_t(threadIdx.x) >> 6);
    const uint32_t ps = wv << kPieceLog;
    if (ps >= tl) return;
    const uint32_t plen = (ps + kPiece < tl ? ps + kPiece : tl) - ps;
    const size_t pid = size_t(gt) * kSub + wv;
    const uint32_t sz = piece_size[pid];
    uint32_t pout;
    if constexpr (LAYOUT) {   // my tile's offset + the pieces of the tile before mine
        pout = my_out;
        for (uint32_t q = 0; q < wv; q++) pout += piece_size[size_t(gt) * kSub + q] & 0x7fffffffu;
    } else pout = piece_out[pid];
    uint8_t* d = dst + pout;
    if (sz & 0x80000000u) {  // raw piece: one literal token
        const Hdr h = lit_header(plen);
        if (uint32_t(lane) < h.n) d[lane] = uint8_t(h.bits >> (8 * lane));
        wave_copy(d + h.n, s + ps, plen, lane);
    } else {
        wave_copy(d, scratch + pid * kPieceScratch, sz, lane);
    }
}

}  // namespace mlz
