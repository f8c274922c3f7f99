// mlz_decode_general.hip.inc — decode of "general" blocks (other encoders' streams and this library's LevelBalanced:
// a copy may read any earlier byte, so the tile-level schedule of the exec pass degenerates into one
// serial chain per block).  Included by mlz_hip.hip after mlz_decode_exec.hip.inc.
//
// Round 4 design (rounds 1-3 kept a 32-bit source word per OUTPUT BYTE in global memory and shortened the chains by
// pointer-jumping rounds over all of them: 4 B of workspace and ~7 random 128-byte line fetches per copy token,
// 1.26 ms of the 2.2 ms a 100 MB stream took).  Now the work is split by what it depends on:
//
//   role E ("explain", every tile of every general block, any order, any CU): the tile's tokens are parsed a lane per
//          token (the token list of D3) and every output byte of the tile is reduced IN LDS to a 16-bit pointer to its
//          TERMINAL byte inside the tile — a literal byte (copied from the stream into the tile image right away) or a
//          byte that a copy token reads from an EARLIER tile ("external": the token leaves one entry {source position,
//          pool slot, length <= 8} per 8 bytes).  Terminals live in the tile's POOL: literals at the bottom, slots at
//          the top.  Chains inside the tile are jumped to their end in LDS (map[j] = map[map[j]], <= 15 rounds of 16-bit
//          words).  Out: 2 B of map per byte, the pool's literal bytes, ~1.4 entries of
//          8 B per copy token — and the tile's ready flag.
//   role S ("settle", one workgroup per general block, the block's tiles IN ORDER): every external entry now reads
//          FINAL bytes — the two preceding tiles are kept in LDS (a ring of three tile images), older ones come from dst
//          with one 8-byte load per entry — into its aligned 8-byte slot of the pool, then every byte takes the value of its
//          terminal (an LDS gather from the pool through the map) and the tile is flushed.  One request per RUN, no per-byte
//          global traffic, no rounds.
//
// One launch: workgroups [0, nE) take E tickets (tiles in position-major order over the general blocks, so that every
// block's chain can start at once), workgroups [nE, nE + nS) settle blocks.  E never waits; S waits only for E's flags;
// workgroups are dispatched in index order, so the S workgroups cannot keep an E workgroup from starting — there is NO
// grid barrier and no co-residency requirement any more (rounds 2-3: one persistent launch that needed every CU).
// Every wait is still bounded (spin_limit): a flag that never comes fails the block with -MLZ_ERR_HIP, not the GPU.
// Measurements, the steps from 14 to 5.3 us per settled tile and what was tried and not kept: DESIGN.md section 4.
//
// The reference (decode.go:178-622) is a sequential loop; this is its data-parallel restatement.

namespace mlz {

constexpr int kGenThreads = 1024;
constexpr int kGenWaves = kGenThreads / 64;
constexpr uint32_t kExtMax = 8;                               // bytes per external entry (one 8-byte pool slot)
constexpr uint32_t kExtPerTile = kTile / kExtMax + 2;         // entries that splitting long copies can add to a tile's tokens
constexpr uint32_t kGenMaxTiles = kMaxBlockSize >> kTileLog;
constexpr uint32_t kPool = kTile;                             // a tile's terminal bytes never outnumber its bytes
constexpr uint32_t kGenLds = 4 * kTile + 256 + 12 * kGenMaxTiles;   // E: map (2 x kTile) + pool; S: ring of three tile images + pool; + shared words + S's per-tile records
static_assert(kTile <= 32768, "15-bit in-tile pointers / pool offsets");

struct GenCtl {
    uint32_t n_general;   // blocks flagged general by D3 (first word: mlz_get_counter 2 reads it)
    uint32_t e_ticket;    // role E: next ticket
    uint32_t max_tiles;   // D3d: the largest tile count among the general blocks
    uint32_t failed;      // somebody gave up waiting (debug)
    uint32_t done_wgs;    // workgroups of dec_general_kernel that have left (the last one writes the batch's results)
    uint32_t team;        // D3d: tiles of a block that role S settles side by side (1, 2 or 4: team_of, the smallest of the batch's general blocks)
};

constexpr uint32_t kL0Done = 2;   // what dec_level0_kernel leaves in a finished tile's done flag: "done" to the exec pass (non-zero), "not explained" to role S (bit 0)
struct ExtEnt { uint32_t src, where; };   // source position in the block's output; pool offset | (length - 1) << 16
struct GenTile { uint32_t n_ext, lit_top; };   // role E -> role S, per tile: entries (bit 31: byte-packed pool, exact stores), literal bytes at the pool's bottom

// 16 bytes at p[i..i+16), bytes at or beyond n read as zero (never touches memory >= p + n)
__device__ __forceinline__ uint4 ld128_clamped(const uint8_t* p, uint32_t i, uint32_t n) {
    uint4 x;
    if (uint64_t(i) + 16 <= n) { __builtin_memcpy(&x, p + i, 16); return x; }
    const uint64_t lo = ld64_clamped(p, i, n), hi = ld64_clamped(p, i + 8, n);
    x.x = uint32_t(lo); x.y = uint32_t(lo >> 32); x.z = uint32_t(hi); x.w = uint32_t(hi >> 32);
    return x;
}

// the first len (1..16) bytes of x to LDS at p, any alignment, nothing beyond p + len
__device__ __forceinline__ void lds_store_exact(uint8_t* p, uint4 x, uint32_t len) {
    if (len >= 16) { __builtin_memcpy(p, &x, 16); return; }
    uint64_t lo = uint64_t(x.x) | (uint64_t(x.y) << 32);
    if (len & 8) { __builtin_memcpy(p, &lo, 8); p += 8; lo = uint64_t(x.z) | (uint64_t(x.w) << 32); }
    if (len & 4) { const uint32_t w = uint32_t(lo); __builtin_memcpy(p, &w, 4); p += 4; lo >>= 32; }
    if (len & 2) { const uint16_t h = uint16_t(lo); __builtin_memcpy(p, &h, 2); p += 2; lo >>= 16; }
    if (len & 1) *p = uint8_t(lo);
}

__device__ __forceinline__ void store8_wt(void* p, uint64_t v) { __hip_atomic_store(reinterpret_cast<uint64_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store16_wt_a(void* p, uint4 v) {   // 16-byte write-through store, 64-bit lane address
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(x) : "memory");
}

// values that ARE the same in every lane, moved to scalar registers (the compiler cannot tell for what it loaded through a vector load:
// a block's record would otherwise sit in ~20 vector registers of every lane, and both roles run short of those)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ __forceinline__ uint64_t uni(uint64_t v) { return (uint64_t(uni(uint32_t(v >> 32))) << 32) | uni(uint32_t(v)); }   // (the builtin returns a signed int: through uni(uint32_t), or the low half is sign-extended over the high one)
// A 32-bit lane offset the optimizer cannot see through: `scalar base + opaque(offset)` stays a scalar-base access with a 32-bit lane
// offset — without it the loop optimizer turns every such access into a 64-bit lane pointer of its own that it carries, and spills, across the loop.
__device__ __forceinline__ uint32_t opaque(uint32_t x) { asm volatile("" : "+v"(x)); return x; }
// (Pointers are NOT passed through these: an integer round trip loses the address space and every access through the result becomes a
//  FLAT instruction with a 64-bit lane address.  A uniform pointer is written as `kernel argument + uni(offset)`: scalar base, global.)

#ifndef MLZ_GEN_DEBUG
#define MLZ_GEN_DEBUG 0
#endif
#ifndef MLZ_GEN_PROF
#define MLZ_GEN_PROF 0    // debug build: phase clocks (100 MHz) of the first E and the first S workgroup, printed by the kernel
#endif
#define MLZ_GP(i) do { if (MLZ_GEN_PROF) { const unsigned long long t_now = __builtin_amdgcn_s_memrealtime(); gp[i] += t_now - gp_prev; gp_prev = t_now; } } while (0)
#ifndef MLZ_GEN_EP
#define MLZ_GEN_EP 3      // role S: external entries per thread that are prefetched (x 1024 threads per tile; the rest take a plain loop)
#endif
#ifndef MLZ_GEN_FORCE_PACKED
#define MLZ_GEN_FORCE_PACKED 0   // tests: every tile takes the byte-packed pool (the fallback for tiles whose slots would not fit)
#endif

// One launch, two roles: workgroups [0, nE) explain (role E), workgroups [nE, nE + nS) settle (role S).  Role E never waits; role S
// waits only for role E's flags; workgroups are dispatched in index order, so a settling workgroup cannot keep an explaining one from
// starting: there is no grid barrier and no co-residency requirement (rounds 2-3: one persistent launch that needed every CU), and
// every wait is bounded.  (Mid-round 4 the roles were two kernels on two streams for a while — blamed for a register-allocation
// fault that turned out to be a sign extension in `uni` —: the event hand-over between the streams cost every decode call, with or
// without general blocks, ~40 us.)
// L0 = true (dec_level0_kernel, round 6): role E only, on ONE tile (tile l0_t of block l0_bi: a level-0 candidate, see the kernel), and instead of
// leaving map and pool for role S the tile is finished here — a level-0 tile reads nothing but itself, so every byte's terminal is a literal of the tile:
// gather through the map, flush, raise the exec pass's done flag.  A tile that turns out to read an earlier one, or to hold a bad token, is left alone —
// found while the tile is parsed, before its first store —: no byte, no flag, no status; the exec pass or the general pass decodes it as if nobody had tried.
template <bool L0>
__device__ __forceinline__ void dec_general_body(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base,
                                                                  const BlockInfo* __restrict__ blocks, DecBlock* __restrict__ dec,
                                                                  const uint32_t* __restrict__ tok_pos, const uint32_t* __restrict__ round_d,
                                                                  const uint32_t* __restrict__ round_rep, const TileStart* __restrict__ tile_start,
                                                                  const uint32_t* __restrict__ gen_list, uint16_t* __restrict__ gmap, uint8_t* __restrict__ gpool,
                                                                  ExtEnt* __restrict__ ext_all, GenTile* __restrict__ tile_info,
                                                                  uint32_t* __restrict__ tile_ready, GenCtl* __restrict__ ctl, uint32_t nE, uint32_t nS,
                                                                  uint32_t spin_limit, uint32_t force_packed,
                                                                  uint32_t l0_bi = 0, uint32_t l0_t = 0, uint32_t* __restrict__ tile_done = nullptr) {
    const uint32_t ngen = L0 ? 0u : __hip_atomic_load(&ctl->n_general, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    extern __shared__ __attribute__((aligned(16))) uint8_t gl[];
    // shared words: [0] ticket / flag verdict, [1] entries, [2] failure, [3] literal bytes.  (Not `volatile`: the address-space inference skips
    // volatile accesses and they become FLAT instructions; every hand-over of these words goes through a barrier anyway.)
    uint32_t* shw = reinterpret_cast<uint32_t*>(gl + 4 * kTile);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long gp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gp_prev = MLZ_GEN_PROF ? __builtin_amdgcn_s_memrealtime() : 0;
    uint32_t gp_tiles = 0, gp_ext = 0;
    // a tile's slice of the entry array: a block's slices start at (first_seg << kSegLog) + first_tile * kExtPerTile + 64 * block, tile t's at rank(t) + t * kExtPerTile
    auto ext_index = [](uint32_t first_seg, uint32_t first_tile, uint32_t bi, uint32_t t, uint32_t rank) -> uint64_t {
        return (uint64_t(first_seg) << kSegLog) + uint64_t(first_tile) * kExtPerTile + 64 * uint64_t(bi) + rank + uint64_t(t) * kExtPerTile;
    };

    // (a settling workgroup that has no unit to settle — fewer blocks x team than settling workgroups — explains instead: tickets are drawn, not dealt)
    // (L0 reads no word of ctl: the verdict workgroup of its launch is writing them)
    const uint32_t team0 = L0 ? 1u : uni(__hip_atomic_load(&ctl->team, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (L0 || blockIdx.x < nE || blockIdx.x - nE >= ngen * (team0 ? team0 : 1u)) {
        // =========================== role E ===========================
        // Every output byte of the tile -> the offset of its TERMINAL in the tile's pool: a literal byte (laid down here, from the
        // stream, at the pool's bottom) or a byte an external entry will bring (an 8-byte slot per entry at the pool's top, filled by
        // role S).  LDS: map[kTile] of 16-bit words (bit 15: "pool offset", else an in-tile position still to be followed), the pool.
        uint16_t* mp = reinterpret_cast<uint16_t*>(gl);
        uint8_t* pool = gl + 2 * kTile;
        uint32_t* toktab = reinterpret_cast<uint32_t*>(gl + 3 * kTile);   // the token table of mlz_toktab.h (role E leaves the fourth 32 KiB alone)
        for (uint32_t i = tid; i < 256; i += kGenThreads) toktab[i] = g_toktab.e[i];
        const uint32_t maxT = L0 ? 1u : __hip_atomic_load(&ctl->max_tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // tickets: groups of nS blocks (a group = the blocks the S workgroups settle side by side), position-major inside a group
        const uint32_t teamE = team0;
        const uint32_t nSb = nS / (teamE ? teamE : 1u);       // blocks role S settles side by side (a team of workgroups per block)
        const uint32_t per_group = L0 ? 1u : maxT * nSb;
        const uint32_t total_tickets = L0 ? 1u : per_group * ((ngen + nSb - 1) / nSb);
        for (uint32_t turn = 0;; turn++) {
            MLZ_GP(7);
            uint32_t t, bi;
            if (L0) {   // the one tile it was called for
                if (turn) break;
                t = l0_t; bi = l0_bi;
            } else {
                __syncthreads();
                if (tid == 0) shw[0] = atomicAdd(&ctl->e_ticket, 1u);
                __syncthreads();
                const uint32_t tk = shw[0];
                if (tk >= total_tickets) break;
                const uint32_t rem = tk % per_group;
                const uint32_t slot = (tk / per_group) * nSb + rem % nSb;
                t = rem / nSb;
                if (slot >= ngen) continue;
                bi = uni(gen_list[slot]);
            }
            const uint32_t dlen = uni(dec[bi].dlen), clen = uni(dec[bi].clen), ntok = uni(dec[bi].ntok);
            if (t >= ((dlen + kTile - 1) >> kTileLog)) continue;
            const uint32_t first_tile = uni(blocks[bi].first_tile), first_seg = uni(blocks[bi].first_seg);
            const uint32_t gt = first_tile + t;
            const uint32_t tstart = t << kTileLog;
            const uint32_t tend = tstart + kTile < dlen ? tstart + kTile : dlen;
            const uint32_t n = tend - tstart;
            const uint8_t* src = src_base + uni(uint64_t(blocks[bi].src_off) + dec[bi].body_off);
            const uint32_t rank0 = uni(tile_start[gt].rank);
            const size_t cofs = size_t(first_seg) << (kSegLog - 6);
            const uint32_t* tpos = tok_pos + (size_t(first_seg) << kSegLog);
            const uint32_t* rdv = round_d + cofs;
            const uint32_t* rrv = round_rep + cofs;
            uint32_t r_last = ntok - 1;
            if (tend < dlen) r_last = uni(tile_start[gt + 1].rank);  // the token covering the next tile's first byte
            const uint32_t j_first = rank0 >> 6, j_last = r_last >> 6;
            gp_tiles++;
            ExtEnt* ext = L0 ? nullptr : ext_all + uni(ext_index(first_seg, first_tile, bi, t, rank0));
            if (MLZ_GEN_DEBUG && tid == 0) printf("E wg %u turn %u bi %u t %u gt %u dlen %u clen %u ntok %u rank0 %u r_last %u first_seg %u first_tile %u ext %p src %p tpos %p\n", blockIdx.x, turn, bi, t, gt, dlen, clen, ntok, rank0, r_last, first_seg, first_tile, (void*)ext, (const void*)src, (const void*)tpos);
            bool tile_failed = false;
            uint32_t packed = (MLZ_GEN_FORCE_PACKED || force_packed) ? 1u : 0u;   // 0: 8-byte slots from the pool's top; 1: byte-packed behind the literals (always fits)
            for (;;) {
                // ---- markers: 0 = none; bit 15 set: a terminal run starts here, map[j] = pool offset (j + marker) mod 2^15; else the offset of the in-tile copy that starts here ----
                __syncthreads();
                for (uint32_t q = tid; q < 2 * kTile / 16; q += kGenThreads) reinterpret_cast<uint4*>(mp)[q] = uint4{0u, 0u, 0u, 0u};
                if (tid == 0) { shw[1] = 0; shw[2] = 0; shw[3] = 0; shw[4] = 0; }
                __syncthreads();
                {
                    // ONE LANE PER TOKEN, rounds of 64 consecutive entries of the block's token list dealt to the waves round-robin (as in the
                    // exec pass); the round record gives the output position of the round's first token and the repeat offset in force there.
                    // A wave takes its rounds FOUR at a time: the four position loads, then the four stream-byte loads, then the parses, then
                    // the literal bytes — four dependent memory round trips per batch instead of three per round (a workgroup is all a CU holds).
                    constexpr uint32_t NB = 4;
                    const uint32_t wvu = rdfirst(uint32_t(wv));
                    bool failed = false;
                    for (uint32_t jb = j_first + wvu; jb <= j_last && !failed; jb += NB * uint32_t(kGenWaves)) {
                        uint32_t spv[NB], Db[NB], Rp[NB];
                        uint64_t wd[NB];
#pragma unroll
                        for (uint32_t u = 0; u < NB; u++) {
                            const uint32_t j = jb + u * uint32_t(kGenWaves), jj = j <= j_last ? j : j_last;
                            const uint32_t R = (jj << 6) + uint32_t(lane);
                            spv[u] = tpos[R < ntok ? R : ntok - 1];   // stream position of my token
                            Db[u] = rdv[jj]; Rp[u] = rrv[jj];
                        }
#pragma unroll
                        for (uint32_t u = 0; u < NB; u++) wd[u] = ld64_clamped(src, spv[u], clen);
                        uint4 lx[NB];
                        uint32_t lnl[NB], ldo[NB];
#pragma unroll
                        for (uint32_t u = 0; u < NB; u++) {
                            const uint32_t j = jb + u * uint32_t(kGenWaves);
                            lnl[u] = 0; ldo[u] = 0; lx[u] = uint4{0u, 0u, 0u, 0u};
                            if (j > j_last || failed) continue;
                            const uint32_t R = (j << 6) + uint32_t(lane);
                            const bool is_tok = R < ntok;
                            const uint32_t sp = spv[u];
                            Tok tk_;
                            {
                                const uint32_t tt = toktab[uint32_t(wd[u]) & 0xff];
                                const uint32_t ol = tok_olen(wd[u], tt);
                                tk_.lit = tok_lit(ol, tt); tk_.cp = ol - tk_.lit; tk_.off = tok_off(uint32_t(wd[u]), tt); tk_.hdr = tok_adv(uint32_t(wd[u]), tt) - tk_.lit;
                            }
                            const uint32_t lit = is_tok ? tk_.lit : 0, len = is_tok ? tk_.cp : 0;
                            const uint32_t olen = lit + len;
                            const uint32_t incl = wave_incl_scan(olen);
                            const uint32_t dtok = Db[u] + incl - olen;
                            // the offset in force: my own, or the last explicit one before me (in this round, else carried in)
                            const uint64_t expl = ballot64(is_tok && tk_.off != 0);
                            const uint64_t before = expl & ((1ull << lane) - 1);
                            const uint32_t prev_off = __shfl(tk_.off, before ? 63 - __builtin_clzll(before) : 0);
                            const uint32_t off = tk_.off ? tk_.off : (before ? prev_off : Rp[u]);
                            const uint32_t dc = dtok + lit;
                            const bool invalid = len != 0 && (off == 0 || off > dc || uint64_t(dc) + len > dlen);
                            const uint32_t lit_s = sp + tk_.hdr;   // stream position of my token's first literal
                            const bool lit_bad = lit != 0 && (uint64_t(lit_s) + lit > clen || uint64_t(dtok) + lit > dlen);
                            const uint64_t b_inv = ballot64(invalid);
                            if (b_inv || ballot64(lit_bad)) {
                                if (lane == 0) { if (!L0) atomicExch(reinterpret_cast<int*>(&dec[bi].status), int(1 | ((b_inv ? 5 : 4) << 8))); shw[2] = 1; }   // (L0: the exec pass gives the verdict)
                                failed = true;
                                continue;
                            }
                            // literal run and copy, clipped to the tile
                            const uint32_t l0 = dtok > tstart ? dtok : tstart, l1 = dc < tend ? dc : tend;
                            const bool has_lit = lit != 0 && l0 < l1;
                            const uint32_t c0 = dc > tstart ? dc : tstart, cend = dc + len, c1 = cend < tend ? cend : tend;
                            const bool has_cp = len != 0 && c0 < c1;
                            // byte j of the copy reads j - off: an EARLIER tile's byte (final when this tile is settled) while j < tstart + off
                            const uint32_t xlim = tstart + off;                       // (off <= dc <= 8 MiB: no overflow)
                            const uint32_t e1 = c1 < xlim ? c1 : xlim;
                            const uint32_t n_ext = has_cp && c0 < e1 ? e1 - c0 : 0;
                            const uint32_t i0 = n_ext ? e1 : c0;                      // first byte that reads this tile
                            const uint32_t nl = has_lit ? l1 - l0 : 0;
                            const uint32_t cnt = L0 ? 0u : (n_ext + kExtMax - 1) / kExtMax;
                            if (L0 && ballot64(n_ext != 0)) {   // the candidate reads an earlier tile (tile 16 of a block without levels): not a level-0 tile after all
                                if (lane == 0) shw[2] = 1;
                                failed = true;
                                continue;
                            }
                            // ---- pool space: literal bytes from the bottom, one 8-byte slot per entry from the top (packed: the entries' bytes behind the literals' too) ----
                            const uint32_t lneed = packed ? nl + n_ext : nl;
                            const uint32_t lincl = wave_incl_scan(lneed), cincl = wave_incl_scan(cnt);
                            const uint32_t ltot = rdlane(lincl, 63), ctot = rdlane(cincl, 63);
                            uint32_t lbase = 0, cbase = 0;
                            if (lane == 0) { if (ltot) lbase = atomicAdd(&shw[3], ltot); if (ctot) cbase = atomicAdd(&shw[1], ctot); }
                            lbase = rdfirst(lbase); cbase = rdfirst(cbase);
                            const uint32_t lat = lbase + lincl - lneed;                // my literal bytes' place in the pool (packed: then my entries' bytes)
                            const uint32_t at = cbase + cincl - cnt;                   // my first entry
                            // (slots: entry i sits at kPool - 8 (i + 1); an overflowing tile is redone packed, so these offsets are only used when they fit)
                            if (has_lit) mp[l0 - tstart] = uint16_t(0x8000u | ((lat - (l0 - tstart)) & 0x7fffu));
                            if (has_cp && i0 < c1) mp[i0 - tstart] = uint16_t(off);   // (i0 >= tstart + off and i0 < tstart + kTile: off < kTile)
                            // ---- literal bytes: stream -> pool (runs of <= 16 bytes: requested here, stored behind the batch's parses) ----
                            const uint32_t lsp = lit_s + (l0 - dtok);                 // stream position of the first literal byte inside the tile
                            if (nl != 0 && nl <= 16) { lnl[u] = nl; ldo[u] = lat; lx[u] = ld128_clamped(src, lsp, clen); }
                            for (uint64_t need = ballot64(nl > 16); need; need &= need - 1) {   // long runs: the whole wave, 16 bytes per lane and step
                                const int fl = int(ctz64(need));
                                const uint32_t nn = rdlane(nl, fl), ss = rdlane(lsp, fl), dd = rdlane(lat, fl);
                                for (uint32_t o = uint32_t(lane) * 16; o < nn; o += 64 * 16)
                                    if (dd + o < kPool) lds_store_exact(pool + dd + o, ld128_clamped(src, ss + o, clen), nn - o < 16 ? nn - o : 16);
                            }
                            // ---- external entries {source position, pool offset | (length - 1) << 16} and their bytes' markers, one per 8 bytes ----
                            if (cnt != 0 && cnt <= 4) {
                                for (uint32_t q = 0; q < cnt; q++) {
                                    const uint32_t m = n_ext - q * kExtMax < kExtMax ? n_ext - q * kExtMax : kExtMax;
                                    const uint32_t po = packed ? lat + nl + q * kExtMax : kPool - 8 * (at + q + 1);
                                    const uint32_t e = c0 - tstart + q * kExtMax;
                                    mp[e] = uint16_t(0x8000u | ((po - e) & 0x7fffu));
                                    if (MLZ_GEN_DEBUG && at + q >= r_last - rank0 + 1 + kExtPerTile) printf("E ext index %u beyond slice (tile %u, cnt %u, n_ext %u)\n", at + q, gt, cnt, n_ext);
                                    store8_wt(&ext[at + q], uint64_t(c0 - off + q * kExtMax) | (uint64_t((po & 0x7fffu) | ((m - 1) << 16)) << 32));
                                }
                            }
                            for (uint64_t need = ballot64(cnt > 4); need; need &= need - 1) {   // long copies: the wave writes the entries together
                                const int fl = int(ctz64(need));
                                const uint32_t nn = rdlane(n_ext, fl), ss = rdlane(c0 - off, fl), dd = rdlane(c0 - tstart, fl), a0 = rdlane(at, fl), p0 = rdlane(lat + nl, fl);
                                for (uint32_t q = uint32_t(lane); q * kExtMax < nn; q += 64) {
                                    const uint32_t m = nn - q * kExtMax < kExtMax ? nn - q * kExtMax : kExtMax;
                                    const uint32_t po = packed ? p0 + q * kExtMax : kPool - 8 * (a0 + q + 1);
                                    const uint32_t e = dd + q * kExtMax;
                                    mp[e] = uint16_t(0x8000u | ((po - e) & 0x7fffu));
                                    store8_wt(&ext[a0 + q], uint64_t(ss + q * kExtMax) | (uint64_t((po & 0x7fffu) | ((m - 1) << 16)) << 32));
                                }
                            }
                        }
#pragma unroll
                        for (uint32_t u = 0; u < NB; u++) if (lnl[u] && ldo[u] + lnl[u] <= kPool) lds_store_exact(pool + ldo[u], lx[u], lnl[u]);
                    }
                }
                __syncthreads();
                tile_failed = shw[2] != 0;
                if (MLZ_GEN_DEBUG && tid == 0) printf("E tile %u parsed: entries %u lit %u failed %u packed %u\n", gt, shw[1], shw[3], shw[2], packed);
                // slots and literals must not meet (the literal region is rounded up to the 32 bytes a role S thread lays down)
                const bool overflow = !packed && ((shw[3] + 31) & ~31u) + 8 * shw[1] > kPool;
                if (tile_failed || !overflow) break;
                packed = 1;   // redo the tile with the byte-packed pool: literal bytes + external bytes <= the tile's bytes
            }
            MLZ_GP(1);
            if (!tile_failed) {
                // ---- the fill: every entry takes the last marker at or before it: (j + marker) as a pool offset, or j - offset as a position ----
                // A wave takes 2048 consecutive entries, a lane 32 of them: the last marker at or before each entry is found in registers,
                // the one in force before a lane's first entry by a scan over the lanes' last markers, the one before the wave's first
                // entry by looking back (markers are a few bytes apart: one look usually finds it).
                const uint32_t w0 = uint32_t(wv) * (kTile / kGenWaves);
                uint32_t carry = 0;
                for (uint32_t back = w0; back > 0 && carry == 0; back -= 64) {
                    const uint32_t mk = mp[back - 64 + lane];
                    const uint64_t has = ballot64(mk != 0);
                    if (has) carry = rdlane(mk, 63 - __builtin_clzll(has));
                }
                const uint32_t e0 = w0 + 32 * uint32_t(lane);
                uint32_t mk[32];
                {
                    uint4 r4[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) r4[q] = *reinterpret_cast<const uint4*>(mp + e0 + 8 * q);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t w4[4] = {r4[q].x, r4[q].y, r4[q].z, r4[q].w};
#pragma unroll
                        for (int x = 0; x < 4; x++) { mk[8 * q + 2 * x] = w4[x] & 0xffffu; mk[8 * q + 2 * x + 1] = w4[x] >> 16; }
                    }
                }
                __syncthreads();   // (nobody overwrites markers another wave still looks for)
                uint32_t cur = 0;
#pragma unroll
                for (int i = 0; i < 32; i++) { cur = mk[i] ? mk[i] : cur; mk[i] = cur; }
                const uint32_t tag = cur ? uint32_t(lane) + 1 : 0;
                const uint32_t t_incl = wave_incl_max_u32(tag);
                const uint32_t t_excl = uint32_t(__builtin_amdgcn_update_dpp(0, int(t_incl), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
                const uint32_t from = __shfl(cur, int(t_excl ? t_excl - 1 : 0));
                const uint32_t cin = t_excl ? from : carry;
                uint32_t ov[16];
#pragma unroll
                for (int i = 0; i < 32; i++) {
                    const uint32_t e = e0 + uint32_t(i);
                    const uint32_t dl = mk[i] ? mk[i] : cin;
                    // (no marker, a pointer below the tile — impossible for a token list that covers the tile — or beyond the block's end: pool byte 0)
                    uint32_t v = (dl & 0x8000u) ? (0x8000u | ((e + dl) & 0x7fffu)) : e - dl;
                    if (dl == 0 || (!(dl & 0x8000u) && dl > e) || e >= n) v = 0x8000u;
                    if (i & 1) ov[i >> 1] |= v << 16; else ov[i >> 1] = v;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) *reinterpret_cast<uint4*>(mp + e0 + 8 * q) = uint4{ov[4 * q], ov[4 * q + 1], ov[4 * q + 2], ov[4 * q + 3]};
                __syncthreads();
                MLZ_GP(2);
                // ---- in-tile chains: an entry that is still a position takes the word of the entry it points at, until every word is a pool offset ----
                // (a chain of copies ends at a literal or an external byte: at most 15 doubling rounds; only the words still open are looked up)
                for (int round = 0; round < 16; round++) {
                    bool changed = false;
#pragma unroll
                    for (int hf = 0; hf < 2; hf++) {   // 16 entries at a time
                        uint16_t* at0 = mp + uint32_t(tid) * 8 + uint32_t(2 * hf) * (kGenThreads * 8);
                        uint16_t* at1 = at0 + kGenThreads * 8;
                        const uint4 va = *reinterpret_cast<const uint4*>(at0), vb = *reinterpret_cast<const uint4*>(at1);
                        const uint32_t w8[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
                        if (((va.x & va.y & va.z & va.w & vb.x & vb.y & vb.z & vb.w) & 0x80008000u) == 0x80008000u) continue;   // all sixteen settled
                        uint32_t h[16];
#pragma unroll
                        for (int x = 0; x < 8; x++) {
                            const uint32_t a = w8[x] & 0xffffu, c = w8[x] >> 16;
                            h[2 * x] = a; h[2 * x + 1] = c;
                            if (!(a & 0x8000u)) h[2 * x] = mp[a];
                            if (!(c & 0x8000u)) h[2 * x + 1] = mp[c];
                        }
#pragma unroll
                        for (int x = 0; x < 16; x++) if (!(h[x] & 0x8000u)) h[x] = mp[h[x]];
                        uint32_t o8[8];
                        bool open = false;
#pragma unroll
                        for (int x = 0; x < 8; x++) { o8[x] = h[2 * x] | (h[2 * x + 1] << 16); open |= (o8[x] & 0x80008000u) != 0x80008000u; }
                        if (o8[0] != w8[0] || o8[1] != w8[1] || o8[2] != w8[2] || o8[3] != w8[3]) *reinterpret_cast<uint4*>(at0) = uint4{o8[0], o8[1], o8[2], o8[3]};
                        if (o8[4] != w8[4] || o8[5] != w8[5] || o8[6] != w8[6] || o8[7] != w8[7]) *reinterpret_cast<uint4*>(at1) = uint4{o8[4], o8[5], o8[6], o8[7]};
                        changed |= open;
                    }
                    if (!__syncthreads_or(changed)) break;
                }
                if (MLZ_GEN_DEBUG && tid == 0) printf("E tile %u jumped\n", gt);
                MLZ_GP(3);
                if constexpr (L0) {
                    // ---- every byte takes its terminal's value (a literal of this tile, in the pool) and the tile goes out: 32 bytes per thread ----
                    const uint32_t my = uint32_t(tid) * 32;
                    uint8_t* dst = dst_base + uni(uint64_t(blocks[bi].dst_off));
                    typedef __attribute__((address_space(1))) uint8_t gbyte;
                    gbyte* mir = reinterpret_cast<gbyte*>(uni(uint64_t(blocks[bi].mirror)));
                    const bool dst_aligned = (uni(uint64_t(reinterpret_cast<uintptr_t>(dst_base)) + uint64_t(blocks[bi].dst_off)) & 15) == 0;
                    const uint4 m0 = reinterpret_cast<const uint4*>(mp + my)[0], m1 = reinterpret_cast<const uint4*>(mp + my)[1],
                                m2 = reinterpret_cast<const uint4*>(mp + my)[2], m3 = reinterpret_cast<const uint4*>(mp + my)[3];
                    const uint32_t m16[16] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z, m3.w};
                    uint32_t ow[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const uint32_t a = m16[2 * q] & 0x7fff7fffu, c = m16[2 * q + 1] & 0x7fff7fffu;
                        ow[q] = uint32_t(pool[a & 0xffffu]) | (uint32_t(pool[a >> 16]) << 8) | (uint32_t(pool[c & 0xffffu]) << 16) | (uint32_t(pool[c >> 16]) << 24);
                    }
                    const uint4 o0{ow[0], ow[1], ow[2], ow[3]}, o1{ow[4], ow[5], ow[6], ow[7]};
                    if (my + 32 <= n && dst_aligned) {
                        store16_wt_a(dst + (tstart + my), o0); store16_wt_a(dst + (tstart + my + 16), o1);
                        if (mir) {   // the caller's pinned buffer: 16-byte stores when they are aligned
                            typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
                            typedef __attribute__((address_space(1))) u32x4_t gvec;
                            if ((uni(uint64_t(blocks[bi].mirror)) & 15) == 0) {
                                *reinterpret_cast<gvec*>(mir + (tstart + my)) = u32x4_t{o0.x, o0.y, o0.z, o0.w};
                                *reinterpret_cast<gvec*>(mir + (tstart + my + 16)) = u32x4_t{o1.x, o1.y, o1.z, o1.w};
                            } else {
#pragma unroll 1
                                for (uint32_t q = 0; q < 8; q++) { const uint32_t w = ow[q]; gbyte* mq = mir + (tstart + my + 4 * q); mq[0] = uint8_t(w); mq[1] = uint8_t(w >> 8); mq[2] = uint8_t(w >> 16); mq[3] = uint8_t(w >> 24); }
                            }
                        }
                    } else {
#pragma unroll 1
                        for (uint32_t q = 0; q < 32 && my + q < n; q++) {   // (a destination that is not 16-byte aligned, the block's ragged end)
                            const uint8_t v = uint8_t(ow[q >> 2] >> (8 * (q & 3)));
                            dst[tstart + my + q] = v;
                            if (mir) mir[tstart + my + q] = v;
                        }
                    }
                    if (!dst_aligned || (n & 31)) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // ordinary stores: written back before the flag
                } else {
                // ---- out: the map (pool offsets, the flag bit dropped), the literal bytes at the pool's bottom ----
                uint8_t* gm = reinterpret_cast<uint8_t*>(gmap + uni(uint64_t(gt) * kTile));
                for (uint32_t q = tid; q < 2 * kTile / 16; q += kGenThreads) {
                    uint4 v = reinterpret_cast<const uint4*>(mp)[q];
                    v.x &= 0x7fff7fffu; v.y &= 0x7fff7fffu; v.z &= 0x7fff7fffu; v.w &= 0x7fff7fffu;
                    store16_wt_a(gm + 16 * size_t(q), v);
                }
                const uint32_t lit_top = shw[3];   // (packed: literal and external bytes interleave below it, role S lays all of them down and then stores the external ones exactly)
                uint8_t* gq = gpool + uni(uint64_t(gt) * kPool);
                for (uint32_t q = tid; 16 * q < lit_top; q += kGenThreads) store16_wt_a(gq + 16 * size_t(q), reinterpret_cast<const uint4*>(pool)[q]);
                if (tid == 0) {
                    store8_wt(&tile_info[gt], uint64_t(shw[1] | (packed << 31)) | (uint64_t(lit_top) << 32));
                }
                }
            } else if (L0) break;   // abandoned: nothing stored, no flag
            else if (tid == 0) store8_wt(&tile_info[gt], 0ull);
            // publish: every store above is a write-through one and only has to have left the CU
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // (L0: the exec pass's done flag of the tile, and kL0Done, not 1: the tile may belong to a block that turns out general, whose tiles' flags role E raises for role S)
            if (tid == 0) __hip_atomic_store(L0 ? &tile_done[gt] : &tile_ready[gt], L0 ? kL0Done : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            MLZ_GP(4);
        }
        if (MLZ_GEN_PROF && blockIdx.x == 0 && tid == 0)
            printf("E wg0: %u tiles; us per tile: ticket %.2f zero+parse %.2f fill %.2f jump %.2f out+publish %.2f\n", gp_tiles, gp[7] / 100.0 / gp_tiles, gp[1] / 100.0 / gp_tiles,
                   gp[2] / 100.0 / gp_tiles, gp[3] / 100.0 / gp_tiles, gp[4] / 100.0 / gp_tiles);
        return;
    }

    // =========================== role S ===========================
    // Software-pipelined over the block's tiles: what step k needs from global memory is requested one or two steps earlier —
    //   B(k)  the thread's 32 bytes of the tile's pool (literals in place)   requested at the top of step k-1
    //   EN(k) the thread's first MLZ_GEN_EP external entries                 requested in step k-2 (two register sets, by parity)
    //   XD(k) the 8 source bytes of those entries that lie below the ring    requested in step k-1, behind its scatter
    //   M(k)  the thread's 32 map entries                                    requested in step k-1, behind its gather
    // — so that a step is LDS work only: pool laid down and entries scattered into their slots (sources: the ring of the last two
    // settled tiles, or XD), barrier, every byte gathered from the pool through the map, barrier.
    // Ready flags are taken in batches (with the tiles' records), ahead of the steps that need them.
    uint8_t* pool = gl;                 // first in the dynamic LDS: a map entry is (nearly) the byte's LDS address
    uint8_t* ring = gl + kPool;         // three tile images: tile q of the block lives at (q % 3) * kTile
    constexpr uint32_t kRing = 3 * kTile;
    constexpr uint32_t EP = MLZ_GEN_EP;
    uint32_t* s_next = reinterpret_cast<uint32_t*>(gl + 4 * kTile + 256);   // entries of tile t (bit 31: packed pool)
    uint32_t* s_ltop = s_next + kGenMaxTiles;                               // literal bytes at the bottom of tile t's pool
    uint32_t* s_rank = s_ltop + kGenMaxTiles;                               // rank of the token covering tile t's first byte
    // TEAMS (round 5).  A block whose copies never read the team - 1 tiles in front of their own (D3's dependency distance; LevelBalanced writes
    // such blocks: far_gap) has `team` consecutive tiles that do not read each other: `team` workgroups settle it, member w the tiles w, w + team,
    // ... — every source of tile k lies in tiles <= k - team, settled (flag value 3 in tile_ready, set behind write-through stores) by the time
    // the other members are one step behind at most; it comes from dst (there is no ring: a member never holds the tiles just before its own).
    // A hand-over between two workgroups — 32 KiB of write-through stores, a flag, an acquire and the reads — measures 1.5 us on this part,
    // same XCD or not (tools/ubench/handover.hip), against 5.3 us for a step.  team = 1 (other encoders' blocks): one workgroup, the ring.
    const uint32_t team = team0;
    // (two copies of the role, the team's and the single workgroup's, chosen once: with `tm` a run-time value the single form — other
    //  encoders' blocks — paid 4 % for the team's branches)
    auto settle = [&](auto TM) {
    constexpr bool tm = decltype(TM)::value;
    for (uint32_t unit = blockIdx.x - nE; unit < ngen * team; unit += nS) {   // (nS is a multiple of 4: a block's members are taken in the same round)
        const uint32_t slot = unit / team, member = unit % team;
        const uint32_t bi = uni(gen_list[slot]);
        if (uni(uint32_t(dec[bi].status)) != 0) continue;
        const uint32_t dlen = uni(dec[bi].dlen);
        const uint32_t first_tile = uni(blocks[bi].first_tile), first_seg = uni(blocks[bi].first_seg);
        uint8_t* dst = dst_base + uni(uint64_t(blocks[bi].dst_off));
        // (a caller's pinned buffer, written through the device's view of it: typed as GLOBAL memory — as a generic pointer made from the
        //  integer its stores were FLAT instructions, and the byte stores' 64-bit lane addresses came out wrong now and then)
        typedef __attribute__((address_space(1))) uint8_t gbyte;
        typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) u32x4_t gvec;
        gbyte* mir = reinterpret_cast<gbyte*>(uni(uint64_t(blocks[bi].mirror)));
        const bool mir_aligned = (uni(uint64_t(blocks[bi].mirror)) & 15) == 0;
        const bool dst_aligned = (uni(uint64_t(reinterpret_cast<uintptr_t>(dst_base)) + uint64_t(blocks[bi].dst_off)) & 15) == 0;
        const uint16_t* bmap = gmap + uni(uint64_t(first_tile) * kTile);
        const uint8_t* bpool = gpool + uni(uint64_t(first_tile) * kPool);
        const ExtEnt* bext = ext_all + uni(ext_index(first_seg, first_tile, bi, 0, 0));
        const uint32_t ntile = (dlen + kTile - 1) >> kTileLog;
        const uint32_t my = uint32_t(tid) * 32;
        uint32_t known = 0;   // tiles [0, known) are ready and their records are in LDS
        // makes tiles [0, want) ready (want - known <= 64 per call): bounded wait for their flags, then their records.  1 = go on
        auto ensure = [&](uint32_t want) -> uint32_t {
            __syncthreads();
            if (wv == 0) {
                // (tiles beyond `want` that happen to be ready are taken along: the next call may then have nothing to wait for)
                const uint32_t t = known + uint32_t(lane);
                uint32_t ok = 1, spins = 0, ready = 0;
                if (t < ntile) {
                    ready = __hip_atomic_load(&tile_ready[first_tile + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u;   // (bit 0: role E's; kL0Done is not)
                    while (!ready && t < want) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins >= spin_limit) { ok = 0; break; }
                        ready = __hip_atomic_load(&tile_ready[first_tile + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u;
                    }
                }
                uint32_t verdict = ballot64(ok == 0) ? 0u : 1u;
                if (verdict == 1 && __hip_atomic_load(reinterpret_cast<int*>(&dec[bi].status), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) verdict = 2;   // role E found the block corrupt
                const uint64_t notready = ballot64(!ready);
                const uint32_t upto = notready ? uint32_t(ctz64(notready)) : 64u;   // the ready prefix
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // role E's stores (another CU, maybe another XCD)
                if (verdict == 1 && uint32_t(lane) < upto && t < ntile) {
                    const GenTile gi = tile_info[first_tile + t];
                    s_next[t] = gi.n_ext; s_ltop[t] = gi.lit_top; s_rank[t] = tile_start[first_tile + t].rank;
                }
                if (lane == 0) { shw[0] = verdict; shw[1] = known + upto < ntile ? known + upto : ntile; }
            }
            __syncthreads();
            known = uni(shw[1]);
            return uni(shw[0]);
        };
        auto fail_block = [&](uint32_t verdict) {
            if (verdict == 0 && tid == 0) {
                atomicCAS(reinterpret_cast<int*>(&dec[bi].status), 0, int(7 | (9 << 8)));  // MLZ_ERR_HIP: the flag never came
                __hip_atomic_store(&ctl->failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        MLZ_GP(4);
        {
            const uint32_t v = ensure(ntile < member + 2 * team + 1 ? ntile : member + 2 * team + 1);
            if (v != 1) { fail_block(v); continue; }
        }
        MLZ_GP(0);
        auto tile_n = [&](uint32_t k) -> uint32_t { return dlen - (k << kTileLog) < kTile ? dlen - (k << kTileLog) : kTile; };
        uint4 M[4], B[2];
        uint2 XD[EP];
        ExtEnt EA[EP], EB[EP];
        auto load_B = [&](uint32_t k) {
            B[0] = uint4{0u, 0u, 0u, 0u}; B[1] = uint4{0u, 0u, 0u, 0u};
            if (my < uni(s_ltop[k])) {
                const uint4* p = reinterpret_cast<const uint4*>(bpool + opaque(k * kPool + my));   // (scalar base + 32-bit lane offset)
                B[0] = p[0]; B[1] = p[1];
            }
        };
        auto load_M = [&](uint32_t k) {
            const uint4* gm = reinterpret_cast<const uint4*>(bmap + opaque(k * kTile + my));
#pragma unroll
            for (int q = 0; q < 4; q++) M[q] = gm[q];
        };
        auto load_EN = [&](uint32_t k, ExtEnt (&EN)[EP]) {
            const ExtEnt* ext = bext + uni(s_rank[k] + k * kExtPerTile);
            const uint32_t ne = uni(s_next[k]) & 0x7fffffffu;
#pragma unroll
            for (uint32_t i = 0; i < EP; i++) {
                const uint32_t e = uint32_t(tid) + i * kGenThreads;
                EN[i] = ExtEnt{0u, 0u};
                if (e < ne) EN[i] = ext[opaque(e)];
            }
        };
        auto ring_lo_of = [](uint32_t k) -> uint32_t { return k >= 2 ? (k - 2) << kTileLog : 0u; };   // positions from here on are in the ring when tile k is settled
        auto load_XD = [&](uint32_t k, const ExtEnt (&EN)[EP]) {   // sources of tile k's prefetched entries that lie below the ring
            const uint32_t ne = uni(s_next[k]) & 0x7fffffffu, rlo = ring_lo_of(k);
#pragma unroll
            for (uint32_t i = 0; i < EP; i++) {
                const uint32_t e = uint32_t(tid) + i * kGenThreads;
                const uint32_t sp = EN[i].src, len = (EN[i].where >> 16) + 1;
                XD[i] = uint2{0u, 0u};
                if (e < ne && sp + len <= rlo) __builtin_memcpy(&XD[i], dst + sp, 8);    // (sp + 8 <= rlo + 7 < tile k's start: inside dst)
            }
        };
        // a team: the sources of tile k's prefetched entries that END in [lo, hi) — those below `lo` were requested a step earlier, when the tiles
        // below `lo` were known to be settled
        auto load_XD_range = [&](uint32_t k, const ExtEnt (&EN)[EP], uint32_t lo, uint32_t hi) {
            const uint32_t ne = uni(s_next[k]) & 0x7fffffffu;
#pragma unroll
            for (uint32_t i = 0; i < EP; i++) {
                const uint32_t e = uint32_t(tid) + i * kGenThreads;
                const uint32_t end = EN[i].src + (EN[i].where >> 16) + 1;
                if (e < ne && end > lo && end <= hi) __builtin_memcpy(&XD[i], dst + EN[i].src, 8);
            }
        };
        // one entry -> its bytes in the pool of the tile being settled
        // Sources in the ring are read as three dword-aligned words and shifted into place (v_alignbyte takes the position's low two
        // bits): an unaligned ds_read_b64 costs the LDS pipe a cycle per lane, these a few cycles per wave.  The rare cases — a source
        // that wraps around the ring's end or straddles the oldest tile kept in LDS — go byte by byte.
        auto place = [&](uint32_t rlo, bool packed, ExtEnt en, uint2 pre, bool has_pre) {
            const uint32_t sp = en.src, where = en.where & 0xffffu, len = (en.where >> 16) + 1;
            uint2 x;
            const uint32_t r = sp >= rlo ? sp % kRing : 0u;
            if (sp >= rlo && r + 12 <= kRing) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(ring + (r & ~3u));
                const uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
                x.x = __builtin_amdgcn_alignbyte(d1, d0, r); x.y = __builtin_amdgcn_alignbyte(d2, d1, r);
            } else if (sp < rlo && sp + len <= rlo) {
                if (has_pre) x = pre; else __builtin_memcpy(&x, dst + sp, 8);
            } else {
                uint64_t acc = 0;
#pragma unroll 1
                for (uint32_t q = 0; q < len; q++) {   // (two branches, not one select between an LDS and a global address: that would be a FLAT load)
                    const uint32_t p = sp + q;
                    uint32_t v;
                    if (p >= rlo) v = ring[p % kRing]; else v = dst[p];
                    acc |= uint64_t(v) << (8 * q);
                }
                x.x = uint32_t(acc); x.y = uint32_t(acc >> 32);
            }
            if (!packed) *reinterpret_cast<uint2*>(pool + where) = x;                // an aligned 8-byte slot of its own
            else lds_store_exact(pool + where, uint4{x.x, x.y, 0u, 0u}, len);       // byte-packed pool: nothing beyond the entry's bytes
        };
        bool dead = false;
        uint32_t xd_safe = 0;   // a team: sources ending at or below this position were requested a step ahead
        auto step = [&](uint32_t k, ExtEnt (&ENc)[EP], ExtEnt (&ENn)[EP]) {
            if (k + 2 * team + 1 > known && known < ntile) {
                const uint32_t v = ensure(k + 2 * team + 1 < ntile ? k + 2 * team + 1 : ntile);
                if (v != 1) { fail_block(v); dead = true; return; }
            }
            const uint32_t k1 = k + team < ntile ? k + team : k, k2 = k + 2 * team < ntile ? k + 2 * team : k1;   // my next tiles (clamped: the loads are then unused)
            const uint32_t n = tile_n(k), tstart = k << kTileLog;
            uint8_t* cur = ring + ((k / team) % 3) * kTile;
            const uint32_t nx = uni(s_next[k]);
            const uint32_t ne = nx & 0x7fffffffu, rlo = tm ? 0xffffffffu : ring_lo_of(k);
            const bool packed = (nx >> 31) != 0;
            if (tm) {
                // every tile up to k - team is settled: my own previous one is, the other members' latest ones at or below it are polled (lane i: tile k - team - 1 - i)
                if (k >= team + 1) {
                    __syncthreads();
                    if (wv == 0) {
                        const uint32_t i = uint32_t(lane);
                        uint32_t ok = 1, spins = 0;
                        if (i + 1 < team && k >= team + 1 + i) {
                            const uint32_t* f = tile_ready + first_tile + (k - team - 1 - i);
                            while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 3u) {
                                __builtin_amdgcn_s_sleep(1);
                                if (++spins >= spin_limit || ((spins & 63) == 0 && __hip_atomic_load(reinterpret_cast<int*>(&dec[bi].status), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) { ok = 0; break; }
                            }
                        }
                        if (lane == 0) shw[0] = ballot64(ok == 0) ? 0u : 1u;
                    }
                    __syncthreads();
                    if (uni(shw[0]) != 1) {   // a member gave up (or the block failed elsewhere): -MLZ_ERR_HIP unless a verdict is there already
                        fail_block(0); dead = true; return;
                    }
                }
                MLZ_GP(5);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the other members' stores (other CUs, maybe other XCDs)
                // every source is final now; those that end at or below tile k - 2 team's end were requested a step ago (xd_safe), the rest here
                load_XD_range(k, ENc, xd_safe, 0xffffffffu);
            } else {
                // This CU's L1 may hold lines of dst from before the workgroup's own stores (a 128-byte line can span two tiles): dropped once
                // per step, before the step's loads of settled bytes (XD) — every store that matters to them has been acknowledged by then
                // (its thread has since waited for newer loads of its own, and a barrier followed).
                asm volatile("buffer_inv sc0" ::: "memory");
            }
            // ---- the pool: literal bytes (from role E), then the entries' bytes; slots and literals are disjoint, a packed pool needs the barrier between ----
            if (my < uni(s_ltop[k])) { reinterpret_cast<uint4*>(pool + my)[0] = B[0]; reinterpret_cast<uint4*>(pool + my)[1] = B[1]; }
            if (packed) __syncthreads();
            load_B(k1);
            if (!packed) {
#pragma unroll
                for (uint32_t i = 0; i < EP; i++) {
                    const uint32_t e = uint32_t(tid) + i * kGenThreads;
                    if (e < ne) place(rlo, false, ENc[i], XD[i], true);
                }
            }
            if (packed || ne > EP * kGenThreads) {   // a packed tile (rare: exact stores), or the entries beyond the prefetched ones: a plain loop
                const ExtEnt* ext = bext + uni(s_rank[k] + k * kExtPerTile);
#pragma unroll 1
                for (uint32_t e = uint32_t(tid) + (packed ? 0u : EP * kGenThreads); e < ne; e += kGenThreads) place(rlo, packed, ext[e], uint2{0u, 0u}, false);
            }
            if (!tm) load_XD(k1, ENn);
            else {   // my next tile's sources in what is settled by now: every tile up to k - team (their bytes were acquired at this step's top)
                xd_safe = k >= team ? (k - team + 1) << kTileLog : 0u;
                load_XD_range(k1, ENn, 0u, xd_safe);
            }
            load_EN(k2, ENc);
            __syncthreads();            // every terminal of the tile has its byte
            MLZ_GP(2);
            gp_tiles++; gp_ext += ne;
            // ---- every byte takes its terminal's value ----
            {
                uint32_t m16[16] = {M[0].x, M[0].y, M[0].z, M[0].w, M[1].x, M[1].y, M[1].z, M[1].w,
                                    M[2].x, M[2].y, M[2].z, M[2].w, M[3].x, M[3].y, M[3].z, M[3].w};
                // the NEXT tile's map words are requested here, a whole step before their use: this tile's are pinned in registers of
                // their own first (a second persistent set of 16 registers made the allocator spill 80)
#pragma unroll
                for (int q = 0; q < 16; q++) asm volatile("" : "+v"(m16[q]));
                load_M(k1);
                uint32_t ow[8];
                // (ds_read_u8_d16 / _d16_hi pairs would pack two bytes per register without a shift, but with SRAM ECC on — MI300 / MI355 — a d16
                //  load clears the half it does not write: measured wrong, not kept)
                // two halves of sixteen bytes, kept apart: with all 32 look-ups in flight at once the indices and the bytes took 64 registers
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
#pragma unroll
                    for (int q = 4 * hf; q < 4 * hf + 4; q++) {
                        const uint32_t a = m16[2 * q], c = m16[2 * q + 1];
                        ow[q] = uint32_t(pool[a & 0xffffu]) | (uint32_t(pool[a >> 16]) << 8) | (uint32_t(pool[c & 0xffffu]) << 16) | (uint32_t(pool[c >> 16]) << 24);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                const uint4 o0{ow[0], ow[1], ow[2], ow[3]}, o1{ow[4], ow[5], ow[6], ow[7]};
                reinterpret_cast<uint4*>(cur + my)[0] = o0;
                reinterpret_cast<uint4*>(cur + my)[1] = o1;
                const uint32_t* cur32 = reinterpret_cast<const uint32_t*>(cur);
                if (my + 32 <= n) {
                    const uint32_t at = opaque(tstart + my);
                    if (tm && dst_aligned) { store16_wt_a(dst + at, o0); store16_wt_a(dst + (at + 16), o1); }   // (write-through: other members read these bytes)
                    else { __builtin_memcpy(dst + at, &o0, 16); __builtin_memcpy(dst + (at + 16), &o1, 16); }
                    if (mir) {   // the caller's pinned buffer (PCIe): 16-byte stores only when they are aligned, like the exec pass's mirror
                        if (mir_aligned) { *reinterpret_cast<gvec*>(mir + at) = u32x4_t{o0.x, o0.y, o0.z, o0.w}; *reinterpret_cast<gvec*>(mir + (at + 16)) = u32x4_t{o1.x, o1.y, o1.z, o1.w}; }
                        else {
#pragma unroll 1
                            for (uint32_t q = 0; q < 32; q += 4) {   // (rolled: the unrolled form was a hundred byte stores under their own exec masks)
                                const uint32_t w = cur32[(my + q) >> 2];
                                mir[at + q] = uint8_t(w); mir[at + q + 1] = uint8_t(w >> 8); mir[at + q + 2] = uint8_t(w >> 16); mir[at + q + 3] = uint8_t(w >> 24);
                            }
                        }
                    }
                } else {
#pragma unroll 1
                    for (uint32_t q = 0; q < 32 && my + q < n; q++) {   // (the block's ragged end; bytes back from the ring)
                        const uint8_t v = cur[my + q];
                        dst[tstart + my + q] = v;
                        if (mir) mir[tstart + my + q] = v;
                    }
                }
            }
            MLZ_GP(3);
            if (tm) {
                // publish: my stores acknowledged (a destination that is not 16-byte aligned took ordinary stores: written back first), then the flag
                if (!dst_aligned) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();            // the tile is in the ring; the pool is free for the next one
            if (tm && tid == 0) __hip_atomic_store(&tile_ready[first_tile + k], 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            MLZ_GP(6);
        };
        // prologue: my first tile's pool bytes, map and entries, my second tile's entries (tiles 0 and 1 have no source below the ring)
        if (member >= ntile) continue;
        load_B(member);
        load_M(member);
        load_EN(member, EA);
        load_EN(member + team < ntile ? member + team : member, EB);
#pragma unroll
        for (uint32_t i = 0; i < EP; i++) XD[i] = uint2{0u, 0u};
        for (uint32_t k = member; k < ntile && !dead; k += 2 * team) {
            step(k, EA, EB);
            if (k + team < ntile && !dead) step(k + team, EB, EA);
        }
    }
    };
    if (team > 1) settle(std::true_type{}); else settle(std::false_type{});
    if (MLZ_GEN_PROF && blockIdx.x == nE && tid == 0)
        printf("S wg0: %u tiles, %.0f entries per tile; us per tile: first flags %.2f team wait %.2f scatter %.2f gather+flush %.2f publish %.2f between blocks %.2f\n", gp_tiles, double(gp_ext) / gp_tiles,
               gp[0] / 100.0 / gp_tiles, gp[5] / 100.0 / gp_tiles, gp[2] / 100.0 / gp_tiles, gp[3] / 100.0 / gp_tiles, gp[6] / 100.0 / gp_tiles, gp[4] / 100.0 / gp_tiles);
}

// The launch: the roles above, and the batch's RESULTS (D5: out_len[i] = decoded length or -MLZ_ERR_*, a kernel of its own — dec_finish_kernel —
// until round 5 and still when this kernel is not launched).  Without a general block (the common case) the exec pass has written every
// block by the time this kernel starts: its first workgroup writes the results and everybody leaves.  With general blocks the results wait
// for the settling workgroups: every workgroup counts itself out, the last one writes them.
__global__ __launch_bounds__(kGenThreads) void dec_general_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base,
                                                                  const BlockInfo* __restrict__ blocks, DecBlock* __restrict__ dec,
                                                                  const uint32_t* __restrict__ tok_pos, const uint32_t* __restrict__ round_d,
                                                                  const uint32_t* __restrict__ round_rep, const TileStart* __restrict__ tile_start,
                                                                  const uint32_t* __restrict__ gen_list, uint16_t* __restrict__ gmap, uint8_t* __restrict__ gpool,
                                                                  ExtEnt* __restrict__ ext_all, GenTile* __restrict__ tile_info,
                                                                  uint32_t* __restrict__ tile_ready, GenCtl* __restrict__ ctl, uint32_t nE, uint32_t nS,
                                                                  uint32_t spin_limit, uint32_t force_packed, int64_t* __restrict__ out_len, int n_blocks, int debug) {
    auto results = [&]() {
        for (int bi = threadIdx.x; bi < n_blocks; bi += kGenThreads) {
            const DecBlock d = dec[bi];
            // status bits 8.. carry the failure site for debugging; callers see the plain error code
            out_len[bi] = d.status ? -int64_t(debug ? d.status : (d.status & 0xff)) : int64_t(d.dlen);
        }
    };
    if (__hip_atomic_load(&ctl->n_general, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        if (blockIdx.x == 0) results();
        return;
    }
    dec_general_body<false>(src_base, dst_base, blocks, dec, tok_pos, round_d, round_rep, tile_start, gen_list, gmap, gpool, ext_all, tile_info, tile_ready, ctl, nE, nS, spin_limit, force_packed);
    __shared__ uint32_t last_out;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();     // what this workgroup wrote (block status words) before it counts itself out
        last_out = atomicAdd(&ctl->done_wgs, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (last_out) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        results();
    }
}

// dec_level0_kernel (round 6): level-0 tiles decoded before the exec pass, when there are no more of them than CUs.  The exec pass runs a batch's
// tiles level by level and a tile's latency is its ordered chain (~73 us whatever else the device does): with twelve 8 MiB blocks the first of its four
// slot-waves holds 191 level-0 tiles and idles four fifths of the device.  A level-0 tile reads nothing but itself, which is the case role E of the
// general pass reduces in parallel — every byte to its terminal by pointer jumping in LDS, ~30 us with 1024 threads —, so these tiles are decoded
// that way BEFORE the exec pass, one per CU; an exec workgroup that finds its tile's done flag up returns at once.
//
// Which tiles: the CANDIDATES, tile 16 j of every block — level 0 under each of the three level patterns, so the kernel needs no verdict and no
// schedule, only the token list: it depends on dec_index2_kernel alone.  The host lists them (L0Cands, a kernel argument: workgroup c takes entry c)
// and launches when they are no more than the device has CUs — many small blocks: the tile chain's throughput is the better one, the exec pass does
// every tile as in rounds 2-5.  A candidate of a failed, stored or empty block, or beyond the block's decoded length, is skipped; one that cannot be
// finished (dec_general_body) is left to the later passes; the tiles 4, 8, 12 (mod 16) of the fast pattern are level 0 and no candidates: the exec pass's.
//
// The LAST workgroup is not a candidate's: it gives the blocks' verdicts (dec_viol_kernel's gather) and then makes the schedule and the general-block
// list (dec_schedule_kernel), on a CU the candidates leave free — two launches less between the index pass and the exec pass, both inside the ~40 us the
// candidates take.  Nothing it writes (DecBlock::viol / general, the order, GenCtl, the call's counters) is read by a candidate's workgroup.
constexpr uint32_t kL0MaxCands = 256, kL0BlockBits = 28;
struct L0Cands { uint32_t e[kL0MaxCands]; };   // block | (tile / 16) << kL0BlockBits
struct L0Sched {   // what the verdict workgroup needs: the arguments of dec_viol_kernel and dec_schedule_kernel
    const uint32_t *seg_block, *tile_block; const uint8_t* seg_viol;
    uint32_t *n_general, *order, *gen_list, *gen_ctl, *call_acc;
    uint32_t segs, tiles, n_blocks, n_settle, acc_reset;
};
__global__ __launch_bounds__(kGenThreads) void dec_level0_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base,
                                                                 const BlockInfo* __restrict__ blocks, DecBlock* __restrict__ dec,
                                                                 const uint32_t* __restrict__ tok_pos, const uint32_t* __restrict__ round_d,
                                                                 const uint32_t* __restrict__ round_rep, const TileStart* __restrict__ tile_start,
                                                                 uint32_t* __restrict__ tile_done, const L0Cands cands, const L0Sched sc) {
    if (blockIdx.x == gridDim.x - 1) {
        for (uint32_t i0 = 0; i0 < sc.segs; i0 += kGenThreads) dec_viol_gather(sc.seg_block, sc.seg_viol, dec, sc.n_general, sc.segs, i0 + threadIdx.x);
        // the verdicts are complete (every atomic has returned) before the schedule reads them: one workgroup, so a barrier orders the two parts;
        // the schedule's loads must not be served from what this CU cached before (nothing, unless a candidate of an earlier launch left it)
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        dec_schedule_body(blocks, sc.tile_block, dec, sc.order, sc.tiles, sc.n_blocks, sc.gen_list, sc.gen_ctl, sc.n_settle, sc.call_acc, sc.acc_reset);
        return;
    }
    const uint32_t e = cands.e[blockIdx.x];
    const uint32_t bi = e & ((1u << kL0BlockBits) - 1), t = (e >> kL0BlockBits) << 4;
    // (DecBlock word by word: viol and general are being written)
    const uint32_t skip = uni(uint32_t(dec[bi].status) | dec[bi].literals | (dec[bi].ntok == 0 ? 1u : 0u) | ((t << kTileLog) >= dec[bi].dlen ? 1u : 0u));
    if (skip) return;
    dec_general_body<true>(src_base, dst_base, blocks, dec, tok_pos, round_d, round_rep, tile_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           1u, 0u, 1u, 0u, bi, t, tile_done);
}

}  // namespace mlz
