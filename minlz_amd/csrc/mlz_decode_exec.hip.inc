// mlz_decode_exec.hip.inc — D4, the exec pass of the parallel decoder (included by mlz_hip.hip
// after mlz_decode.hip.inc).
//
// One 192-thread workgroup (3 wavefronts; four tiles per CU, bounded by the 32 KiB tile image in LDS) per 32 KiB output tile, in schedule order
// (workgroup i takes the i-th tile of the schedule: a tile only ever waits on tiles of workgroups dispatched before its own).  The index pass (D3) left the block's
// TOKEN LIST — the stream position of every token, in stream order — and, for every 64th token, the output position where
// it starts and the repeat offset in force there.  ROUNDS of 64 consecutive tokens are dealt round-robin to the waves and
// the tile is built in LDS; lane k handles the round's k-th token:
//
//   part 1  (no ordering)  everything whose source is NOT this tile: literal bytes (from the
//           stream) and copies that read only earlier tiles (already published output, global
//           memory).  The next round's stream bytes and the positions of the round after it are requested before the
//           current round is parsed.
//   part 2  (in stream order: the wave waits for its turn, an LDS counter)  copies that read this
//           tile, LDS -> LDS only, in dependency passes: a plain copy of <= 32 bytes goes as soon as its source
//           window ends below the first byte still to be written; overlapping, long or straddling copies go alone,
//           with 64 lanes, when they are the lowest ones left.  Only this part is serial per tile.
//
// then all waves flush the tile with 16-byte stores and the tile's done flag is published.
//
// History of this pass (enwik-like 100 MB, ms): one wave per tile 32 -> 4 waves, a lane per stream BYTE, turns per
// chunk 0.84 -> 8 waves, turns per 2 chunks 0.645 -> branch-free ordered copy 0.625 (0.70 with the dense level pattern)
// -> a lane per TOKEN (the token starts of four 64-byte chunks compacted through LDS by every wave), 4-wave tiles,
// dependency passes 0.53 -> three-level pattern 0.467 -> token list from the index pass, full rounds 0.402 -> 3 waves per
// tile 0.385 (4: 0.403, 2: 0.426, 5 / 6 / 8: 0.46 / 0.50 / 0.49: a wave's own work per round and the ordered chain are of one size).
// The reference (decode.go:178-622) is one sequential loop over the tokens of a block.

namespace mlz {

#ifndef MLZ_EXEC_WAVES
#define MLZ_EXEC_WAVES 3
#endif
constexpr int kExecWaves = MLZ_EXEC_WAVES;
constexpr int kExecThreads = 64 * kExecWaves;
#ifndef MLZ_EXEC_MINWAVES
#define MLZ_EXEC_MINWAVES 4   // waves per SIMD the register allocation has to leave room for
#endif
#ifndef MLZ_EXEC_PAIR
#define MLZ_EXEC_PAIR 2    // rounds per turn of the ordered section (1 = rounds 3-5; see the kernel).  (Measured and not kept in round 6: "early copies",
                           // in-tile copies that read nothing of the previous round going before the turn — profiles/r06_a_exec_early_copies.txt.)
#endif
constexpr uint32_t kExecLds = kTile + 64 + 1024;   // tile image, shared words, the token table (mlz_toktab.h)

// non-overlapping copy of len (1..32) bytes inside LDS, any alignment (unaligned DS access is on).
// ALL lanes read four 8-byte pieces at offsets min(8k, max(len, 8) - 8) first — one LDS round trip whatever the mix of
// lengths in the wave (a branch per length class made the classes take their round trips one after the other, and this
// copy is the ordered section of the exec pass: the critical path of a tile) — and only the stores, which nobody waits
// for, differ: len >= 8 stores the four pieces (the clamped ones re-copy the tail), 4..7 two overlapping 4-byte pieces,
// 1..3 (repeats) bytes.  Short copies read up to 7 bytes beyond their source (inside the tile buffer's padding at worst).
struct CopyPlan { uint8_t* dp; const uint8_t* sp; uint32_t o1, o2, o3; };   // made before the wave asks for its turn: only the copy itself is serial
__device__ __forceinline__ CopyPlan lds_copy_plan(uint8_t* dp, const uint8_t* sp, uint32_t len) {
    const uint32_t last = len >= 8 ? len - 8 : 0;
    CopyPlan c;
    c.dp = dp; c.sp = sp; c.o1 = last < 8 ? last : 8; c.o2 = last < 16 ? last : 16; c.o3 = last;
    return c;
}
__device__ __forceinline__ void lds_copy_small(const CopyPlan& c, uint32_t len) {
    uint8_t* dp = c.dp; const uint8_t* sp = c.sp;
    const uint32_t o1 = c.o1, o2 = c.o2, o3 = c.o3;
    uint64_t x0, x1, x2, x3;
    __builtin_memcpy(&x0, sp, 8);
    __builtin_memcpy(&x1, sp + o1, 8);
    __builtin_memcpy(&x2, sp + o2, 8);
    __builtin_memcpy(&x3, sp + o3, 8);
    if (len >= 8) {
        __builtin_memcpy(dp, &x0, 8);
        __builtin_memcpy(dp + o1, &x1, 8);
        __builtin_memcpy(dp + o2, &x2, 8);
        __builtin_memcpy(dp + o3, &x3, 8);
    } else if (len >= 4) {
        const uint32_t y0 = uint32_t(x0), y1 = uint32_t(x0 >> (8 * (len - 4)));
        __builtin_memcpy(dp, &y0, 4);
        __builtin_memcpy(dp + len - 4, &y1, 4);
    } else {
        dp[0] = uint8_t(x0); dp[len >> 1] = uint8_t(x0 >> (8 * (len >> 1))); dp[len - 1] = uint8_t(x0 >> (8 * (len - 1)));
    }
}

// 16-byte write-through store (sc1: the line does not stay dirty in this XCD's L2).  A tile flushed this
// way needs no L2 write-back before its done flag: `s_waitcnt vmcnt(0)` + the flag store publish it
// (MI355X guide, "publish-large": write-through wins for tens of KB per workgroup).
__device__ __forceinline__ void store16_wt(uint8_t* base /* wave-uniform */, uint32_t off, uint4 v) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1" ::"v"(off), "v"(x), "s"(base) : "memory");
}

__global__ __launch_bounds__(kExecThreads, MLZ_EXEC_MINWAVES) void dec_exec2_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base,
                                                                 const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ tile_block,
                                                                 DecBlock* __restrict__ dec, const TileStart* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ tok_pos, const uint32_t* __restrict__ round_d,
                                                                 const uint32_t* __restrict__ round_rep, const uint32_t* __restrict__ order,
                                                                 uint32_t* __restrict__ tile_done, uint32_t* __restrict__ ticket, uint32_t total_tiles,
                                                                 unsigned long long* __restrict__ prof,
                                                                 uint32_t l0_ran /* dec_level0_kernel ran before this pass: some tiles' done flags may be up already */) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tilebuf[];
    volatile uint32_t* sh = reinterpret_cast<volatile uint32_t*>(tilebuf + kTile);  // [0] ticket, [2] failure site, [3] turn: first chunk not yet complete
    // ([2] and [3] are polled together with one 8-byte read)
    const int tid = threadIdx.x, lane = tid & 63, wv = int(rdfirst(uint32_t(tid) >> 6));   // (readfirstlane: the compiler then knows that everything dealt out per wave is wave-uniform and keeps it in scalar registers)
    unsigned long long t_prev = MLZ_PROFILE && prof ? __builtin_readcyclecounter() : 0;
    unsigned long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define MLZ_PHASE(i) do { if (MLZ_PROFILE && prof) { unsigned long long t_now = __builtin_readcyclecounter(); pc[i] += t_now - t_prev; t_prev = t_now; } } while (0)
    // The workgroup's place in the schedule is its index: workgroups are dispatched in index order, so a tile only ever waits for tiles
    // whose workgroups were dispatched before its own (rounds 2-4a drew a ticket from a global counter instead: a thousand atomics on
    // one address when the launch starts, 18 us of this pass).
    (void)ticket;
    if (tid == 0) { sh[2] = 0; if (MLZ_PROFILE) { sh[4] = 0; sh[5] = 0; } }
    uint32_t* toktab = reinterpret_cast<uint32_t*>(tilebuf + kTile + 64);
    for (int i = tid; i < 256; i += kExecThreads) toktab[i] = g_toktab.e[i];
    __syncthreads();
    uint32_t gt = blockIdx.x;
    if (gt >= total_tiles) return;
    const uint32_t my_ticket = gt;
    unsigned long long* trace = MLZ_PROFILE && prof && my_ticket < 4096 ? prof + 32 + 4 * size_t(my_ticket) : nullptr;  // debug timeline (100 MHz clock)
    if (trace && tid == 0) {  // + where the tile runs (debug): XCC id, SE / SH / CU id of HW_ID
        const unsigned long long hw = __builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xffffu, xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu;
        trace[0] = __builtin_amdgcn_s_memrealtime() | (hw << 44) | (xcc << 40);
    }
    gt = rdfirst(order[gt]);  // ticket -> tile (D3d)
    // A tile that dec_level0_kernel has decoded and published (a level-0 candidate it could finish): nothing left to do.  One load by one lane; the flag was
    // raised before this launch began and only this workgroup would raise it now, so the waves agree.
    // (Requested here, beside the descriptor loads, and looked at behind them.)
    uint32_t l0_flag = 0;
    if (l0_ran && lane == 0) l0_flag = __hip_atomic_load(&tile_done[gt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t bi = tile_block[gt];
    const BlockInfo b = blocks[bi];
    const DecBlock db = dec[bi];
    const uint32_t k = gt - b.first_tile;
    const uint32_t tstart = k << kTileLog;
    uint32_t* done = tile_done + b.first_tile;
    uint32_t bad = 0;  // 0 ok, else failure site (reported as corrupt)
    bool plain_stores = false;  // the tile was (partly) written with ordinary stores: publish needs the L2 write-back
    uint8_t* dst = dst_base + b.dst_off;
    if (rdfirst(l0_flag) != 0) return;
    if (db.general & 2) return;  // decoded as a whole by dec_general_kernel; nobody waits for its tiles
    if (db.status == 0 && db.literals) {
        // Stored block: a straight copy.  No tile of such a block is ever the source of a copy, so
        // nothing is published (the release fence of 32 768 tiles was 80 % of the time of config 4).
        const uint32_t tend = tstart + kTile < db.dlen ? tstart + kTile : db.dlen;
        const uint8_t* src = src_base + b.src_off + db.body_off;
        for (uint32_t j = tstart + tid * 16; j < tend; j += kExecThreads * 16) {
            if (j + 16 <= tend) {
                uint4 x;
                __builtin_memcpy(&x, src + j, 16);
                __builtin_memcpy(dst + j, &x, 16);
                if (b.mirror) __builtin_memcpy(reinterpret_cast<uint8_t*>(b.mirror) + j, &x, 16);
            } else {
                for (uint32_t q = j; q < tend; q++) { dst[q] = src[q]; if (b.mirror) reinterpret_cast<uint8_t*>(b.mirror)[q] = src[q]; }
            }
        }
        return;
    }
    if (db.status == 0 && tstart < db.dlen) {
        const uint32_t tend = tstart + kTile < db.dlen ? tstart + kTile : db.dlen;
        const uint8_t* src = src_base + b.src_off + db.body_off;
        const uint32_t clen = db.clen;
        {
            const TileStart ts = tile_start[gt];
            // The block's token list (D3): stream position of every token in stream order, and per ROUND of 64 consecutive tokens
            // (rounds are aligned to the block's token numbering, not to tiles) the output position of its first token and the
            // repeat offset in force there.  My tile's tokens are r_first (the token covering its first byte) .. r_last (the one
            // covering the next tile's first byte); the rounds they lie in are dealt round-robin to the waves, in full: tokens of
            // a round that belong to a neighbour tile are parsed like the others (the round's positions and offsets come out of
            // a scan over all 64 lanes) and then clipped away by the same tests that clip a token straddling the tile's ends.
            const size_t cofs = size_t(b.first_seg) << (kSegLog - 6);
            const uint32_t* tpos = tok_pos + (size_t(b.first_seg) << kSegLog);
            const uint32_t* rdv = round_d + cofs;
            const uint32_t* rrv = round_rep + cofs;
            const uint32_t ntok = db.ntok;   // (> 0: the block decodes to dlen > 0 bytes)
            uint32_t r_last = ntok - 1;
            if (tend < db.dlen) r_last = tile_start[gt + 1].rank;
            const uint32_t j_first = rdfirst(ts.rank) >> 6, j_last = rdfirst(r_last) >> 6;
            if (tid == 0) sh[3] = 0;   // the turn: first UNIT (of MLZ_EXEC_PAIR rounds) not yet complete
            uint64_t known_done = 0, known_done2 = 0;  // bit t: tile (k-1-t) / (k-65-t) of this block already observed done
            bool all_known = false;

            // wait until tile tt of this block is published
            auto wait_tile = [&](uint32_t tt) {
                const uint32_t age = k - 1 - tt;
                if (age < 64 && ((known_done >> age) & 1)) return;
                if (age >= 64 && age < 128 && ((known_done2 >> (age - 64)) & 1)) return;
                uint32_t spins = 0;
                while (__hip_atomic_load(&done[tt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > (1u << 24)) { bad = 6; break; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                if (age < 64) known_done |= 1ull << age;
                else if (age < 128) known_done2 |= 1ull << (age - 64);
            };

            // Level-conformant block: every tile this one reads from has a lower level and an earlier
            // ticket; wait for all of them at once (lane t polls tile k-1-t) and pay ONE acquire.
            if (!db.general && tile_level_p(k, block_pattern(db)) > 0) {
                const int32_t tt = int32_t(k) - 1 - lane, tt2 = tt - 64;
                const bool want = tt >= 0 && tile_level_p(uint32_t(tt), block_pattern(db)) < tile_level_p(k, block_pattern(db));
                const bool want2 = tt2 >= 0 && tile_level_p(uint32_t(tt2), block_pattern(db)) < tile_level_p(k, block_pattern(db));
                uint32_t spins = 0;
                while (true) {
                    const bool ready = (!want || __hip_atomic_load(&done[tt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) &&
                                       (!want2 || __hip_atomic_load(&done[tt2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
                    if (ballot64(!ready) == 0) break;
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > (1u << 22)) { bad = 6; break; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                known_done = ballot64(want);
                known_done2 = ballot64(want2);
                all_known = !bad;
            }
            __syncthreads();  // shared words initialised
            if (trace && tid == 0) trace[1] = __builtin_amdgcn_s_memrealtime() | ((unsigned long long)(j_last - j_first + 1) << 48);  // + round count (debug)
            MLZ_PHASE(3);

            // ONE LANE PER TOKEN, 64 tokens per round.  Per round a wave does part 1 (unordered: literals, copies from earlier
            // tiles), waits for its turn, does part 2 (copies that read this tile, in dependency passes) and passes the turn on.
            // Loads are two rounds deep: the token positions of round i + 2 and the stream bytes of round i + 1 are requested
            // while round i is processed.  The per-round words (first output position, repeat offset) of up to 64 of MY rounds
            // are fetched with one vector load each — lane i holds those of my i-th round, read with readlane: a scalar load per
            // round would put a memory round trip in front of every parse.
            bool stop = false;
            const uint8_t* dummy = reinterpret_cast<const uint8_t*>(blocks);     // 40 readable bytes for lanes without a request
            const bool tiny = clen < 8;          // a stream shorter than one load: kept in tiny_w, the loads go to the dummy
            uint64_t tiny_w = 0;
            if (tiny) for (uint32_t q = 0; q < clen; q++) tiny_w |= uint64_t(src[q]) << (8 * q);
            const uint8_t* fsrc = tiny ? dummy : src;
            const uint32_t fclen = tiny ? 8u : clen;
            // stream position of my token in round j (a lane beyond the list reads its last entry; beyond my rounds: harmless)
            auto fetch_pos = [&](uint32_t j) -> uint32_t {
                const uint32_t R = (j << 6) + uint32_t(lane);
                return tpos[R < ntok ? R : ntok - 1];
            };
            // the 8 stream bytes at sp, bytes beyond the stream read as zero.  ONE load on every path (a stream shorter than 8
            // bytes sits in tiny_w and the load goes to a dummy address): with two code paths the compiler cannot count the loads
            // in flight and would wait for this request — the NEXT round's — at the current round's parse.
            auto fetch_bytes = [&](uint32_t sp) -> uint64_t {
                const uint32_t a0 = sp < fclen - 8 ? sp : fclen - 8;
                return ld64u(fsrc + a0);   // raw: realigned by stream_word() where it is used (a shift here would be a wait for the load)
            };
            auto stream_word = [&](uint32_t sp, uint64_t raw) -> uint64_t {
                if (tiny) return sp < 8 ? tiny_w >> (8 * sp) : 0;
                const uint32_t a0 = sp < fclen - 8 ? sp : fclen - 8;
                const uint32_t shb = 8 * (sp - a0);
                return shb < 64 ? raw >> shb : 0;
            };
            // UNITS of kP consecutive rounds (round 6; kP = MLZ_EXEC_PAIR, 2 by default, 1 = rounds 3-5): a wave prepares BOTH rounds of its unit —
            // parse, classification, requests and the unordered stores (part 1), their loads in flight together — then asks for the turn ONCE
            // and runs the ordered copies of the first round, then of the second.  The turn word counts units: half the hand-overs on a tile's
            // critical path (a hand-over, the poll that sees the new turn plus the first LDS round trip behind it, was 1.2 k of the 2.7 k cycles a
            // round's link of the chain took), and twice the loads in flight per wave for the part that is not on it.
            constexpr uint32_t kP = MLZ_EXEC_PAIR;
            static_assert(kP == 1 || kP == 2 || kP == 4, "one, two or four rounds per turn (64 % kP == 0)");
            struct Prep { CopyPlan plan; uint32_t len, off, dc, mine_v, iv_lo, iv_hi; uint64_t pmask, smask; };
            const uint32_t n_units = (j_last - j_first) / kP + 1;
            auto unit_of = [&](uint32_t ii) -> uint32_t { return uint32_t(wv) + uint32_t(kExecWaves) * ii; };   // ii: my ii-th unit
            auto round_of = [&](uint32_t ii, uint32_t sub) -> uint32_t { return j_first + kP * unit_of(ii) + sub; };
            // ---- part 1 of round j: everything before the turn (the body of rounds 3-5's loop, unchanged); leaves what the ordered copies need in `out` ----
            auto prep = [&](const uint32_t j, const uint32_t sp_c, const uint64_t w_t, const uint32_t Dbase, const uint32_t rep_in, Prep& out) {
                        const uint32_t R = (j << 6) + uint32_t(lane);
                        const bool is_tok = R < ntok && !bad;
                        // ---- parse ----
                        // (the table form: ~36 instructions and an LDS word against ~65 of decode_tok's select form)
                        Tok t;
                        const uint32_t tt = toktab[uint32_t(w_t) & 0xff];
                        const uint32_t ol = tok_olen(w_t, tt);
                        t.lit = tok_lit(ol, tt); t.cp = ol - t.lit; t.off = tok_off(uint32_t(w_t), tt); t.hdr = tok_adv(uint32_t(w_t), tt) - t.lit;
                        const uint32_t lit = is_tok ? t.lit : 0, len = is_tok ? t.cp : 0;
                        const uint32_t olen = lit + len;
                        const uint32_t incl = wave_incl_scan(olen);
                        const uint32_t dtok = Dbase + incl - olen;
                        const uint64_t expl = ballot64(is_tok && t.off != 0);
                        const uint64_t before = expl & ((1ull << lane) - 1);
                        const int srcl = before ? 63 - __builtin_clzll(before) : 0;
                        const uint32_t prev_off = __shfl(t.off, srcl);
                        const uint32_t off = t.off ? t.off : (before ? prev_off : rep_in);
                        MLZ_PHASE(4);

                        // ---- copies: validate, classify ----
                        const uint32_t dc = dtok + lit;
                        const bool is_cp = len != 0;
                        const bool invalid = is_cp && (off == 0 || off > dc || uint64_t(dc) + len > db.dlen);
                        const uint32_t lit_s = sp_c + t.hdr;                                   // stream offset of my first literal byte
                        const bool lit_bad = lit != 0 && uint64_t(lit_s) + lit > clen;
                        if (ballot64(invalid)) bad = 5;
                        else if (ballot64(lit_bad)) bad = 4;
                        const bool in_tile = !bad && is_cp && dc < tend && dc + len > tstart;
                        const uint32_t sw0 = dc - off;
                        const uint32_t sw1 = off >= len ? sw0 + len : dc;  // end of the source window
                        const bool far_src = in_tile && off >= len && sw1 <= tstart;  // plain copy that reads earlier tiles only
                        const bool cls_f = far_src && len <= 32 && dc >= tstart && dc + len <= tend && sw0 + 32 <= db.dlen;
                        const bool cls_l = far_src && !cls_f;
                        const bool p2 = in_tile && !far_src;
                        if (!all_known || (k >= 129 && ballot64(far_src && (k - 1 - (sw0 >> kTileLog)) >= 128))) {  // sources not covered by the up-front wait (rare)
                            uint64_t need = all_known ? ballot64(far_src && (k - 1 - (sw0 >> kTileLog)) >= 128) : ballot64(far_src);
                            while (need) {
                                const int fl = int(ctz64(need));
                                need &= need - 1;
                                const uint32_t a0 = rdlane(sw0, fl) >> kTileLog, a1 = (rdlane(sw1, fl) - 1) >> kTileLog;
                                for (uint32_t tt = a0; tt <= a1; tt++) wait_tile(tt);
                            }
                        }
                        // literals: F = up to 32 bytes, fetched like a far copy; L = the rest (long, clipped by the tile, or in the stream's last 32 bytes: wave loop).
                        // (Runs that fit the token's own 8 stream bytes had a path of their own — two exact stores from the register — until
                        // the F request went out with the copies': the request is made for all lanes anyway, and the pass is no slower with one path less.)
                        const bool l_in = !bad && lit != 0 && dtok < tend && dc > tstart;
                        const bool l_whole = l_in && dtok >= tstart && dc <= tend;
                        const bool lit_f = l_whole && lit <= 32 && uint64_t(lit_s) + 32 <= clen;
                        const bool lit_l = l_in && !lit_f;
                        // ---- requests: 32 source bytes + the last 8 of the copy, the same for literal runs; lanes without one read the dummy ----
                        // (four 8-byte pieces at offsets min(8k, max(n, 8) - 8): the clamped pieces re-read the tail, and the stores need no
                        // branch on the length within the class of 8 bytes and more).  Both requests go out here, before anything is stored.
                        auto piece_off = [](uint32_t n, uint32_t& o1, uint32_t& o2, uint32_t& o3) {
                            const uint32_t l8 = n >= 8 ? n - 8 : 0;
                            o1 = l8 < 8 ? l8 : 8; o2 = l8 < 16 ? l8 : 16; o3 = l8;
                        };
                        uint64_t fx0, fx1, fx2, fx3;
                        {
                            const bool f_ok = cls_f && !bad;
                            const uint8_t* sp = f_ok ? dst + sw0 : dummy;
                            uint32_t o1, o2, o3;
                            piece_off(f_ok ? len : 0, o1, o2, o3);
                            fx0 = ld64u(sp); fx1 = ld64u(sp + o1); fx2 = ld64u(sp + o2); fx3 = ld64u(sp + o3);
                        }
                        uint64_t lx0, lx1, lx2, lx3;   // the literal runs' (9 .. 32 bytes) request goes out with the copies': eight more registers in flight, dec_exec 0.344 -> 0.331 ms
                        {
                            const uint8_t* lp = lit_f && !bad ? src + lit_s : dummy;
                            uint32_t o1, o2, o3;
                            piece_off(lit_f && !bad ? lit : 0, o1, o2, o3);
                            lx0 = ld64u(lp); lx1 = ld64u(lp + o1); lx2 = ld64u(lp + o2); lx3 = ld64u(lp + o3);
                        }
                        // Which lanes of this round a simple copy has to wait for, exactly: destinations lie in lane order and do not
                        // overlap, so the tokens whose copied bytes intersect my source window [sw0, sw1) are a lane INTERVAL [a, h] —
                        // a = number of lanes whose copy ends at or below sw0, h = number of lanes whose copy starts below sw1, less one
                        // — found by two binary searches over the lanes' (monotone) copy starts and ends, six lane reads each.  A pass
                        // then costs an and + compare against the mask of copies still to do, and a round takes as many passes as its
                        // longest dependency chain (enwik-like: 3.0 / 2.3 / 2.0 on tiles of level 0 / 1 / 2) instead of 4.5 / 4.2 / 3.9
                        // with "my source ends below the lowest destination still to be written".
                        uint32_t iv_lo = 0, iv_hi = 0;
                        if (ballot64(!bad && p2)) {
                            const uint32_t cend = dc + len;
                            uint32_t nh = 0, na = 0;
#pragma unroll
                            for (uint32_t st = 32; st >= 1; st >>= 1) {
                                const uint32_t vh = uint32_t(__builtin_amdgcn_ds_bpermute(int((nh + st - 1) << 2), int(dc)));
                                const uint32_t va = uint32_t(__builtin_amdgcn_ds_bpermute(int((na + st - 1) << 2), int(cend)));
                                nh += vh < sw1 ? st : 0;      // lanes 0 .. nh-1 start their copy below sw1 (my own start is not below it: nh <= lane)
                                na += va <= sw0 ? st : 0;     // lanes 0 .. na-1 end their copy at or below sw0
                            }
                            // bits a .. nh-1
                            const uint64_t below_h = nh >= 64 ? ~0ull : (1ull << nh) - 1, below_a = na >= 64 ? ~0ull : (1ull << na) - 1;
                            const uint64_t iv = nh > na ? below_h & ~below_a : 0;
                            iv_lo = uint32_t(iv); iv_hi = uint32_t(iv >> 32);
                        }
                        asm volatile("" : "+v"(iv_lo), "+v"(iv_hi));
                        MLZ_PHASE(5);
                        // ---- long / clipped literal runs: 64 lanes per token, 8 bytes per lane ----
                        {
                            uint64_t lmask = ballot64(lit_l);
                            while (lmask) {
                                const int cl = int(ctz64(lmask));
                                lmask &= lmask - 1;
                                const uint32_t sd = rdlane(dtok, cl), sl = rdlane(lit, cl), ss = rdlane(lit_s, cl);
                                uint32_t j0_ = sd, j1 = sd + sl;
                                if (j0_ < tstart) j0_ = tstart;
                                if (j1 > tend) j1 = tend;
                                const uint8_t* sp = src + ss + (j0_ - sd);
                                uint8_t* dp = tilebuf + (j0_ - tstart);
                                const uint32_t n = j1 - j0_;
                                uint32_t q = lane * 8;
                                for (; q + 8 <= n; q += 512) {
                                    const uint64_t x = ld64u(sp + q);
                                    __builtin_memcpy(dp + q, &x, 8);
                                }
                                if (q < n) for (uint32_t rr = q; rr < n; rr++) dp[rr] = sp[rr];  // the one lane holding the ragged end
                            }
                        }
                        MLZ_PHASE(6);
                        // ---- store what was requested: literal runs, then copies from earlier tiles ----
                        auto store32 = [&](uint8_t* dp, uint32_t n, uint32_t o1, uint32_t o2, uint32_t o3, uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3) {
                            if (n >= 8) {
                                __builtin_memcpy(dp, &x0, 8);
                                __builtin_memcpy(dp + o1, &x1, 8);
                                __builtin_memcpy(dp + o2, &x2, 8);
                                __builtin_memcpy(dp + o3, &x3, 8);
                            } else if (n >= 4) {
                                const uint32_t y0 = uint32_t(x0), y1 = uint32_t(x0 >> (8 * (n - 4)));
                                __builtin_memcpy(dp, &y0, 4);
                                __builtin_memcpy(dp + n - 4, &y1, 4);
                            } else {
                                dp[0] = uint8_t(x0); dp[n >> 1] = uint8_t(x0 >> (8 * (n >> 1))); dp[n - 1] = uint8_t(x0 >> (8 * (n - 1)));
                            }
                        };
                        if (!bad) {
                            {
                                uint32_t o1, o2, o3;
                                piece_off(len, o1, o2, o3);
                                if (cls_f) store32(tilebuf + (dc - tstart), len, o1, o2, o3, fx0, fx1, fx2, fx3);
                            }
                            {
                                uint32_t o1, o2, o3;
                                piece_off(lit, o1, o2, o3);
                                if (lit_f) store32(tilebuf + (dtok - tstart), lit, o1, o2, o3, lx0, lx1, lx2, lx3);
                            }
                            // ---- long / clipped copies from earlier tiles: 64 lanes per token, 8 bytes per lane ----
                            uint64_t lmask = ballot64(cls_l);
                            while (lmask) {
                                const int cl = int(ctz64(lmask));
                                lmask &= lmask - 1;
                                const uint32_t sdc = rdlane(dc, cl), slen = rdlane(len, cl), soff = rdlane(off, cl);
                                uint32_t j0_ = sdc, j1 = sdc + slen;
                                if (j0_ < tstart) j0_ = tstart;
                                if (j1 > tend) j1 = tend;
                                const uint8_t* sp = dst + (j0_ - soff);
                                uint8_t* dp = tilebuf + (j0_ - tstart);
                                const uint32_t n = j1 - j0_;
                                uint32_t q = lane * 8;
                                for (; q + 8 <= n; q += 512) {
                                    const uint64_t x = ld64u(sp + q);
                                    __builtin_memcpy(dp + q, &x, 8);
                                }
                                if (q < n) for (uint32_t rr = q; rr < n; rr++) dp[rr] = sp[rr];
                            }
                        }
                        // ---- classification of the ordered copies (before the turn: only LDS traffic is serial) ----
                        const uint64_t pmask = ballot64(!bad && p2);
                        const bool simple = p2 && off >= len && len <= 32 && dc >= tstart && dc + len <= tend && sw0 >= tstart;
                        const uint64_t smask = ballot64(!bad && p2 && !simple);   // copies that go alone
                        if (bad && lane == 0) sh[2] = bad;
                        // what the ordered copies need, computed before the wait (-1 %)
                        CopyPlan plan = lds_copy_plan(tilebuf + (dc - tstart), tilebuf + (sw0 - tstart), len);
                        uint32_t mine_v = uint32_t((pmask >> lane) & 1);
                        {
                            uint32_t dpa = uint32_t(reinterpret_cast<uintptr_t>(plan.dp)), spa = uint32_t(reinterpret_cast<uintptr_t>(plan.sp));
                            asm volatile("" : "+v"(dpa), "+v"(spa), "+v"(plan.o1), "+v"(plan.o2), "+v"(plan.o3), "+v"(mine_v));
                            plan.dp = tilebuf + (dpa - uint32_t(reinterpret_cast<uintptr_t>(tilebuf)));
                            plan.sp = tilebuf + (spa - uint32_t(reinterpret_cast<uintptr_t>(tilebuf)));
                        }
                        out.plan = plan; out.len = len; out.off = off; out.dc = dc; out.mine_v = mine_v; out.iv_lo = iv_lo; out.iv_hi = iv_hi;
                        out.pmask = pmask; out.smask = smask;
                        MLZ_PHASE(0);
            };
            // ---- part 2 of a round: its ordered copies, in dependency passes ----
            auto passes = [&](const Prep& in) {
                        const CopyPlan plan = in.plan;
                        const uint32_t len = in.len, off = in.off, dc = in.dc, mine_v = in.mine_v, iv_lo = in.iv_lo, iv_hi = in.iv_hi;
                        const uint64_t pmask = in.pmask, smask = in.smask;
                        if (pmask) {
                            // Ordered copies of the round, in passes: a copy goes in the first pass in which none of the lanes in its
                            // dependency interval is still to do.  "Simple" copies (plain, <= 32 bytes, source and destination inside
                            // the tile) go lane-parallel; the others (overlapping, long, straddling the tile) one per pass with 64 lanes.
                            bool mine = mine_v != 0;          // my copy is still to be done
                            if (MLZ_PROFILE && prof && lane == 0) atomicAdd(const_cast<uint32_t*>(&sh[4]), uint32_t(__builtin_popcountll(smask)));   // (debug: copies that go alone)
                            while (true) {
                                const uint64_t todo = ballot64(mine);
                                if (!todo) break;
                                if (MLZ_PROFILE && prof && lane == 0) atomicAdd(const_cast<uint32_t*>(&sh[5]), 1u);   // (debug: passes)
                                // clear: nothing I read is still to be written.  The lowest copy left always is, so every pass makes progress.
                                const bool clear = mine && ((iv_lo & uint32_t(todo)) | (iv_hi & uint32_t(todo >> 32))) == 0;
                                const uint64_t ready_alone = ballot64(clear) & smask;
                                const bool go = clear && !((smask >> lane) & 1);
                                if (go) lds_copy_small(plan, len);
                                mine = mine && !go;
                                if (ready_alone) {   // one of the copies that take the whole wave (it was clear before this pass: it reads nothing this pass wrote)
                                    const int cl = int(ctz64(ready_alone));
                                    mine = mine && lane != cl;
                                    const uint32_t clen_c = rdlane(len, cl);
                                    const uint32_t soff = rdlane(off, cl);
                                    const uint32_t sdc = rdlane(dc, cl);
                                    uint32_t j0_ = sdc, j1 = sdc + clen_c;
                                    if (j0_ < tstart) j0_ = tstart;
                                    if (j1 > tend) j1 = tend;
                                    const uint32_t sfirst = sdc - soff;  // pre-copy window is [sdc-soff, sdc)
                                    if (sfirst < tstart) {
                                        // part of the window lies in earlier tiles: make sure they are published
                                        const uint32_t shi = (soff < clen_c ? sdc : sfirst + clen_c) - 1;  // last source byte used
                                        const uint32_t thi = (shi < tstart ? shi : tstart - 1) >> kTileLog;
                                        for (uint32_t tt = sfirst >> kTileLog; tt <= thi; tt++) wait_tile(tt);
                                        if (bad) break;
                                    }
                                    if (soff >= clen_c) {
                                        for (uint32_t j = j0_ + lane; j < j1; j += 64) {
                                            const uint32_t sj = sfirst + (j - sdc);
                                            tilebuf[j - tstart] = sj >= tstart ? tilebuf[sj - tstart] : dst[sj];
                                        }
                                    } else {  // overlapping: out[d+i] = out[d-off + i mod off] (decode.go:352-358)
                                        for (uint32_t j = j0_ + lane; j < j1; j += 64) {
                                            const uint32_t sj = sfirst + (j - sdc) % soff;
                                            tilebuf[j - tstart] = sj >= tstart ? tilebuf[sj - tstart] : dst[sj];
                                        }
                                    }
                                }
                            }
                        }
            };
            for (uint32_t i0 = 0; unit_of(i0) < n_units && !stop; i0 += 64 / kP) {
                // lane L holds the round words of round (L % kP) of my unit i0 + L / kP
                uint32_t d0_v = 0, rep_v = 0;
                {
                    const uint32_t jj = round_of(i0 + uint32_t(lane) / kP, uint32_t(lane) % kP);
                    if (jj <= j_last) { d0_v = rdv[jj]; rep_v = rrv[jj]; }
                }
                asm volatile("" : "+v"(d0_v), "+v"(rep_v));
                uint32_t p_a[kP], p_b[kP];
                uint64_t w_a[kP];
#pragma unroll
                for (uint32_t sub = 0; sub < kP; sub++) {
                    p_a[sub] = fetch_pos(round_of(i0, sub));          // positions of the rounds about to be processed
                    w_a[sub] = fetch_bytes(p_a[sub]);                 // their stream bytes
                    p_b[sub] = fetch_pos(round_of(i0 + 1, sub));      // positions of the rounds after them
                }
            for (uint32_t i = 0; i < 64 / kP; i++) {
                const uint32_t u = unit_of(i0 + i);
                if (u >= n_units) break;
                // this unit's stream bytes (requested while the previous unit was processed) are taken BEFORE the next requests
                // go out: the wait for them is then a wait for the oldest loads in flight only.
                uint32_t sp_c[kP];
                uint64_t w_t[kP];
#pragma unroll
                for (uint32_t sub = 0; sub < kP; sub++) {
                    sp_c[sub] = p_a[sub];
                    w_t[sub] = stream_word(sp_c[sub], w_a[sub]);
                    asm volatile("" : "+v"(w_t[sub]));
                }
#pragma unroll
                for (uint32_t sub = 0; sub < kP; sub++) {
                    p_a[sub] = p_b[sub];
                    w_a[sub] = fetch_bytes(p_a[sub]);                  // in flight while this unit is processed
                    p_b[sub] = fetch_pos(round_of(i0 + i + 2, sub));
                }
                uint32_t failed = 0;
                Prep P[kP];
#pragma unroll
                for (uint32_t sub = 0; sub < kP; sub++) {
                    const uint32_t j = round_of(i0 + i, sub);
                    P[sub].pmask = 0; P[sub].smask = 0; P[sub].mine_v = 0;
                    // (the unit's second round may lie beyond my tile's last one: nothing to do — its words were not fetched either)
                    if (j <= j_last) prep(j, sp_c[sub], w_t[sub], rdlane(d0_v, int(i * kP + sub)), rdlane(rep_v, int(i * kP + sub)), P[sub]);
                }
                {
                        // ---- my turn comes when every unit before mine is complete ----
                        if (!bad) {
                            uint32_t spins = 0;
                            while (true) {
                                const uint64_t ft = *reinterpret_cast<volatile uint64_t*>(tilebuf + kTile + 8);  // failure site, turn
                                failed = uint32_t(ft);
                                const uint32_t tn = uint32_t(ft >> 32);
                                if (tn == u || failed) break;
                                if (u - tn > 1) __builtin_amdgcn_s_sleep(1);   // next in line polls back to back (sleep 0 / 3, no priority raise below, poll sleep 2 / 32 above: all the same speed)
                                if (++spins > (1u << 26)) { bad = 6; break; }
                            }
                            asm volatile("" ::: "memory");
                            __builtin_amdgcn_s_setprio(3);   // the ordered section is the tile's critical path
                        }
                        MLZ_PHASE(1);
                        if (failed || bad) { if (bad && lane == 0) sh[2] = bad; stop = true; break; }  // some wave failed: the tile is abandoned
#pragma unroll
                        for (uint32_t sub = 0; sub < kP; sub++) passes(P[sub]);
                        if (bad) { if (lane == 0) sh[2] = bad; stop = true; break; }
                }
                // this unit is complete.  No wait for my LDS writes: the LDS executes a wave's operations in issue order,
                // so whoever reads the new counter value reads behind them.
                asm volatile("" ::: "memory");
                if (lane == 0) sh[3] = u + 1;
                __builtin_amdgcn_s_setprio(0);
                MLZ_PHASE(2);
            }
            }
            __syncthreads();
            if (trace && tid == 0)   // + (debug) copies that went alone (cap 4095) and passes / 4 (cap 4095) in the top bits
                trace[2] = (__builtin_amdgcn_s_memrealtime() & ((1ull << 40) - 1)) | (uint64_t(sh[4] < 4095 ? sh[4] : 4095) << 52) | (uint64_t((sh[5] >> 2) < 4095 ? (sh[5] >> 2) : 4095) << 40);
            bad = sh[2];
            MLZ_PHASE(3);
            // ---- flush the tile ----
            if (!bad) {
                const uint32_t n = tend - tstart;
                uint8_t* o = dst + tstart;
                if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                    const uint32_t nv = n >> 4;
                    const uint64_t oa = reinterpret_cast<uint64_t>(o);  // pinned to SGPRs: the store takes a scalar base
                    uint8_t* os = reinterpret_cast<uint8_t*>((uint64_t(rdfirst(uint32_t(oa >> 32))) << 32) | rdfirst(uint32_t(oa)));
                    for (uint32_t q = tid; q < nv; q += kExecThreads) store16_wt(os, 16 * q, reinterpret_cast<const uint4*>(tilebuf)[q]);
                    plain_stores = (n & 15) != 0;
                    for (uint32_t q = (nv << 4) + tid; q < n; q += kExecThreads) o[q] = tilebuf[q];
                } else {
                    plain_stores = true;
                    for (uint32_t q = tid; q < n; q += kExecThreads) o[q] = tilebuf[q];
                }
            }
        }
    }
    // A wait that gave up (site 6: a tile flag or the turn never came — liveness here rests on workgroups being dispatched in index order, which
    // the hardware does but HIP does not promise) is a DEVICE failure, not a verdict on the stream: status 7 = -MLZ_ERR_HIP, the one code
    // mlz_decode_block forwards as < 0 so that the Go shim falls back to minLZDecodeGo (dec_general_kernel's role S reports its waits the same way).
    if (bad && tid == 0) atomicExch(reinterpret_cast<int*>(&dec[bi].status), bad == 6 ? int(7 | (6 << 8)) : int(1 | (bad << 8)));
    // publish: every wave's stores have left the CU (write-through ones are then visible device-wide;
    // ordinary ones need the L2 write-back of a release fence), then one lane raises the flag
    if (plain_stores) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&done[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // Host-pointer calls with a pinned destination: the tile also goes straight into the caller's buffer (PCIe writes from
    // the kernel, after the tile is published so that no dependent tile waits for them) — there is no copy-out pass.
    if (b.mirror && !bad && db.status == 0 && tstart < db.dlen) {
        const uint32_t n = (tstart + kTile < db.dlen ? tstart + kTile : db.dlen) - tstart;
        uint8_t* mo = reinterpret_cast<uint8_t*>(b.mirror) + tstart;
        if ((reinterpret_cast<uintptr_t>(mo) & 15) == 0) {
            const uint32_t nv = n >> 4;
            for (uint32_t q = tid; q < nv; q += kExecThreads) reinterpret_cast<uint4*>(mo)[q] = reinterpret_cast<const uint4*>(tilebuf)[q];
            for (uint32_t q = (nv << 4) + tid; q < n; q += kExecThreads) mo[q] = tilebuf[q];
        } else {
            for (uint32_t q = tid; q < n; q += kExecThreads) mo[q] = tilebuf[q];
        }
    }
    if (trace && tid == 0) trace[3] = __builtin_amdgcn_s_memrealtime() | (uint64_t(tile_level_p(k, block_pattern(db))) << 60);
    MLZ_PHASE(3);
    if (MLZ_PROFILE && prof && tid == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&prof[8 + i], pc[i]);
#undef MLZ_PHASE
}

}  // namespace mlz
