// mlz_search_compressed.h — what the readers of compressed block search tables share (chunk 0x46, SPEC_SEARCH.md 2.2 and 2.2.1): the kernels
// that expand such tables once per handle (mlz_stream_search_compressed.hip.inc), the host call mlz_search_table_expand
// (include/minlz_hip_search_compressed.h) and the host check (tools/search_compressed_check.cpp).  A 0x46 chunk carries the fixed fields of
// a 0x45 chunk (`T M B field R crc`), then `h0_bs h0_tc`, h0_tc huff0 table descriptions and one record per sub-block of 2^h0_bs bitmap
// bytes: a table index 0 .. 15 with a uvarint length and four Huffman streams behind a jump table, 16 = the bytes themselves, 17 = one
// byte repeated, 18 = a sparse bit table.  Table descriptions and streams are RFC 8878 4.2's: direct 4-bit weights or FSE-compressed
// weights (two interleaved states, accuracy log 5 or 6), a decode table of 2^log entries (log <= 11), streams read backwards from an
// end marker.  Here: the parse of a chunk into at most 16 job records (cst_parse), the weights of a description (cst_weights), the decode
// table's layout and fill (cst_table_starts, cst_table_fill), one stream's decode loop (cst_decode_stream) and the sparse walk
// (cst_sparse_decode).  Every read is bounded by the chunk body the caller names: a malformed chunk yields an error, or garbage inside its
// own sub-block that the CRC then rejects, never a read outside [body, body + clen) or a write outside the sub-block.
// Behind the read side stands the write side (cst_w_*, cst_compress_host): a bitmap -> its huff0 section by the model's default writer's
// rule, shared by the host call mlz_search_bitmap_compress, the kernels of mlz_search_tables_compress.hip.inc and
// tools/search_compress_check.cpp.
// Plain C++: compiles for the host alone and for gfx950.  tests/search_compressed_model.py is the same format in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "mlz_stream_search.h"   // search_info, search_field_len; mlz_stream_walk.h's walk_uvarint

namespace mlz {

constexpr uint8_t kChunkSearchTableCompressed = 0x46;
constexpr uint32_t kCstRaw = 16, kCstRle = 17, kCstSparse = 18;
constexpr uint32_t kCstMaxTables = 16, kCstMaxSub = 16, kCstMinBs = 5, kCstMaxBs = 17;
constexpr uint32_t kCstMaxTableLog = 11, kCstMaxWeight = 12, kCstFseMaxLog = 6, kCstFseMaxSize = 1u << kCstFseMaxLog;
constexpr uint32_t kCstTableEntries = 1u << kCstMaxTableLog;

// One sub-block's work: kind (a table index, or kCstRaw / kCstRle / kCstSparse), where its bytes lie in the chunk body and where its
// 2^bs bitmap bytes go
struct CstJob { uint32_t kind, table, src_off, src_len, dst_off, rle; };
// A chunk as cst_parse leaves it.  ok = 0: refused.  n: the bitmap's bytes; tab_off[t]: table description t in the body
struct CstPlan {
    uint32_t ok, R, crc, bs, tc, nsub, n, pad;
    uint32_t tab_off[kCstMaxTables];
    CstJob job[kCstMaxSub];
};

// The fixed fields of a 0x46 payload against a stream's (T, M, B, field): the reductions R when they fit (B > R + 3 and room for
// `R crc h0_bs h0_tc`), else -1.  With f = search_field_len(T, field): R at p[3 + f], the CRC at p + 4 + f, h0_bs at p[8 + f].
// R <= B - 8 as in a 0x45 chunk: a sub-block has at least 32 bytes (h0_bs >= 5), so a smaller bitmap can be no valid chunk, and every
// candidate's bitmap is a power of two of at least 32 bytes.
MLZ_SEARCH_HD int cst_fixed_fields(const uint8_t* p, uint32_t clen, uint32_t M, uint32_t B, uint32_t T, const uint8_t* field) {
    const uint32_t f = search_field_len(T, field);
    if (clen < 10 + f || p[0] != T || p[1] != M || p[2] != B) return -1;
    for (uint32_t i = 0; i < f; i++) if (p[3 + i] != field[i]) return -1;
    const uint32_t R = p[3 + f];
    return R + 8 <= B ? int(R) : -1;
}

// The bytes of the table description at d (left: the body's bytes from d on), 0 when it does not fit: the sizes are self-described
MLZ_SEARCH_HD uint32_t cst_desc_len(const uint8_t* d, uint32_t left) {
    if (left < 1) return 0;
    const uint32_t h = d[0], len = h >= 128 ? 1 + (h - 127 + 1) / 2 : 1 + h;
    return h == 0 || len > left ? 0 : len;
}

// body[0, clen) with a field of f bytes and a base table size B -> *out.  Returns out->ok.
MLZ_SEARCH_HD bool cst_parse(const uint8_t* body, uint32_t clen, uint32_t f, uint32_t B, CstPlan* out) {
    out->ok = 0;
    if (clen < 10 + f) return false;
    const uint8_t* q = body + 3 + f;
    const uint32_t R = q[0], bs = q[5], tc = q[6];
    out->R = R; out->bs = bs; out->tc = tc;
    out->crc = uint32_t(q[1]) | uint32_t(q[2]) << 8 | uint32_t(q[3]) << 16 | uint32_t(q[4]) << 24;
    if (bs < kCstMinBs || bs > kCstMaxBs || tc > kCstMaxTables || B <= R + 3 || B - R - 3 > 20) return false;
    const uint32_t lg = B - R - 3;
    if (lg < bs || lg - bs > 4) return false;   // n = 2^lg divisible by the sub-block size, 1 .. 16 sub-blocks
    const uint32_t n = 1u << lg, sub = 1u << bs, nsub = n >> bs;
    out->n = n; out->nsub = nsub;
    uint32_t p = 10 + f;
    for (uint32_t t = 0; t < tc; t++) {
        const uint32_t len = cst_desc_len(body + p, clen - p);
        if (!len) return false;
        out->tab_off[t] = p;
        p += len;
    }
    for (uint32_t j = 0; j < nsub; j++) {
        if (p >= clen) return false;
        const uint32_t kind = body[p++];
        CstJob jb{kind, kind < 16 ? kind : 0, 0, 0, j << bs, 0};
        if (kind < 16 || kind == kCstSparse) {
            if (kind < 16 && kind >= tc) return false;
            uint64_t len = 0;
            const int used = walk_uvarint(body + p, clen - p, &len);
            if (used <= 0) return false;
            p += uint32_t(used);
            if (len > clen - p) return false;
            jb.src_off = p; jb.src_len = uint32_t(len);
            p += uint32_t(len);
        } else if (kind == kCstRaw) {
            if (sub > clen - p) return false;
            jb.src_off = p; jb.src_len = sub;
            p += sub;
        } else if (kind == kCstRle) {
            if (p >= clen) return false;
            jb.rle = body[p++];
        } else {
            return false;
        }
        out->job[j] = jb;
    }
    if (p != clen) return false;
    out->ok = 1;
    return true;
}

// ---- the weights of a table description ----

MLZ_SEARCH_HD uint32_t cst_highbit(uint32_t v) { uint32_t b = 0; while (v >>= 1) b++; return b; }

// n <= 16 bits from bit `pos` of s[0, len) on, little-endian; bytes beyond len read as zeros
MLZ_SEARCH_HD uint32_t cst_bits(const uint8_t* s, uint32_t len, uint32_t pos, uint32_t n) {
    const uint32_t i = pos >> 3;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 3; k++) if (i + k < len) v |= uint32_t(s[i + k]) << (8 * k);
    return (v >> (pos & 7)) & ((1u << n) - 1);
}

// FSE-compressed weights: s[0, len) = table description + the stream of two interleaved states -> w[0, return value), 0 for a section
// that is refused.  At most 255 weights.
struct CstFseScratch {   // the counts and the decode table of a weight section: the caller's memory (the kernel's lies in LDS)
    int8_t norm[kCstMaxWeight + 1];
    uint8_t nxt[kCstMaxWeight + 1], sym[kCstFseMaxSize], nbits[kCstFseMaxSize], base[kCstFseMaxSize];
};
MLZ_SEARCH_HD uint32_t cst_fse_weights(const uint8_t* s, uint32_t len, uint8_t* w, CstFseScratch* fs) {
    int8_t* norm = fs->norm;
    uint8_t *sym = fs->sym, *nbits = fs->nbits, *nxt = fs->nxt, *base = fs->base;
    if (len < 1) return 0;
    const uint32_t avail = 8 * len, log = (s[0] & 15) + 5;
    if (log > kCstFseMaxLog) return 0;
    const uint32_t size = 1u << log;
    uint32_t pos = 4, nsym = 0, threshold = size, nb = log + 1;
    int remaining = int(size) + 1;
    bool prev0 = false;
    while (remaining > 1 && nsym <= kCstMaxWeight) {
        if (prev0) {
            uint32_t n0 = nsym;
            while (cst_bits(s, len, pos, 2) == 3) { n0 += 3; pos += 2; if (pos > avail) return 0; }
            n0 += cst_bits(s, len, pos, 2);
            pos += 2;
            if (n0 > kCstMaxWeight) return 0;
            while (nsym < n0) norm[nsym++] = 0;
        }
        const int mx = int(2 * threshold - 1) - remaining;
        int count = int(cst_bits(s, len, pos, nb - 1));
        if (count < mx) pos += nb - 1;
        else {
            count = int(cst_bits(s, len, pos, nb));
            if (count >= int(threshold)) count -= mx;
            pos += nb;
        }
        count--;
        remaining -= count < 0 ? -count : count;
        norm[nsym++] = int8_t(count);
        prev0 = count == 0;
        while (remaining < int(threshold)) { nb--; threshold >>= 1; }
        if (pos > avail) return 0;
    }
    if (remaining != 1) return 0;
    const uint32_t used = (pos + 7) >> 3;
    // the decode table: symbols of probability "less than one" from the top, the others spread
    uint32_t high = size - 1;
    for (uint32_t i = 0; i < nsym; i++) {
        if (norm[i] == -1) { sym[high--] = uint8_t(i); nxt[i] = 1; }
        else nxt[i] = uint8_t(norm[i]);
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t at = 0;
    for (uint32_t i = 0; i < nsym; i++)
        for (int k = 0; k < norm[i]; k++) {
            sym[at] = uint8_t(i);
            at = (at + step) & mask;
            while (at > high) at = (at + step) & mask;
        }
    if (at != 0) return 0;
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t x = nxt[sym[u]]++;
        nbits[u] = uint8_t(log - cst_highbit(x));
        base[u] = uint8_t((x << nbits[u]) - size);
    }
    // the stream, read backwards from its end marker
    const uint8_t* b = s + used;
    const uint32_t m = len - used;
    if (used >= len || b[m - 1] == 0) return 0;
    int left = int(8 * (m - 1) + cst_highbit(b[m - 1]));   // bits below the end marker
    auto read = [&](uint32_t n) -> uint32_t {
        left -= int(n);
        if (left >= 0) return cst_bits(b, m, uint32_t(left), n);
        const int have = int(n) + left;                   // the bits that exist, zeros below them
        return have > 0 ? (cst_bits(b, m, 0, uint32_t(have)) << uint32_t(-left)) : 0;
    };
    uint32_t st[2];
    st[0] = read(log);
    st[1] = read(log);
    if (left < 0) return 0;
    uint32_t nw = 0, i = 0;
    for (;;) {
        if (nw > 253) return 0;
        w[nw++] = sym[st[i]];
        st[i] = base[st[i]] + read(nbits[st[i]]);
        if (left < 0) { w[nw++] = sym[st[i ^ 1]]; return nw; }   // a read beyond the first bit: the other state's symbol is the last
        i ^= 1;
    }
}

// The description at d[0, dlen) (dlen = cst_desc_len) -> w[0, 256): every symbol's weight, the implied last one included, zeros behind it.
// Returns the table log 1 .. 11, or 0: weights that miss a power of two, a log above 11, fewer than two symbols, a refused FSE section.
MLZ_SEARCH_HD uint32_t cst_weights(const uint8_t* d, uint32_t dlen, uint8_t* w, CstFseScratch* fs) {
    uint32_t nw;
    if (d[0] >= 128) {
        nw = d[0] - 127u;
        for (uint32_t i = 0; i < nw; i++) w[i] = (i & 1) ? d[1 + i / 2] & 15 : d[1 + i / 2] >> 4;
    } else {
        nw = cst_fse_weights(d + 1, dlen - 1, w, fs);
        if (!nw) return 0;
    }
    uint32_t total = 0, used = 0;
    for (uint32_t i = 0; i < nw; i++) {
        if (w[i] > kCstMaxWeight) return 0;
        total += (1u << w[i]) >> 1;
        used += w[i] ? 1 : 0;
    }
    if (!total) return 0;
    const uint32_t log = cst_highbit(total) + 1;
    if (log > kCstMaxTableLog) return 0;
    const uint32_t rest = (1u << log) - total;
    if ((rest & (rest - 1)) || nw > 255 || used < 1) return 0;
    w[nw] = uint8_t(cst_highbit(rest) + 1);
    for (uint32_t i = nw + 1; i < 256; i++) w[i] = 0;
    return log;
}

// The decode table's layout: symbols by ascending weight, by value within a weight; symbol s takes the 2^(w - 1) entries from start[s] on
MLZ_SEARCH_HD void cst_table_starts(const uint8_t* w, uint32_t log, uint16_t* start) {
    uint32_t at = 0;
    for (uint32_t wt = 1; wt <= log; wt++)
        for (uint32_t s = 0; s < 256; s++)
            if (w[s] == wt) { start[s] = uint16_t(at); at += 1u << (wt - 1); }
}

// The entries of the 2^log table, two bytes each (symbol | bits << 8): worker `lane` of `lanes` writes its share of every symbol's span
MLZ_SEARCH_HD void cst_table_fill(const uint8_t* w, const uint16_t* start, uint32_t log, uint16_t* table, uint32_t lane, uint32_t lanes) {
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t wt = w[s];
        if (!wt) continue;
        const uint32_t span = 1u << (wt - 1);
        const uint16_t e = uint16_t(s | (log + 1 - wt) << 8);
        for (uint32_t i = lane; i < span; i += lanes) table[start[s] + i] = e;
    }
}

// One stream: s[0, len) read backwards from its end marker -> `count` symbols at dst.  The 64-bit container is refilled 32 bits at a time
// from bytes at or above s[0] only; the next 32 bits are loaded one refill ahead (`ahead`), so that the load's latency lies behind the
// symbols in between, and eight symbols leave in one store.  True when the stream holds an end marker, never runs beyond its first bit
// and ends exactly there.  (Little-endian hosts.)
MLZ_SEARCH_HD uint32_t cst_load32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
MLZ_SEARCH_HD bool cst_decode_stream(const uint8_t* s, uint32_t len, const uint16_t* table, uint32_t log, uint8_t* dst, uint32_t count) {
    if (len == 0 || s[len - 1] == 0) return false;
    uint32_t p = len - 1;
    // The container holds the stream's next `nbit` bits at its top and zeros below them: a lookup beyond the first bit reads zeros, and
    // nbit, which then goes below zero and stays there (nothing is refilled once p is 0), is looked at behind the loop.
    int nbit = int(cst_highbit(s[p]));
    uint64_t acc = nbit ? uint64_t(s[p]) << (64 - nbit) : 0;   // (the marker itself is shifted out)
    // s[p - 4, p) while there are four bytes below p; else four bytes that are never used (the load stands unconditionally, so that it
    // can stay in flight until the next refill)
    uint32_t ahead = len >= 4 ? cst_load32(s + (p >= 4 ? p - 4 : 0)) : 0;
    uint64_t out = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (nbit <= 32) {
            if (p >= 4) {
                p -= 4;
                acc |= uint64_t(ahead) << (32 - nbit);
                nbit += 32;
                ahead = cst_load32(s + (p >= 4 ? p - 4 : 0));
            } else {
                while (p > 0) { p--; acc |= uint64_t(s[p]) << (56 - nbit); nbit += 8; }
            }
        }
        const uint32_t e = table[uint32_t(acc >> 32) >> (32 - log)];
        acc <<= e >> 8;
        nbit -= int(e >> 8);
        out |= uint64_t(e & 0xff) << (8 * (i & 7));
        if ((i & 7) == 7) { memcpy(dst + i - 7, &out, 8); out = 0; }
    }
    for (uint32_t i = count & ~7u; i < count; i++) dst[i] = uint8_t(out >> (8 * (i & 7)));
    return p == 0 && nbit == 0;
}

// A tabled sub-block's four streams: src[0, len) = jump table + streams, n = 2^bs symbols.  Stream q (0 .. 3) -> where it lies and what it
// decodes; false for sizes beyond the sub-block's bytes.
struct CstStream { uint32_t off, len, dst_off, count; };
MLZ_SEARCH_HD bool cst_stream_of(const uint8_t* src, uint32_t len, uint32_t n, uint32_t q, CstStream* out) {
    if (len < 6) return false;
    const uint32_t l1 = src[0] | uint32_t(src[1]) << 8, l2 = src[2] | uint32_t(src[3]) << 8, l3 = src[4] | uint32_t(src[5]) << 8;
    if (6 + l1 + l2 + l3 > len) return false;
    const uint32_t seg = (n + 3) / 4;
    const uint32_t off[5] = {6, 6 + l1, 6 + l1 + l2, 6 + l1 + l2 + l3, len};
    *out = CstStream{off[q], off[q + 1] - off[q], q * seg, q < 3 ? seg : n - 3 * seg};
    return true;
}

// A sparse bit table: src[0, len) = the gaps between set bits (255: add and go on) -> dst[0, n), zeroed here.  False for a position at or
// beyond the bit count and for a table that ends in 255.  (The kernel walks 64 bytes a round by a scan; the rule is this one.)
MLZ_SEARCH_HD bool cst_sparse_decode(const uint8_t* src, uint32_t len, uint8_t* dst, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) dst[i] = 0;
    uint64_t pos = 0, gap = 0;
    for (uint32_t i = 0; i < len; i++) {
        gap += src[i];
        if (src[i] == 255) continue;
        pos += gap;
        if (pos >= uint64_t(n) * 8) return false;
        dst[pos >> 3] |= uint8_t(1u << (pos & 7));
        pos++;
        gap = 0;
    }
    return gap == 0;
}

// A bitmap's room in the arena: whole 16-byte units, so that every bitmap starts where 16-byte stores and dword atomics may go whatever
// the sizes in front of it are
MLZ_SEARCH_HD uint64_t cst_arena_slot(uint64_t n) { return (n + 15) & ~uint64_t(15); }

// What the candidates of one locate round become (cst_resolve's rule; the host checks run it too).  Candidate i is (*tabs)[who[i]], its
// bitmap of sizes[i] bytes lies at arena_off[i].  ok == nullptr: there is no arena (it could not be allocated) and every candidate counts
// as NO TABLE, nothing is skipped.  Else a candidate with ok[i] == 0 (the parse or the decode refused it), or, with crc != nullptr, whose
// bitmap's CRC crc[i] is not the one its chunk states, is passed over: skip[who[i]]++, and the return value says "locate once more"; every
// other candidate becomes a table in the arena (off = arena_off[i], bytes = sizes[i], pad stays kSearchTabArena).
inline bool cst_settle(std::vector<SearchTab>* tabs, const std::vector<size_t>& who, const uint64_t* arena_off, const uint64_t* sizes, const uint32_t* ok, const uint32_t* crc,
                       std::vector<uint32_t>* skip) {
    bool again = false;
    for (size_t i = 0; i < who.size(); i++) {
        SearchTab& t = (*tabs)[who[i]];
        if (!ok) { t = SearchTab{0, 0, kSearchNoTable, 0, 0}; continue; }
        if (!ok[i] || (crc && crc[i] != t.crc)) { (*skip)[who[i]]++; again = true; continue; }
        t.off = arena_off[i];
        t.bytes = uint32_t(sizes[i]);
    }
    return again;
}

// The masked CRC32C of a table's bytes on the host (the device has the CRC pass of mlz_crc.hip.inc)
inline uint32_t cst_crc_host(const uint8_t* p, size_t n) {
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82f63b78u & (0u - (c & 1)));
    }
    c = ~c;
    return (c >> 15 | c << 17) + 0xa282ead8u;
}

// The whole expansion in plain loops (the host call and the host check): body[0, clen), whose fixed fields state a valid configuration ->
// bitmap[0, cap).  Returns the bitmap's bytes, 0 for a chunk that is refused (the CRC is the caller's), -1 when cap is too small.
inline int64_t cst_expand_host(const uint8_t* body, uint32_t clen, uint8_t* bitmap, size_t cap, CstPlan* plan) {
    uint32_t T, M, B;
    uint8_t field[kSearchMaxField];
    if (!search_info(body, clen, &T, &M, &B, field)) return 0;
    if (!cst_parse(body, clen, search_field_len(T, field), B, plan)) return 0;
    if (plan->n > cap) return -1;
    std::vector<uint16_t> tables(size_t(plan->tc) * kCstTableEntries);
    uint32_t logs[kCstMaxTables];
    uint8_t w[256];
    uint16_t start[256];
    CstFseScratch fs;
    for (uint32_t t = 0; t < plan->tc; t++) {
        const uint8_t* d = body + plan->tab_off[t];
        logs[t] = cst_weights(d, cst_desc_len(d, clen - plan->tab_off[t]), w, &fs);
        if (!logs[t]) return 0;
        cst_table_starts(w, logs[t], start);
        cst_table_fill(w, start, logs[t], tables.data() + size_t(t) * kCstTableEntries, 0, 1);
    }
    const uint32_t sub = 1u << plan->bs;
    for (uint32_t j = 0; j < plan->nsub; j++) {
        const CstJob& jb = plan->job[j];
        uint8_t* dst = bitmap + jb.dst_off;
        const uint8_t* src = body + jb.src_off;
        if (jb.kind == kCstRaw) memcpy(dst, src, sub);
        else if (jb.kind == kCstRle) memset(dst, int(jb.rle), sub);
        else if (jb.kind == kCstSparse) { if (!cst_sparse_decode(src, jb.src_len, dst, sub)) return 0; }
        else
            for (uint32_t q = 0; q < 4; q++) {
                CstStream st;
                if (!cst_stream_of(src, jb.src_len, sub, q, &st)) return 0;
                if (!cst_decode_stream(src + st.off, st.len, tables.data() + size_t(jb.table) * kCstTableEntries, logs[jb.table], dst + st.dst_off, st.count)) return 0;
            }
    }
    return int64_t(plan->n);
}

// ---- the write side: a bitmap -> its huff0 section (`h0_bs h0_tc | table descriptions | sub-blocks`, what a 0x46 payload carries behind
// the CRC).  The rule is tests/search_compressed_model.py's default writer, byte for byte: the partition cst_w_bs; per sub-block one byte
// value -> RLE, else the smallest of raw (sub), sparse (its bytes + 3) and huff (description + 9 + ceil(bits / 8) + 3), ties in that
// order; a table of its own per tabled sub-block.  The host call (cst_compress_host), the kernels (mlz_search_tables_compress.hip.inc)
// and tools/search_compress_check.cpp share what follows. ----

// The partition: bitmaps up to 32 KiB are one sub-block; up to 512 KiB, 32 KiB sub-blocks; else 64 KiB ones.  n: a power of two
MLZ_SEARCH_HD uint32_t cst_w_bs(uint32_t n) { return n <= (32u << 10) ? cst_highbit(n) : n <= (512u << 10) ? 15u : 16u; }
MLZ_SEARCH_HD bool cst_w_size_ok(uint64_t n) { return n >= 32 && n <= (1u << 20) && !(n & (n - 1)); }
// The longest section of an n-byte bitmap: every sub-block raw
MLZ_SEARCH_HD uint32_t cst_w_bound(uint32_t n) { return n + 2 + kCstMaxSub; }

// Code lengths.  Nodes are merged two at a time, the smallest first by (weight, smallest symbol in the node); where the tree is deeper
// than 11 all counts are halved once more (max(1, count >> shift)) and the tree is built again.  A slot holds a live node: key =
// weight << 8 | smallest symbol (weights are at most 2^16), ~0 for none; node ids 0 .. 255 are the symbols, 256 .. 510 the merges in the
// order they were made, so that a parent's id is above its children's.
struct CstHuffScratch { uint32_t key[256]; uint16_t node[256], parent[512]; uint8_t d[512]; };
constexpr uint32_t kCstNoNode = 0xffffffffu;

// The keys of a round: symbol s of the histogram under `shift`
MLZ_SEARCH_HD uint32_t cst_w_key(uint32_t count, uint32_t shift, uint32_t s) {
    if (!count) return kCstNoNode;
    const uint32_t w = count >> shift;
    return (w ? w : 1u) << 8 | s;
}
// Two nodes' keys -> their merge's
MLZ_SEARCH_HD uint32_t cst_w_merge_key(uint32_t ka, uint32_t kb) {
    const uint32_t sa = ka & 255, sb = kb & 255;
    return ((ka >> 8) + (kb >> 8)) << 8 | (sa < sb ? sa : sb);
}
// parent[] of `nodes` ids (root = nodes - 1) -> depth[s] of the symbols with hist[s] > 0, 0 for the others.  Returns the largest depth.
MLZ_SEARCH_HD uint32_t cst_w_depths(const uint32_t* hist, uint32_t nodes, CstHuffScratch* hs, uint8_t* depth) {
    uint32_t deepest = 0;
    hs->d[nodes - 1] = 0;
    for (uint32_t id = nodes - 1; id-- > 0;) {
        if (id < 256 && !hist[id]) { depth[id] = 0; continue; }
        const uint32_t dd = hs->d[hs->parent[id]] + 1u;
        hs->d[id] = uint8_t(dd);
        if (id < 256) { depth[id] = uint8_t(dd); if (dd > deepest) deepest = dd; }
    }
    return deepest;
}
// hist[256] with at least two counts above 0 -> depth[256]; returns the table log (the deepest leaf, 1 .. 11); *out_shift: the halvings
inline uint32_t cst_w_code_lengths(const uint32_t* hist, uint8_t* depth, CstHuffScratch* hs, uint32_t* out_shift) {
    for (uint32_t shift = 0;; shift++) {
        uint32_t live = 0, next = 256;
        for (uint32_t s = 0; s < 256; s++) {
            hs->key[s] = cst_w_key(hist[s], shift, s);
            hs->node[s] = uint16_t(s);
            live += hist[s] ? 1 : 0;
        }
        while (live > 1) {
            uint32_t a = 0, b = 0, ka = kCstNoNode, kb = kCstNoNode;   // the smallest and the next
            for (uint32_t s = 0; s < 256; s++) {
                const uint32_t k = hs->key[s];
                if (k < ka) { kb = ka; b = a; ka = k; a = s; }
                else if (k < kb) { kb = k; b = s; }
            }
            hs->parent[hs->node[a]] = hs->parent[hs->node[b]] = uint16_t(next);
            hs->key[a] = cst_w_merge_key(ka, kb);
            hs->node[a] = uint16_t(next++);
            hs->key[b] = kCstNoNode;
            live--;
        }
        const uint32_t deepest = cst_w_depths(hist, next, hs, depth);
        if (deepest <= kCstMaxTableLog) { if (out_shift) *out_shift = shift; return deepest; }
    }
}

// depth[256], log -> w[256] (weight log + 1 - depth, 0 for an absent symbol) and the canonical codes: symbols by ascending weight, by
// value within a weight; code[s] = code | length << 16.  Returns `last`, the largest present symbol: the description lists w[0, last).
MLZ_SEARCH_HD uint32_t cst_w_codes(const uint8_t* depth, uint32_t log, uint8_t* w, uint32_t* code) {
    uint32_t last = 0;
    for (uint32_t s = 0; s < 256; s++) {
        w[s] = depth[s] ? uint8_t(log + 1 - depth[s]) : 0;
        code[s] = 0;
        if (depth[s]) last = s;
    }
    uint32_t at = 0;
    for (uint32_t wt = 1; wt <= log; wt++)
        for (uint32_t s = 0; s < 256; s++)
            if (w[s] == wt) { code[s] = (at >> (wt - 1)) | (log + 1 - wt) << 16; at += 1u << (wt - 1); }
    return last;
}

// v's low k bits (k <= 16) at bit `pos` of a zeroed buffer, little-endian
MLZ_SEARCH_HD void cst_w_put(uint8_t* buf, uint32_t pos, uint32_t v, uint32_t k) {
    uint32_t x = (v & ((1u << k) - 1)) << (pos & 7);
    for (uint32_t i = pos >> 3; x; i++, x >>= 8) buf[i] |= uint8_t(x);
}

// FSE-compressed weights: w[0, n), 2 <= n <= 255, each at most 11 -> out[0, return value), the model's fse_encode_weights: accuracy log
// 6, counts c * 64 / n rounded and at least 1, the largest (the first of them) moved until they sum to 64; one value only: a second
// symbol of probability 1 that never occurs; the two-state stream written from the decoder's last read up.  out: kCstFseOutCap bytes.
constexpr uint32_t kCstFseOutCap = 256;   // a description of at most 13 counts (below 20 bytes) and at most 253 * 6 + 12 + 1 bits of stream
MLZ_SEARCH_HD uint32_t cst_w_fse_weights(const uint8_t* w, uint32_t n, uint8_t* out, CstFseScratch* fs) {
    if (n < 2) return 0;
    const uint32_t log = kCstFseMaxLog, size = 1u << log;
    uint32_t hist[kCstMaxWeight + 1], nsym = 0, present = 0, only = 0;
    int norm[kCstMaxWeight + 2];
    for (uint32_t i = 0; i <= kCstMaxWeight; i++) hist[i] = 0;
    for (uint32_t i = 0; i < n; i++) { hist[w[i]]++; if (w[i] + 1u > nsym) nsym = w[i] + 1u; }
    for (uint32_t i = 0; i < nsym; i++) if (hist[i]) { present++; only = i; }
    for (uint32_t i = 0; i < kCstMaxWeight + 2; i++) norm[i] = 0;
    if (present == 1) {
        const uint32_t spare = only ? 0 : 1;
        if (spare + 1 > nsym) nsym = spare + 1;
        norm[only] = int(size) - 1;
        norm[spare] = 1;
    } else {
        int sum = 0;
        for (uint32_t i = 0; i < nsym; i++) {
            if (hist[i]) { const uint32_t v = (hist[i] * size + n / 2) / n; norm[i] = v ? int(v) : 1; }
            sum += norm[i];
        }
        while (sum != int(size)) {
            uint32_t big = 0;
            for (uint32_t i = 1; i < nsym; i++) if (norm[i] > norm[big]) big = i;
            const int step = sum < int(size) ? 1 : -1;
            norm[big] += step;
            sum += step;
        }
    }
    for (uint32_t i = 0; i < kCstFseOutCap; i++) out[i] = 0;
    // the description
    cst_w_put(out, 0, log - 5, 4);
    uint32_t pos = 4, threshold = size, nb = log + 1, s = 0;
    int remaining = int(size) + 1;
    while (remaining > 1) {
        int count = norm[s] + 1;
        const int mx = int(2 * threshold) - 1 - remaining;
        if (count >= int(threshold)) count += mx;
        cst_w_put(out, pos, uint32_t(count), nb);
        pos += count < mx ? nb - 1 : nb;
        remaining -= norm[s];
        while (remaining < int(threshold)) { nb--; threshold >>= 1; }
        s++;
        if (norm[s - 1] == 0 && remaining > 1) {
            const uint32_t n0 = s;
            while (s < nsym && norm[s] == 0) s++;
            uint32_t run = s - n0;
            while (run >= 3) { cst_w_put(out, pos, 3, 2); pos += 2; run -= 3; }
            cst_w_put(out, pos, run, 2);
            pos += 2;
        }
    }
    const uint32_t used = (pos + 7) >> 3;
    // The decode table's states as the reader builds them (no count is "less than one"): the spread, then per symbol its states in ascending
    // order, list[cum[v] + k] the k-th of symbol v.  That state has x = norm[v] + k, reads log - highbit(x) bits and its range starts at
    // (x << bits) - size: the ranges of a symbol's states tile 0 .. size - 1.
    uint8_t *sym = fs->sym, *nxt = fs->nxt, *list = fs->nbits, *cum = fs->base;   // (nbits and base lend their bytes: size and 13 of them)
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t at = 0, run = 0;
    for (uint32_t i = 0; i < nsym; i++) {
        cum[i] = uint8_t(run);
        run += uint32_t(norm[i]);
        nxt[i] = 0;
        for (int k = 0; k < norm[i]; k++) { sym[at] = uint8_t(i); at = (at + step) & mask; }
    }
    for (uint32_t u = 0; u < size; u++) list[cum[sym[u]] + nxt[sym[u]]++] = uint8_t(u);
    // the stream.  The decoder reads init(state 0), init(state 1), then the update behind weight 0, 1, ..., n - 3; written here from the
    // last of these reads, which lies lowest.  A final state is the symbol's first state (the most bits, the first of them); an earlier
    // one the symbol's state whose range holds the state that follows: with s = that state + size, x = s >> bits lies in [norm, 2 norm).
    uint8_t* b = out + used;
    uint32_t tot = 0, st[2] = {size, size};
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t c = i & 1, v = w[i], cnt = uint32_t(norm[v]);
        if (st[c] == size) { st[c] = list[cum[v]]; continue; }
        const uint32_t s = st[c] + size;
        uint32_t nb = log - cst_highbit(cnt), x = s >> nb;
        if (x < cnt) { nb--; x = s >> nb; }
        cst_w_put(b, tot, s - (x << nb), nb);
        tot += nb;
        st[c] = list[cum[v] + x - cnt];
    }
    cst_w_put(b, tot, st[1], log);
    tot += log;
    cst_w_put(b, tot, st[0], log);
    tot += log;
    cst_w_put(b, tot, 1, 1);
    return used + ((tot + 8) >> 3);
}

// The description of w[0, last), last >= 1: direct 4-bit weights where last <= 128, FSE-compressed where that section has fewer than 128
// bytes, the shorter of them, direct in a tie -> desc[0, return value), at most 129 bytes; 0 where neither form carries the weights.
// desc: 1 + kCstFseOutCap bytes (the FSE section is written in place and kept or overwritten).
MLZ_SEARCH_HD uint32_t cst_w_description(const uint8_t* w, uint32_t last, uint8_t* desc, CstFseScratch* fs) {
    const uint32_t direct = last <= 128 ? 1 + (last + 1) / 2 : 0;
    uint32_t fse = cst_w_fse_weights(w, last, desc + 1, fs);
    fse = fse && fse < 128 ? fse + 1 : 0;
    if (fse && (!direct || fse < direct)) { desc[0] = uint8_t(fse - 1); return fse; }
    if (!direct) return 0;
    desc[0] = uint8_t(127 + last);
    for (uint32_t i = 0; i < (last + 1) / 2; i++) desc[1 + i] = uint8_t(w[2 * i] << 4 | (2 * i + 1 < last ? w[2 * i + 1] : 0));
    return direct;
}

// The kind of a sub-block with more than one byte value: sparse_len = the sparse table's bytes; desc_len = 0: no description, huff is no
// candidate; bits = the sum of the code lengths of its bytes.  -> kCstRaw, kCstSparse or 0 (a table of its own)
MLZ_SEARCH_HD uint32_t cst_w_pick(uint32_t sub, uint32_t sparse_len, uint32_t desc_len, uint32_t bits) {
    const uint32_t raw = sub, sparse = sparse_len + 3, huff = desc_len ? desc_len + 9 + (bits + 7) / 8 + 3 : 0xffffffffu;
    if (raw <= sparse && raw <= huff) return kCstRaw;
    return sparse <= huff ? kCstSparse : 0;
}

MLZ_SEARCH_HD uint32_t cst_w_uvarint_len(uint32_t v) { return v < 0x80 ? 1 : v < 0x4000 ? 2 : v < 0x200000 ? 3 : 4; }
MLZ_SEARCH_HD uint32_t cst_w_put_uvarint(uint8_t* p, uint32_t v) {
    uint32_t i = 0;
    while (v >= 0x80) { p[i++] = uint8_t(v | 0x80); v >>= 7; }
    p[i++] = uint8_t(v);
    return i;
}
// The bytes a gap of `gap` zeros in front of a set bit takes in a sparse table: a 255 per full 255, then the rest
MLZ_SEARCH_HD uint32_t cst_w_gap_bytes(uint32_t gap) { return gap / 255 + 1; }

// One stream of a tabled sub-block: data[0, count) -> out[0, return value): the codes from the last symbol up, the first one just below
// the end marker, little-endian.  out: count * 11 / 8 + 1 bytes at most
inline uint32_t cst_w_encode_stream(const uint8_t* data, uint32_t count, const uint32_t* code, uint8_t* out) {
    uint64_t acc = 0;
    uint32_t nbit = 0, p = 0;
    for (uint32_t i = count; i-- > 0;) {
        const uint32_t c = code[data[i]];
        acc |= uint64_t(c & 0xffff) << nbit;
        nbit += c >> 16;
        while (nbit >= 8) { out[p++] = uint8_t(acc); acc >>= 8; nbit -= 8; }
    }
    acc |= uint64_t(1) << nbit;
    out[p++] = uint8_t(acc);
    return p;
}

// The records of the kernels (mlz_search_tables_compress.hip.inc).  An item is a bitmap and its room; a job one of its sub-blocks
struct CstwItem { uint64_t dst_off, dst_cap; uint32_t n, first_job, nsub, bs; };   // n = 0: a size that is refused
struct CstwJob { uint64_t src_off; uint32_t item, sub; };                          // where the sub-block's bytes lie, 2^bs of them
// What the plan leaves of a sub-block.  kind: kCstRaw, kCstRle, kCstSparse or 0 (a table of its own).  body_len: the whole record.
// The layout kernel adds table, out_off and desc_off (places in the section).
struct CstwRec { uint32_t kind, desc_len, body_len, rle, sparse_len, four_len, slen[4], table, out_off, desc_off, pad[3]; };
constexpr uint32_t kCstwDescSlot = 144;      // a description's room in workspace (at most 129 bytes)

// What the write side found on the way (tools/search_compress_check.cpp reports it)
struct CstWriteStats { uint32_t raw, rle, sparse, huff, direct, fse, flattened, no_description; };

// The whole compression in plain loops: bitmap[0, n), cst_w_size_ok(n) -> dst[0, return value), the section; -1 when cap is too small
// (nothing useful is written).  Works in memory of its own (a section is at most cst_w_bound(n) bytes).
inline int64_t cst_compress_host(const uint8_t* bitmap, uint32_t n, uint8_t* dst, size_t cap, CstWriteStats* stats = nullptr) {
    const uint32_t bs = cst_w_bs(n), sub = 1u << bs, nsub = n >> bs;
    std::vector<uint8_t> descs, recs, stream(size_t(sub / 4) * 11 / 8 + 8);
    CstHuffScratch hs;
    CstFseScratch fs;
    uint8_t depth[256], w[256], desc[1 + kCstFseOutCap], uv[5];
    uint32_t hist[256], code[256], tc = 0;
    for (uint32_t j = 0; j < nsub; j++) {
        const uint8_t* b = bitmap + size_t(j) * sub;
        for (uint32_t s = 0; s < 256; s++) hist[s] = 0;
        for (uint32_t i = 0; i < sub; i++) hist[b[i]]++;
        if (hist[b[0]] == sub) {
            recs.push_back(uint8_t(kCstRle));
            recs.push_back(b[0]);
            if (stats) stats->rle++;
            continue;
        }
        uint32_t sparse_len = 0, prev = 0;   // prev: one behind the last set bit
        for (uint32_t i = 0; i < sub; i++)
            for (uint32_t v = b[i]; v; v &= v - 1) {
                const uint32_t pos = 8 * i + uint32_t(__builtin_ctz(v));
                sparse_len += cst_w_gap_bytes(pos - prev);
                prev = pos + 1;
            }
        uint32_t shift = 0;
        const uint32_t log = cst_w_code_lengths(hist, depth, &hs, &shift);
        const uint32_t last = cst_w_codes(depth, log, w, code);
        const uint32_t dlen = cst_w_description(w, last, desc, &fs);
        uint32_t bits = 0;
        for (uint32_t s = 0; s < 256; s++) bits += hist[s] * (code[s] >> 16);
        const uint32_t kind = cst_w_pick(sub, sparse_len, dlen, bits);
        if (stats) { stats->flattened += shift ? 1 : 0; stats->no_description += dlen ? 0 : 1; }
        if (kind == kCstRaw) {
            recs.push_back(uint8_t(kCstRaw));
            recs.insert(recs.end(), b, b + sub);
            if (stats) stats->raw++;
        } else if (kind == kCstSparse) {
            recs.push_back(uint8_t(kCstSparse));
            recs.insert(recs.end(), uv, uv + cst_w_put_uvarint(uv, sparse_len));
            prev = 0;
            for (uint32_t i = 0; i < sub; i++)
                for (uint32_t v = b[i]; v; v &= v - 1) {
                    const uint32_t pos = 8 * i + uint32_t(__builtin_ctz(v));
                    uint32_t gap = pos - prev;
                    for (; gap >= 255; gap -= 255) recs.push_back(255);
                    recs.push_back(uint8_t(gap));
                    prev = pos + 1;
                }
            if (stats) stats->sparse++;
        } else {
            descs.insert(descs.end(), desc, desc + dlen);
            const uint32_t seg = sub / 4;
            std::vector<uint8_t> four(6);
            for (uint32_t q = 0; q < 4; q++) {
                const uint32_t len = cst_w_encode_stream(b + q * seg, seg, code, stream.data());
                if (q < 3) { four[2 * q] = uint8_t(len); four[2 * q + 1] = uint8_t(len >> 8); }
                four.insert(four.end(), stream.begin(), stream.begin() + len);
            }
            recs.push_back(uint8_t(tc++));
            recs.insert(recs.end(), uv, uv + cst_w_put_uvarint(uv, uint32_t(four.size())));
            recs.insert(recs.end(), four.begin(), four.end());
            if (stats) { stats->huff++; (desc[0] >= 128 ? stats->direct : stats->fse)++; }
        }
    }
    const size_t total = 2 + descs.size() + recs.size();
    if (total > cap) return -1;
    dst[0] = uint8_t(bs);
    dst[1] = uint8_t(tc);
    if (!descs.empty()) memcpy(dst + 2, descs.data(), descs.size());
    memcpy(dst + 2 + descs.size(), recs.data(), recs.size());
    return int64_t(total);
}

}  // namespace mlz
