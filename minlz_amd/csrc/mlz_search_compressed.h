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

}  // namespace mlz
