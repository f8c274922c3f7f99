// mlz_stream_search.h — what the block search tables' writer, the device-resident pattern search (mlz_stream_search.hip.inc) and their host
// check (tools/stream_search_check.cpp) share: the table hash (SPEC_SEARCH.md 3.1), the size and the bytes of a table chunk (2.0, 2.1, 3.2),
// the probe of one table and the rule that turns the probes of all chunks into the set of chunks to decode (Appendix B.4.1).
// Both searches (one pattern, and many in one call: mlz_stream_search_many.hip.inc, tools/stream_search_many_check.cpp) use one rule per
// chunk (search_decoded_mark), one pattern record with its window hashes (search_pattern_hashes) and one layout of the decoded set in the
// scratch (search_layout, for patterns of lengths lmin .. lmax); the search for many adds the pattern index and the scan rule of one tile.
// The sidecar section adds what a stream of tables for ANOTHER stream needs: the remote reference chunk (0x47) written and parsed, the
// check of a reference against the main stream's chunks, and the rule over several table sets (search_decoded_mark_all).
// The case-folding section adds what MLZ_SEARCH_IGNORE_CASE needs: the byte and the dword fold, and the plan rule over the windows' case variants
// (search_windows_fold, search_pattern_hashes_fold, search_probe_fold; tools/stream_search_fold_check.cpp).
// Plain C++: compiles for the host alone and for gfx950.  Table types 1 (no prefix), 2 (1 to 8 prefix byte values), 3 (a 256-bit mask of
// prefix byte values; SPEC_SEARCH.md 3.3) and 4 (a long prefix of 1 to 256 bytes with extra matches; 3.3.4), uncompressed table chunks (0x45); compressed ones (0x46): mlz_search_compressed.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mlz_stream_walk.h"   // walk_uvarint, for a sidecar's remote references

#if defined(__HIPCC__)
#define MLZ_SEARCH_HD __host__ __device__ inline
#else
#define MLZ_SEARCH_HD inline
#endif

namespace mlz {

constexpr uint8_t kChunkSearchInfo = 0x44, kChunkSearchTable = 0x45;
constexpr uint32_t kSearchMaxPattern = 256, kSearchDefaultMatchLen = 6;
constexpr uint32_t kSearchNoTable = 0xffffffffu;

// A data chunk's table as the search keeps it: where its bytes lie in the stream, their number, the reductions (kSearchNoTable: no usable
// table) and the CRC its chunk states.  pad = kSearchTabArena: the table came from a compressed chunk (0x46) and its expanded bytes lie in
// the handle's arena, at arena + off, not in the stream (between the locate kernel and the expansion: off and bytes name the chunk's body).
struct SearchTab { uint64_t off; uint32_t bytes, R, crc, pad; };
constexpr uint32_t kSearchTabArena = 1;
static_assert(sizeof(SearchTab) == 24, "a record shared with the kernels");

// HashValue(val, tableSize, matchLen): `val` holds the window's bytes little-endian (bytes beyond matchLen are ignored).
MLZ_SEARCH_HD uint32_t search_hash(uint64_t val, uint32_t B, uint32_t M) {
    switch (M) {
    case 1: return uint32_t(val & 0xff);
    case 2: return B >= 16 ? uint32_t(val & 0xffff) : (uint32_t(val << 16) * 40503u) >> (32 - B);
    case 3: return (uint32_t(val << 8) * 506832829u) >> (32 - B);
    case 4: return (uint32_t(val) * 2654435761u) >> (32 - B);
    case 5: return uint32_t(((val << 24) * 889523592379ull) >> (64 - B));
    case 6: return uint32_t(((val << 16) * 227718039650203ull) >> (64 - B));
    case 7: return uint32_t(((val << 8) * 58295818150454627ull) >> (64 - B));
    default: return uint32_t((val * 0xcf1bbcdcb7a56463ull) >> (64 - B));
    }
}

// autoTableSize: bits of (block_size - 1), within 8 .. 23.
MLZ_SEARCH_HD uint32_t search_table_bits(uint32_t block_size) {
    uint32_t b = 0;
    for (uint32_t v = block_size - 1; v; v >>= 1) b++;
    return b < 8 ? 8 : b > 23 ? 23 : b;
}

// The prefix field that follows `T M B` in the info chunk and in every table chunk: none for type 1, the 8 values of type 2 (unused places
// repeat the last value), the 32 bytes of type 3's mask (value v is a prefix byte when field[v >> 3] >> (v & 7) & 1), type 4's `K-1 | E | pfx`
// (2 + K bytes: the prefix of K = 1 .. 256 bytes and the extras E = 0 .. 15, M + E <= 16).  The length of a type 4 field stands in its first
// byte, so search_field_len reads the field (which may be NULL for the other types).
constexpr uint32_t kSearchMaxField = 258, kSearchMaxPrefix = 256, kSearchMaxExtras = 15, kSearchMaxGroupWindows = 16;
// The most window starts search_windows writes: L of type 1 .. 3, 255 groups of 16 windows of type 4
constexpr uint32_t kSearchMaxWindows = 255 * kSearchMaxGroupWindows;
MLZ_SEARCH_HD uint32_t search_field_len(uint32_t T, const uint8_t* field) { return T == 2 ? 8 : T == 3 ? 32 : T == 4 ? 3u + field[0] : 0; }
// Type 4: the prefix's bytes, their number K and the extras E of a field
MLZ_SEARCH_HD uint32_t search_long_k(const uint8_t* field) { return 1u + field[0]; }
MLZ_SEARCH_HD uint32_t search_long_e(const uint8_t* field) { return field[1]; }
MLZ_SEARCH_HD const uint8_t* search_long_prefix(const uint8_t* field) { return field + 2; }
// mask[v >> 5] >> (v & 31) & 1: v is a prefix byte of (T, field).  Type 1 has no prefix bytes.
MLZ_SEARCH_HD void search_prefix_mask(uint32_t T, const uint8_t* field, uint32_t mask[8]) {
    for (uint32_t i = 0; i < 8; i++) mask[i] = 0;
    if (T == 2) for (uint32_t i = 0; i < 8; i++) mask[field[i] >> 5] |= 1u << (field[i] & 31);
    if (T == 3) for (uint32_t i = 0; i < 32; i++) mask[i >> 2] |= uint32_t(field[i]) << (8 * (i & 3));
}
MLZ_SEARCH_HD bool search_is_prefix(const uint32_t mask[8], uint8_t v) { return (mask[v >> 5] >> (v & 31)) & 1; }

// Bytes a table chunk takes at the most: 4 (chunk header) + 8 (type, M, B, R, CRC) + the prefix field + the unreduced table.
MLZ_SEARCH_HD uint64_t search_chunk_bound(uint32_t B, uint32_t field_len = 0) { return 12 + field_len + (uint64_t(1) << (B - 3)); }

// The payload of a 0x45 chunk (`clen` bytes at p, all readable): the reductions R of a table of the stream's (T, M, B, field) whose length
// fits, else -1 (a type 4 table whose prefix or extras differ from the stream's included).  With f = search_field_len(T, field): the CRC is the little-endian word at p + 4 + f, the table's bytes are p[8 + f .. clen).
MLZ_SEARCH_HD int search_table_reductions(const uint8_t* p, uint32_t clen, uint32_t M, uint32_t B, uint32_t T = 1, const uint8_t* field = nullptr) {
    const uint32_t f = search_field_len(T, field);
    if (clen < 8 + f + 32 || p[0] != T || p[1] != M || p[2] != B) return -1;
    for (uint32_t i = 0; i < f; i++) if (p[3 + i] != field[i]) return -1;
    const uint32_t R = p[3 + f];
    if (R > B - 8) return -1;
    return clen - 8 - f == (1u << (B - R - 3)) ? int(R) : -1;
}

// The payload of a 0x44 chunk: (T, M, B) and the prefix field (kSearchMaxField bytes of room, zeros behind the field) of a stream of type
// 1 .. 4, else false (a payload shorter than the field and a type 4 field with more than 15 extras or M + E > 16 included).
MLZ_SEARCH_HD bool search_info(const uint8_t* p, uint32_t clen, uint32_t* T, uint32_t* M, uint32_t* B, uint8_t* field) {
    if (clen < 3 || p[0] < 1 || p[0] > 4 || p[1] < 1 || p[1] > 8 || p[2] < 8 || p[2] > 23) return false;
    if (p[0] == 4 && (clen < 5 || p[4] > kSearchMaxExtras || p[1] + p[4] > kSearchMaxGroupWindows)) return false;
    const uint32_t f = search_field_len(p[0], p + 3);
    if (clen < 3 + f) return false;
    *T = p[0]; *M = p[1]; *B = p[2];
    for (uint32_t i = 0; i < kSearchMaxField; i++) field[i] = i < f ? p[3 + i] : 0;
    return true;
}

// The bytes behind a block that its table indexes into: the longest reach of a window (a group) that belongs to the block
MLZ_SEARCH_HD uint32_t search_overlap(uint32_t T, uint32_t M, const uint8_t* field) {
    return T == 1 ? M - 1 : T == 4 ? search_long_k(field) - 1 + M + search_long_e(field) : M;
}

// An ASCII letter: the bytes that have a case variant
MLZ_SEARCH_HD bool search_is_letter(uint8_t b) { return (uint32_t(b | 0x20u) - 0x61u) < 26u; }

// The pattern's windows that the tables can answer for, in groups of *gsize windows that one block's table holds together, and t_min.
// w[g * gsize + j] = where window j of group g starts in the pattern, groups ascending; room for kSearchMaxWindows values (L for types
// 1 .. 3).  Returns the number of groups; 0 = the tables cannot serve this pattern.
// Type 1: every window 0 .. L - M is a group of one, t_min = 1.  Types 2 and 3: the windows 1 <= i <= L - M behind a prefix byte P[i - 1],
// groups of one; t_min = 1 when P[0] is a prefix byte, else 0.  Type 4: a group per prefix occurrence P[i, i + K) == pfx with
// i + K + M + E <= L, its E + 1 windows start at i + K + j; t_min = 1 when the first group has i = 0, else 0.
// fold (MLZ_SEARCH_IGNORE_CASE; the rule's reasons stand in the case-folding section below): types 2 and 3 take window i, and t_min = 1, only when
// EVERY case variant of the byte in front is a prefix byte; type 4 has no group when the prefix holds a letter.  pat may be folded or not.
// A pattern without letters gets the same windows either way.
MLZ_SEARCH_HD uint32_t search_windows(const uint8_t* pat, uint32_t L, uint32_t T, uint32_t M, const uint8_t* field, uint32_t* w, uint32_t* t_min,
                                      uint32_t* gsize = nullptr, bool fold = false) {
    *t_min = 1;
    if (gsize) *gsize = 1;
    if (L < M) return 0;
    uint32_t nw = 0;
    if (T == 1) { for (uint32_t i = 0; i + M <= L; i++) w[nw++] = i; return nw; }
    if (T == 4) {
        const uint32_t K = search_long_k(field), E = search_long_e(field), gs = E + 1;
        const uint8_t* pfx = search_long_prefix(field);
        if (gsize) *gsize = gs;
        *t_min = 0;
        if (fold) for (uint32_t j = 0; j < K; j++) if (search_is_letter(pfx[j])) return 0;
        for (uint32_t i = 0; i + K + M + E <= L; i++) {
            uint32_t j = 0;
            while (j < K && pat[i + j] == pfx[j]) j++;
            if (j < K) continue;
            if (nw == 0 && i == 0) *t_min = 1;
            for (j = 0; j < gs; j++) w[nw * gs + j] = i + K + j;
            nw++;
        }
        return nw;
    }
    uint32_t mask[8];
    search_prefix_mask(T, field, mask);
    auto prefix = [&](uint8_t b) {   // b is a prefix byte; under folding: every case variant of b is one
        if (!fold || !search_is_letter(b)) return search_is_prefix(mask, b);
        return search_is_prefix(mask, uint8_t(b | 0x20u)) && search_is_prefix(mask, uint8_t(b & ~0x20u));
    };
    *t_min = prefix(pat[0]) ? 1 : 0;
    for (uint32_t i = 1; i + M <= L; i++) if (prefix(pat[i - 1])) w[nw++] = i;
    return nw;
}

// One pattern as the plan sees it: its nw groups of gsize window hashes lie at hashes[h_off ...); t_min and L as in search_decoded_mark.
struct SearchManyPat { uint32_t h_off, nw, gsize, t_min, L, pad; };
static_assert(sizeof(SearchManyPat) == 24, "a record shared with the kernels");

// The pattern's record and its window hashes, appended to *hs: search_windows (win: its room), then per window the M bytes little-endian,
// hashed at B bits.  False, and nothing appended: the tables cannot serve this pattern.
inline bool search_pattern_hashes(const uint8_t* pat, uint32_t L, uint32_t T, uint32_t M, uint32_t B, const uint8_t* field, uint32_t* win, std::vector<uint32_t>* hs,
                                  SearchManyPat* out) {
    uint32_t t_min = 1, gsize = 1;
    const uint32_t nw = search_windows(pat, L, T, M, field, win, &t_min, &gsize);
    if (!nw) return false;
    *out = SearchManyPat{uint32_t(hs->size()), nw, gsize, t_min, L, 0};
    for (uint32_t w = 0; w < nw * gsize; w++) {
        uint64_t v = 0;
        for (uint32_t j = 0; j < M; j++) v |= uint64_t(pat[win[w] + j]) << (8 * j);
        hs->push_back(search_hash(v, B, M));
    }
    return true;
}

// One table against the pattern's nw groups of gsize windows (h[g * gsize + j] = the hash of window j of group g at B bits; bits = B - R of
// this table): a = the leading groups whose windows are all present, s = the trailing ones.  Both are nw when all are present.
MLZ_SEARCH_HD void search_probe(const uint8_t* table, uint32_t bits, const uint32_t* h, uint32_t nw, uint32_t* a, uint32_t* s, uint32_t gsize = 1) {
    const uint32_t mask = (1u << bits) - 1;
    auto has = [&](uint32_t g) {
        for (uint32_t j = 0; j < gsize; j++) {
            const uint32_t x = h[g * gsize + j] & mask;
            if (!((table[x >> 3] >> (x & 7)) & 1)) return false;
        }
        return true;
    };
    uint32_t lead = 0, trail = 0;
    while (lead < nw && has(lead)) lead++;
    if (lead == nw) { *a = *s = nw; return; }
    while (trail < nw && has(nw - 1 - trail)) trail++;
    *a = lead; *s = trail;
}

// ---- case folding (MLZ_SEARCH_IGNORE_CASE: grep -i in the C locale) ----
// fold(b) = b | 0x20 for 0x41 <= b <= 0x5A ('A' .. 'Z'), b otherwise.  The patterns are folded once on the host; the scans fold every data
// byte in registers on its way into a comparison (the scratch keeps the stream's bytes).
MLZ_SEARCH_HD uint8_t search_fold(uint8_t b) { return uint8_t(b | ((uint32_t(b) - 0x41u < 26u) ? 0x20u : 0u)); }
// Four bytes at once, no carry between them: with y = the low 7 bits of every byte, bit 7 of y + 0x3f is set for y >= 0x41 and bit 7 of
// y + 0x25 for y >= 0x5b (both sums stay below 0x100 per byte); a byte with its own bit 7 set is no letter.  The 0x80 marks, shifted to 0x20.
MLZ_SEARCH_HD uint32_t search_fold4(uint32_t x) {
    const uint32_t y = x & 0x7f7f7f7fu;
    const uint32_t m = ((y + 0x3f3f3f3fu) & ~(y + 0x25252525u) & ~x & 0x80808080u) >> 2;
    return x | m;
}

// The plan under folding.  A table bit stands for the exact bytes of a window, so a window of the folded pattern is PRESENT in a table when
// the bit of ANY of its case variants is set (the 2^k strings that differ in the case of its k letters).  search_candidate and
// search_chunk_candidate are monotone in presence, so whatever errs towards "present" keeps a verdict a necessary condition:
//   a window with more than kSearchFoldMaxLetters letters ABSTAINS: present in every table, no hashes (at a table population of 10 %, one of
//   2^k variants is present by chance with probability 1 - 0.9^(2^k): 0.57 for k = 3, 0.998 for k = 6: such a window proves nothing);
//   types 2 and 3: window i is one the tables answer for only when EVERY case variant of P[i - 1] is a prefix byte (the data may hold
//   either case in front of the window, and only a prefix byte makes a block index it); t_min = 1 only when every variant of P[0] is one;
//   type 4: a group at i exists only when P[i, i + K) equals the prefix byte for byte and the prefix holds no letter (the data may hold the
//   prefix in another case, which no block indexes).
// A pattern whose windows all abstain is not served.  The variant hashes lie CSR-wise: voff[w] .. voff[w + 1] are window w's in hs
// (none: the window abstains); a pattern's record (SearchManyPat) has h_off = where its nw * gsize + 1 offsets start in voff.
constexpr uint32_t kSearchFoldMaxLetters = 3, kSearchFoldMaxHashes = 1u << 22;

// search_windows for a search that folds: the one window rule with its fold parameter set
MLZ_SEARCH_HD uint32_t search_windows_fold(const uint8_t* pat, uint32_t L, uint32_t T, uint32_t M, const uint8_t* field, uint32_t* w, uint32_t* t_min,
                                           uint32_t* gsize = nullptr) {
    return search_windows(pat, L, T, M, field, w, t_min, gsize, true);
}

// search_pattern_hashes for a search that folds: per window one offset appended to *voff (and one behind the last) and its variant hashes to
// *hs — variant v of a window with k <= kSearchFoldMaxLetters letters has its j-th letter in upper case where bit j of v is set, v = 0 .. 2^k - 1.
// False, and nothing appended: the tables cannot serve the pattern (no window, or every window abstains), or its hashes do not fit into
// `budget` (what is left of kSearchFoldMaxHashes: *over = true then).
inline bool search_pattern_hashes_fold(const uint8_t* pat, uint32_t L, uint32_t T, uint32_t M, uint32_t B, const uint8_t* field, uint32_t* win, std::vector<uint32_t>* voff,
                                       std::vector<uint32_t>* hs, SearchManyPat* out, uint32_t budget = kSearchFoldMaxHashes, bool* over = nullptr) {
    uint32_t t_min = 1, gsize = 1;
    if (over) *over = false;
    const uint32_t nw = search_windows_fold(pat, L, T, M, field, win, &t_min, &gsize);
    if (!nw) return false;
    const size_t v0 = voff->size(), h0 = hs->size();
    auto undo = [&]() { voff->resize(v0); hs->resize(h0); return false; };
    for (uint32_t w = 0; w < nw * gsize; w++) {
        voff->push_back(uint32_t(hs->size()));
        uint32_t k = 0, at[kSearchFoldMaxLetters];
        uint64_t v = 0;
        for (uint32_t j = 0; j < M; j++) {
            const uint8_t b = search_fold(pat[win[w] + j]);
            if (search_is_letter(b)) { if (k < kSearchFoldMaxLetters) at[k] = j; k++; }
            v |= uint64_t(b) << (8 * j);
        }
        if (k > kSearchFoldMaxLetters) continue;   // (abstains)
        if (hs->size() - h0 + (size_t(1) << k) > budget) { if (over) *over = true; return undo(); }
        for (uint32_t var = 0; var < (1u << k); var++) {
            uint64_t x = v;
            for (uint32_t j = 0; j < k; j++) if ((var >> j) & 1) x &= ~(uint64_t(0x20) << (8 * at[j]));
            hs->push_back(search_hash(x, B, M));
        }
    }
    if (hs->size() == h0) return undo();
    voff->push_back(uint32_t(hs->size()));
    *out = SearchManyPat{uint32_t(v0), nw, gsize, t_min, L, 0};
    return true;
}

// search_probe under folding: voff = the pattern's nw * gsize + 1 offsets into hs.  A window is present when it abstains or one of its
// variants' bits is set; a group when all its windows are.
MLZ_SEARCH_HD void search_probe_fold(const uint8_t* table, uint32_t bits, const uint32_t* voff, const uint32_t* hs, uint32_t nw, uint32_t* a, uint32_t* s, uint32_t gsize = 1) {
    const uint32_t mask = (1u << bits) - 1;
    auto has = [&](uint32_t g) {
        for (uint32_t j = 0; j < gsize; j++) {
            uint32_t e = voff[g * gsize + j];
            const uint32_t e1 = voff[g * gsize + j + 1];
            if (e == e1) continue;
            for (; e < e1; e++) {
                const uint32_t x = hs[e] & mask;
                if ((table[x >> 3] >> (x & 7)) & 1) break;
            }
            if (e == e1) return false;
        }
        return true;
    };
    uint32_t lead = 0, trail = 0;
    while (lead < nw && has(lead)) lead++;
    if (lead == nw) { *a = *s = nw; return; }
    while (trail < nw && has(nw - 1 - trail)) trail++;
    *a = lead; *s = trail;
}

// Chunk k may hold the start of an occurrence: all windows in its own table, or a split of them between its table (the first j, t_min <= j < nw,
// tail windows included) and the next chunk's (the last nw - j).  s_next = nw when the next chunk has no usable table or decodes to fewer
// bytes than the pattern has.  t_min: the fewest windows an occurrence that starts in chunk k leaves in k's table — 1 for type 1 (window 0
// starts with the occurrence) and for a prefix table whose pattern starts with a prefix byte, else 0 (a window is indexed in the block that
// holds the byte in front of it, so a short head of the occurrence may leave none).  Type 4 counts groups, not windows: a group lies in the
// table of the block in which its prefix starts, all its windows together, so an occurrence splits between two tables at a group border only;
// t_min = 1 when the pattern starts with the prefix.
MLZ_SEARCH_HD bool search_candidate(uint32_t a_k, uint32_t s_next, uint32_t nw, bool last, uint32_t t_min = 1) {
    if (a_k == nw) return true;
    if (last) return false;
    const uint32_t lo = nw - s_next > t_min ? nw - s_next : t_min;
    return lo <= a_k;   // (a_k < nw here)
}

// The decoded set: every candidate plus the chunks behind it that hold any of the L - 1 bytes after its end.  a_of(k), s_of(k): the probe
// of chunk k (nw, nw without a usable table); n_of(k) > 0: its decoded bytes.  The rule has two halves, each said once:
// search_chunk_candidate is the verdict of ONE table set on chunk k (s_next is looked at only where it decides); search_mark_from marks a
// candidate and the chunks behind it.  search_decoded_mark is the two together for one table set, marking only: nothing is cleared, every
// store is a 1, so lanes may run it side by side and the union of several patterns' sets is this function over every (k, pattern) on one array.
// ov: how many bytes behind chunk k its table was built over when those bytes come from the NEXT chunk alone (a sidecar's tables:
// search_overlap of the set; 0 for a stream's inline tables, which the Writer builds over the bytes that follow in the stream, whichever chunks hold them).  Where the
// next chunk is shorter than that, the windows that reach beyond it were hashed over zeros, the table proves nothing about an occurrence
// that starts in k, and the set abstains: it admits k.
template <class A, class S, class N>
MLZ_SEARCH_HD bool search_chunk_candidate(size_t k, size_t nck, A a_of, S s_of, N n_of, uint32_t nw, uint32_t L, uint32_t t_min = 1, uint32_t ov = 0) {
    const bool last = k + 1 == nck;
    if (!last && n_of(k + 1) < ov) return true;
    const uint32_t a_k = a_of(k);
    if (a_k == nw) return true;
    if (last) return false;
    const uint32_t s_next = n_of(k + 1) < L ? nw : s_of(k + 1);
    return search_candidate(a_k, s_next, nw, last, t_min);
}
template <class N>
MLZ_SEARCH_HD void search_mark_from(size_t k, size_t nck, N n_of, uint32_t L, uint8_t* take) {
    take[k] = 1;
    uint64_t need = L - 1;
    for (size_t j = k + 1; j < nck && need; j++) {
        const uint64_t nj = n_of(j);
        if (nj) take[j] = 1;
        need = nj >= need ? 0 : need - nj;
    }
}
template <class A, class S, class N>
MLZ_SEARCH_HD void search_decoded_mark(size_t k, size_t nck, A a_of, S s_of, N n_of, uint32_t nw, uint32_t L, uint8_t* take, uint32_t t_min = 1) {
    if (!n_of(k)) return;   // (a chunk of no bytes holds nothing)
    if (search_chunk_candidate(k, nck, a_of, s_of, n_of, nw, L, t_min)) search_mark_from(k, nck, n_of, L, take);
}
// Several table sets over one stream (the configurations of a sidecar; a stream's inline tables are one set): chunk k is a candidate when
// EVERY set admits it.  admits(c) is set c's search_chunk_candidate; a set that cannot serve the pattern (search_windows gives no group)
// or has no usable table for k admits it, and so does a sidecar's set in front of a chunk shorter than its overlap (search_chunk_candidate's
// ov).  Each set's verdict alone is then a necessary condition for an occurrence that starts in k, so their conjunction is one too.
template <class Admits, class N>
MLZ_SEARCH_HD void search_decoded_mark_all(size_t k, size_t nck, uint32_t n_sets, Admits admits, N n_of, uint32_t L, uint8_t* take) {
    if (!n_of(k)) return;
    for (uint32_t c = 0; c < n_sets; c++) if (!admits(c)) return;
    search_mark_from(k, nck, n_of, L, take);
}
// One pattern's set: take[k] = 1 for the chunks to decode, 0 for the others.  Returns their number.
template <class A, class S, class N>
size_t search_decoded_set(size_t nck, A a_of, S s_of, N n_of, uint32_t nw, uint32_t L, uint8_t* take, uint32_t t_min = 1) {
    for (size_t k = 0; k < nck; k++) take[k] = 0;
    for (size_t k = 0; k < nck; k++) search_decoded_mark(k, nck, a_of, s_of, n_of, nw, L, take, t_min);
    size_t cnt = 0;
    for (size_t k = 0; k < nck; k++) cnt += take[k];
    return cnt;
}

// ---- the decoded set in the scratch ----
// The chunks of the decoded set ("jobs", in stream order) are decoded group by group into one scratch buffer that every group reuses.  A group
// starts behind kSearchPad bytes of room; chunks that are neighbours in the decoded stream lie side by side, so a run of neighbours is one
// piece of decoded stream, and where a run goes on in the next group its last lmax - 1 bytes are copied in front of that group's first chunk.
// The patterns of a call have lengths lmin .. lmax (one pattern: both are L).  A tile is up to `tile` start positions of one run in one
// group: position i is scratch[src_off + i], decoded byte gpos + i, and EVERY pattern is examined at each i < count, a pattern of L bytes
// under i + L <= hi_end (hi_end: where the run's bytes end in this group, counted from src_off; with one length that holds for every i).
// A start position belongs to the first group that holds lmax bytes of the run from it on, or to the group in which the run ends: where the
// run goes on in the next group, the tiles stop lmax - 1 bytes before the run's end in this one, and exactly those positions are the
// carried bytes in front of the next group's first chunk.  So every position of a run at which a pattern fits is in exactly one tile, with
// all its patterns at once, and the tiles ascend: the pairs come out in (position, pattern) order.  (Examining a pair in the first group
// that holds ITS bytes would find a short pattern at p + 1 a group before a long one at p.)
// kSearchTile: the tile of the search for one pattern, tied to its bitmap kernels; kSearchManyTile: of the search for many.
constexpr uint32_t kSearchTile = 8192, kSearchTileWords = kSearchTile / 64, kSearchManyTile = 16384, kSearchPad = 256;
struct SearchTile { int64_t src_off; uint64_t gpos; uint32_t count, hi_end; };
static_assert(sizeof(SearchTile) == 24 && kSearchPad >= kSearchMaxPattern, "a record shared with the kernels; the carried bytes fit in front of a group");
struct SearchLayout {
    std::vector<uint64_t> at;            // per job: where its chunk lies in the scratch
    std::vector<SearchTile> tiles;       // group by group
    std::vector<size_t> tile_end;        // per group: one past its last tile
    std::vector<uint32_t> carry;         // per group: bytes that go from its end, scratch[used - carry, used), to scratch[kSearchPad - carry, kSearchPad)
    std::vector<uint64_t> used;          // per group: the end of its last chunk in the scratch
    uint64_t scratch_max = 0;
};
// gend[g]: one past the last job of group g; out_off_of(j), n_of(j): job j's place in the decoded stream and its decoded bytes
template <class Off, class N>
void search_layout(size_t n_jobs, const std::vector<size_t>& gend, Off out_off_of, N n_of, uint32_t lmin, uint32_t lmax, uint32_t tile, SearchLayout* lay) {
    const size_t ng = gend.size();
    lay->at.assign(n_jobs, 0); lay->tiles.clear(); lay->tile_end.assign(ng, 0); lay->carry.assign(ng, 0); lay->used.assign(ng, 0); lay->scratch_max = 0;
    auto adjacent = [&](size_t i) { return out_off_of(i - 1) + n_of(i - 1) == out_off_of(i); };
    uint64_t run_have = 0;   // bytes of the current run that lie in the scratch in front of the next chunk
    for (size_t g = 0, j0 = 0; g < ng; j0 = gend[g++]) {
        const size_t j1 = gend[g];
        uint64_t o = kSearchPad;
        for (size_t j = j0; j < j1;) {
            size_t e = j + 1;   // a part: jobs [j, e) are neighbours
            while (e < j1 && adjacent(e)) e++;
            if (!(j == j0 && j0 > 0 && adjacent(j0))) run_have = 0;
            const uint64_t ps = o, gp = out_off_of(j);
            for (size_t i = j; i < e; i++) { lay->at[i] = o; o += n_of(i); }
            const uint64_t lower = ps - (run_have < lmax - 1 ? run_have : lmax - 1);
            const uint32_t keep = e == j1 && j1 < n_jobs && adjacent(j1) ? lmax : lmin;   // (the run goes on in the next group : it ends here)
            if (o - lower >= keep)
                for (uint64_t s0 = lower, upper = o - keep + 1; s0 < upper; s0 += tile)
                    lay->tiles.push_back(SearchTile{int64_t(s0), gp + s0 - ps, uint32_t(upper - s0 < tile ? upper - s0 : tile), uint32_t(o - s0)});
            run_have += o - ps;
            j = e;
        }
        lay->used[g] = o;
        if (j1 < n_jobs && adjacent(j1)) lay->carry[g] = uint32_t(run_have < lmax - 1 ? run_have : lmax - 1);
        if (o > lay->scratch_max) lay->scratch_max = o;
        lay->tile_end[g] = lay->tiles.size();
    }
}

// ---- many patterns in one call (mlz_dev_reader_search_many) ----
constexpr uint32_t kSearchMaxPatterns = 4096;

// The pattern index of the scan: the key of a pattern is its first m = min(4, lmin) bytes, hashed to hb bits; heads[h] .. heads[h + 1] are the
// places in `order` of the patterns whose key hashes to h, ascending by pattern index (a CSR), so a lane that walks a bucket meets the
// patterns that match at its position in pattern order.  off[i] .. off[i + 1]: pattern i's bytes in the blob.  n <= 4096: 16-bit values do.
// hb = the bits of n - 1 within 8 .. 12: about one entry per bucket at the most patterns, and at 12 bits the heads take 8 KiB of LDS.
MLZ_SEARCH_HD uint32_t search_many_bits(uint32_t n) {
    uint32_t b = 0;
    for (uint32_t v = n ? n - 1 : 0; v; v >>= 1) b++;
    return b < 8 ? 8 : b > 12 ? 12 : b;
}
// v: the bytes at a position, little-endian; those beyond m do not enter
MLZ_SEARCH_HD uint32_t search_many_key(uint32_t v, uint32_t m, uint32_t hb) {
    if (m < 4) v &= (1u << (8 * m)) - 1;
    return (v * 2654435761u) >> (32 - hb);
}
struct SearchManyIndex {
    uint32_t m = 0, hb = 0, lmin = 0, lmax = 0;
    std::vector<uint16_t> heads, order;
    std::vector<uint32_t> off;
};
// blob: the patterns back to back; len[i] in 1 .. 256, n in 1 .. kSearchMaxPatterns
inline void search_many_index(const uint8_t* blob, const uint32_t* len, size_t n, SearchManyIndex* ix) {
    ix->lmin = kSearchMaxPattern; ix->lmax = 1;
    ix->off.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        ix->off[i + 1] = ix->off[i] + len[i];
        if (len[i] < ix->lmin) ix->lmin = len[i];
        if (len[i] > ix->lmax) ix->lmax = len[i];
    }
    ix->m = ix->lmin < 4 ? ix->lmin : 4;
    ix->hb = search_many_bits(uint32_t(n));
    auto key = [&](size_t i) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < ix->m; j++) v |= uint32_t(blob[ix->off[i] + j]) << (8 * j);
        return search_many_key(v, ix->m, ix->hb);
    };
    const size_t nb = size_t(1) << ix->hb;
    std::vector<uint32_t> fill(nb + 1, 0);
    for (size_t i = 0; i < n; i++) fill[key(i) + 1]++;
    for (size_t b = 0; b < nb; b++) fill[b + 1] += fill[b];
    ix->heads.assign(fill.begin(), fill.end());
    ix->order.assign(n, 0);
    for (size_t i = 0; i < n; i++) ix->order[fill[key(i)]++] = uint16_t(i);   // (a counting sort: pattern order inside a bucket)
}

// The scan and write rule of one tile, as search_many_kernel applies it (and as the host check restates it with plain loops): the byte at
// tile position i is s[i]; emit(i, pattern) is called for every pair the tile examines, positions ascending, patterns in bucket order.
// fold (MLZ_SEARCH_IGNORE_CASE): the blob and the index are those of the FOLDED patterns (search_fold over every byte, then search_many_index:
// the key is taken over folded pattern bytes), and every data byte is folded on its way into the key and into the comparison.
template <class Emit>
inline void search_many_tile_pairs(const uint8_t* s, const SearchTile& t, const SearchManyIndex& ix, const uint8_t* blob, Emit emit, bool fold = false) {
    auto at = [&](uint32_t i) { return fold ? search_fold(s[i]) : s[i]; };
    for (uint32_t i = 0; i < t.count; i++) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < ix.m; j++) v |= uint32_t(at(i + j)) << (8 * j);
        const uint32_t h = search_many_key(v, ix.m, ix.hb);
        for (uint32_t e = ix.heads[h]; e < ix.heads[h + 1]; e++) {
            const uint32_t p = ix.order[e], L = ix.off[p + 1] - ix.off[p];
            if (i + L > t.hi_end) continue;
            uint32_t j = 0;
            while (j < L && at(i + j) == blob[ix.off[p] + j]) j++;
            if (j == L) emit(i, p);
        }
    }
}

// ---- sidecars (SPEC_SEARCH.md 1.1, 2.3): a stream of table chunks that names the blocks of ANOTHER stream ----
// A sidecar is a valid stream without data chunks: identifier, one info chunk (0x44) per table configuration, then per block of the main
// stream its table chunks (0x45) followed by a remote block reference (0x47), EOF.  A 0x47 payload is a list of pairs
// uvarint(offset) uvarint(max block size - decoded bytes): the first offset is where the block's data chunk header lies in the main stream,
// further offsets count from the one before and are not 0.  Only the first reference of a chunk owns the tables in front of it.
constexpr uint8_t kChunkRemoteRef = 0x47;
constexpr uint32_t kSidecarMaxConfigs = 4;
// One table configuration: what search_info reads from an info chunk
struct SearchConfig { uint32_t T, M, B, ok; uint8_t field[kSearchMaxField + 2]; };
static_assert(sizeof(SearchConfig) == 276, "a record shared with the kernels");

MLZ_SEARCH_HD uint32_t search_put_uvarint(uint8_t* b, uint64_t v) {
    uint32_t i = 0;
    for (; v >= 0x80; v >>= 7) b[i++] = uint8_t(v) | 0x80;
    b[i++] = uint8_t(v);
    return i;
}
// The 0x47 chunk of one reference (24 bytes of room); returns its bytes
MLZ_SEARCH_HD uint32_t sidecar_put_ref(uint8_t* b, uint64_t hdr_off, uint64_t max_minus_actual) {
    uint32_t n = search_put_uvarint(b + 4, hdr_off);
    n += search_put_uvarint(b + 4 + n, max_minus_actual);
    b[0] = kChunkRemoteRef; b[1] = uint8_t(n); b[2] = b[3] = 0;
    return 4 + n;
}
constexpr uint32_t kSidecarRefBound = 4 + 10 + 10;
MLZ_SEARCH_HD uint32_t search_uvarint_len(uint64_t v) { uint32_t n = 1; for (; v >= 0x80; v >>= 7) n++; return n; }
MLZ_SEARCH_HD uint32_t sidecar_ref_bytes(uint64_t hdr_off, uint64_t max_minus_actual) { return 4 + search_uvarint_len(hdr_off) + search_uvarint_len(max_minus_actual); }
// The references of a 0x47 payload (parseRemoteBlockRef): ref(offset, decoded bytes) for each, in order.  Returns their number, or -1: an
// empty payload, a varint that is cut short or overflows, a relative offset of 0, an offset beyond 2^63, a size outside 1 .. max_block.
template <class Ref>
MLZ_SEARCH_HD int sidecar_parse_refs(const uint8_t* p, uint32_t clen, uint64_t max_block, Ref ref) {
    if (clen == 0) return -1;
    int cnt = 0;
    uint64_t prev = 0;
    for (uint32_t o = 0; o < clen; cnt++) {
        uint64_t off = 0, mma = 0;
        const int n1 = walk_uvarint(p + o, clen - o, &off);
        if (n1 <= 0) return -1;
        o += uint32_t(n1);
        const int n2 = walk_uvarint(p + o, clen - o, &mma);
        if (n2 <= 0) return -1;
        o += uint32_t(n2);
        if (cnt && off == 0) return -1;
        const uint64_t abs = cnt ? prev + off : off;
        if (abs >> 63 || (cnt && abs < prev)) return -1;
        if (mma >= max_block) return -1;   // (the decoded bytes are max_block - mma: 1 .. max_block)
        ref(abs, max_block - mma);
        prev = abs;
    }
    return cnt;
}
// The data chunk of the main stream whose header lies at `off` (hdr_of(k): ascending), or -1
template <class H>
MLZ_SEARCH_HD int64_t sidecar_find_chunk(size_t nck, H hdr_of, uint64_t off) {
    size_t lo = 0, hi = nck;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (hdr_of(mid) < off) lo = mid + 1; else hi = mid;
    }
    return lo < nck && hdr_of(lo) == off ? int64_t(lo) : -1;
}
// One 0x47 chunk against the main stream, as the attach applies it: every reference names a data chunk (hdr_of), states its decoded bytes
// (n_of) and lies behind `floor` (the last reference of the 0x47 chunk before this one; none: have_floor = false).  Returns the chunk the
// FIRST reference names (the owner of the tables in front of the 0x47) and *last = the last reference's offset, or -1.
template <class H, class N>
MLZ_SEARCH_HD int64_t sidecar_check_refs(const uint8_t* p, uint32_t clen, uint64_t max_block, size_t nck, H hdr_of, N n_of, bool have_floor, uint64_t floor, uint64_t* last) {
    int64_t first = -1;
    bool bad = false, have = have_floor;
    uint64_t prev = floor;
    int seen = 0;
    const int cnt = sidecar_parse_refs(p, clen, max_block, [&](uint64_t off, uint64_t size) {
        if (have && off <= prev) bad = true;
        const int64_t k = sidecar_find_chunk(nck, hdr_of, off);
        if (k < 0 || n_of(size_t(k)) != size) bad = true;
        if (seen++ == 0) first = k;
        have = true; prev = off;
    });
    if (cnt <= 0 || bad) return -1;
    *last = prev;
    return first;
}

// ---- the writer's side: the reductions of one table (3.2, the reference's population rules) ----
// A block whose unfolded table has more than 70 % of its 2^B bits set gets no table; a fold to half_bits bits is accepted while a quarter of
// them at the most are set (a tenth with a prefix table).  (stab_reduce_kernel applies the two fold by fold; search_reduce_rule is the whole rule over given counts.)
MLZ_SEARCH_HD bool search_table_dropped(uint32_t pop, uint32_t B) { return uint64_t(pop) * 100 / (uint64_t(1) << B) > 70; }
MLZ_SEARCH_HD uint32_t search_fold_limit(uint32_t T) { return T == 1 ? 25 : 10; }
MLZ_SEARCH_HD bool search_fold_accepted(uint32_t pop_folded, uint64_t half_bits, uint32_t limit = 25) { return uint64_t(pop_folded) * 100 <= half_bits * limit; }
// pop[r] = the set bits of the table folded r times (r = 0: as built), for r = 0 .. B - 8.  Returns the bytes of the table to store and *R,
// or 0 when the block gets no table (more than 70 % of the unfolded bits are set).
MLZ_SEARCH_HD uint32_t search_reduce_rule(const uint32_t* pop, uint32_t B, uint32_t* R, uint32_t limit = 25) {
    const uint64_t total = uint64_t(1) << B;
    *R = 0;
    if (search_table_dropped(pop[0], B)) return 0;
    uint32_t r = 0;
    uint64_t bytes = total >> 3;
    while (bytes >= 64) {
        const uint64_t half_bits = (bytes >> 1) << 3;
        if (!search_fold_accepted(pop[r + 1], half_bits, limit)) break;
        bytes >>= 1; r++;
    }
    *R = r;
    return uint32_t(bytes);
}

// ---- tables built already folded (the batch Writer: a table's size comes from the call's block size, and every stream's last block is short) ----
// A table folded r times is the bitmap of h & (2^(B - r) - 1).  pop[r] never exceeds `marks`, the distinct window positions a block indexes,
// so with marks * 100 <= 2^(B - r) * limit and B - r >= 8 every fold up to r passes search_reduce_rule's two conditions whatever the data,
// and the unfolded table holds a quarter of 2^(B - 1) bits at the most: the 70 % rule cannot drop it.  A builder may then set bit
// h & (2^(B - r) - 1) of a table of 2^(B - r) bits and run the fold rule from R = r: the same (table, R).  search_prefold is the largest
// such r, 0 when none >= 1 qualifies; marks = 0 gives B - 8, the all-zero table of 32 bytes.
MLZ_SEARCH_HD uint32_t search_prefold(uint64_t marks, uint32_t B, uint32_t limit) {
    for (uint32_t r = B - 8; r >= 1; r--)
        if (marks * 100 <= (uint64_t(1) << (B - r)) * limit) return r;
    return 0;
}
// The window positions a block of n bytes can index (the kernels' npos, and for type 4 the windows behind its prefix starts).  next: a block
// follows in the stream.  Type 1: every position, the last block those whose window lies inside it; types 2 and 3: positions 1 .. n, the last
// block's 1 .. n - M; type 4: the prefix starts 0 .. hi (hi = n - 1, the last block's n - K - M - E) reach the windows K .. hi + K + E.
MLZ_SEARCH_HD uint64_t search_table_marks(uint32_t T, uint32_t M, const uint8_t* field, uint64_t n, bool next) {
    if (T == 1) return next ? n : (n + 1 >= M ? n + 1 - M : 0);
    if (T != 4) return next ? n : (n >= M ? n - M : 0);
    const uint64_t K = search_long_k(field), E = search_long_e(field);
    if (next) return n ? n + E : 0;
    return n >= K + M + E ? n - K - M - E + 1 + E : 0;
}

}  // namespace mlz
