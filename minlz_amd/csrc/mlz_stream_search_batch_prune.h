// mlz_stream_search_batch_prune.h — what the pruned search over a batch of streams in HBM (mlz_stream_search_batch_prune.hip.inc) shares with its
// kernels and its host check (tools/stream_search_batch_prune_check.cpp): the key a stream's info chunk leaves, the numbering of the batch's
// table configurations ("classes"), the byte-for-byte check of a stream against its class, the hop of one data chunk to its table, a class's
// pattern records, the plan rule of one (data chunk, pattern) with its index arithmetic inside the chunk's own stream, and the stats rule.
// The probes and the rule itself are those of mlz_stream_search.h.  Plain C++: compiles for the host alone and for gfx950.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mlz_stream_search.h"

namespace mlz {

constexpr uint8_t kBatchNoClass = 0xff;

// What search_batch_info_kernel leaves per stream: (T, M, B) and whether the info chunk is usable (search_info's verdict), the prefix field's
// length and a 64-bit hash over `T M B field` — the 16 bytes that come home per stream —, and, in an array that stays on the device, where
// the info chunk's payload lies (counted from the batch's base).
struct BatchInfoKey { uint8_t T, M, B, ok; uint16_t flen, pad; uint64_t hash; };
static_assert(sizeof(BatchInfoKey) == 16, "a record shared with the kernels");
// A class's configuration on its way home: the info payload of the class's first stream, `T M B field`, in a slot of this size
constexpr uint32_t kBatchPayloadSlot = 264;
static_assert(kBatchPayloadSlot >= 3 + kSearchMaxField, "a slot holds the longest payload");

// search_info's verdict on a 0x44 payload without the copy of the field (a lane has no room for 258 bytes); *flen = the field's length
MLZ_SEARCH_HD bool batch_info_fits(const uint8_t* p, uint32_t clen, uint32_t* flen) {
    *flen = 0;
    if (clen < 3 || p[0] < 1 || p[0] > 4 || p[1] < 1 || p[1] > 8 || p[2] < 8 || p[2] > 23) return false;
    if (p[0] == 4 && (clen < 5 || p[4] > kSearchMaxExtras || p[1] + p[4] > kSearchMaxGroupWindows)) return false;
    const uint32_t f = search_field_len(p[0], p + 3);
    if (clen < 3 + f) return false;
    *flen = f;
    return true;
}

// FNV-1a over n bytes
MLZ_SEARCH_HD uint64_t batch_hash(const uint8_t* p, uint32_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// The hop of search_info_kernel over one stream of the batch: from the stream's first byte (`start`, counted from src) to `limit`, its first
// data chunk's body or its end.  The first 0x44 behind an identifier decides; no key: ok = 0.  *at = where the payload lies.
MLZ_SEARCH_HD BatchInfoKey batch_info_key(const uint8_t* src, uint64_t start, uint64_t limit, uint64_t* at) {
    BatchInfoKey key{0, 0, 0, 0, 0, 0, 0};
    *at = 0;
    bool seen_id = false;
    for (uint64_t p = start; p + 4 <= limit;) {
        const uint8_t type = src[p];
        const uint32_t clen = uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
        if (type >= 1 && type <= 3) break;
        if (type == 0xff) seen_id = true;
        else if (type == kChunkSearchInfo && seen_id) {
            uint32_t flen = 0;
            if (p + 4 + clen <= limit && batch_info_fits(src + p + 4, clen, &flen)) {
                const uint8_t* q = src + p + 4;
                key = BatchInfoKey{q[0], q[1], q[2], 1, uint16_t(flen), 0, batch_hash(q, 3 + flen)};
                *at = p + 4;
            }
            break;
        }
        p += 4 + uint64_t(clen);
    }
    return key;
}

MLZ_SEARCH_HD bool batch_key_equal(const BatchInfoKey& a, const BatchInfoKey& b) { return a.T == b.T && a.M == b.M && a.B == b.B && a.flen == b.flen && a.hash == b.hash; }

// The classes: the distinct keys of the streams that take part (part[i] != 0, key ok), numbered in descriptor order.  cls[i] = the stream's
// class when it is one of the first kSidecarMaxConfigs, else kBatchNoClass; rep[c] = the first stream of class c.  Returns the number of
// classes found, which may exceed kSidecarMaxConfigs.
inline uint32_t batch_assign_classes(const BatchInfoKey* keys, const uint8_t* part, size_t n, uint8_t* cls, size_t* rep) {
    std::vector<BatchInfoKey> seen;
    for (size_t i = 0; i < n; i++) {
        cls[i] = kBatchNoClass;
        if (!part[i] || !keys[i].ok) continue;
        size_t c = 0;
        while (c < seen.size() && !batch_key_equal(seen[c], keys[i])) c++;
        if (c == seen.size()) {
            if (c < kSidecarMaxConfigs) rep[c] = i;
            seen.push_back(keys[i]);
        }
        if (c < kSidecarMaxConfigs) cls[i] = uint8_t(c);
    }
    return uint32_t(seen.size());
}

// A stream's info payload (`T M B field` at p) against its class's configuration, byte for byte: a hash collision must never prune
MLZ_SEARCH_HD bool batch_class_same(const uint8_t* p, uint32_t flen, const SearchConfig& cf) {
    if (p[0] != cf.T || p[1] != cf.M || p[2] != cf.B || flen != search_field_len(cf.T, cf.field)) return false;
    for (uint32_t i = 0; i < flen; i++) if (p[3 + i] != cf.field[i]) return false;
    return true;
}

// search_locate_kernel's hop for one data chunk: the headers in [from, limit) (the previous data chunk's end, or the stream's first byte, to
// the chunk's body), the first 0x45 that fits the configuration behind `skip` fitting ones that an earlier round found broken.  A 0x46
// chunk is stepped over like any other chunk.
MLZ_SEARCH_HD SearchTab batch_locate(const uint8_t* src, uint64_t from, uint64_t limit, uint32_t skip, const SearchConfig& cf) {
    SearchTab t{0, 0, kSearchNoTable, 0, 0};
    for (uint64_t p = from; p + 4 <= limit;) {
        const uint8_t type = src[p];
        const uint32_t clen = uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
        if (type >= 1 && type <= 3) break;
        if (type == kChunkSearchTable && p + 4 + clen <= limit) {
            const int R = search_table_reductions(src + p + 4, clen, cf.M, cf.B, cf.T, cf.field);
            if (R >= 0 && skip-- == 0) {
                const uint32_t f = search_field_len(cf.T, cf.field);
                const uint8_t* q = src + p + 8 + f;
                return SearchTab{p + 12 + f, clen - 8 - f, uint32_t(R), uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24, 0};
            }
        }
        p += 4 + uint64_t(clen);
    }
    return t;
}

// One class's view of the call's patterns (off[i] .. off[i + 1]: pattern i in `patterns`, folded under `fold`): pats[i] and the hashes they
// name, appended to *hs (and *voff under folding) — a class's records index the call's ONE hash array.  False: the configuration cannot
// serve every pattern (no window, every window abstains, or under folding the class's kSearchFoldMaxHashes are spent), and every stream
// of the class is decoded whole; what was appended is taken back.
inline bool batch_class_patterns(const SearchConfig& cf, const uint8_t* patterns, const uint32_t* off, size_t n, bool fold, SearchManyPat* pats,
                                 std::vector<uint32_t>* hs, std::vector<uint32_t>* voff) {
    std::vector<uint32_t> win(kSearchMaxWindows);
    const size_t h0 = hs->size(), v0 = voff->size();
    for (size_t i = 0; i < n; i++) {
        const uint32_t L = off[i + 1] - off[i];
        pats[i] = SearchManyPat{0, 0, 1, 1, L, 0};
        const bool ok = fold ? search_pattern_hashes_fold(patterns + off[i], L, cf.T, cf.M, cf.B, cf.field, win.data(), voff, hs, &pats[i],
                                                          uint32_t(kSearchFoldMaxHashes - (hs->size() - h0)))
                             : search_pattern_hashes(patterns + off[i], L, cf.T, cf.M, cf.B, cf.field, win.data(), hs, &pats[i]);
        if (!ok) {
            hs->resize(h0); voff->resize(v0);
            for (size_t j = 0; j < n; j++) pats[j] = SearchManyPat{0, 0, 1, 1, off[j + 1] - off[j], 0};
            return false;
        }
    }
    return true;
}

// A stream of the batch as the plan sees it: its data chunks [c0, c1) of the batch's chunk list, where it starts in the source (the first
// chunk's `from`) and how it is planned.
constexpr uint32_t kBatchPlanSkip = 0, kBatchPlanWhole = 1, kBatchPlanPrune = 2;   // not searched (a framing error) | decoded whole | pruned by its class
struct BatchPlanStream { uint64_t start, limit; uint32_t c0, c1, mode, cls; };
static_assert(sizeof(BatchPlanStream) == 32, "a record shared with the kernels");

// The plan rule of one lane, (data chunk k of the batch's list, one pattern as the chunk's stream's class sees it): the rule of
// mlz_stream_search.h with k and the number of chunks taken inside the chunk's own stream [c0, c1) — the last chunk of a stream has no
// next chunk, and the marking never runs into the next stream.  probe(j, lead): the leading (trailing) groups present in the table of chunk
// j of the list (pt.nw without a usable table); n_of(j): its decoded bytes.  Marks take[] (stores of 1 only).
template <class Probe, class N>
MLZ_SEARCH_HD void batch_plan_mark(size_t k, const BatchPlanStream& st, const SearchManyPat& pt, Probe probe, N n_of, uint8_t* take) {
    if (st.mode == kBatchPlanSkip) return;
    if (st.mode == kBatchPlanWhole) { if (n_of(k)) take[k] = 1; return; }
    const size_t c0 = st.c0, nck = st.c1 - st.c0;
    auto sizes = [&](size_t j) { return n_of(c0 + j); };
    auto admits = [&](uint32_t) {
        if (!pt.nw) return true;
        return search_chunk_candidate(k - c0, nck, [&](size_t j) { return probe(c0 + j, true); }, [&](size_t j) { return probe(c0 + j, false); }, sizes, pt.nw, pt.L, pt.t_min, 0);
    };
    search_decoded_mark_all(k - c0, nck, 1, admits, sizes, pt.L, take + c0);
}

// The plan's traffic to the host (contract: at most 32 bytes per stream and one byte per data chunk, a class's configuration apart): the
// key and the class verdict per stream, the byte per chunk, and per CRC round one word (the tiles of the tables the round checks; none: the
// rounds are over).  batch_crc_rounds: the most rounds the bound pays for — a batch of one stream affords three; a table that is still
// stale when they are spent counts as no table, and its chunk is admitted.
constexpr uint64_t kBatchHomePerStream = sizeof(BatchInfoKey) + 1, kBatchHomePerRound = 4;
MLZ_SEARCH_HD uint64_t batch_plan_bound(uint64_t n_streams, uint64_t n_chunks) { return 32 * n_streams + n_chunks; }
MLZ_SEARCH_HD uint64_t batch_crc_rounds(uint64_t n_streams) { return (32 - kBatchHomePerStream) * n_streams / kBatchHomePerRound; }

// The stats rule: values 4, 5 and 7 of the call's stats from the plan.  tabbed[k] != 0: chunk k has a usable table.
//   4: chunks with a usable table in a stream that is pruned; 5: streams of which no chunk is taken although they hold bytes;
//   7: streams that hold bytes and are decoded whole (no usable info chunk, a class beyond the first kSidecarMaxConfigs, a field that differs from
//      its class's, or a class that cannot serve a pattern).
template <class N>
inline void batch_prune_stats(const BatchPlanStream* st, size_t n, const uint8_t* take, const uint8_t* tabbed, N n_of, uint64_t* s4, uint64_t* s5, uint64_t* s7) {
    *s4 = *s5 = *s7 = 0;
    for (size_t i = 0; i < n; i++) {
        if (st[i].mode == kBatchPlanSkip) continue;
        bool bytes = false, any = false;
        for (size_t k = st[i].c0; k < st[i].c1; k++) {
            bytes = bytes || n_of(k);
            any = any || take[k];
            if (st[i].mode == kBatchPlanPrune && tabbed[k]) ++*s4;
        }
        if (bytes && !any) ++*s5;
        if (bytes && st[i].mode == kBatchPlanWhole) ++*s7;
    }
}

}  // namespace mlz
