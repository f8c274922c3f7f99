// mlz_stream_set_tables.h — the rules of a set of streams that keeps its streams' inline block search tables
// (mlz_stream_open_batch_device_tables, mlz_stream_set_tables.hip.inc), shared with its kernels and its host check
// (tools/stream_set_tables_check.cpp, which runs them as plain loops).  Plain C++: compiles for the host alone and for gfx950.
//
// A set is the streams' concatenation (mlz_stream_set.h), and a stream's tables were built over that stream alone: they say nothing about an
// occurrence that crosses the stream's end.  The plan of one (data chunk k of the handle's list, pattern of L bytes), ORed into take[]:
//   a  inside a stream that a class prunes: the rule of mlz_stream_search.h with chunk numbers and the chunk count taken inside the
//      chunk's own stream (search_chunk_candidate, as batch_plan_mark applies it); the classes are those of the pruned batch search
//      (batch_assign_classes, batch_class_same, batch_class_patterns: mlz_stream_search_batch_prune.h);
//   b  a stream that is decoded whole: every chunk with bytes is a candidate;
//   c  cross[i]: an occurrence may run from stream i into a later stream.  Then every chunk of stream i that holds one of the stream's last
//      L - 1 decoded bytes is a candidate whatever its table says (set_tables_tail): a crossing occurrence starts there, and its first
//      windows may straddle the end and stand in no table.
//      Position calls: cross[i] = stream i has bytes and a later stream with bytes exists (set_tables_cross).
//      Record-bound calls (an occurrence lies inside one record): in addition the record that holds stream i's last byte runs on into the
//      next stream, which is set_joined of the handle's record index (mlz_stream_set.h).
//   d  the marking from a candidate (set_tables_mark_from) runs forward over the handle's chunk list for L - 1 bytes.  It stops at the end
//      of a stream whose cross is false and otherwise passes on into the next streams, whatever their mode.  Chunks and streams without
//      bytes hold nothing and end nothing: the end that counts is that of the last stream with bytes the marking went through.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_search_compressed.h"
#include "mlz_stream_search_batch_prune.h"
#include "mlz_stream_set.h"

namespace mlz {

// A data chunk of the handle as the plan sees it: its stream, its decoded bytes, and the decoded bytes of its stream that lie behind it
struct SetTabChunk { uint64_t n, behind; uint32_t stream, pad; };
static_assert(sizeof(SetTabChunk) == 24, "a record shared with the kernels");

// What mlz_dev_reader_set_tables_info reports
constexpr uint32_t kSetTabInfoValues = 6;

// cross[i] of a position call: stream i has bytes and a later stream has bytes
MLZ_RINDEX_HD bool set_tables_cross(const uint64_t* bases, uint32_t n, uint32_t i) { return bases[i + 1] > bases[i] && bases[i + 1] < bases[n]; }
// cross[i] of a record-bound call.  at(j) = D[j] of the record index, k its delimiters.
template <class At>
MLZ_RINDEX_HD bool set_tables_cross_records(At at, uint64_t k, const uint64_t* bases, uint32_t n, uint32_t i) { return set_joined(at, k, bases, n, i); }

// Rule c: a chunk of n bytes with `behind` bytes of its stream behind it holds one of the stream's last L - 1 bytes
MLZ_SEARCH_HD bool set_tables_tail(uint64_t n, uint64_t behind, uint32_t L) { return n != 0 && behind + 1 < L; }

// Rule d.  ck(j): chunk j of the handle's list (SetTabChunk); cross_of(i): stream i's flag.  Chunk k has bytes.
template <class Ck, class Cross>
MLZ_SEARCH_HD void set_tables_mark_from(size_t k, size_t nck, Ck ck, Cross cross_of, uint32_t L, uint8_t* take) {
    take[k] = 1;
    uint64_t need = L - 1;
    uint32_t last = ck(k).stream;
    for (size_t j = k + 1; j < nck && need; j++) {
        const SetTabChunk c = ck(j);
        if (!c.n) continue;
        if (c.stream != last) {
            if (!cross_of(last)) break;
            last = c.stream;
        }
        take[j] = 1;
        need = c.n >= need ? 0 : need - c.n;
    }
}

// The plan rule of one lane: chunk k of the handle's list and one pattern as the class of the chunk's stream sees it (pt; pt.L is set in
// every record).  st: the chunk's stream (c0, c1: its chunks in the list; mode: kBatchPlanSkip / Whole / Prune).  probe(j, lead): the
// leading (trailing) groups present in the table of chunk j of the list, pt.nw without a usable table.
template <class Probe, class Ck, class Cross>
MLZ_SEARCH_HD void set_tables_plan_mark(size_t k, size_t nck, const BatchPlanStream& st, const SearchManyPat& pt, Probe probe, Ck ck, Cross cross_of, uint8_t* take) {
    const SetTabChunk me = ck(k);
    if (!me.n || st.mode == kBatchPlanSkip) return;
    bool cand = st.mode == kBatchPlanWhole || !pt.nw || (cross_of(me.stream) && set_tables_tail(me.n, me.behind, pt.L));
    if (!cand) {
        const size_t c0 = st.c0;
        cand = search_chunk_candidate(k - c0, size_t(st.c1 - st.c0), [&](size_t j) { return probe(c0 + j, true); }, [&](size_t j) { return probe(c0 + j, false); },
                                      [&](size_t j) { return ck(c0 + j).n; }, pt.nw, pt.L, pt.t_min, 0);
    }
    if (cand) set_tables_mark_from(k, nck, ck, cross_of, pt.L, take);
}

// batch_locate with compressed tables: the first fitting table chunk in [from, limit) behind `skip` fitting ones that an earlier round found
// broken, whichever of 0x45 and 0x46 it is.  A 0x46 chunk is a candidate as search_locate_kernel leaves it: pad = kSearchTabArena, off and
// bytes = its body, which cst_resolve expands or has passed over.
MLZ_SEARCH_HD SearchTab set_tables_locate(const uint8_t* src, uint64_t from, uint64_t limit, uint32_t skip, const SearchConfig& cf) {
    for (uint64_t p = from; p + 4 <= limit;) {
        const uint8_t type = src[p];
        const uint32_t clen = uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
        if (type >= 1 && type <= 3) break;
        if ((type == kChunkSearchTable || type == kChunkSearchTableCompressed) && p + 4 + clen <= limit) {
            const bool packed = type == kChunkSearchTableCompressed;
            const int R = packed ? cst_fixed_fields(src + p + 4, clen, cf.M, cf.B, cf.T, cf.field) : search_table_reductions(src + p + 4, clen, cf.M, cf.B, cf.T, cf.field);
            if (R >= 0 && skip-- == 0) {
                const uint32_t f = search_field_len(cf.T, cf.field);
                const uint8_t* q = src + p + 8 + f;
                const uint32_t crc = uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24;
                return packed ? SearchTab{p + 4, clen, uint32_t(R), crc, kSearchTabArena} : SearchTab{p + 12 + f, clen - 8 - f, uint32_t(R), crc, 0};
            }
        }
        p += 4 + uint64_t(clen);
    }
    return SearchTab{0, 0, kSearchNoTable, 0, 0};
}

}  // namespace mlz
