// mlz_stream_set.h — the rules of a set of streams opened as ONE handle (mlz_stream_open_batch_device and the calls of
// mlz_stream_set.hip.inc), shared with their kernels and their host check (tools/stream_set_check.cpp, which runs them as plain loops).
// Plain C++: compiles for the host alone and for gfx950.
//
// The handle's decoded address space is the streams' decoded bytes one behind the other, in descriptor order:
//   bases     stream i occupies [bases[i], bases[i] + size[i]); bases[0] = 0, bases[i + 1] = bases[i] + size[i]; bases[n] = the handle's size.
//             A stream without bytes (empty, or left out after a framing error) has bases[i] == bases[i + 1]: the bases ascend, not strictly.
//   stream    of position p < size: the LAST i with bases[i] <= p (set_stream_of).  bases[i + 1] > p then (i is the last one), so that stream
//             has bytes whatever empty streams stand in front of it, between or behind.
//   ranges    (which, off, len) names bytes of one stream: which < n, off <= size, len <= size - off, in this order so that nothing wraps
//             (set_range_ok); its place in the handle is bases[which] + off.
//   records   with the record index D[0] < ... < D[k-1] of the handle (mlz_stream_record_index.h; N records): record 0 starts at 0, record
//             r >= 1 at D[r-1] + 1.  first[i] = the records that start below bases[i]: 0 for bases[i] == 0, else min(N, 1 + #{D[j] < bases[i] - 1})
//             (set_first).  first[n] = N.  The stream of record r < N is the stream of its first byte, its number inside r - first[stream].
//   joined    stream i is joined to the next one when it has bytes, its last byte (bases[i + 1] - 1) is no delimiter and bytes follow it
//             (bases[i + 1] < size): a record then continues into the next stream that has bytes (set_joined).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_record_index.h"

namespace mlz {

constexpr uint32_t kSetNoStream = 0xffffffffu;
constexpr uint64_t kSetMaxItems = uint64_t(1) << 31;   // positions, ranges or record numbers of one call: one launch, a lane each

// What comes home from a launch over n items: the items in range (locate, locate_records), "a range is bad" (the range check)
struct SetSums { uint64_t total, bad; };
static_assert(sizeof(SetSums) == sizeof(RindexSums), "the header the record calls zero serves the set's kernels too");

inline void set_bases(const uint64_t* size, size_t n, uint64_t* bases) {
    bases[0] = 0;
    for (size_t i = 0; i < n; i++) bases[i + 1] = bases[i] + size[i];
}

// The last i in [0, n) with bases[i] <= p; n >= 1 and p < bases[n] (bases[0] = 0 <= p always holds)
MLZ_RINDEX_HD uint32_t set_stream_of(const uint64_t* bases, uint32_t n, uint64_t p) {
    uint32_t lo = 0, hi = n;   // bases[lo] <= p; every i >= hi has bases[i] > p
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (bases[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Position p -> (*which, *local); false (kSetNoStream, 0) for p >= size = bases[n]
MLZ_RINDEX_HD bool set_locate(const uint64_t* bases, uint32_t n, uint64_t p, uint32_t* which, uint64_t* local) {
    if (n == 0 || p >= bases[n]) { *which = kSetNoStream; *local = 0; return false; }
    const uint32_t i = set_stream_of(bases, n, p);
    *which = i; *local = p - bases[i];
    return true;
}

// The range check; *global = the range's first byte in the handle
MLZ_RINDEX_HD bool set_range_ok(const uint64_t* bases, uint32_t n, uint32_t which, uint64_t off, uint64_t len, uint64_t* global) {
    *global = 0;
    if (which >= n) return false;
    const uint64_t size = bases[which + 1] - bases[which];
    if (off > size || len > size - off) return false;
    *global = bases[which] + off;
    return true;
}

// The records that start below position b <= size.  at(j) = D[j]; N = the records of the handle.
template <class At>
MLZ_RINDEX_HD uint64_t set_first(At at, uint64_t k, uint64_t N, uint64_t b) {
    if (b == 0) return 0;
    const uint64_t r = 1 + rindex_number(at, k, b - 1);
    return r < N ? r : N;
}

// Stream i is joined to the stream with bytes behind it
template <class At>
MLZ_RINDEX_HD bool set_joined(At at, uint64_t k, const uint64_t* bases, uint32_t n, uint32_t i) {
    const uint64_t b = bases[i], e = bases[i + 1];
    if (e == b || e >= bases[n]) return false;
    const uint64_t j = rindex_number(at, k, e - 1);   // D[j] is the first delimiter at or behind the stream's last byte
    return !(j < k && at(j) == e - 1);
}

// Record r -> (*which, *local_no); false (kSetNoStream, 0) for r >= N.  size = bases[n].
template <class At>
MLZ_RINDEX_HD bool set_locate_record(At at, uint64_t k, uint64_t N, const uint64_t* bases, uint32_t n, uint64_t r, uint32_t* which, uint64_t* local_no) {
    *which = kSetNoStream; *local_no = 0;
    if (n == 0 || r >= N) return false;
    const uint64_t start = r == 0 ? 0 : at(r - 1) + 1;   // r < N: r - 1 < k, and the record's first byte lies below the size
    if (start >= bases[n]) return false;                 // (never, for a table that belongs to the handle)
    const uint32_t i = set_stream_of(bases, n, start);
    *which = i; *local_no = r - set_first(at, k, N, bases[i]);
    return true;
}

}  // namespace mlz
