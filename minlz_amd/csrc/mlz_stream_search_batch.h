// mlz_stream_search_batch.h — what the search over a batch of streams in HBM (mlz_stream_search_batch.hip.inc) shares with its kernels and its
// host check (tools/stream_search_batch_check.cpp): the virtual positions that lay the streams of a batch out as ONE decoded sequence with holes,
// the rule that turns a virtual position back into (stream, position), the streams of the tiles and the count of a stream from the running
// prefix over the tile counts.  Plain C++: compiles for the host alone and for gfx950.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_search.h"

namespace mlz {

// Stream i of a batch occupies the virtual positions [vbase[i], vbase[i] + size[i]); vbase[i + 1] = vbase[i] + size[i] + 1.  The one-byte
// hole behind every stream means that the last chunk of one stream and the first chunk of the next are never neighbours for search_layout
// (out_off + n of the one is not out_off of the other), so no run, no tile and no carried byte crosses a stream, while the chunks of one
// stream are neighbours as they are in a single-stream search.  vbase has n + 1 values and ascends strictly (an empty stream still takes its hole).
inline void batch_vbases(const uint64_t* size, size_t n, uint64_t* vbase) {
    vbase[0] = 0;
    for (size_t i = 0; i < n; i++) vbase[i + 1] = vbase[i] + size[i] + 1;
}

// The one rule that turns a virtual position into its stream: the last i in [0, n) with vbase[i] <= v (n >= 1, v < vbase[n]).  The position
// inside the stream is v - vbase[i].
MLZ_SEARCH_HD size_t batch_stream_of(const uint64_t* vbase, size_t n, uint64_t v) {
    size_t lo = 0, hi = n;   // vbase[lo] <= v < vbase[hi]
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (vbase[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// The streams of the tiles.  The jobs of a batch stand in descriptor order and the groups ascend, so the tiles of one stream are contiguous in
// the tile list: tile_stream[t] = the stream of tile t (of its first position), tile_first[i] .. tile_first[i + 1] = the tiles of stream i
// (n + 1 values, tile_first[n] = the number of tiles; a stream without a tile: an empty range).  Returns false where the tiles' streams
// do not ascend or a tile reaches over its stream's end (never, for a layout made from the virtual positions).
inline bool batch_tile_streams(const SearchTile* tiles, size_t nt, const uint64_t* vbase, size_t n, uint32_t* tile_stream, uint32_t* tile_first) {
    bool ok = true;
    size_t s = 0;
    tile_first[0] = 0;
    for (size_t t = 0; t < nt; t++) {
        const size_t i = batch_stream_of(vbase, n, tiles[t].gpos);
        if (i < s || tiles[t].gpos + tiles[t].hi_end > vbase[i + 1] - 1) ok = false;
        tile_stream[t] = uint32_t(i);
        for (; s < i; s++) tile_first[s + 1] = uint32_t(t);
    }
    for (; s < n; s++) tile_first[s + 1] = uint32_t(nt);
    return ok;
}

// The finish rule's count: prefix_of(t) = the pairs of the tiles in front of tile t (t < nt), total = the pairs of all tiles; a stream's
// count is the pairs of its tiles.
template <class P>
MLZ_SEARCH_HD uint64_t batch_stream_count(P prefix_of, size_t nt, uint64_t total, const uint32_t* tile_first, size_t i) {
    const size_t a = tile_first[i], b = tile_first[i + 1];
    return (b < nt ? prefix_of(b) : total) - (a < nt ? prefix_of(a) : total);
}

}  // namespace mlz
