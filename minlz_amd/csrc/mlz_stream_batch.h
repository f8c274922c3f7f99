// mlz_stream_batch.h — what the batch calls over many streams in HBM (mlz_stream_batch.hip.inc) share with their host check
// (tools/stream_batch_check.cpp): the chunk walk one lane runs over one stream of the batch (mlz_stream_walk.h's header step under a cap),
// the verdict of one decoded chunk (the host Reader's too), and the verdicts of the streams from those of their chunks.  Plain C++: compiles for the host alone and for gfx950.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_walk.h"

namespace mlz {

// The most chunk headers one lane of walk_batch_kernel steps over.  A stream with more of them is LONG: the lane stops, the stream's
// count is 0 and its flag is set, and the call walks it by the region kernels of mlz_stream_walk.hip.inc instead.
constexpr uint32_t kBatchWalkSteps = 4096;

// The chunk walk of the whole stream src[0, n), header by header (walk_headers, which walk_list_kernel runs inside one region), under a
// step cap.  EMIT: the records go to out[0, limit); without it they are counted.  Returns the entries; *is_long: the stream has more than
// max_steps headers (the entries are then void).  Reads what walk_headers and walk_classify read: src[0, n) and nothing else.
template <bool EMIT>
MLZ_WALK_HD uint32_t batch_walk_lane(const uint8_t* src, uint64_t n, uint32_t max_steps, WalkChunk* out, uint32_t limit, bool* is_long) {
    uint32_t cnt = 0;
    *is_long = !walk_headers(src, n, 0, n, false, max_steps, [&](uint64_t e) {
        if (EMIT && cnt < limit) out[cnt] = walk_classify(src, n, e);
        cnt++;
        return true;
    });
    return *is_long ? 0 : cnt;
}

// Error codes as in include/minlz_hip.h (MLZ_ERR_*), negated on return.
constexpr int kBatchErrCorrupt = 1, kBatchErrCrc = 5;

// One chunk after its decode and CRC: 0 or its error.  compressed: a 0x02 / 0x03 chunk, whose decode left `got` (the decoded length or
// -MLZ_ERR_*) for a chunk of n bytes; check_crc: crc_got against the chunk's own.  The body's error comes before the CRC's.
inline int64_t chunk_job_verdict(bool compressed, int64_t got, uint64_t n, bool check_crc, uint32_t crc_got, uint32_t crc_want) {
    if (compressed && got != int64_t(n)) return got < 0 ? got : -int64_t(kBatchErrCorrupt);
    if (check_crc && crc_got != crc_want) return -int64_t(kBatchErrCrc);
    return 0;
}

// Per-stream verdicts of a batch: stream i owns jobs [job_first[i], job_first[i + 1]) of the one job list, in its own chunk order, and
// parsed[i] is what the walk of its framing said (or the error that kept its chunks out of the list).  out[i] = the first failing job's
// error in the stream's order, else parsed[i]: the Reader decodes the chunks in front of a framing error before it reports that error.
inline void batch_stream_verdicts(const int64_t* parsed, const size_t* job_first, const int64_t* job_rc, size_t n_streams, int64_t* out) {
    for (size_t i = 0; i < n_streams; i++) {
        out[i] = parsed[i];
        for (size_t j = job_first[i]; j < job_first[i + 1]; j++)
            if (job_rc[j] < 0) { out[i] = job_rc[j]; break; }
    }
}

}  // namespace mlz
