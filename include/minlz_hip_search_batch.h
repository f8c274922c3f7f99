/* minlz_hip_search_batch.h — the search over a batch of .mz streams in HBM: an extension of the C ABI of minlz_hip.h (which it includes; the same
 * library, libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_SEARCH_BATCH_H
#define MINLZ_HIP_SEARCH_BATCH_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_stream_search_batch_device: mlz_dev_reader_search_many over a BATCH of streams in HBM, in one call — which of these objects hold any of these keys,
 *   and where (grep -l -F -f keys, and the positions).  `streams[i]` (src_off, src_len; dst_off and dst_cap are ignored) names stream i of the buffer at d_src as
 *   in the batch calls of minlz_hip.h; the patterns as for mlz_dev_reader_search_many (host; 1 .. MLZ_SEARCH_MAX_PATTERNS of them, each 1 .. 256 bytes).  Synchronous;
 *   `stream`, the device routing and the checks of the descriptors are those of mlz_stream_decode_batch_device.
 *   Returns the number of all triples (stream, position, pattern) over the healthy streams (it may exceed cap), or -MLZ_ERR_ARG / -MLZ_ERR_HIP.
 *   Per stream: out_count[i] (host, n_streams values) = what mlz_stream_open_device on stream i alone followed by mlz_dev_reader_search_many under
 *     MLZ_SEARCH_NO_TABLES returns, summed over the patterns: a framing error gives the walk's code and nothing of that stream is searched; a decode or CRC
 *     error gives the first failing chunk's code in the stream's own order; else the stream's count.  One stream's error changes nothing for another.
 *     Descriptors may name the same source bytes more than once (there are no destinations that could overlap).
 *   Positions count inside the stream's own decoded bytes, as mlz_stream_decode_batch_device produces them (a source that holds two concatenated
 *     streams is one decoded sequence).  A pattern never matches across the end of one stream and the start of the next.
 *   Triples: d_hit_stream[k], d_hit_pos[k], d_hit_which[k] (device; all may be NULL when cap == 0) receive the smallest min(total, cap) triples in
 *     ascending order of (index in the descriptor list, position, pattern index).  Nothing at index cap or beyond is ever written; cap == 0 counts only.
 *   d_stream_counts (device, n_streams values, may be NULL): the same counts as out_count, 0 for a failed stream.  d_pattern_counts (device, n_patterns
 *     values, may be NULL): every pattern's occurrences over the healthy streams.
 *   Presence matrix: d_present (device, n_streams rows of ceil(n_patterns / 32) words, may be NULL): bit (p & 31) of word p / 32 of row i = pattern p
 *     occurs in stream i.  Exact whatever cap is (a frequent pattern does not force a large cap); the call clears it, and rows of failed streams stay zero.
 *   Flags: MLZ_STREAM_IGNORE_CRC, MLZ_SEARCH_IGNORE_CASE (the fold of mlz_dev_reader_search), MLZ_SEARCH_NO_TABLES (accepted and implied); any other
 *     bit is -MLZ_ERR_ARG.  Streams that carry search tables are accepted: the walk steps over their chunks and every data chunk with bytes is decoded
 *     (pruning a batch by tables is out of scope).
 *   Failures in the decode are known only after the scan has seen that stream's garbage, so the first pass's results cannot be returned: the failed
 *     streams are dropped from the job list and the scan runs once more over the rest, with the outputs cleared first.  Failures are deterministic, so
 *     there are at most two passes, and the second happens only on corrupt input.
 *   Output on error: an argument error (-MLZ_ERR_ARG: the batch calls' conditions; n_patterns 0 or above MLZ_SEARCH_MAX_PATTERNS; a length of 0 or above
 *     256; a NULL hit array with cap > 0; a device output that is not on the source's device; an unknown flag) launches and writes nothing.  After a
 *     per-stream error the device outputs hold exactly the healthy streams' results; after a second pass the hit positions and patterns between the healthy
 *     triples and min(the first pass's total, cap) are zero.  n_streams == 0 returns 0 and launches nothing.
 *   stats (host, may be NULL, 4 values): data chunks of all streams; chunks decoded over all passes; streams that failed in the decode; scan passes
 *     (0: no chunk with bytes, 1, or 2).  mlz_get_counter 10 reports the second, 12 the streams the walk sent through the region kernels.
 *   How: the streams are laid out as one decoded sequence with a one-byte hole behind each, so that the layout, the scratch decode and the scan kernel of
 *     mlz_dev_reader_search_many run unchanged and no run of chunks, tile or carried byte crosses a stream; a kernel per group sets the presence bits,
 *     and one finishing kernel gives every stream its count and turns the written positions back into (stream, position).
 *   Out of scope: pruning by inline tables or sidecars, records / grep / line numbers over batches, a per-(stream, pattern) count matrix, an asynchronous
 *     form, a batch fanned out over several devices. */
int64_t mlz_stream_search_batch_device(mlz_ctx* ctx, void* stream, uint32_t flags,
                                       const uint8_t* d_src, const mlz_block_desc* streams, int n_streams,   /* src_off, src_len; dst_off = dst_cap = 0 */
                                       const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns,   /* host, as mlz_dev_reader_search_many */
                                       int64_t* out_count,               /* host, n_streams: occurrences in stream i (all patterns), or -MLZ_ERR_* */
                                       uint64_t* d_stream_counts,        /* device, n_streams, may be NULL */
                                       uint64_t* d_pattern_counts,       /* device, n_patterns, may be NULL */
                                       uint32_t* d_present,              /* device, n_streams x ceil(n_patterns / 32) words, may be NULL */
                                       uint32_t* d_hit_stream, uint64_t* d_hit_pos, uint32_t* d_hit_which, size_t cap,   /* device; may be NULL when cap == 0 */
                                       uint64_t* stats /* host, may be NULL: 4 values */);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_SEARCH_BATCH_H */
