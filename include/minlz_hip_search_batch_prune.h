/* minlz_hip_search_batch_prune.h — the search over a batch of .mz streams in HBM, pruned by the streams' inline block search tables: an extension of
 * the C ABI of minlz_hip_search_batch.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_SEARCH_BATCH_PRUNE_H
#define MINLZ_HIP_SEARCH_BATCH_PRUNE_H

#include "minlz_hip_search_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_stream_search_batch_device_pruned: mlz_stream_search_batch_device that decodes only the chunks the streams' block search tables cannot rule out.
 *   Arguments, outputs, checks, the second pass on a decode failure and what is written on error are those of mlz_stream_search_batch_device; `stats` has
 *   8 values.  Flags: MLZ_STREAM_IGNORE_CRC, MLZ_SEARCH_IGNORE_CASE, MLZ_SEARCH_NO_TABLES (the call then IS mlz_stream_search_batch_device; stats 4 .. 7
 *   are 0); any other bit is -MLZ_ERR_ARG.
 *   Results: the total, out_count, d_stream_counts, d_pattern_counts, the presence matrix and the triples are defined as for the unpruned call, and for
 *     streams with truthful tables they are identical to it.  out_count[i] = what mlz_stream_open_device on stream i alone followed by
 *     mlz_dev_reader_search_many with the same CRC and case flags and WITHOUT MLZ_SEARCH_NO_TABLES returns, summed over the patterns: an error in a chunk
 *     the plan pruned goes unnoticed, as in every search that prunes.  A pattern never matches across two streams; one stream's error changes nothing
 *     for another.
 *   A batch with inline tables is written in one call by mlz_stream_encode_batch_device_tables (include/minlz_hip_encode_batch_tables.h).
 *   Which chunks are decoded: for stream i exactly the set mlz_dev_reader_search_many on stream i alone decodes — the union over the patterns of the
 *     rule of SPEC_SEARCH.md Appendix B.4.1, and every chunk with bytes once any pattern is not served by the stream's configuration (a pattern
 *     shorter than M, no window behind a prefix byte; under MLZ_SEARCH_IGNORE_CASE the budget of case-variant hashes as well) — with two exceptions:
 *     Configuration classes: the distinct configurations (T, M, B, prefix field) of the batch's streams are numbered in descriptor order, and only the
 *       first 4 classes prune.  A stream of a later class, or without a usable info chunk (0x44), is decoded whole.
 *     Compressed tables: only uncompressed table chunks (0x45) are used.  A compressed table chunk (0x46) counts as no table and its data chunk is
 *       admitted: this call owns no handle that could keep the expanded tables, so it would pay the expansion in every call, and expanding 96 tables of
 *       64 KiB was measured at 2.03 ms where decoding the 96 blocks of 1 MiB they stand for takes about 1.0 ms.
 *   A table that fails its CRC, or does not fit the stream's info chunk, is passed over for the next fitting one in front of the same data chunk, as in
 *     the single-stream search, in rounds over the whole batch that stay on the device; under MLZ_STREAM_IGNORE_CRC the tables' CRCs are not checked.
 *     The traffic bound below pays for 15 * n_streams / 4 rounds (a batch of one stream: three); a table that is still stale when they are spent
 *     counts as no table, and its chunk is admitted.
 *   stats (host, may be NULL, 8 values): 0 data chunks of all streams; 1 chunks decoded over all passes; 2 streams that failed in the decode; 3 scan
 *     passes; 4 chunks with a usable table in a stream that is pruned (its class serves every pattern); 5 streams of which no chunk was decoded although
 *     they hold bytes; 6 configuration classes found (it may exceed 4); 7 streams that hold bytes and are decoded whole because their class does not
 *     prune or cannot serve a pattern.  mlz_get_counter 10 and 11 report values 1 and 4; counter 14 is 0.
 *   Traffic to the host for the plan, besides the walk's: at most 32 bytes per stream plus one byte per data chunk — 16 bytes of key and one of class
 *     verdict per stream, one byte per data chunk, and unless MLZ_STREAM_IGNORE_CRC is given 4 bytes per CRC round (two rounds where no table is
 *     stale) —, and a class's configuration (264 bytes) once per class.  mlz_get_counter 16 reports the bytes of the last call, the configurations apart.
 *   Out of scope: compressed tables (0x46) and sidecars in batches, more than 4 pruning classes, a
 *     per-(stream, pattern) count matrix, an asynchronous form, a batch fanned out over several devices. */
int64_t mlz_stream_search_batch_device_pruned(mlz_ctx* ctx, void* stream, uint32_t flags,
                                              const uint8_t* d_src, const mlz_block_desc* streams, int n_streams,
                                              const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns,
                                              int64_t* out_count,
                                              uint64_t* d_stream_counts, uint64_t* d_pattern_counts, uint32_t* d_present,
                                              uint32_t* d_hit_stream, uint64_t* d_hit_pos, uint32_t* d_hit_which, size_t cap,
                                              uint64_t* stats /* host, may be NULL: 8 values */);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_SEARCH_BATCH_PRUNE_H */
