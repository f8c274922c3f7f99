/* minlz_hip_encode_batch_tables.h — the batch Writer with block search tables: many inputs in HBM written as .mz streams of their own, each with
 * the tables the device Writer gives one stream, in one call.  An extension of the C ABI of minlz_hip.h (which it includes; the same library,
 * libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_ENCODE_BATCH_TABLES_H
#define MINLZ_HIP_ENCODE_BATCH_TABLES_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_stream_encode_batch_device_tables: mlz_stream_encode_batch_device whose streams carry block search tables of ONE configuration, table type 1 .. 4
 *   (cfg: the sidecar's mlz_search_config).  Arguments, checks and per-stream results are those of mlz_stream_encode_batch_device; cfg == NULL IS that call.
 *   out_len[i] and stream i's bytes are byte for byte what mlz_stream_encode_gather_device_tables (types 1 .. 3) or _long_prefix (type 4) writes for the
 *     one range d_src + src_off with the same level, block size and MLZ_STREAM_ADD_INDEX: the info chunk (0x44) behind the identifier, an uncompressed
 *     table chunk (0x45) in front of every block that is stored compressed and none in front of a stored one, index entries that point at a block's
 *     table chunk, no head for an empty input.  A block sees the bytes of ITS stream that follow it (the configuration's overlap at the most, zeros
 *     beyond the stream's end), never the next stream's.  mlz_stream_search_batch_device_pruned reads what this call writes.
 *   Room: stream i needs dst_cap >= mlz_stream_bound_config(src_len, block_size, flags, cfg), which equals mlz_stream_bound_tables / _long_prefix for the
 *     same configuration; with less it gets -MLZ_ERR_DST_TOO_SMALL and nothing of it is written.  One stream's error changes nothing for another.
 *   -MLZ_ERR_ARG, before anything is launched or written: a configuration the single Writers refuse (a type outside 1 .. 4, match_len > 8, type 2 with 0
 *     or more than 8 values, a prefix of 0 or more than 256 bytes, extras > 15 or match_len + extras > 16, extras with types 1 .. 3, a reserved byte
 *     that is not 0); flags that carry MLZ_STREAM_SEARCH_TABLES or match-length bits beside a cfg; MLZ_STREAM_SEARCH_COMPRESS — the pruned batch search
 *     does not read compressed table chunks (0x46), and the compress stage was measured at 2.3 x the Writer it would ride on.
 *   Tables: a table's size comes from the block size (B = the bits of block_size - 1), and in a batch every stream's last block is short.  A block is
 *     therefore built already folded r0 = mlz_search_table_prefold(marks, B, type) times, marks = the window positions its length lets it index: the folds
 *     that the Writer's rule is certain to accept whatever the data.  Its slot of workspace has 2^(B - r0 - 3) bytes, not 2^(B - 3), and the bytes are
 *     the single Writer's.  mlz_get_counter(ctx, 17): the bytes of table slots the last call carved, over the blocks of the streams that had room.
 *   Traffic to the host: 12 more bytes per block than the plain call (table bytes, R, the table's CRC); the tables' CRCs come from the library's CRC
 *     pass over the kept tables, behind ONE more host synchronisation than the plain call has.  Synchronous; `stream` as for the plain call.
 *   Out of scope: compressed table chunks (0x46) and sidecars in batches, a configuration per stream, a batch fanned out over several devices.
 * mlz_stream_bound_config: host only; mlz_stream_bound for a stream written with cfg (NULL: mlz_stream_bound), or -MLZ_ERR_ARG.
 * mlz_search_table_prefold: host only; the rule above — the largest r with B - r >= 8 and marks * 100 <= 2^(B - r) * limit, limit 25 for type 1 and 10
 *   for the others, 0 when no r >= 1 qualifies — or -MLZ_ERR_ARG (B outside 8 .. 23, a type outside 1 .. 4, marks above 2^32). */
int64_t mlz_stream_bound_config(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_config* cfg);
int64_t mlz_search_table_prefold(uint64_t marks, uint32_t B, uint32_t table_type);
int mlz_stream_encode_batch_device_tables(mlz_ctx* ctx, void* stream, int level, uint32_t block_size, uint32_t flags,
                                          const mlz_search_config* cfg, const uint8_t* d_src, uint8_t* d_dst,
                                          const mlz_block_desc* streams, int n_streams, int64_t* out_len);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_ENCODE_BATCH_TABLES_H */
