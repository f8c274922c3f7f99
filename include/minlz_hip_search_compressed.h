/* minlz_hip_search_compressed.h — compressed block search tables (chunk 0x46 of the reference's SPEC_SEARCH.md 2.2) on the read side: an extension of the
 * C ABI of minlz_hip.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++.
 *
 * The searches of minlz_hip.h read such tables by themselves: the first search on a handle (and mlz_dev_reader_attach_sidecar for a sidecar) expands every
 * fitting 0x46 table once into device memory the handle owns, and the plan then probes it like an uncompressed one.  mlz_get_counter(ctx, 14) reports, of
 * the chunks behind counter 11, those whose usable table came from a 0x46 chunk.  The write side is minlz_hip_search_compress.h: the device Writer and build_sidecar emit
 * 0x46 chunks under MLZ_STREAM_SEARCH_COMPRESS, and two calls compress single bitmaps.
 *
 * The one call of this header is the same expansion on the host, for a client that holds a table chunk in host memory. */
#ifndef MINLZ_HIP_SEARCH_COMPRESSED_H
#define MINLZ_HIP_SEARCH_COMPRESSED_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_search_table_expand: the payload of a 0x46 chunk, body[0, len) (the bytes behind the 4-byte chunk header), -> its bitmap, bitmap[0, return value):
 *   2^(B - R - 3) bytes, what a 0x45 chunk of the same table carries behind its CRC.  *out_R (may be NULL) receives the reductions R.  The
 *   configuration is the chunk's own: `T M B field` must be a valid one (types 1 to 4), it is compared with no stream's.
 *   Host only: no context, no GPU.  The rules are the kernels' (the parse, the Huffman table build, the stream decode loop and the sparse walk run as
 *   plain loops).  flags: 0 or MLZ_STREAM_IGNORE_CRC (the bitmap's CRC is not compared with the one the chunk states); any other bit is -MLZ_ERR_ARG.
 *   Returns the bitmap's size; -MLZ_ERR_ARG (a NULL body, a NULL bitmap with cap > 0, len >= 2^24); -MLZ_ERR_CORRUPT for a chunk that is refused:
 *   h0_bs outside 5 .. 17, more than 16 tables, B <= R + 3, a bitmap that is no 1 .. 16 sub-blocks, a table description or a length that leaves the
 *   chunk, weights that miss a power of two, a table log above 11, fewer than two symbols, a table index at or above the table count, a kind above 18,
 *   a stream without end marker or one that does not end exactly at its first bit, a sparse position at or beyond the sub-block's bits, a sparse table
 *   that ends in 255, bytes behind the last sub-block; -MLZ_ERR_DST_TOO_SMALL (cap below the bitmap's size; nothing useful is written);
 *   -MLZ_ERR_CRC.  After an error bitmap's contents are unspecified. */
int64_t mlz_search_table_expand(const uint8_t* body, size_t len, uint8_t* bitmap, size_t cap, uint32_t* out_R, uint32_t flags);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_SEARCH_COMPRESSED_H */
