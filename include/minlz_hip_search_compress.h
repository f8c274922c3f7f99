/* minlz_hip_search_compress.h — compressed block search tables (chunk 0x46 of the reference's SPEC_SEARCH.md 2.2) on the write side: an extension of the
 * C ABI of minlz_hip.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++.  The read side is minlz_hip_search_compressed.h.
 *
 * Both calls turn a table's bitmap (what a 0x45 chunk carries behind its CRC: 2^(B - R - 3) bytes) into the HUFF0 SECTION of the 0x46 chunk of the same
 * table: everything behind the CRC, `h0_bs | h0_tc | table descriptions | sub-blocks`.  A client frames it itself: the 0x46 payload is the 0x45 payload's
 * fixed fields (`T M B | field | R | crc32 of the bitmap`) followed by the section, and the reference's rule is to write the 0x46 chunk where it is strictly
 * smaller than the 0x45 chunk, that is where the section is shorter than the bitmap.
 *
 * The section is a function of the bitmap's bytes alone:
 *   partition   up to 32 KiB one sub-block; up to 512 KiB, 32 KiB sub-blocks; larger, 64 KiB sub-blocks
 *   kind        one byte value: 17 (RLE); else the smallest of raw (the sub-block's bytes), sparse (its table's bytes + 3) and huff (description + 9 +
 *               ceil(bits / 8) + 3), ties in that order; a table of its own per tabled sub-block, so at most 16 tables
 *   lengths     Huffman: the two smallest nodes by (weight, smallest symbol in the node) are merged; deeper than 11: all counts halved (at least 1), again
 *   description direct 4-bit weights where at most 128 are listed, FSE-compressed (accuracy log 6, two states) where that takes fewer than 128 bytes; the
 *               shorter, direct in a tie; where neither carries the weights the sub-block is raw or sparse
 *   streams     four streams over a quarter of the sub-block each behind a 6-byte jump table, RFC 8878 4.2
 * mlz_search_table_expand (minlz_hip_search_compressed.h) and every search of minlz_hip.h read what these calls write.
 * The device Writer and mlz_dev_reader_build_sidecar run the same kernels under MLZ_STREAM_SEARCH_COMPRESS (minlz_hip.h).
 * Out of scope: tables shared between sub-blocks, the reference's popcount-band and minimum-size skips. */
#ifndef MINLZ_HIP_SEARCH_COMPRESS_H
#define MINLZ_HIP_SEARCH_COMPRESS_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_search_bitmap_compress: bitmap[0, n) -> its section, dst[0, return value).  Host only: no context, no GPU.
 *   Returns the section's length, never above n + 2 + 16; -MLZ_ERR_ARG (a NULL bitmap, a NULL dst with cap > 0, n not a power of two in 32 .. 2^20);
 *   -MLZ_ERR_DST_TOO_SMALL (cap below the section's length; nothing useful is written). */
int64_t mlz_search_bitmap_compress(const uint8_t* bitmap, size_t n, uint8_t* dst, size_t cap);

/* mlz_search_bitmaps_compress_device: the same for n bitmaps in device memory, by kernels, in one launch sequence on `stream` (0: the default stream); the
 *   call returns when they have run.  Item i: the bitmap d_src[tables[i].src_off, + src_len) -> d_dst[tables[i].dst_off, + the section's length), at most
 *   dst_cap bytes; d_len[i] (device memory) receives the section's length, or the item's own error: -MLZ_ERR_ARG (src_len not a power of two in
 *   32 .. 2^20), -MLZ_ERR_DST_TOO_SMALL (nothing is written for this item).  One item's error changes nothing for another item.  tables is host memory.
 *   Nothing is written outside the sections.  Returns 0, -MLZ_ERR_ARG (a NULL pointer with n > 0, n < 0, buffers on a device the context does not hold),
 *   -MLZ_ERR_HIP. */
int mlz_search_bitmaps_compress_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* tables, int n, int64_t* d_len);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_SEARCH_COMPRESS_H */
