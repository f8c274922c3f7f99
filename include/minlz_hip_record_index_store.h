/* minlz_hip_record_index_store.h — the record index of a stream in device memory saved, loaded and built without a decode: an extension of the C ABI of
 * minlz_hip.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++.
 *
 * mlz_dev_reader_index_records decodes the whole stream to find the delimiters, and its table (8 bytes per delimiter) dies with the handle.  The calls
 * here keep the index in a compact stored form, the RECORD INDEX BLOB: a valid MinLZ stream that holds no data (a Reader decodes it to zero bytes).
 * All integers are little-endian.
 *
 *   ff 06 00 00 "MinLz" 0d                                              stream identifier, block-size value 13
 *   90 <len24> crc32 <fixed header, 62 B> <directory: nsections x u32>  header chunk (user-defined skippable)
 *   91 <len24> crc32 <section>                                          one per section, in order
 *   20 01 00 00 00                                                      EOF, size 0
 *
 * crc32: the masked CRC32C of the rest of the chunk's body, the data chunks' function.
 * Fixed header: 0 "MLZRIDX1" | 8 u32 flags (bit 0 = bound to a stream, bit 1 = longest record known) | 12 u8 delimiter, 3 zero bytes | 16 u64 decoded
 *   size | 24 u64 k, the delimiters | 32 u64 N, the records | 40 u64 longest record (all ones when unknown) | 48 u32 stream tag | 52 u32 data chunks with
 *   bytes | 56 u32 nsections | 60 u16 zero.  62 bytes, so that every section starts at a multiple of 4 inside the blob.
 * Directory: each entry is the length of that section, the chunk's body behind its CRC.
 * A tile is 65 536 decoded positions, tile t = [t * 65536, (t + 1) * 65536) in ABSOLUTE positions; a section is 1024 consecutive tiles;
 *   nsections = ceil(ceil(size / 65536) / 1024), 0 for size 0.
 * Section: u32 section number | u32 tiles | u64 rank of the section's first delimiter | tiles + 1 u32 cumulative delimiter counts inside the section
 *   (the first is 0) | the tiles' payloads in order.  Payload of a tile with c delimiters: c <= 4096 (sparse): c u16 of D[j] - t * 65536, strictly
 *   ascending, and one zero u16 when c is odd; c > 4096 (dense): 8192 bytes, bit j & 7 of byte j >> 3 set when position t * 65536 + j is a delimiter,
 *   bits at or beyond the size zero.  The choice is a rule: the blob is a function of (D, size, delimiter, binding, longest).
 * Size: at most overhead + min(2 k + 2 tiles, 8192 tiles): about 2 bytes per record for text, never more than an eighth of the data.
 * Bound: a blob saved from a handle carries the handle's tag — the masked CRC32C over 9 bytes per data chunk with bytes, in the handle's order: u32 decoded
 *   length, u32 stored CRC field, u8 chunk type — and the number of those chunks.  A blob built from raw bytes is unbound: flag bit 0 clear, tag 0, chunks 0.
 *
 * All calls with a reader or a context are synchronous, run under the context's lock and take `stream` as the other reader calls do.  Handles over a
 * set of streams (mlz_stream_open_batch_device) save and load like any handle.
 *
 * mlz_dev_reader_record_index_bound: bytes that always suffice for save; -MLZ_ERR_ARG without an index.
 * mlz_dev_reader_save_record_index: the handle's index as a bound blob at d_dst -> the blob's bytes.  info (4 values, may be NULL): bytes, sections,
 *   sparse tiles (empty ones among them), dense tiles.  Flag bit 1 and `longest` where the handle knows the longest record (after a grep_regex).
 *   -MLZ_ERR_ARG (NULL, no index, d_dst not on the handle's device), -MLZ_ERR_DST_TOO_SMALL (nothing written; info[0] holds the size), -MLZ_ERR_HIP.
 * mlz_dev_reader_load_record_index: the blob at d_blob[0, len) becomes the handle's index -> N.  Nothing is decoded.  flags: 0 or MLZ_STREAM_IGNORE_CRC
 *   (the CRCs of the blob's chunks are not looked at).  info (4 values, may be NULL): as mlz_dev_reader_index_records', with info[3] (chunks decoded) = 0.
 *   The checks, in this order, and the handle keeps exactly what it had on every error:
 *   -MLZ_ERR_ARG          NULL reader or blob, len 0, other flags, a blob that is not in the memory of the handle's device
 *   -MLZ_ERR_CORRUPT      no identifier or header chunk, a malformed fixed header (unknown flags, padding, k > size, N not k or k + 1, nsections or the
 *                         chunk length not the size's, longest against its flag, an unbound blob with a tag)
 *   -MLZ_ERR_UNSUPPORTED  an unknown magic
 *   -MLZ_ERR_ARG          a well-formed header of another size than the handle's
 *   -MLZ_ERR_CORRUPT      a directory entry outside what its tiles allow; a blob shorter or longer than the directory says
 *   -MLZ_ERR_CRC          the header chunk's CRC
 *   -MLZ_ERR_ARG          a bound blob whose tag or data chunks are not the handle's (an unbound blob is checked by its size only)
 *   -MLZ_ERR_CRC          a section's CRC
 *   -MLZ_ERR_CORRUPT      a section's chunk header or the EOF chunk; a section header against the directory; counts that descend or exceed 65 536 a tile; ranks
 *                         that do not continue from section to section or do not end at k; a payload outside its section; sparse entries not strictly
 *                         ascending or at or beyond the size, a non-zero pad; a dense tile's popcount off its count or a bit at or beyond the size; N against
 *                         the last byte.  No byte of the blob is read that the length has not bounded.
 *   The delimiter is what the header says; the longest record, when the header has it, is taken over unverified.
 * mlz_record_index_bound: host only, no context: bytes that always suffice for mlz_record_index_build_device over raw_len bytes; -MLZ_ERR_TOO_LARGE
 *   beyond 2^32 - 2^17 bytes, the most one build call takes.
 * mlz_record_index_build_device: an unbound blob from raw_len raw bytes at d_raw (device memory, one contiguous buffer, any alignment) -> its bytes; the
 *   index "while the Writer encodes": the process that hands d_raw to the device Writer runs this over the same buffer.  info as save's.  Errors as save's.
 * mlz_record_index_parse: HOST memory, no context and no device: the identifier, the header chunk (its CRC included) and the directory of blob[0, len)
 *   checked against len -> nsections.  info (8 values): flags, delimiter, size, k, N, longest, stream tag, data chunks.  The sections are not looked at.
 *
 * Out of scope: the blob as chunks inside the main stream or a search sidecar (the section chunks are self-contained so that this can follow), a gather
 * list for the build, entropy-coded payloads, delimiters of more than one byte, blobs in host memory other than for parse. */
#ifndef MINLZ_HIP_RECORD_INDEX_STORE_H
#define MINLZ_HIP_RECORD_INDEX_STORE_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t mlz_dev_reader_record_index_bound(const mlz_dev_reader* reader);
int64_t mlz_dev_reader_save_record_index(mlz_dev_reader* reader, void* stream, uint8_t* d_dst, size_t dst_cap, uint64_t* info);
int64_t mlz_dev_reader_load_record_index(mlz_dev_reader* reader, void* stream, uint32_t flags, const uint8_t* d_blob, size_t len, uint64_t* info);
int64_t mlz_record_index_bound(uint64_t raw_len);
int64_t mlz_record_index_build_device(mlz_ctx* ctx, void* stream, const uint8_t* d_raw, size_t raw_len, uint8_t delimiter, uint8_t* d_dst, size_t dst_cap, uint64_t* info);
int64_t mlz_record_index_parse(const uint8_t* blob, size_t len, uint64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_RECORD_INDEX_STORE_H */
