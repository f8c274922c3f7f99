/* minlz_hip_sidecar_extract.h — a stream's inline search tables moved into a sidecar, and the stream written again without them, in device memory: an
 * extension of the C ABI of minlz_hip.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++.
 *
 * The reference's ExtractSidecar (sidecar.go, SEARCH.md "Three ways to produce a sidecar") for one stream that a handle of mlz_stream_open_device holds.
 * mlz_dev_reader_build_sidecar decodes every block and builds fresh tables; this call decodes nothing: the search chunks the stream carries (0x44 info,
 * 0x45 tables, 0x46 compressed tables) are copied byte for byte, whoever wrote them and whatever they hold.
 *
 * The sidecar (d_side): the stream identifier with the main stream's block-size byte; then, in stream order, every 0x44 / 0x45 / 0x46 chunk of the source,
 *   header included, and for every data chunk (0x01, 0x02, 0x03) one remote block reference 0x47 with a single entry `uvarint(offset) uvarint(max block -
 *   decoded bytes)`; the EOF chunk `20 01 00 00 00` where the source's EOF chunk lies (search chunks behind it follow it, as in the reference).  Index
 *   chunks (0x40, legacy 0x99), padding, user chunks and 0x47 chunks of the source do not enter the sidecar.
 * Without d_main (mode a) a reference names the data chunk's header offset in the source, and the source stays the stream to search.
 * With d_main (mode b) d_main receives, in source order: the identifier; every data chunk, header and payload as they are; every other skippable chunk
 *   as it is (padding, user chunks, a 0x47), but not the search chunks and not the index chunks; in the place of the source's EOF chunk an EOF chunk with
 *   the decoded size and, behind it, a fresh seek index (Index.add(new chunk offset, decoded offset) per data chunk, appendTo(decoded size, -1)), written
 *   whether or not the source had one.  The references name the offsets in d_main.  The device Writer followed by this call gives the sidecar of the
 *   reference's WriterSidecar: both put the data chunks from offset 10 on.
 * d_main MUST NOT overlap the source or d_side; the call does not check it.
 * Chunks in front of the identifier (a Reader accepts skippable ones there) are treated like the others: the outputs begin with the identifier.
 *
 * mlz_dev_reader_extract_sidecar_bound: host only, from what the handle holds.  Returns a side_cap that always suffices: 10 + 5 + every byte of the source
 *   outside its data chunks (the search chunks are among them) + 24 per data chunk (a reference: 4 + two uvarints of at most 10 bytes).  *main_bound (may
 *   be NULL): a main_cap that always suffices: the source's length (identifier, data chunks and passed chunks are bytes of the source) + 14 (the EOF
 *   chunk) + 64 + 20 per index entry (at most 65537 entries, never more than data chunks).  Errors as the call's, below: -MLZ_ERR_ARG (NULL reader),
 *   -MLZ_ERR_UNSUPPORTED, -MLZ_ERR_CORRUPT.
 *
 * mlz_dev_reader_extract_sidecar: runs on `stream` (0: the default stream) and returns when the bytes are in place.  flags: 0 or MLZ_STREAM_IGNORE_CRC,
 *   which is accepted and without effect (nothing is decoded, no CRC is looked at; the copied tables are not validated either).  Returns side_len, or
 *   -MLZ_ERR_ARG          NULL reader, NULL d_side, NULL out, d_main with main_cap 0 (or main_cap without d_main), other flags, buffers not on the handle's device
 *   -MLZ_ERR_UNSUPPORTED  a handle over a set of streams; concatenated streams; a source with more than one EOF chunk
 *   -MLZ_ERR_CORRUPT      a stream without an identifier (the empty stream); a data chunk of no bytes (no reference can name it); bytes between the data
 *                         chunks that are no row of skippable chunks (they cannot lie behind a successful open)
 *   -MLZ_ERR_DST_TOO_SMALL  side_cap or main_cap is below the actual size; out->side_len and out->main_len then carry the sizes needed
 *   -MLZ_ERR_HIP
 *   No error writes a byte to d_side or d_main.  *out is zeroed by every call that gets past the argument checks. */
#ifndef MINLZ_HIP_SIDECAR_EXTRACT_H
#define MINLZ_HIP_SIDECAR_EXTRACT_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t side_len, main_len;      /* bytes written to d_side / d_main (main_len 0 without d_main) */
    uint64_t blocks;                  /* data chunks referenced (one 0x47 each) */
    uint64_t info_chunks, tables, tables_compressed;   /* 0x44, 0x45 + 0x46, of which 0x46, copied */
    uint64_t passed_bytes, dropped_bytes;  /* with d_main: other skippable chunks passed through to d_main; index chunks dropped (both 0 without d_main) */
} mlz_sidecar_extract_result;

int64_t mlz_dev_reader_extract_sidecar_bound(const mlz_dev_reader* reader, uint64_t* main_bound);
int64_t mlz_dev_reader_extract_sidecar(mlz_dev_reader* reader, void* stream, uint32_t flags, uint8_t* d_side, size_t side_cap, uint8_t* d_main, size_t main_cap,
                                       mlz_sidecar_extract_result* out);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_SIDECAR_EXTRACT_H */
