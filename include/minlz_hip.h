/*
 * minlz_hip.h — C ABI of the MI355X (gfx950) MinLZ block codec.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch
 * types, re-entrant, no exceptions.  Each entry point names the reference interface it
 * replaces (file:line into the upstream minio/minlz tree); INTEGRATION.md shows the cgo stub a
 * maintainer adds on the Go side.
 *
 * Two families:
 *   host-pointer calls   — buffers live in host memory for the duration of the call; the
 *                          library stages them through pinned buffers it owns (PCIe-bound).
 *   device-resident calls — src/dst already in HBM; work is queued on the caller's HIP stream
 *                          and nothing is synchronised (this is what bench.py times).
 *
 * Return codes: >= 0 success (or a byte count), < 0 = -MLZ_ERR_*.
 */
#ifndef MINLZ_HIP_H
#define MINLZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLZ_MAX_BLOCK_SIZE (8u << 20) /* minlz.go:84 MaxBlockSize */

/* compression levels, encode.go:25-43.  LevelSmallest (3) is not offered on the device: encode calls
 * return -MLZ_ERR_INVALID_LEVEL for it, which a WriterCustomEncoder treats as "decline". */
#define MLZ_LEVEL_SUPERFAST (-1)
#define MLZ_LEVEL_UNCOMPRESSED 0
#define MLZ_LEVEL_FASTEST 1
#define MLZ_LEVEL_BALANCED 2

/* error codes; 1..5 mirror the reference's sentinel errors (decode.go:29-40) */
#define MLZ_OK 0
#define MLZ_ERR_CORRUPT 1       /* ErrCorrupt */
#define MLZ_ERR_TOO_LARGE 2     /* ErrTooLarge */
#define MLZ_ERR_UNSUPPORTED 3   /* ErrUnsupported: Snappy/S2 fallback blocks (src[0] != 0) */
#define MLZ_ERR_INVALID_LEVEL 4 /* ErrInvalidLevel */
#define MLZ_ERR_CRC 5           /* ErrCRC */
#define MLZ_ERR_DST_TOO_SMALL 6 /* caller's dst cannot hold the result */
#define MLZ_ERR_HIP 7           /* HIP runtime failure: caller should fall back to its CPU path */
#define MLZ_ERR_ARG 8           /* bad argument */

typedef struct mlz_ctx mlz_ctx; /* one per (process, device) from mlz_init, or one over several devices from mlz_init_devices; thread-safe */

/* One block of a batch.  Offsets are relative to the base pointers passed with the batch. */
typedef struct {
    uint64_t src_off; /* start of this block's input  */
    uint64_t src_len; /* its length (encode: <= 8 MiB uncompressed; decode: compressed bytes) */
    uint64_t dst_off; /* start of this block's output */
    uint64_t dst_cap; /* room there (encode: >= mlz_max_encoded_len(src_len)) */
} mlz_block_desc;

/* ---- lifetime ---- */
/* Creates the context on HIP device `device` (-1 = current).  Replaces nothing in the
 * reference (its kernels need no state beyond sync.Pool tables, encode_amd64.go:119-189). */
int mlz_init(int device, mlz_ctx** out);
void mlz_destroy(mlz_ctx* ctx);
/* Several devices behind ONE context, in one process (the reference's Writer and Reader fan the blocks of a stream out to goroutines inside
 * one process: writer.go:501-560, in-order emit writer.go:219-272, reader.go:830-859 — a Go host is one process, so the fan-out over the GPUs
 * of a node sits behind this ABI, not above it).  devices[0 .. n_devices): HIP device ordinals, one per-device context each (an ordinal may be
 * repeated: two contexts on one GPU overlap one's copies with the other's kernels, and it is how the path is tested on a one-GPU box);
 * devices == NULL: every visible device (n_devices > 0: the first n_devices of them).
 * With such a context
 *   mlz_encode_batch / mlz_decode_batch   deal contiguous block ranges of about equal bytes to the devices, one host thread and one PCIe link per
 *                                          device; every result lands at the caller's dst[i] (page-locked destinations are written by the kernels of
 *                                          whichever device ran the block), so there is nothing to gather and no collective;
 *   mlz_stream_encode                      deals the stream's 64 MiB groups of blocks to the devices in turn (group g to device g mod n); a group's chunks go
 *                                          to their final place in dst as soon as the sizes of the groups before it are known (the in-order emit: they
 *                                          belong to the same pipeline step of the other devices), under the kernels of the device's next group;
 *                                          the stream is byte-identical to the one-device call's;
 *   mlz_stream_decode                      deals contiguous chunk ranges of about equal output (every chunk's output offset is known from the chunk walk);
 *   mlz_encode / mlz_decode / *_block / mlz_crc   go to the devices in turn, each with its own combining queue;
 *   the *_batch_device calls               run on the device that holds d_src (-MLZ_ERR_ARG if none of the context's devices does);
 *   mlz_stream_encode_gather_device        (below) is the device-resident form: sources in each device's HBM, the framed stream gathered GPU-to-GPU;
 *   mlz_set_option applies to every device, mlz_get_counter sums (which = 6: the maximum), mlz_get_timers reports the slowest device per family.
 * A context from mlz_init behaves as before everywhere (mlz_device_count = 1).  mlz_device_ctx(ctx, i) is the i-th per-device context — owned by
 * ctx, valid until mlz_destroy(ctx) — for callers that place device-resident work themselves. */
int mlz_init_devices(const int* devices, int n_devices, mlz_ctx** out);
int mlz_device_count(mlz_ctx* ctx);
mlz_ctx* mlz_device_ctx(mlz_ctx* ctx, int i);
const char* mlz_last_error(mlz_ctx* ctx); /* text of the last HIP failure on this context */
/* Library/ABI version and the name of the device the context runs on. */
int mlz_version(void);
int mlz_device_name(mlz_ctx* ctx, char* buf, size_t cap);

/* ---- sizes ---- */
/* MaxEncodedLen (encode.go:234-244): n+2, 1 for n == 0, -1 if n > 8 MiB. */
int64_t mlz_max_encoded_len(uint64_t n);
/* DecodedLen / isMinLZ (decode.go:107-156) on a host buffer: >= 0 decoded size, < 0 error. */
int64_t mlz_decoded_len(const uint8_t* src, size_t n);

/* ---- host-pointer block calls ---- */
/* minlz.Encode(dst, src, level) (encode.go:74-139): full block `00 uvarint(n) tokens`, or the
 * stored form `00 00 raw` when incompressible / n < 16.  Returns bytes written. */
int64_t mlz_encode(mlz_ctx* ctx, int level, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap);
/* minlz.Decode(dst, src) (decode.go:50-78).  Returns decoded bytes. */
int64_t mlz_decode(mlz_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap);
/* WriterCustomEncoder contract (writer.go:1293-1304) == encodeBlock(dst, src) (asm_none.go:51):
 * token stream only, no header.  > 0 bytes, 0 = incompressible, < 0 = error (decline). */
int64_t mlz_encode_block(mlz_ctx* ctx, int level, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap);
/* minLZDecode(dst[:n], src) (decode.go:178, decode_amd64.go:28-36): 0 ok, 1 corrupt, < 0 error. */
int mlz_decode_block(mlz_ctx* ctx, const uint8_t* src, size_t c, uint8_t* dst, size_t n);
/* Batched host-pointer forms used by the wrapper's Writer/Reader (writer.go:501-560,
 * reader.go:830-859 fan blocks to goroutines; here one launch covers the batch).
 * out_len[i] receives the bytes produced for block i or -MLZ_ERR_*.
 * Pinned destinations: when every dst[i] .. dst[i] + dst_cap[i] lies in page-locked host memory (hipHostMalloc /
 * hipHostRegister), the kernels store their results straight into it and there is no copy-out.  A block that FAILS
 * (out_len[i] < 0) may then have left partial output in its dst[i] — with pageable destinations a failed block's
 * buffer is not touched.  Nothing outside dst[i][0 .. dst_cap[i]) is ever written either way. */
int mlz_encode_batch(mlz_ctx* ctx, int level, int n_blocks, const uint8_t* const* src, const size_t* src_len,
                     uint8_t* const* dst, const size_t* dst_cap, int64_t* out_len);
int mlz_decode_batch(mlz_ctx* ctx, int n_blocks, const uint8_t* const* src, const size_t* src_len,
                     uint8_t* const* dst, const size_t* dst_cap, int64_t* out_len);

/* ---- device-resident batch calls (asynchronous on `stream`, a hipStream_t; NULL = default) ----
 * d_src / d_dst / d_out_len are device pointers.  d_out_len[i] (int64) receives what
 * mlz_encode / mlz_decode would have returned for block i.  `desc` is a host array (copied).
 * A context owns ONE workspace: calls issued on different streams are ordered on the device (each waits for the
 * previous call's last kernel through an event, recorded when a call arrives on a stream other than the last one's: a stream that was
 * used for a call must stay alive until the context's next call or mlz_destroy), so they are safe but do not overlap; use one context per stream
 * for concurrency.
 * Workspace: a batch runs in internal groups of about 512 MiB of uncompressed data (MLZ_OPT_DEVICE_GROUP; at least one block per group;
 * throughput is flat from 64 blocks of 8 MiB on), one after the other on `stream`, so the workspace is bounded by the group, not by the
 * batch.  It grows to the largest group seen and is kept (mlz_get_counter 3 / 4 report it).  Per group, decode holds about 7 bytes per
 * compressed byte (region exits, the token list — sized for one token per stream byte —, 16-bit token positions) and, for the
 * general-block pass (blocks of other encoders, LevelBalanced's own), 3 bytes per output byte + 8 bytes per stream byte: about 10 bytes
 * per output byte on text-like data, 5.3 GB for a full group.  Encode holds about 3.3 bytes per input byte (token records, piece
 * scratch) plus the far tables (1.5 MiB per 8 MiB block, LevelBalanced 8 MiB): about 3 GB per group.  If the general pass's buffers
 * cannot be allocated, general blocks decode on the exec pass's tile chain instead (slow, correct; mlz_get_counter 5 counts such calls). */
/* A stream that was used for a *_batch_device call and is about to be destroyed: call this first (any time after the last call on it).  The context
 * then records its ordering event on the stream while it is alive; without it the event is recorded lazily, by the context's NEXT call, on the previous
 * call's stream — which must therefore still exist then.  Not needed for streams that outlive the context's use, nor for the host-pointer calls. */
int mlz_release_stream(mlz_ctx* ctx, void* stream);
int mlz_encode_batch_device(mlz_ctx* ctx, void* stream, int level, const uint8_t* d_src, uint8_t* d_dst,
                            const mlz_block_desc* desc, int n_blocks, int64_t* d_out_len);
int mlz_decode_batch_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src, uint8_t* d_dst,
                            const mlz_block_desc* desc, int n_blocks, int64_t* d_out_len);

/* ---- masked CRC32C (stream chunks) ----
 * crc(b) of minlz.go:133-140: Castagnoli CRC, rotated by 15, plus 0xa282ead8; computed over the
 * uncompressed bytes of each block (writer.go:887, reader.go:341-351).
 * The CRC is a pass of its own over the block's bytes (0.059 ms per 100 MB, 4 % of an encode + decode step), not fused into the encoder's read
 * or the decoder's write as SURVEY.md 8(f1) words it: the match kernel is bound by instruction issue and the separate pass also serves the
 * Reader's check and chunk 0x03 (CRC over the token bytes) unchanged.
 * mlz_crc: host buffer, returns the 32-bit value (>= 0) or -MLZ_ERR_*.
 * mlz_crc_batch_device: blocks described by desc[i].src_off/src_len relative to d_base; d_out[i]
 * (uint32, device) receives the masked CRC of block i. */
int64_t mlz_crc(mlz_ctx* ctx, const uint8_t* src, size_t n);
int mlz_crc_batch_device(mlz_ctx* ctx, void* stream, const uint8_t* d_base, const mlz_block_desc* desc, int n_blocks,
                         uint32_t* d_out);

/* ---- whole-buffer streams (host pointers) ----
 * mlz_stream_encode: NewWriter(dst, WriterLevel(level), WriterBlockSize(block_size), WriterAddIndex(flag))
 *   .EncodeBuffer(src) followed by Close() (writer.go:441-563, :854-965, :1051-1126): stream header,
 *   one 0x02 / 0x01 chunk per block with the masked CRC32C of its uncompressed bytes, EOF chunk, and
 *   with MLZ_STREAM_ADD_INDEX the seek index (index.go:191-269).  Returns the stream size.
 * mlz_stream_decode: NewReader(src) read to EOF (reader.go:248-543), MinLZ streams only; CRCs are
 *   verified unless MLZ_STREAM_IGNORE_CRC (ReaderIgnoreCRC).  Returns the decoded size.
 * Copies to and from the device overlap the kernels group by group (~256 MiB). */
#define MLZ_STREAM_ADD_INDEX 1u
#define MLZ_STREAM_IGNORE_CRC 2u
/* Block search tables (SPEC_SEARCH.md; the reference's Writer with search tables and WithoutCompression(), table type 1): honoured by
 * mlz_stream_encode_gather_device and mlz_stream_bound only — mlz_stream_encode returns -MLZ_ERR_ARG when it is set.  See below; table types 2 and 3
 * (byte prefixes) are configured with an mlz_search_tables through mlz_stream_encode_gather_device_tables. */
#define MLZ_STREAM_SEARCH_TABLES 4u
#define MLZ_STREAM_SEARCH_MATCH_LEN(m) ((uint32_t)(m) << 8) /* bits 8..11; 0 = the reference's default 6; 1..8 valid; 9..15: -MLZ_ERR_ARG */
/* Compressed table chunks (0x46, SPEC_SEARCH.md 2.2) from the device-resident Writer: honoured by mlz_stream_encode_gather_device, _tables and
 * _long_prefix, where it needs tables (-MLZ_ERR_ARG without a configuration), and by mlz_dev_reader_build_sidecar; accepted and without effect in
 * mlz_stream_bound* (a 0x46 chunk is only written where it is smaller than the 0x45 chunk of the same table); without effect in mlz_stream_encode and
 * mlz_stream_encode_batch_device (its form with tables, mlz_stream_encode_batch_device_tables, refuses the flag).  See mlz_stream_encode_gather_device below and include/minlz_hip_search_compress.h. */
#define MLZ_STREAM_SEARCH_COMPRESS (1u << 6)   /* 64u */
int64_t mlz_stream_bound(uint64_t n, uint32_t block_size, uint32_t flags); /* dst_cap that always suffices */
int64_t mlz_stream_encode(mlz_ctx* ctx, int level, uint32_t block_size, uint32_t flags, const uint8_t* src, size_t n, uint8_t* dst,
                          size_t dst_cap);
int64_t mlz_stream_decoded_len(const uint8_t* src, size_t n); /* host-only chunk walk: total decoded bytes */
/* Host-only: the decoded bytes of the chunks in front of the stream's first framing error (the total when it has none).  The Reader
 * reports the first error in stream order: mlz_stream_decode into this much room decodes those chunks and returns their first error,
 * or the framing error when they all pass. */
int64_t mlz_stream_decoded_prefix_len(const uint8_t* src, size_t n);
int64_t mlz_stream_decode(mlz_ctx* ctx, uint32_t flags, const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap);

/* The device-resident Writer over several devices: range j of the stream lies in HBM at d_src[j] (src_len[j] bytes; every range but the last a whole
 * number of blocks), on any device of the context — normally range j on device j, the concurrent Writer's workers (writer.go:501-560) being the GPUs —
 * and the framed stream (header, the chunks in order, EOF, index with MLZ_STREAM_ADD_INDEX) is assembled in d_dst, a buffer on ONE device.  Every device
 * encodes and checksums its range and frames its run of chunks in its own HBM; 12 bytes per block (size, CRC) visit the host, so that every run's place
 * is known (the in-order emit, writer.go:219-272); the runs then travel GPU to GPU into d_dst (hipMemcpyPeerAsync: xGMI between the GPUs of a node; a run
 * already on d_dst's device is framed in place).  No payload crosses PCIe and there is no collective: a gather of variable-length runs to one consumer
 * is n - 1 point-to-point copies, which is also all RCCL's gather would issue.  Bytes are identical to mlz_stream_encode of the concatenated ranges.
 * Synchronous; returns the stream size.  Works on a one-device context too (n_ranges ranges encoded one after the other).
 * MLZ_STREAM_SEARCH_TABLES (| MLZ_STREAM_SEARCH_MATCH_LEN(M)): the stream also carries the reference's block search tables, type 1 (no prefix), as uncompressed
 * table chunks: `44 03 00 00 01 M B` directly behind the stream header (B = the bits of block_size - 1, within 8 .. 23) and `45 len24 | 01 M B | R | crc32le |
 * table` in front of the data chunk of every block that was stored compressed and whose table has at most 70 % of its 2^B bits set (stored blocks get none,
 * writer.go:528-540).  Bit HashValue(window of M bytes, B, M) is set for every position of the block; the last M - 1 positions take their missing bytes from
 * the next block (of the next range, too: 7 bytes of it visit the host), zeros beyond it; the stream's last block has no such positions.  The table is folded in
 * halves R times, while at most a quarter of the folded bits are set and 32 bytes remain.  Two kernels build and fold the tables over the raw blocks in HBM;
 * 12 more bytes per block visit the host (table bytes or 0, R, CRC).  The seek index names a block by the offset at which its chunks start: its table chunk
 * when it has one.  mlz_stream_bound with the flag adds 7 + (12 + max(32, 2^(B - 3))) per block.  Without the flag every byte is what it was before the
 * flag existed.  Table type 4 (the long prefix) is written by mlz_stream_encode_gather_device_long_prefix below.  Tables for a stream that exists
 * already — any writer's — go into a sidecar: mlz_dev_reader_build_sidecar below.
 * MLZ_STREAM_SEARCH_COMPRESS (with any of the three table configurations): every table is also compressed on the device, by the rule of
 * include/minlz_hip_search_compress.h (the reference's default writer without its shared tables and its skips), and its chunk is written as
 * `46 len24 | the same fixed fields | h0_bs h0_tc | table descriptions | sub-blocks` where that is strictly smaller than the 0x45 chunk, that is where the
 * section is shorter than the table; else the 0x45 chunk is written as without the flag.  A stream whose tables do not compress (tables of 512 bytes and
 * below never did) is byte for byte the stream without the flag, and mlz_stream_bound* holds unchanged.  Payload stays on the device: 8 more bytes per
 * table (the section's length) visit the host, in the read-back of the tables' CRCs.  mlz_get_counter(ctx, 15): the chunks the last call wrote as 0x46.
 * Out of scope: tables shared between sub-blocks and the reference's popcount-band and minimum-size skips, and a Writer that emits a sidecar while it
 * encodes (the reference's WriterSidecar). */
int64_t mlz_stream_encode_gather_device(mlz_ctx* ctx, int level, uint32_t block_size, uint32_t flags, const uint8_t* const* d_src, const size_t* src_len,
                                        int n_ranges, uint8_t* d_dst, size_t dst_cap);

/* Search tables with byte prefixes (SPEC_SEARCH.md 3.3; the reference's WithBytePrefix / WithMaskPrefix): table type 2 (1 to 8 prefix byte values) and
 * type 3 (a 256-bit mask of them: value v is a prefix byte when prefix[v >> 3] >> (v & 7) & 1; an empty mask is valid).  A flags word cannot carry a byte
 * set, hence the struct.  The info chunk is `44 len24 | T M B | field` and a table chunk `45 len24 | T M B | field | R | crc32le | table`, the field being
 * 8 bytes for type 2 (the values in the order given, unused places repeat the last one) and the 32 mask bytes for type 3.  A block's table holds bit
 * HashValue(window at q, B, M) for the positions q whose preceding byte block[q - 1] is a prefix byte: 1 <= q <= n in a block of n bytes that is not the
 * stream's last (position n is the window that lies wholly in the next block's first M bytes, zeros beyond a shorter one; across ranges 8 bytes of the next
 * range visit the host), 1 <= q <= n - M in the last; position 0 belongs to the block before.  A fold is accepted while at most a tenth of the folded bits
 * are set (type 1: a quarter); a block without any indexed position gets the all-zero table of 32 bytes (R = B - 8), which lets a searcher skip it.  The
 * 70 % rule, the 32-byte minimum, stored blocks (no table), the table's place in front of its block and the seek index are as for type 1.
 * mlz_stream_encode_gather_device_tables: cfg == NULL is mlz_stream_encode_gather_device.  With a cfg, flags must not carry MLZ_STREAM_SEARCH_TABLES or
 *   match-length bits; table_type 1 gives the bytes the flag gives for the same match length.  -MLZ_ERR_ARG: those flags, a type outside 1 .. 3,
 *   match_len > 8, type 2 with n_prefix outside 1 .. 8, reserved != 0.
 * mlz_stream_bound_tables: the dst_cap that always suffices for that call: mlz_stream_bound without tables + 7 + f + (12 + f + max(32, 2^(B - 3))) per
 *   block, f = 0, 8 or 32 bytes of prefix field.  cfg == NULL is mlz_stream_bound. */
typedef struct {
    uint8_t table_type; /* 1, 2 or 3 */
    uint8_t match_len;  /* 0 = 6; 1 .. 8 */
    uint8_t n_prefix;   /* type 2: 1 .. 8 values in prefix[0 .. n_prefix); ignored otherwise */
    uint8_t reserved;   /* 0 */
    uint8_t prefix[32]; /* type 2: the values; type 3: the mask */
} mlz_search_tables;
int64_t mlz_stream_bound_tables(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_tables* cfg);
int64_t mlz_stream_encode_gather_device_tables(mlz_ctx* ctx, int level, uint32_t block_size, uint32_t flags, const mlz_search_tables* cfg,
                                               const uint8_t* const* d_src, const size_t* src_len, int n_ranges, uint8_t* d_dst, size_t dst_cap);

/* Search tables with a long prefix and extra matches (SPEC_SEARCH.md 3.3.4, A.4, B.1; the reference's WithLongPrefix / WithExtras): table type 4.  The
 * prefix field of the info chunk and of every table chunk is `K-1 | E | pfx` (2 + K bytes).  A block of n bytes indexes every start p of the K-byte prefix
 * — 0 <= p <= n - 1 when a block follows, 0 <= p <= n - K - M - E in the stream's last block — with the E + 1 bits HashValue(window at p + K + j, B, M),
 * j = 0 .. E.  Prefix and windows run into the K - 1 + M + E bytes that follow the block in the stream (across ranges these bytes visit the host); the
 * windows run into zeros beyond the stream's end, a prefix does not.  An occurrence belongs to the block in which its prefix starts.  The table rules are
 * those of types 2 and 3: dropped above 70 %, a fold accepted up to a tenth, 32 bytes at the least, the all-zero table (R = B - 8) for a block without an
 * indexed start, none for a stored block, in front of its block, the seek index points at the table chunk.
 * mlz_stream_encode_gather_device_long_prefix: -MLZ_ERR_ARG for a NULL cfg, prefix_len outside 1 .. 256, match_len > 8, match_len + extras > 16 (after the
 *   default), extras > 15, reserved bytes that are not 0, flags that carry MLZ_STREAM_SEARCH_TABLES or match-length bits; nothing is written then.  An
 *   empty stream has no header and no info chunk.  mlz_stream_encode_gather_device_tables keeps refusing table_type 4.
 * mlz_stream_bound_long_prefix: the dst_cap that always suffices: mlz_stream_bound without tables + (7 + 2 + K) + (12 + 2 + K + max(32, 2^(B - 3))) per
 *   block.  Needs no device.
 * mlz_dev_reader_search uses these tables with no new call: the pattern's groups are the prefix's occurrences P[i, i + K) == pfx with i + K + M + E <= L,
 *   a table is probed for whole groups, and a pattern without a group (the reference's prefix-only query included) decodes every chunk. */
typedef struct {
    uint8_t match_len;   /* 1 .. 8; 0 = 6 */
    uint8_t extras;      /* 0 .. 15, match_len + extras <= 16 */
    uint16_t prefix_len; /* 1 .. 256 */
    uint8_t reserved[4]; /* 0 */
    uint8_t prefix[256];
} mlz_search_long_prefix;
int64_t mlz_stream_bound_long_prefix(uint64_t n, uint32_t block_size, uint32_t flags, const mlz_search_long_prefix* cfg);
int64_t mlz_stream_encode_gather_device_long_prefix(mlz_ctx* ctx, int level, uint32_t block_size, uint32_t flags, const mlz_search_long_prefix* cfg,
                                                    const uint8_t* const* d_src, const size_t* src_len, int n_ranges, uint8_t* d_dst, size_t dst_cap);

/* The device-resident Reader: the stream lies in HBM at d_src (n bytes), on a device of the context; the call runs on that device (-MLZ_ERR_ARG if none
 * of the context's devices holds d_src, as for the *_batch_device calls; one HBM-resident stream is not fanned out over several devices).  `stream` is
 * a hipStream_t (NULL = default); both calls are synchronous, like mlz_stream_encode_gather_device.  n is at most 2^36.
 *
 * mlz_stream_decoded_len_device: the chunk walk alone.  Returns what mlz_stream_decoded_len returns for the same bytes; *prefix_len (may be NULL)
 *   receives what mlz_stream_decoded_prefix_len returns.
 * mlz_stream_decode_device: NewReader(src) read to EOF, into d_dst on the same device.  Returns what mlz_stream_decode returns for the same bytes,
 *   flags and dst_cap: the decoded size, or the first error in stream order (the chunks in front of a framing error are decoded and checked first).
 *   On success d_dst[0, result) holds the decoded bytes; nothing outside d_dst[0, dst_cap) is written in any case, d_src is only read, and no byte
 *   at d_src + n or beyond enters the verdict.
 *
 * The chunk starts are found on the device from the bytes alone (every chunk type advances the Reader by 4 + its length, so the step is defined for every
 * byte offset: exits of 4 KiB and 256 KiB regions for every offset, then the true entries top-down).  No payload crosses PCIe: 32 bytes per chunk visit
 * the host (offset, type and length, decoded length, CRC, the header checks' outcome; skippable chunks inside the stream: none), where the Reader's running
 * state is applied to them, and 12 bytes per chunk of results come back after the decode.  Workspace: 8 bytes per stream
 * byte + 12 bytes per 4 KiB of stream + 32 bytes per chunk, part of the decode workspace that mlz_get_counter(ctx, 4) reports, next to what the block
 * decode of the chunks takes (above). */
int64_t mlz_stream_decoded_len_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src, size_t n, uint64_t* prefix_len);
int64_t mlz_stream_decode_device(mlz_ctx* ctx, void* stream, uint32_t flags, const uint8_t* d_src, size_t n, uint8_t* d_dst, size_t dst_cap);

/* Batches of streams in HBM: many .mz streams of one buffer walked, decoded or encoded by ONE call (an object store keeps each object as its own stream:
 * the per-tensor streams of a checkpoint, the objects of a request batch).  `streams[i]` is an mlz_block_desc for one stream: offsets count from d_src and
 * d_dst as in the *_batch_device calls, both buffers lie on one device of the context, and out_len is a HOST array.  All three calls are synchronous
 * and take `stream` like mlz_stream_decode_device.  They return 0 when the call ran (n_streams == 0: at once, nothing is launched); every stream's own result is
 * in out_len[i], and one stream's error changes nothing for any other.  -MLZ_ERR_ARG, with nothing launched and nothing written: a NULL array with
 * n_streams > 0, n_streams < 0 or above 2^20, d_src or d_dst that no device of the context holds (or not the same one), a src_len above 2^36, a span that
 * leaves the allocation its base pointer lies in, two destinations with dst_cap > 0 that overlap (source spans may overlap or repeat), a batch whose chunk
 * table could pass 2^32 entries.  -MLZ_ERR_HIP: a HIP failure.
 *
 * mlz_stream_decoded_len_batch_device: the chunk walk alone.  out_len[i] / prefix_len[i] (may be NULL) = what mlz_stream_decoded_len_device returns / stores
 *   for (d_src + src_off, src_len); dst_off and dst_cap are ignored.
 * mlz_stream_decode_batch_device: NewReader(src_i) read to EOF, for every i.  out_len[i] = what mlz_stream_decode_device(ctx, stream, flags, d_src + src_off,
 *   src_len, d_dst + dst_off, dst_cap) returns for stream i alone: the decoded size, or the first error in that stream's order (the chunks in front of a
 *   framing error are decoded and checked first; a stream that decodes to more than dst_cap gives -MLZ_ERR_DST_TOO_SMALL and nothing of it is decoded).
 *   Nothing outside the streams' [dst_off, dst_off + dst_cap) is written, d_src is only read, and no byte at src_off + src_len or beyond enters stream
 *   i's verdict (the next stream of the batch lies there).  MLZ_STREAM_IGNORE_CRC as in the single call.
 * mlz_stream_encode_batch_device: NewWriter(dst_i, level, block size, index).EncodeBuffer(src_i) + Close(), for every i.  out_len[i] and
 *   d_dst[dst_off, +out_len[i]) are byte for byte what mlz_stream_encode_gather_device gives for the one range (d_src + src_off, src_len); dst_cap below
 *   mlz_stream_bound(src_len, block_size, flags) gives that stream -MLZ_ERR_DST_TOO_SMALL and writes nothing of it.  MLZ_STREAM_ADD_INDEX is honoured;
 *   MLZ_STREAM_SEARCH_TABLES or match-length bits fail the whole call with -MLZ_ERR_ARG (tables in batches: mlz_stream_encode_batch_device_tables, include/minlz_hip_encode_batch_tables.h), and the level and the
 *   block size are checked as in the single call.
 *
 * The walk: one lane per stream steps through its chunk headers from offset 0, first counting the table's entries, then — after a scan of the counts —
 * writing them; no region tables.  Workspace: 32 bytes per table entry + 8 bytes and a flag bit per stream, part of mlz_get_counter(ctx, 4) (the streams'
 * descriptors, 32 bytes each, lie with the other descriptors).  Two read-backs for the whole batch: the places with the sum, then the table; the Reader's
 * state is applied per stream on the host.  A lane stops after 4096 chunk headers: such a LONG stream (many skippable chunks) is walked inside the same
 * call by the region kernels of mlz_stream_decoded_len_device, one after the other — the same answers, only slower; mlz_get_counter(ctx, 12) counts them.
 * Decode: the chunks of all streams run as one list through the decode and CRC kernels (groups of about 64 MiB), stored chunks by one copy kernel; 12 bytes
 * per chunk come back.  Encode: the blocks of all streams through one encode and one CRC launch sequence; 12 bytes per block visit the host, which lays
 * every stream out; bodies, identifiers, EOF chunks and indexes are placed by one kernel, chunk headers by another.
 * Search tables in batches are written by mlz_stream_encode_batch_device_tables (include/minlz_hip_encode_batch_tables.h) and read by mlz_stream_search_batch_device_pruned.
 * Out of scope: sidecars in batches, an asynchronous form, a batch fanned out over several devices. */
int mlz_stream_decoded_len_batch_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src, const mlz_block_desc* streams, int n_streams, int64_t* out_len,
                                        uint64_t* prefix_len);
int mlz_stream_decode_batch_device(mlz_ctx* ctx, void* stream, uint32_t flags, const uint8_t* d_src, uint8_t* d_dst, const mlz_block_desc* streams,
                                   int n_streams, int64_t* out_len);
int mlz_stream_encode_batch_device(mlz_ctx* ctx, void* stream, int level, uint32_t block_size, uint32_t flags, const uint8_t* d_src, uint8_t* d_dst,
                                   const mlz_block_desc* streams, int n_streams, int64_t* out_len);

/* The device-resident ReadSeeker: Reader.ReadSeeker / ReadSeeker.ReadAt (reader.go:1322-1487) for a stream that lies in HBM, with the chunk walk's table
 * in the place of the seek index (index.go:114 Index.Find): any byte ranges of the decoded stream, decoded on the device into device memory.
 *
 * mlz_stream_open_device: runs the chunk walk once and keeps its result on the host, in the handle (mlz_dev_reader_read plans against it there; the
 *   first mlz_dev_reader_read_device of a handle also uploads it, 24 bytes per data chunk, into device memory that the handle owns until it is closed): the data chunks with body offset and length, decoded
 *   length, CRC, type and output offset.  Returns the decoded size (what mlz_stream_decoded_len_device returns for the same bytes) and the handle in *out.
 *   A stream with a framing error gets no handle: that same negative value is returned and *out is NULL (a seeker over a stream whose end nobody can
 *   vouch for is not offered; mlz_stream_decode_device keeps its "prefix first" behaviour).  Arguments as for mlz_stream_decode_device (d_src on a device
 *   of the context, n at most 2^36); an empty stream opens with size 0.  The handle REFERS to d_src, which the caller keeps alive and unchanged until
 *   mlz_dev_reader_close, and to the context, which must outlive the handle.  Several handles may be open on one context; they share its workspace
 *   (calls are serialised by the context's lock), not their tables.
 * mlz_dev_reader_size: the decoded size again.
 * mlz_dev_reader_read: for every i, decoded bytes [ranges[i].off, + len) to d_dst[ranges[i].dst_off, + len); returns the sum of the lengths.  d_dst is on
 *   the handle's device.  Source ranges may overlap, repeat, come in any order and be empty.  -MLZ_ERR_ARG: a range runs beyond the decoded size, two
 *   destinations overlap, d_dst is not on the handle's device; -MLZ_ERR_DST_TOO_SMALL: dst_off + len > dst_cap.  These are decided before anything is
 *   launched, and nothing is written.
 *   Exactly the chunks that hold at least one requested byte are decoded, each of them ONCE per call however many ranges touch it and always whole (the
 *   block is the granularity of random access, as in the reference), and each one's CRC is checked over the whole chunk unless flags has
 *   MLZ_STREAM_IGNORE_CRC (types 0x01 and 0x02 over the decoded bytes, 0x03 over the token bytes).  The result is the error of the first failing touched
 *   chunk in stream order (-MLZ_ERR_CORRUPT, -MLZ_ERR_CRC, -MLZ_ERR_HIP); a broken chunk that no range touches is not noticed: that is what seeking
 *   means.  After an error the contents of the ranges' destinations are unspecified.  In every case nothing outside the union of the ranges'
 *   destinations is written (gaps between them included), d_src is only read, and no byte at d_src + n or beyond enters any result.
 *   A compressed chunk that exactly one range touches and covers wholly is decoded straight into its place in d_dst; any other touched compressed chunk is
 *   decoded into a scratch buffer of the context and its wanted parts are copied out; stored chunks are copied from the stream where it lies.  The work
 *   runs in groups of about 64 MiB of chunk output, so the scratch is at most a group plus one block whatever the ranges; it is part of the decode
 *   workspace (mlz_get_counter 4).  Synchronous; `stream` as for mlz_stream_decode_device.
 * mlz_dev_reader_read_device: the same read with the ranges in DEVICE memory, planned by kernels: d_off[i], d_len[i] (i < n_ranges) are the offsets and
 *   lengths, on the handle's device like d_dst and d_starts.  The output is PACKED: range i goes to d_dst[s_i, s_i + d_len[i]) with s_i = the sum of the
 *   lengths in front of it, in the order given; when d_starts is not NULL it receives the n_ranges + 1 values s_0 ... s_n (s_n = the total).  Returns the
 *   total.  (Explicit destination offsets stay with mlz_dev_reader_read: that they do not overlap takes a sort to check.)
 *   -MLZ_ERR_ARG: a pointer that is not device memory of the handle's device (decided with hipPointerGetAttributes before anything is launched);
 *   n_ranges > 2^31; a range that runs beyond the decoded size (off > size or len > size - off: an int64 -1 is such a value); more than 2^31 - 1
 *   workgroups in one copy launch (total / 64 KiB + n_ranges / 16).  -MLZ_ERR_DST_TOO_SMALL: the total exceeds dst_cap.  The last three are found by the
 *   kernels and reported after the call's first read-back, before any decode or copy is enqueued: nothing is written to d_dst or d_starts.
 *   Everything else is mlz_dev_reader_read's contract: exactly the touched chunks are decoded, each once and whole, with its CRC; the same three classes
 *   (straight into its place / through the scratch / stored, copied from the stream) chosen by the same rule; the first failing touched chunk's error in
 *   stream order; nothing outside d_dst[0, total) is written; d_src, d_off and d_len are only read; empty, overlapping, repeated and unordered source
 *   ranges are allowed; groups of about 64 MiB, the scratch at most a group plus one block; synchronous.  n_ranges == 0 returns 0 and launches nothing.
 *   What visits the host is proportional to the touched chunks, never to the ranges: a 32-byte header (error word, total, copy pieces, touched chunks),
 *   then 16 bytes per touched chunk down (chunk, class, place) and 16 up (group, class, scratch offset) — mlz_get_counter(ctx, 9) —, and the decode's
 *   12 bytes of results per chunk.  Workspace: 16 bytes per range + 28 per data chunk of the stream, part of mlz_get_counter(ctx, 4).
 * mlz_dev_reader_close: frees the handle (NULL: nothing). */
typedef struct mlz_dev_reader mlz_dev_reader;
typedef struct {
    uint64_t off;     /* first decoded byte wanted */
    uint64_t len;     /* how many */
    uint64_t dst_off; /* where in d_dst they go */
} mlz_range;
int64_t mlz_stream_open_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src, size_t n, mlz_dev_reader** out);
int64_t mlz_dev_reader_size(const mlz_dev_reader* reader);
int64_t mlz_dev_reader_read(mlz_dev_reader* reader, void* stream, uint32_t flags, const mlz_range* ranges, size_t n_ranges, uint8_t* d_dst, size_t dst_cap);
int64_t mlz_dev_reader_read_device(mlz_dev_reader* reader, void* stream, uint32_t flags, const uint64_t* d_off, const uint64_t* d_len, size_t n_ranges,
                                   uint8_t* d_dst, size_t dst_cap, uint64_t* d_starts /* may be NULL */);
void mlz_dev_reader_close(mlz_dev_reader* reader);

/* Pattern search over a stream that lies in HBM, with the reference's block search tables (SPEC_SEARCH.md; search_table.go, search_index.go) where
 * the stream has them: table types 1 (no prefix), 2 (1 to 8 prefix byte values), 3 (a mask of prefix byte values) and 4 (a long prefix with extra
 * matches) in uncompressed table chunks (0x45) and in compressed ones (0x46: expanded once per handle, by its first search, into device memory the handle
 * owns; minlz_hip_search_compressed.h, mlz_get_counter 14) behind an info chunk (0x44); the first fitting table in front of a block is taken, whichever of
 * the two it is, and a 0x46 table that does not parse, decode or pass its CRC is passed over like a broken 0x45 one.  The tables may also come from a sidecar, a second stream that names the blocks of this one with remote references (0x47):
 * mlz_dev_reader_build_sidecar and mlz_dev_reader_attach_sidecar below; remote references inside the searched stream itself are stepped over.
 *
 * mlz_dev_reader_search: returns the number of positions p of the decoded stream with decoded[p, p + pattern_len) == pattern (overlapping occurrences
 *   count; the value may exceed cap); d_offsets (on the handle's device; may be NULL when cap == 0) receives the min(total, cap) smallest positions in
 *   ascending order and nothing beyond them is written.  `pattern` is host memory, pattern_len 1 .. 256.  -MLZ_ERR_ARG: pattern_len 0 or above 256, a
 *   NULL pattern, d_offsets NULL with cap > 0 or not on the handle's device.  Synchronous; `stream` as for mlz_dev_reader_read.
 *   Tables: (T, M, B, prefix field) is that of the stream's info chunk, the first 0x44 between the identifier and the first data chunk, when its type
 *   is 1 .. 4 and its payload holds the field (type 4: with E <= 15 and M + E <= 16).  A data chunk's table is the first 0x45 chunk between the previous data chunk's end and its own start
 *   whose T, M, B and prefix field are byte-equal to the stream's, with R <= B - 8, a payload of 8 + field + 2^(B - R - 3) bytes and a good CRC (not checked
 *   under MLZ_STREAM_IGNORE_CRC).  Anything else — no info chunk, pattern_len < M, a broken CRC — means the chunk has no usable table.  The tables are located by a kernel (one lane per data chunk) and their CRCs checked once per handle.
 *   Plan: the pattern's pattern_len - M + 1 windows are looked up in every table; a chunk is a candidate when all are present in its own table, or
 *   when its table holds the first j and the next chunk's the others for some 1 <= j (SPEC_SEARCH B.4.1; a next chunk without a usable table or of
 *   fewer than pattern_len bytes holds everything).  Exactly the candidates and the chunks that hold any of the pattern_len - 1 bytes behind a
 *   candidate's end are decoded (stored chunks: copied), each once, with their CRCs as in mlz_dev_reader_read; chunks without a usable table are always
 *   candidates.  Errors as for mlz_dev_reader_read: the first failing decoded chunk in stream order; a broken chunk the plan skips goes unnoticed.
 *   Prefix tables (types 2 and 3): the windows looked up are those that start at 1 <= i <= pattern_len - M behind a prefix byte pattern[i - 1] — the only
 *   ones a block indexes, each in the block that holds the byte in front of it.  Without any such window the tables cannot serve the pattern: every data
 *   chunk is decoded and the third statistic is 0.  The split rule is the same over these windows, with j >= 0 when pattern[0] is no prefix byte.
 *   MLZ_SEARCH_NO_TABLES: every data chunk is decoded and scanned (cross-checks, the timing baseline).
 *   MLZ_SEARCH_IGNORE_CASE (grep -i in the C locale; also taken by the three calls below, with every flag they take): with fold(b) = b | 0x20 for
 *   0x41 <= b <= 0x5A and b otherwise — ASCII only: 0x40, 0x5B, 0x60, 0x7B and every byte >= 0x80 stay — the call returns what the call without the
 *   flag returns for fold(decoded stream) and fold(pattern): positions, counts, pairs and their order, record numbers, kinds and totals.  Two
 *   exceptions: the record bytes mlz_dev_reader_search_records packs are the stream's original bytes, and records are split at the delimiter's own
 *   byte, which is never folded (so that call and mlz_dev_reader_grep_records return -MLZ_ERR_ARG for the flag with a delimiter that is an ASCII
 *   letter, before anything is launched).  Patterns that become equal under folding count each for itself.  The pattern is folded once on the host,
 *   the scan folds every data byte in a register, the stream and the scratch are never rewritten.  Plan under the flag: a table bit stands for a
 *   window's exact bytes, so a window counts as present when the bit of ANY of its case variants is set; a window with more than 3 letters abstains
 *   (present everywhere, no look-up); a pattern whose windows all abstain is not served (every chunk is decoded, as for pattern_len < M).  Types 2
 *   and 3 use a window only when every case variant of the byte in front of it is a prefix byte; a type 4 prefix that holds a letter cannot serve a
 *   folded pattern.  At most 2^22 variant hashes are made per call; a pattern beyond that is not served.  A pattern without ASCII letters gives
 *   exactly the plan, stats and result of the call without the flag.
 *   stats (host, may be NULL) receives: data chunks of the stream, chunks decoded or copied, chunks with a usable table, 0.  mlz_get_counter 10 / 11
 *   report the second and third for the context's last search.
 *   Workspace: the decoded chunks go through the ReadSeeker's scratch in groups of about 64 MiB; one bit per decoded byte of the set marks the
 *   occurrences between the count pass and the write pass (part of mlz_get_counter 4). */
#define MLZ_SEARCH_NO_TABLES 8u
#define MLZ_SEARCH_IGNORE_CASE (1u << 5)   /* 32u */
int64_t mlz_dev_reader_search(mlz_dev_reader* reader, void* stream, uint32_t flags, const uint8_t* pattern, size_t pattern_len, uint64_t* d_offsets, size_t cap,
                              uint64_t* stats /* host, may be NULL: 4 values */);

/* mlz_dev_reader_search_many: up to MLZ_SEARCH_MAX_PATTERNS patterns in one call; the chunks that any pattern's tables admit are decoded once
 *   and scanned once for all of them.  `patterns` (host) holds the patterns' bytes back to back, pattern_len (host) their n_patterns lengths, each 1 .. 256.
 *   Returns the number of pairs (p, i) with decoded[p, p + pattern_len[i]) == pattern i (overlapping occurrences count; duplicate patterns count each for
 *   itself; the value may exceed cap).  d_counts (device, n_patterns values; may be NULL) receives every pattern's own number of occurrences, complete
 *   whatever cap is.  d_offsets[k] and d_which[k] (device; both may be NULL when cap == 0) receive the min(total, cap) smallest pairs in ascending order
 *   of (position, pattern index): two patterns that match at one position give two pairs, and the cut at cap may fall between them.  Nothing beyond
 *   these is written, and nothing outside the three arrays.  After an error return the arrays' contents are unspecified (never beyond their sizes).
 *   Equivalence: for a stream whose tables are truthful — every stream this library or the reference writes — the result is that of n_patterns calls
 *   of mlz_dev_reader_search on the same handle with the same flags: d_counts[i] is call i's return value and the pairs are the merge of the n_patterns
 *   position lists.  A table with a good CRC that lies (a cleared bit) may make the two differ: this call scans every chunk it decodes for every
 *   pattern, so it also reports occurrences of pattern i in chunks that only another pattern's tables admitted.
 *   Flags: MLZ_STREAM_IGNORE_CRC, MLZ_SEARCH_NO_TABLES and MLZ_SEARCH_IGNORE_CASE as for mlz_dev_reader_search (under the last one the index key is taken
 *   over folded bytes; patterns the letter cap or the hash budget leaves unserved count in stats[3]).
 *   -MLZ_ERR_ARG, each decided before anything is launched, nothing written: n_patterns > MLZ_SEARCH_MAX_PATTERNS; a length of 0 or above 256; NULL
 *   patterns or pattern_len with n_patterns > 0; d_offsets or d_which NULL with cap > 0; a device pointer that is not on the handle's device.
 *   n_patterns == 0 returns 0 and launches nothing.  Decode and CRC errors as for mlz_dev_reader_search: the first failing decoded chunk in stream order.
 *   Plan: per pattern the rule of mlz_dev_reader_search, unchanged; a chunk is decoded when any pattern's set holds it.  The host computes the
 *   patterns' windows and hashes; a kernel over (data chunk, pattern) probes the tables and marks one byte per data chunk, and only those bytes come
 *   back.  A pattern the tables cannot serve (shorter than M; no window behind a prefix under table types 2 to 4) puts every non-empty chunk into the set.
 *   stats (host, may be NULL): data chunks of the stream; chunks decoded or copied; chunks with a usable table, or 0 when no pattern could use the
 *   tables; patterns the tables could not serve (all of them under MLZ_SEARCH_NO_TABLES or without usable tables).  mlz_get_counter 10 / 11 report
 *   the second and third for this call too. */
#define MLZ_SEARCH_MAX_PATTERNS 4096
int64_t mlz_dev_reader_search_many(mlz_dev_reader* reader, void* stream, uint32_t flags,
                                   const uint8_t* patterns,          /* host: the patterns' bytes back to back */
                                   const uint32_t* pattern_len,      /* host: n_patterns lengths, each 1 .. 256 */
                                   size_t n_patterns,
                                   uint64_t* d_counts,               /* device, n_patterns values; may be NULL */
                                   uint64_t* d_offsets, uint32_t* d_which, size_t cap,   /* device; both may be NULL when cap == 0 */
                                   uint64_t* stats /* host, may be NULL: 4 values */);

/* The search over a BATCH of streams in HBM — which of these objects hold any of these keys, and where — is declared in a header of its own,
 * include/minlz_hip_search_batch.h, which includes this one.  A batch of streams opened as ONE handle (mlz_stream_open_batch_device), on which every
 * mlz_dev_reader_* call below and above works as on the streams' concatenation, and the calls that turn its positions and record numbers back into
 * (stream, position or record inside the stream), are declared in include/minlz_hip_stream_set.h; the open of such a handle whose searches prune by
 * every stream's inline search tables in include/minlz_hip_stream_set_tables.h. */

/* mlz_dev_reader_search_records: the RECORDS of the decoded stream that hold the pattern, each once, in stream order, packed into d_dst — what
 *   `mz search pattern file.mz` prints, and with rec_cap == 0 and dst_cap == 0 what `-c` counts.  A record is a maximal run of decoded bytes that
 *   holds no `delimiter`; the delimiter itself belongs to no record.  The call looks at most W = max_reach bytes to either side of an occurrence
 *   (0 = 65536; above MLZ_RECORDS_MAX_REACH: -MLZ_ERR_ARG).  With size = the decoded size and L = pattern_len, an occurrence at p (what
 *   mlz_dev_reader_search reports) has the window lo = max(0, p - W), hi = min(size, p + L + W), and
 *     s(p) = the position behind the last delimiter in [lo, p), or lo when there is none (then, when lo > 0, the record is CUT LEFT);
 *     e(p) = the position of the first delimiter in [p + L, hi), or hi when there is none (then, when hi < size, the record is CUT RIGHT).
 *   Occurrences are taken in ascending order; occurrence i opens a record when i == 0 or s(p_i) != s(p_i-1), else it belongs to the record of the
 *   occurrence before it.  A record is [s, e) with s of the occurrence that opens it and e of its last occurrence (e ascends with p).  When no
 *   record is longer than W this is exactly "every line that contains the pattern, once, in stream order".  Records longer than W come out cut
 *   and flagged, and two cut records may overlap: that is the price of a bounded reach.
 *   Returns the number of records R (it may exceed rec_cap).  The first k records are written, whole: k is the largest value with k <= rec_cap
 *   and the first k records' bytes summing to at most dst_cap.  d_rec_off[0 .. k): each record's start in the decoded stream; d_rec_start[0 .. k]
 *   (may be NULL): each record's start in d_dst, d_rec_start[k] = the bytes written; d_rec_flags[0 .. k) (may be NULL): bit 0 = cut left, bit 1 =
 *   cut right; d_dst[0, d_rec_start[k]): the records' bytes.  Nothing beyond these is written and no record is written in part.  All four are
 *   device memory of the handle's device; d_dst may be NULL when dst_cap == 0, d_rec_off when rec_cap == 0.
 *   totals (host, may be NULL): R, the bytes of all R records, the occurrences, the records with a flag.
 *   `pattern` is host memory, pattern_len 1 .. 256.  -MLZ_ERR_ARG, each decided before anything is launched, nothing written: the argument
 *   errors of mlz_dev_reader_search; a pattern that contains the delimiter (a line search cannot match across lines); max_reach above the
 *   maximum; d_dst NULL with dst_cap > 0 or d_rec_off NULL with rec_cap > 0; one of d_dst (dst_cap > 0), d_rec_off (rec_cap > 0), d_rec_start
 *   (not NULL) and d_rec_flags (not NULL, rec_cap > 0) that is not on the handle's device.  Found later: more than 2^31 occurrences (-MLZ_ERR_ARG).
 *   Two phases under one lock.  The search phase is mlz_dev_reader_search's plan, decode and scan with the same pattern and flags
 *   (MLZ_STREAM_IGNORE_CRC, MLZ_SEARCH_NO_TABLES, MLZ_SEARCH_IGNORE_CASE — with the last one a delimiter that is an ASCII letter is -MLZ_ERR_ARG, and the
 *   packed record bytes are the stream's original ones; an attached sidecar is used): stats and mlz_get_counter 10 / 11 describe it exactly as there.
 *   Zero occurrences returns 0 behind it and launches nothing more.  The read phase is mlz_dev_reader_read_device over the occurrences' windows,
 *   merged where they touch or overlap: every chunk a window touches is decoded once, with its CRC — also a chunk that the tables pruned in the
 *   search phase and a record reaches into; mlz_get_counter 7 / 8 / 9 describe it.  Kernels then find the bounds (a wavefront per occurrence),
 *   number the records, cut at the caps and copy; a 16-byte and a 48-byte header visit the host, nothing per occurrence or per record does.
 *   Decode and CRC errors: the first failing decoded chunk of the search phase, else of the read phase; the arrays' contents are then
 *   unspecified, but never beyond their sizes.  Synchronous; `stream` as for mlz_dev_reader_read.
 *   Workspace, grow-only and part of mlz_get_counter 4: about 100 bytes per occurrence, and a window buffer of the merged windows' bytes —
 *   at most min(decoded size, occurrences * (2 W + L)). */
#define MLZ_RECORDS_MAX_REACH (1u << 20)
int64_t mlz_dev_reader_search_records(mlz_dev_reader* reader, void* stream, uint32_t flags,
                                      const uint8_t* pattern, size_t pattern_len,   /* host, 1 .. 256 */
                                      uint8_t delimiter, uint32_t max_reach,        /* 0 = 65536; 1 .. MLZ_RECORDS_MAX_REACH */
                                      uint8_t* d_dst, size_t dst_cap,               /* device: the records' bytes, packed */
                                      uint64_t* d_rec_off,                          /* device, rec_cap values: where each record starts in the decoded stream */
                                      uint64_t* d_rec_start,                        /* device, rec_cap + 1 values: where each record starts in d_dst; may be NULL */
                                      uint8_t* d_rec_flags,                         /* device, rec_cap values; may be NULL */
                                      size_t rec_cap,
                                      uint64_t* totals /* host, may be NULL: 4 values */, uint64_t* stats /* host, may be NULL: as mlz_dev_reader_search */);

/* The record index: read records of a stream in HBM by NUMBER, and number positions by record (`mz search -n`, `sed -n 'a,bp'`).  With size = the
 * decoded size and D[0] < D[1] < ... < D[k-1] the positions of all decoded bytes equal to `delimiter`, the stream has N records: N = k + 1 when
 * size > 0 and the last byte is no delimiter (k == 0 included), else N = k.  Record r (0-based) is [start(r), end(r)): start(0) = 0,
 * start(r) = D[r-1] + 1; end(r) = D[r] for r < k, end(k) = size.  Empty records (doubled delimiters) exist and are counted; the delimiter
 * belongs to no record: data.split(delimiter) with one trailing empty piece dropped, what `grep -n` counts.  A record that
 * mlz_dev_reader_search_records returns without a left cut starts at some start(r).  The record number of a position p < size is the count of
 * D[j] < p: a delimiter's own position has the number of the record it ends.  All calls are synchronous and run under the context's lock;
 * `stream` and MLZ_STREAM_IGNORE_CRC as for mlz_dev_reader_read.
 *
 * mlz_dev_reader_index_records: builds the index for `delimiter` and returns N.  Every data chunk with bytes is decoded exactly once, in groups of
 *   about 64 MiB through the ReadSeeker's scratch (a group's chunks side by side; stored chunks are copied there), and its CRC checked unless the
 *   flag says otherwise.  Per group two passes over the decoded bytes (count per 64 KiB tile, then emit) and 8 bytes that visit the host.  info
 *   (host, may be NULL): N, k, the bytes of index the handle now holds, the chunks this call decoded.  The index is 8 bytes per delimiter (allocated
 *   exactly for a stream of one group, else grown geometrically: at most twice that) in device memory that the handle owns: freed by
 *   mlz_dev_reader_close, not part of the workspace that mlz_get_counter 4 reports, kept until the handle closes or another delimiter is indexed.  A
 *   second call with the same delimiter returns N and decodes nothing (info[3] == 0); a call with another delimiter replaces the index.  On a decode
 *   or CRC error the first failing chunk's error in stream order is returned, as by mlz_dev_reader_read, and the handle keeps whatever index it
 *   had; an allocation failure returns -MLZ_ERR_HIP.  An empty stream indexes to N = 0.
 * mlz_dev_reader_record_count: N, or -MLZ_ERR_ARG when the handle has no index.  Every call below returns -MLZ_ERR_ARG without an index too, before
 *   anything is launched.
 * mlz_dev_reader_record_spans: d_off[i] = start(d_idx[i]), d_len[i] = end - start for every i < n; all three arrays are device memory of the handle's
 *   device.  Returns the sum of the lengths (what a destination must hold).  Indices may repeat and come in any order.  An index >= N: -MLZ_ERR_ARG,
 *   found by the kernel; the two arrays are then unspecified, never beyond n entries.  Also -MLZ_ERR_ARG: n > 2^31, a pointer that is not on the
 *   handle's device.  n == 0 returns 0 and launches nothing.  16 bytes visit the host.
 * mlz_dev_reader_read_records: the records d_idx[0 .. n) packed into d_dst in the order given; d_starts (may be NULL) receives n + 1 values, where each
 *   record starts in d_dst and the total.  The spans go into context workspace (16 bytes per record, part of mlz_get_counter 4) and
 *   mlz_dev_reader_read_device's plan reads them: exactly the touched chunks are decoded, each once, with its CRC (mlz_get_counter 7 / 8 / 9), and
 *   everything else is that call's contract.  An index >= N returns -MLZ_ERR_ARG, a total above dst_cap -MLZ_ERR_DST_TOO_SMALL; both are decided
 *   before anything is written to d_dst or d_starts.  n == 0 returns 0 and writes nothing.  Returns the bytes written.
 * mlz_dev_reader_record_numbers: d_no[i] = the record number of position d_pos[i], or UINT64_MAX for d_pos[i] >= size; returns how many positions
 *   were < size.  A binary search in the index, a lane per position.  Fed with d_rec_off of mlz_dev_reader_search_records it gives the line
 *   numbers (0-based) of the matching lines.
 * mlz_dev_reader_record_range: host convenience for "records first .. first + count - 1 as ONE range": *off = start(first), *len = end(first + count
 *   - 1) - start(first), the inner delimiters included; count == 0 gives length 0 (at start(first), or at size for first == N).  first + count > N:
 *   -MLZ_ERR_ARG.  Two table entries visit the host; the caller reads the range with mlz_dev_reader_read.  Returns 0.
 * The index saved as a compact blob, loaded from one without a decode, and built from the raw bytes that go to the Writer: include/minlz_hip_record_index_store.h.
 * Out of scope: delimiters of more than one byte; the stored index as chunks inside the stream or inside a search sidecar.  Record
 *   numbers of the matching records come from mlz_dev_reader_grep_records below (mlz_dev_reader_search_records' signature stays). */
int64_t mlz_dev_reader_index_records(mlz_dev_reader* reader, void* stream, uint32_t flags, uint8_t delimiter,
                                     uint64_t* info /* host, may be NULL: 4 values */);
int64_t mlz_dev_reader_record_count(const mlz_dev_reader* reader);
int64_t mlz_dev_reader_record_spans(mlz_dev_reader* reader, void* stream, const uint64_t* d_idx, size_t n, uint64_t* d_off, uint64_t* d_len);
int64_t mlz_dev_reader_read_records(mlz_dev_reader* reader, void* stream, uint32_t flags, const uint64_t* d_idx, size_t n, uint8_t* d_dst, size_t dst_cap,
                                    uint64_t* d_starts /* may be NULL */);
int64_t mlz_dev_reader_record_numbers(mlz_dev_reader* reader, void* stream, const uint64_t* d_pos, size_t n, uint64_t* d_no);
int64_t mlz_dev_reader_record_range(mlz_dev_reader* reader, uint64_t first, uint64_t count, uint64_t* off, uint64_t* len);

/* mlz_dev_reader_grep_records: grep over the record index — many patterns, inverted match, context records and record numbers in one call: what
 *   `mz search -f keys -n -v -A a -B b file.mz` selects, and with rec_cap == 0 what `-c` counts.  N, start, end and number(p) are those of the
 *   handle's record index above, and so is the delimiter.  `patterns`, pattern_len and n_patterns (host) as for mlz_dev_reader_search_many.
 *     M = the records r for which some pattern i occurs at a position p with number(p) == r (patterns hold no delimiter, so an occurrence lies
 *         inside one record);
 *     S = M, or {0 .. N-1} \ M with MLZ_GREP_INVERT (empty records exist, never match, and are therefore selected under invert);
 *     C = the records r < N with some s in S and s - before <= r <= s + after.  Any value of before / after is valid; values >= N behave like N.
 *   Returns R = |C| (it may exceed rec_cap).  d_rec_no[0 .. k), k = min(R, rec_cap), receives the k smallest members of C in ascending order;
 *   d_rec_kind[j] (may be NULL) is 1 when record d_rec_no[j] is in S and 0 when it is context only (grep's `:` against `-`).  Nothing beyond k entries of either
 *   array is written, and after any error return nothing has been written to either.  totals (host, may be NULL): R; |S|; the bytes of the k
 *   written records — exactly what mlz_dev_reader_read_records over d_rec_no[0 .. k) needs as dst_cap —; the bytes of all R records.  No record
 *   is cut, there is no reach and no position list: a match goes from the scan kernel into one bit per record.
 *   Equivalence: for truthful tables, M is the set of mlz_dev_reader_record_numbers of the positions that mlz_dev_reader_search_many reports
 *   with the same patterns and flags.
 *   Flags: MLZ_STREAM_IGNORE_CRC, MLZ_SEARCH_NO_TABLES, MLZ_GREP_INVERT, MLZ_SEARCH_IGNORE_CASE (-MLZ_ERR_ARG when the index was built on an ASCII letter).
 *   -MLZ_ERR_ARG, each decided before anything is launched, nothing written: a handle without an index; the argument errors of
 *   mlz_dev_reader_search_many (n_patterns, the lengths, NULL patterns); a pattern that contains the index's delimiter (as
 *   mlz_dev_reader_search_records decides it); d_rec_no NULL with rec_cap > 0; d_rec_no or d_rec_kind (not NULL), with rec_cap > 0, that is not
 *   on the handle's device; N >= 2^32.  n_patterns == 0 is valid: M is empty, no chunk is decoded, and under invert every record is selected.
 *   N == 0 returns 0.
 *   The search phase is mlz_dev_reader_search_many's plan and decode with the same patterns and flags (an attached sidecar is used): stats
 *   (host, may be NULL: 4 values) and mlz_get_counter 10 / 11 describe it exactly as there.  Decode and CRC errors as there: the first failing
 *   decoded chunk in stream order; a broken chunk that the tables prune goes unnoticed.  Each decoded group is scanned ONCE (no count pass, no
 *   write pass); two kernels then select (complement, context by a forward and a backward scan of the nearest selected record: independent of
 *   the sizes of before / after) and compact.  32 bytes visit the host, behind the search phase's own; nothing per record or per occurrence does.
 *   Synchronous; `stream` as for mlz_dev_reader_read.  Workspace, grow-only and part of mlz_get_counter 4: 16 bytes per 32 records (two
 *   bitmaps and two scan arrays) beside the search phase's.
 *   Regular expressions: mlz_dev_reader_grep_regex (include/minlz_hip_regex.h), the same call with M decided by a compiled expression;
 *   include/minlz_hip_regex_prune.h: that call decoding only the chunks the search tables admit for the expression's required literals.
 *   Out of scope: Unicode or locale folding; per-record lists of which pattern matched; delimiters of more than one byte; a grep over
 *   batches of streams other than on a set handle (include/minlz_hip_stream_set.h: the streams' concatenation); a call that works without a record
 *   index (mlz_dev_reader_search_records remains the bounded-reach form for that). */
#define MLZ_GREP_INVERT 16u
int64_t mlz_dev_reader_grep_records(mlz_dev_reader* reader, void* stream, uint32_t flags,
                                    const uint8_t* patterns, const uint32_t* pattern_len, size_t n_patterns,   /* host, as mlz_dev_reader_search_many */
                                    uint64_t before, uint64_t after,                                          /* context records: -B, -A */
                                    uint64_t* d_rec_no,                                                       /* device, rec_cap values; may be NULL when rec_cap == 0 */
                                    uint8_t* d_rec_kind,                                                      /* device, rec_cap values; may be NULL */
                                    size_t rec_cap,
                                    uint64_t* totals /* host, may be NULL: 4 values */, uint64_t* stats /* host, may be NULL: as mlz_dev_reader_search_many */);

/* Sidecar search indexes (SEARCH.md "Sidecar Streams", SPEC_SEARCH.md 1.1 and 2.3; the reference's BuildSidecar and SidecarSearcher): search tables
 * for a stream that exists already, in a separate valid MinLZ stream.  The main stream is never touched, so this serves ANY stream in HBM: the
 * reference Writer's (whose tables are compressed, 0x46), old ones, mlz_stream_encode's and the Python Writer's, stored blocks.  A sidecar carries up to
 * MLZ_SIDECAR_MAX_CONFIGS table configurations; a block is skipped when any one of them proves the pattern absent.  All three calls are synchronous;
 * `stream` and MLZ_STREAM_IGNORE_CRC as for mlz_dev_reader_read.
 *
 * mlz_dev_reader_build_sidecar: writes the sidecar of the handle's stream to d_dst (on the handle's device) and returns its size.  Its bytes: the main
 *   stream's 10-byte identifier; one info chunk `44 len24 | T M B | field` per configuration in the order given, B = the table bits of the identifier's
 *   block size; for every data chunk of the main stream that decodes to at least one byte, in order, one `45 len24 | T M B | field | R | crc32le | table`
 *   per configuration whose table is kept and then `47 len24 | uvarint(offset of the data chunk's 4-byte header in the main stream) | uvarint(block size
 *   - decoded bytes)`; the EOF chunk `20 01 00 00 00`.  A table is what the device Writer's rules give for that type (above: the 70 % rule, folds up to
 *   25 % for type 1 and 10 % for the others, 32 bytes at the least, the all-zero table for a block without an indexed position), with two differences, both
 *   the reference's (sidecar.go): stored chunks (0x01) get tables like any other, and a block's overlap is the first bytes of the NEXT DATA CHUNK only, cut
 *   at that chunk's length, zeros beyond it even when more chunks follow; the last data chunk has none.
 *   Every chunk is decoded (groups of about 64 MiB through the ReadSeeker's scratch, a group plus one block at the most; a group's table slots take
 *   64 MiB of workspace at the most) and its CRC checked unless the flag says otherwise; a decode or CRC error of the first failing chunk is returned as
 *   by mlz_dev_reader_read, and d_dst's contents are then unspecified.  12 bytes per (chunk, configuration) visit the host (table bytes, R, CRC), no payload.
 *   -MLZ_ERR_ARG: n_cfgs outside 1 .. 4, a configuration the Writer calls above would refuse (reserved bytes that are not 0 included), d_dst not on the
 *   handle's device.  -MLZ_ERR_DST_TOO_SMALL: the result exceeds dst_cap (with a dst_cap below mlz_dev_reader_sidecar_bound the sizes are found by a
 *   pass of their own first).  -MLZ_ERR_UNSUPPORTED: the main stream holds a second stream identifier (concatenated streams).  These are decided
 *   before anything is written; nothing outside d_dst[0, result) is written in any case.
 * mlz_dev_reader_sidecar_bound: host only; a dst_cap that always suffices for the handle and these configurations, or -MLZ_ERR_ARG.
 * mlz_dev_reader_attach_sidecar: from this call on, mlz_dev_reader_search and mlz_dev_reader_search_many on the handle use the sidecar's tables
 *   (d_side[0, n_side), on the handle's device; the handle REFERS to it, the caller keeps it alive) instead of the main stream's inline ones;
 *   d_side == NULL with n_side == 0 detaches.  The sidecar is walked on the device like any stream.  Its configurations are the first up to 4 valid
 *   info chunks in front of its first 0x45 or 0x47.  A 0x47 payload is a list of (offset, block size - decoded bytes) pairs, the first offset
 *   absolute, the others relative and not 0; every reference must name the header offset of a data chunk of the handle's stream and state its
 *   decoded bytes, and references ascend over the whole sidecar.  The first reference of a 0x47 owns the tables in front of it: per configuration the
 *   first 0x45 or 0x46 between the previous 0x47 and this one that fits it (type, M, B, field, R, length) with a good CRC (not checked under
 *   MLZ_STREAM_IGNORE_CRC); a broken one is passed over for the next that fits; 0x46 tables are expanded by the attach; a data chunk without a reference has
 *   no table.  Errors — nothing is attached, the handle keeps what it had: -MLZ_ERR_ARG for a pointer not on the handle's device; the walk's own
 *   error for a framing error or a missing EOF chunk; -MLZ_ERR_CORRUPT for a bad varint, an empty 0x47, a reference that names no data chunk, a size
 *   that disagrees, an order that does not ascend, a data chunk inside the sidecar; -MLZ_ERR_UNSUPPORTED for a second identifier.  A sidecar
 *   without a usable info chunk attaches, and the searches then decode everything.
 *   Plan with several configurations: a configuration votes on a chunk when it serves the pattern and has a usable table for the chunk, by the rule of
 *   mlz_dev_reader_search (probing the next chunk's table of the same configuration); a chunk is a candidate when no vote is "no".  A sidecar's table
 *   is built over the next chunk's bytes alone, so a configuration does not vote on a chunk that is followed by one with fewer bytes than its overlap
 *   (M - 1, M, or K - 1 + M + E for types 1, 2 and 3, 4): that chunk is decoded, and every position is returned as without a sidecar.  The third
 *   statistic counts the chunks with a usable table of at least one configuration that serves a pattern, the fourth the patterns no configuration serves.
 * flags may hold MLZ_STREAM_SEARCH_COMPRESS: every table chunk is then written compressed (0x46) where that is strictly smaller, as the device Writer does it; the size returned, and
 *   the one a capacity is checked against, are the real ones; mlz_get_counter(ctx, 15) counts the 0x46 chunks.  The reference's ExtractSidecar — the tables a stream carries inline copied into a sidecar, the stream written again without them — is
 *   mlz_dev_reader_extract_sidecar in include/minlz_hip_sidecar_extract.h.  Out of scope: a Writer that diverts tables while it encodes (the device Writer followed by that call gives
 *   WriterSidecar's sidecar), concatenated streams, sidecars read from host memory. */
#define MLZ_SIDECAR_MAX_CONFIGS 4
typedef struct {
    uint8_t table_type;   /* 1 .. 4 */
    uint8_t match_len;    /* 0 = 6; 1 .. 8 */
    uint8_t extras;       /* type 4: 0 .. 15, match_len + extras <= 16; else 0 */
    uint8_t reserved;     /* 0 */
    uint16_t prefix_len;  /* type 2: 1 .. 8 values; type 4: 1 .. 256 bytes; types 1, 3: ignored */
    uint8_t reserved2[2]; /* 0 */
    uint8_t prefix[256];  /* type 2: the values; type 3: the 32 mask bytes; type 4: the prefix */
} mlz_search_config;
int64_t mlz_dev_reader_sidecar_bound(const mlz_dev_reader* reader, const mlz_search_config* cfgs, int n_cfgs);
int64_t mlz_dev_reader_build_sidecar(mlz_dev_reader* reader, void* stream, uint32_t flags, const mlz_search_config* cfgs, int n_cfgs, uint8_t* d_dst,
                                     size_t dst_cap);
int64_t mlz_dev_reader_attach_sidecar(mlz_dev_reader* reader, void* stream, uint32_t flags, const uint8_t* d_side, size_t n_side);

/* ---- tuning / introspection (not part of the reference surface) ---- */
#define MLZ_OPT_DECODE_ALGO 1  /* 0 = parallel (default), 1 = serial one-wave-per-block, 3 = parallel with every block on the tile path (cross-checks) */
#define MLZ_OPT_ENCODE_FAR 2   /* 0 = tile-local matches only, 1 = + far matches (default) */
#define MLZ_OPT_L2_FREE 14     /* LevelBalanced: 1 (default) = no tile levels — a copy may read any earlier tile of its window: the ratio of the
                                * reference's encode_l2.go and better (0.93 - 1.05 x its restatement), and the blocks decode, like the reference's own,
                                * through the general-block path; 0 = the four-level tile pattern of rounds 1-3 (1.08 - 1.09 x, level-scheduled decode) */
#define MLZ_OPT_DEVICE_GROUP 17 /* MiB of uncompressed data per internal group of a device batch (default 512): bounds the workspace */
#define MLZ_OPT_L2_GAP 19      /* LevelBalanced without tile levels: a copy from another tile reads at least this many tiles back (default 4; 1 = anywhere,
                                * rounds 4's form).  With K >= 2 the K tiles in front of a tile never feed it, and the decoder settles K (2 or 4) tiles of a
                                * block side by side instead of one: 0.3 - 1.0 % (K = 2) / 0.8 - 2.6 % (K = 4) of output for 2 - 3 x the decode rate of
                                * batches of few large blocks.  The decoder measures the distance itself: any stream that keeps it decodes this way. */
#define MLZ_OPT_FUSED_SERIALIZER 21 /* encode: 1 (default) = the match kernel's waves turn their own token records into token bytes (tile bytes and ring in LDS, records and
                                * far-source lines still in the L2); 0 = the separate serializer kernel of rounds 2-5 on the same records (byte-identical; cross-checks) */
#define MLZ_OPT_LEVEL0_KERNEL 23 /* decode: 1 (default) = a batch's level-0 candidates (tile 16 j of every block), when no more than the device has CUs, are decoded by dec_level0_kernel before the exec pass,
                                * with the blocks' verdicts and the tile schedule made in the same launch; 0 = verdicts and schedule by kernels of their own, every tile by the exec pass (cross-checks) */
#define MLZ_OPT_FOLD_LAYOUT 24  /* encode: 1 (default) = a group whose every block has tiles and room gets its layout (piece offsets, stored-or-not, header, length) from the gather kernel; 0 = always encode_layout_kernel (cross-checks) */
#define MLZ_OPT_GEN_SPIN 9     /* patience of the general-block decode with a tile's ready flag, in polls (~0.3 us each; default 2^24); tests */
#define MLZ_OPT_GEN_PACKED 13  /* tests: 1 = general blocks settle through the byte-packed pool (the fallback of tiles whose slots do not fit) */
#define MLZ_OPT_DEBUG_STATUS 3      /* debug: 1 = a failed block's negative length carries the failure site (bits 8 and up) besides the error code */
#define MLZ_OPT_PROFILE 4           /* debug: 1 = per-phase cycle counters on (16 x u64: 0-7 encode, 8-15 decode) */
#define MLZ_OPT_PROFILE_READ 5      /* debug: copy the counters (128 bytes) to the host buffer whose address is the value */
#define MLZ_OPT_TILE_TIMELINE_READ 7 /* debug: copy the exec pass's per-tile timeline (4 x u64 per tile, 100 MHz clock) to the host buffer whose address is the value */
#define MLZ_OPT_GENERAL_ALGO 8      /* decode: 0 = general blocks by the pointer-jumping pass (default), 1 = on the exec pass's tile chain */
#define MLZ_OPT_HOST_GROUP_ENC 10   /* tuning: MiB per group of a host-pointer encode batch */
#define MLZ_OPT_HOST_GROUP_DEC 11   /* tuning: MiB per group of a host-pointer decode batch */
#define MLZ_OPT_TIMER_MASK 12       /* which timers record events (bit i = mlz_timer_name(i); default all) */
#define MLZ_OPT_FAR_SLICES_L2 18    /* debug, cross-checks: 1 = LevelBalanced's far tables by far_build_kernel (the slice kernel of round 4) even without tile levels */
#define MLZ_OPT_GEN_SETTLE_CAP 20   /* tuning: role S workgroups of the general-block pass at most (default: a quarter of the device) */
/* 25 (debug, tests; it has no name here or in the Python module): level-0 candidates dec_level0_kernel is launched for at most (default 0: the device's CU count);
 * a group with more takes the path of option 23 = 0 */
/* (15 and 16 are retired: they selected a removed index pass and a debug stop; the numbers are not reused) */
int mlz_set_option(mlz_ctx* ctx, int opt, int64_t value);
/* Milliseconds spent in each kernel family, measured with HIP events on the caller's stream.
 * mlz_set_option(ctx, MLZ_TIMER_ENABLE, 1): the last *_batch_device call (mlz_get_timers waits for it);
 * (ctx, MLZ_TIMER_ENABLE, 2): running mean over all calls since then — events are read back several calls
 * late, so nothing waits on the device per call; 0 = off. */
#define MLZ_TIMER_ENABLE 100
int mlz_get_timers(mlz_ctx* ctx, float* ms, int cap); /* returns number of timers written */
const char* mlz_timer_name(int idx);
/* Counters of the combining queue behind the single-block host calls (mlz_encode, mlz_encode_block, mlz_decode,
 * mlz_decode_block): concurrent callers — one goroutine per block in the reference's Writer/Reader, writer.go:501-560,
 * reader.go:830-859 — are run as one batched launch.  which: 0 = batches run, 1 = requests served.
 * which = 2: blocks of the last decode call that matched no tile-level pattern of this library's encoder and went through the
 * general-block path (mlz_decode_general.hip.inc): the reference's own blocks, and this library's LevelBalanced ones
 *            (summed over the whole call: the internal groups of a device batch, the host groups of mlz_decode_batch /
 *            mlz_decode_block, the groups of mlz_stream_decode; 0 after a call with no block to decode in tiles).
 * which = 3 / 4: bytes of device workspace the context holds for encoding / decoding (grow-only: the high-water mark so far).
 * which = 5: decode calls whose general blocks fell back to the tile chain because the general pass's buffers could not be allocated.
 * which = 6: workgroups per block (1, 2 or 4) the general-block pass of the last decode call settled with (the largest over the
 *            groups of the call, as for 2); 0 = it had no general block.
 * which = 7 / 8: the plan of the context's last mlz_dev_reader_read or mlz_dev_reader_read_device (or the read phase of mlz_dev_reader_search_records): 7 = chunks it decoded or copied (each touched chunk counts once), 8 = decoded bytes
 *            it put into the scratch (chunks decoded straight into d_dst and stored chunks: none).
 * which = 9: bytes of plan data that crossed between host and device, both directions together, during the context's last mlz_dev_reader_read_device:
 *            32 + 32 per touched chunk (32 alone for a refused call or one that touches nothing).  Not counted: the results of the chunks' decode and CRC
 *            (12 bytes per chunk, as in every stream decode) and the one-time upload of a handle's chunk table.
 * which = 10 / 11: the context's last mlz_dev_reader_search, mlz_dev_reader_search_many or search phase of mlz_dev_reader_search_records or mlz_dev_reader_grep_records: 10 = chunks it decoded or copied, 11 = chunks with a usable search table (0 when the call
 *            used none: MLZ_SEARCH_NO_TABLES, no info chunk, a pattern shorter than M).
 * which = 12: streams that the context's last mlz_stream_*_batch_device call sent through the region walk because they hold more than 4096 chunk headers.
 * which = 17: bytes of table slots the context's last mlz_stream_encode_batch_device_tables call carved (include/minlz_hip_encode_batch_tables.h).
 * which = 13 (debug, tests; no name in the Python module): internal groups of the last decode call whose level-0 candidates, verdicts and schedule went in one launch (MLZ_OPT_LEVEL0_KERNEL); 0 = every group took the separate kernels. */
int64_t mlz_get_counter(mlz_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
