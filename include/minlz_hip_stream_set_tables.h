/* minlz_hip_stream_set_tables.h — a batch of .mz streams in HBM opened as ONE ReadSeeker handle whose searches prune by every stream's inline block
 * search tables: an extension of the C ABI of minlz_hip_stream_set.h (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_STREAM_SET_TABLES_H
#define MINLZ_HIP_STREAM_SET_TABLES_H

#include "minlz_hip_stream_set.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A TABLED SET is a set (minlz_hip_stream_set.h) in every respect: the same arguments, results, errors and bases at the open, every call of that header and
 *   every mlz_dev_reader_* call of minlz_hip.h works on it as on the streams' concatenation, and mlz_dev_reader_build_sidecar, _attach_sidecar and
 *   _extract_sidecar still return -MLZ_ERR_UNSUPPORTED.  What minlz_hip_stream_set.h says about inline tables ("not used on a set") holds for a handle from
 *   mlz_stream_open_batch_device and is what THIS open changes: the searches of a tabled set use every stream's inline tables (chunks 0x44, 0x45 and 0x46, as
 *   mlz_stream_encode_batch_device_tables and the stream Writers emit them).  The results of every call are those of the same call on the plain set of the
 *   same streams; only the number of decoded chunks changes.
 *
 *   The open itself is the plain set's: the batch walk's two read-backs and a loop over the chunk table.  Nothing of the tables is touched before the first
 *   search that does not carry MLZ_SEARCH_NO_TABLES.  That search finds the tables, once per handle and CRC mode, by the rules of
 *   mlz_stream_search_batch_device_pruned (minlz_hip_search_batch_prune.h), and keeps them on the handle:
 *     - a lane per stream hops to the stream's info chunk (0x44) and leaves a key of 16 bytes; the host numbers the distinct configurations
 *       (T, M, B, prefix field) in descriptor order.  The first 4 classes prune.  A stream of a later class, a stream without a usable info chunk and a stream
 *       whose field differs from its class's byte for byte are decoded whole;
 *     - a lane per data chunk locates the first fitting table chunk between the previous data chunk's end (the stream's first byte) and its own body; the hop
 *       never leaves the stream's source span;
 *     - unlike the batch call, a fitting 0x46 chunk is taken and expanded once into an arena the handle owns.  The first fitting table in front of a block is
 *       taken, whichever of 0x45 and 0x46 it is; a 0x46 table that does not parse, does not decode or has a stale CRC, and a stale 0x45, are passed over for
 *       the next fitting one.  Without a next one the chunk has no table and is admitted.  Table CRCs are checked unless MLZ_STREAM_IGNORE_CRC is set, in one
 *       CRC pass per round over the tables of all streams;
 *     - host traffic: once per handle the key and the class verdict per stream and a class's configuration once per class; once per CRC mode and locate
 *       round (one round, and one more for every table that was passed over in front of one block) per data chunk the 24-byte record of its own class's table
 *       (where it lies, never a byte of it), as on a single handle, and a CRC word per table; once per handle and record index a crossing flag per stream;
 *       per call one byte per data chunk.  No chunk body and no table comes home.
 *   mlz_dev_reader_close frees what the handle took.
 *
 *   THE PLAN.  A stream's tables were built over that stream alone and say nothing about an occurrence that crosses the stream's end.  Per (data chunk,
 *   pattern of L bytes), ORed over the patterns:
 *     a. inside a stream that a class prunes, the single stream's rule with chunk numbers and the chunk count taken inside the chunk's own stream.  A class
 *        prunes only when its configuration serves every pattern of the call; otherwise its streams are decoded whole;
 *     b. a stream decoded whole takes every chunk with bytes;
 *     c. cross[i] = stream i has bytes and a later stream with bytes exists; for a RECORD-BOUND call in addition: the record that holds stream i's last byte
 *        runs on into the next stream (the `joined` of mlz_dev_reader_stream_records, per stream).  Under cross[i] every chunk of stream i that holds one of
 *        the stream's last L - 1 decoded bytes is a candidate unconditionally: a crossing occurrence starts there, and its first windows may straddle the end
 *        and stand in no table;
 *     d. from any candidate the chunks that hold the L - 1 bytes behind it are taken too, over the handle's chunk list; that stops at the end of a stream
 *        whose cross is false and otherwise passes on into the next streams, whatever their mode.  Streams without bytes end nothing.
 *   POSITION calls — mlz_dev_reader_search, _search_many and through them _search_records — use cross without the record condition: an occurrence may lie
 *     anywhere in the concatenation.  Consequence: on objects of a single chunk they prune little (every chunk holds its stream's last bytes), and
 *     mlz_stream_search_batch_device_pruned, which never crosses a stream's end, stays the call for "which objects hold this key".
 *   RECORD-BOUND calls — mlz_dev_reader_grep_records and mlz_dev_reader_grep_regex_pruned — find occurrences inside one record by contract (the literals that
 *     hold the delimiter are dropped), so they use the joined form.  A batch whose objects all end with the delimiter has joined == 0, and the grep prunes
 *     exactly as each stream alone would: the case this header exists for.  The flags are made on the device once per handle and record index.
 *   Statistics keep their meaning: stats[0] data chunks, stats[1] chunks decoded, stats[2] chunks with a usable table in pruned streams; for the many-pattern
 *     calls stats[3] = the patterns to which no pruning class of the set gives a window.  mlz_get_counter 10, 11 and 14 follow them.  MLZ_SEARCH_NO_TABLES
 *     gives the plain set's plan and launches nothing of the above; MLZ_SEARCH_IGNORE_CASE, MLZ_GREP_INVERT, the context counts and MLZ_REGEX_IGNORE_CASE
 *     combine as on a single handle.
 *   Out of scope: a flag that makes position searches never cross a stream's end (it would let them prune single-chunk objects); sidecars on sets; more than
 *     four pruning classes; a configuration chosen per pattern instead of per class; a per-(stream, pattern) count matrix; sets over several devices; an
 *     asynchronous form; a faster 0x46 expansion. */

/* mlz_stream_open_batch_device_tables: mlz_stream_open_batch_device (its arguments, out_len, results and errors) for a handle whose searches use the
 *   streams' inline tables as described above. */
int64_t mlz_stream_open_batch_device_tables(mlz_ctx* ctx, void* stream, const uint8_t* d_src,
                                            const mlz_block_desc* streams, int n_streams,   /* src_off, src_len; dst_off = dst_cap = 0 */
                                            int64_t* out_len,                 /* host, n_streams: the stream's decoded size, or -MLZ_ERR_* */
                                            mlz_dev_reader** out);

/* mlz_dev_reader_set_tables_info: the last plan on the handle (host; all 0 before the first, and left as it is by a call under MLZ_SEARCH_NO_TABLES):
 *   out[0] the classes found (may exceed 4); out[1] the streams pruned by a class; out[2] the streams with bytes that were decoded whole; out[3] the chunks with
 *   a usable table in pruned streams; out[4] those of them whose table came from a 0x46 chunk; out[5] the stream ends treated as crossed (rule c; 0 when no
 *   stream was pruned: the rule was not evaluated).
 *   Returns the number of 0x46 tables that stand expanded in the handle's arenas (those that parsed, decoded and passed their CRC; both CRC modes added) —
 *   it stays as it is from the second search in a CRC mode on —, or
 *   -MLZ_ERR_ARG for NULL or for a handle that mlz_stream_open_batch_device_tables did not open. */
int64_t mlz_dev_reader_set_tables_info(const mlz_dev_reader* rd, uint64_t* out /* host, 6 values */);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_STREAM_SET_TABLES_H */
