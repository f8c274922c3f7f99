/* minlz_hip_stream_set.h — a batch of .mz streams in HBM opened as ONE ReadSeeker handle: an extension of the C ABI of minlz_hip.h (which it includes; the
 * same library, libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_STREAM_SET_H
#define MINLZ_HIP_STREAM_SET_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A SET is an mlz_dev_reader whose decoded address space is the decoded bytes of many streams one behind the other, in the order of their descriptors: what
 *   the reference's Reader yields for `cat a.mz b.mz`.  Every handle call of minlz_hip.h then is a call on the whole batch, with its documented contract and
 *   `size` = the set's size: mlz_dev_reader_size, _read, _read_device, _search, _search_many, _search_records, _index_records, _record_count, _record_spans,
 *   _read_records, _record_numbers, _record_range, _grep_records, _close.  The calls below translate between the handle's positions and record numbers and
 *   (stream, position or record number inside the stream), in device memory, so that a sampler or a grep over objects never visits the host.
 *   What concatenation means:
 *     - a range may span two streams;
 *     - a pattern may match across the end of one stream and the start of the next (mlz_dev_reader_locate shows it: local + pattern length > the stream's
 *       size).  mlz_stream_search_batch_device (minlz_hip_search_batch.h) stays the call that never does that;
 *     - a record may continue from one stream into the next when the first does not end with the delimiter: see mlz_dev_reader_stream_records.
 *   Decode and CRC errors are those of the first failing touched chunk in the handle's order; which stream it belongs to is not reported.
 *   Inline search tables are not used on a set (the hops that find them run through one stream's framing): the handle counts as having no usable table, every
 *     search decodes every chunk with bytes as under MLZ_SEARCH_NO_TABLES, and the searches' third statistic is 0.  mlz_dev_reader_build_sidecar and
 *     mlz_dev_reader_attach_sidecar return -MLZ_ERR_UNSUPPORTED before anything is launched, as the first does for concatenated streams.
 *   Out of scope: searches on a set that never cross a stream end, inline tables or sidecars on a set, the stream of a decode error, sets over several
 *     devices, an asynchronous open. */

/* mlz_stream_open_batch_device: opens the streams streams[i] (src_off, src_len; dst_off and dst_cap are ignored) of the buffer at d_src as one handle.
 *   Synchronous; `stream`, the device routing and the checks of the descriptors are those of mlz_stream_search_batch_device: source spans may overlap,
 *   repeat and come in any order.  One lock, the batch walk's two read-backs, nothing per stream beyond them.
 *   out_len[i] (host, n_streams values) = what mlz_stream_open_device returns for stream i alone: its decoded size, or its framing error.  A stream with a
 *     framing error is left out of the set: size 0 and no chunk, not even those in front of its error; it changes nothing for any other stream.
 *   Stream i occupies [bases[i], bases[i] + size_i) of the handle; bases[0] = 0, bases[i + 1] = bases[i] + size_i.  The handle's chunk table is the healthy
 *     streams' data chunks in descriptor order.  The bases also live in device memory that the handle owns until mlz_dev_reader_close.
 *   Returns the set's size, the sum of the healthy streams' sizes, and the handle in *out; or -MLZ_ERR_ARG / -MLZ_ERR_HIP and *out = NULL.
 *   n_streams == 0 opens a set of size 0 with no stream; d_src, streams and out_len may be NULL then.  d_src must stay valid until the handle is closed. */
int64_t mlz_stream_open_batch_device(mlz_ctx* ctx, void* stream, const uint8_t* d_src,
                                     const mlz_block_desc* streams, int n_streams,   /* src_off, src_len; dst_off = dst_cap = 0 */
                                     int64_t* out_len,                 /* host, n_streams: the stream's decoded size, or -MLZ_ERR_* */
                                     mlz_dev_reader** out);

/* mlz_dev_reader_stream_count / mlz_dev_reader_stream_bases: the number of descriptors the handle was opened with, failed ones included, and the count + 1
 *   bases (host).  Both return the count, or -MLZ_ERR_ARG.  A handle from mlz_stream_open_device answers as a set of one, {0, size}, here and in the four
 *   calls below: callers need no second code path. */
int64_t mlz_dev_reader_stream_count(const mlz_dev_reader* rd);
int64_t mlz_dev_reader_stream_bases(const mlz_dev_reader* rd, uint64_t* bases /* host, count + 1 */);

/* mlz_dev_reader_locate: positions of the handle -> (stream, position inside the stream), a lane per position; all arrays in device memory, n values each.
 *   d_which[k] = the last i with bases[i] <= d_pos[k], which is a stream that has bytes; d_local[k] = d_pos[k] - bases[i].  A position >= size gives
 *   0xFFFFFFFF and 0.  Returns the number of positions below size, or -MLZ_ERR_ARG / -MLZ_ERR_HIP.  Synchronous.
 *   This turns the offsets of mlz_dev_reader_search / _search_many and the rec_off of _search_records into (object, offset). */
int64_t mlz_dev_reader_locate(mlz_dev_reader* rd, void* stream, const uint64_t* d_pos, size_t n, uint32_t* d_which, uint64_t* d_local);

/* mlz_dev_reader_read_streams_device: mlz_dev_reader_read_device with ranges relative to their stream: range k is [d_off[k], d_off[k] + d_len[k]) of stream
 *   d_which[k].  A kernel checks every range (d_which[k] < count, d_off[k] <= size_i, d_len[k] <= size_i - d_off[k]) and writes its place in the handle into
 *   context workspace; any bad range gives -MLZ_ERR_ARG before a decode or copy is enqueued, with nothing written to d_dst or d_starts.  A range into a failed
 *   or empty stream is valid only as off == 0, len == 0.  Everything else is mlz_dev_reader_read_device's contract: packed output, d_starts (n_ranges + 1
 *   values, may be NULL), exactly the touched chunks decoded once, the errors, nothing per range on the host. */
int64_t mlz_dev_reader_read_streams_device(mlz_dev_reader* rd, void* stream, uint32_t flags,
                                           const uint32_t* d_which, const uint64_t* d_off, const uint64_t* d_len, size_t n_ranges,
                                           uint8_t* d_dst, size_t dst_cap, uint64_t* d_starts /* may be NULL */);

/* mlz_dev_reader_stream_records: the records of every stream.  Needs the record index (mlz_dev_reader_index_records); without one -MLZ_ERR_ARG, as the other
 *   record calls.  first[i] (host, count + 1 values) = the number of the handle's records that start below bases[i]; first[count] = the record count.
 *   *joined (host, may be NULL) = the streams that have bytes, whose last byte is not the delimiter and that have a stream with bytes behind them: a record
 *   runs on from each of them into the next stream.  When it is 0 the handle's records are exactly every stream's own records in order (the stream's bytes
 *   split at the delimiter, one trailing empty piece dropped), and stream i owns the record numbers [first[i], first[i + 1]).
 *   One kernel, a lane per stream.  Returns the record count, or -MLZ_ERR_ARG / -MLZ_ERR_HIP.  Synchronous. */
int64_t mlz_dev_reader_stream_records(mlz_dev_reader* rd, void* stream, uint64_t* first /* host, count + 1 */, uint64_t* joined /* host, 1 value, may be NULL */);

/* mlz_dev_reader_locate_records: record numbers -> (the stream in which the record starts, its number inside that stream = r - first[which]), a lane per
 *   number; all arrays in device memory, n values each.  A number >= the record count gives 0xFFFFFFFF and 0.  Returns how many were in range, or
 *   -MLZ_ERR_ARG (no record index) / -MLZ_ERR_HIP.  Synchronous.  This turns the output of mlz_dev_reader_grep_records into grep -H -n. */
int64_t mlz_dev_reader_locate_records(mlz_dev_reader* rd, void* stream, const uint64_t* d_rec_no, size_t n, uint32_t* d_which, uint64_t* d_local_no);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_STREAM_SET_H */
