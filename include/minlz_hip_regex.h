/* minlz_hip_regex.h — regular expressions in the grep over the record index of a .mz stream in HBM (grep -E): an extension of the C ABI of minlz_hip.h
 * (which it includes; the same library, libminlz_hip.so, exports it).  C99 and C++. */
#ifndef MINLZ_HIP_REGEX_H
#define MINLZ_HIP_REGEX_H

#include "minlz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An mlz_regex is a set of regular expressions over BYTES, compiled on the host into one search automaton: a table of S states by C byte classes (16 bits
 *   an entry) and a class map of 256 bytes.  Run over a record's bytes from left to right it decides "some substring of the record is in the language of
 *   one of the expressions".  Compiling, mlz_regex_info, mlz_regex_test and mlz_regex_free need no context and no GPU.
 *   Syntax: a subset of Python's `re` on bytes, chosen so that every accepted expression means the same there (with re.DOTALL, and ^ / $ read as \A / \Z
 *   of a record):
 *     alt := cat ('|' cat)*      cat := rep*  (may be empty: "a|" and "()" are valid)      rep := atom quant?
 *     quant: * + ? {m} {m,} {m,n} with 0 <= m <= n <= 255.  -MLZ_ERR_ARG: a second quantifier on one atom (a**, a{2}{3}), a quantifier with nothing
 *       to repeat (*a, ^*, |+), a { that opens none of the three forms ({,n} included).  -MLZ_ERR_UNSUPPORTED: lazy and possessive quantifiers
 *       (*? +? ?? {m,n}? *+).
 *     atom: a literal byte (any byte but the metacharacters \ . [ ] ( ) { } * + ? | ^ $), . (ANY byte), a class, ( alt ), (?: alt ), ^, $, an escape.
 *       "(?" followed by anything but ':' (inline flags, lookaround, named groups) and groups nested more than 256 deep: -MLZ_ERR_UNSUPPORTED.
 *     escape: \ and a metacharacter or one of - / " is that byte; \n \r \t \f \v \0 are control bytes; \xHH is a byte value; \d \D \w \W \s \S are
 *       ASCII as `re` on bytes has them (\w = [A-Za-z0-9_], \s = [ \t\n\r\f\v]; bytes >= 0x80 are in \W \D \S).  \ followed by anything else
 *       (\b \B \A \Z, \1 .. \9, every other letter) and \0 followed by a digit (Python's octal escapes): -MLZ_ERR_UNSUPPORTED.
 *     class: '[' '^'? items ']', an item being a byte, a range lo-hi (lo <= hi, else -MLZ_ERR_ARG) or any escape above.  A ] or ^ meant literally is
 *       escaped; - is literal as the first or the last item.  -MLZ_ERR_ARG: an empty class, an unescaped ^ behind the first place, a range from or to
 *       \d \w \s, a - behind a range that is not the last item.  -MLZ_ERR_UNSUPPORTED: "[:" (the POSIX bracket names).
 *     ^ matches only in front of a record's first byte and $ only behind its last; both may stand wherever an atom may ("(a|^b)c$|d"); a branch
 *       that can never be satisfied ("a^") never matches.  An empty expression matches every record.
 *   MLZ_REGEX_IGNORE_CASE: every byte set of an expression (a literal as a singleton, a class before its ^, \d \w \s) is closed under the ASCII
 *     case swap before a negation is applied: re.IGNORECASE on bytes ([^a] does not match A; [Z-a] matches z).  The fold lives in the class map.
 *   Limits, checked while the automaton is built (a blow-up is never built first): 1 .. 256 expressions of 0 .. 4096 bytes each (-MLZ_ERR_ARG);
 *     4096 byte positions behind the expansion of the counted repetitions, 4096 states, and 64 KiB for the class map and the table together, the
 *     memory a workgroup of the mark kernel keeps them in (-MLZ_ERR_UNSUPPORTED).
 *   Out of scope: back-references, lookaround, word boundaries, Unicode, submatch positions, which expression matched; records longer than
 *     MLZ_REGEX_MAX_RECORD (a record is walked by one lane; a cooperative path for longer records does not exist). */
typedef struct mlz_regex mlz_regex;

#define MLZ_REGEX_IGNORE_CASE 1u
#define MLZ_REGEX_MAX_RECORD 1048576u /* bytes: mlz_dev_reader_search_records' largest reach */

/* mlz_regex_compile: n_exprs expressions (grep -E -e a -e b), back to back in `exprs` with their lengths in expr_len, -> *out, one automaton for their
 *   union.  flags: 0 or MLZ_REGEX_IGNORE_CASE.  Returns 0; or -MLZ_ERR_ARG / -MLZ_ERR_UNSUPPORTED with *out = NULL and, in where (host, may be NULL: 2
 *   values), the index of the expression and the byte offset in it at which the compiler stopped (a limit of the automaton as a whole: the last
 *   expression and its length; a bad n_exprs: n_exprs and 0). */
int mlz_regex_compile(const uint8_t* exprs, const uint32_t* expr_len, size_t n_exprs, uint32_t flags,
                      mlz_regex** out, uint64_t* where /* host, may be NULL: 2 values */);
void mlz_regex_free(mlz_regex* re);
/* mlz_regex_info: info[0 .. 4) = states, byte classes, bytes of class map and table as the kernel holds them, bit 0 = the expression matches the
 *   empty record.  Returns 0 or -MLZ_ERR_ARG. */
int mlz_regex_info(const mlz_regex* re, uint64_t* info /* 4 values */);
/* mlz_regex_test: 1 when record[0, len) holds a match, else 0, by the rule the kernel runs; -MLZ_ERR_ARG for a NULL. */
int mlz_regex_test(const mlz_regex* re, const uint8_t* record, size_t len);

/* mlz_dev_reader_grep_regex: mlz_dev_reader_grep_records (minlz_hip.h) with M decided by a compiled expression:
 *     M = the records whose bytes, the delimiter excluded, hold a match.  An empty record is in M exactly when the expression matches the empty
 *         string: "^$" selects the empty lines.
 *   S, C, R, the order, d_rec_no, d_rec_kind, the cut at rec_cap, totals, before / after and N == 0 are word for word mlz_dev_reader_grep_records'.
 *   Flags: MLZ_STREAM_IGNORE_CRC and MLZ_GREP_INVERT; any other bit is -MLZ_ERR_ARG (case folding is a property of the compiled expression).
 *   -MLZ_ERR_ARG, each decided before anything is launched, nothing written: a handle without an index; re == NULL; N >= 2^32; d_rec_no NULL with
 *   rec_cap > 0; d_rec_no or d_rec_kind (not NULL), with rec_cap > 0, that is not on the handle's device.
 *   -MLZ_ERR_UNSUPPORTED, before any chunk is decoded, nothing written: the index's longest record exceeds MLZ_REGEX_MAX_RECORD bytes.  (The first
 *   call on an index finds that length with one reduction over the index, 8 bytes home, and the handle keeps it beside the index.)
 *   No table can prune for a regular expression: every data chunk with bytes is decoded once, group by group as mlz_dev_reader_index_records does it, and
 *   each group is marked by one kernel, a lane per record, a record that crosses a group's border carrying its state over.  stats (host, may be
 *   NULL: 4 values) = data chunks, chunks decoded, 0, 0, and mlz_get_counter 10 / 11 describe the call as a search phase that decoded every chunk
 *   and used no table.  Decode and CRC errors are those of the first failing chunk in stream order, with nothing written.
 *   The select and compact kernels are mlz_dev_reader_grep_records' own; 32 bytes visit the host behind the decode's verdicts, and 16 bytes per group
 *   (its first and last record) in front of it.  Synchronous; `stream` as for mlz_dev_reader_read.
 *   On a set handle (minlz_hip_stream_set.h) the call works on the streams' concatenation, like every handle call. */
int64_t mlz_dev_reader_grep_regex(mlz_dev_reader* reader, void* stream, uint32_t flags, const mlz_regex* re,
                                  uint64_t before, uint64_t after, uint64_t* d_rec_no, uint8_t* d_rec_kind, size_t rec_cap,
                                  uint64_t* totals /* host, may be NULL: 4 values */, uint64_t* stats /* host, may be NULL: 4 values */);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_REGEX_H */
