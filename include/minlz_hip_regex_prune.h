/* minlz_hip_regex_prune.h — the regex grep pruned by block search tables: the required literals of a compiled expression and the grep that decodes only
 * the chunks the tables admit for them.  An extension of include/minlz_hip_regex.h (which it includes; the same library, libminlz_hip.so, exports it).
 * C99 and C++. */
#ifndef MINLZ_HIP_REGEX_PRUNE_H
#define MINLZ_HIP_REGEX_PRUNE_H

#include "minlz_hip_regex.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mlz_regex_compile also derives a set L of REQUIRED LITERALS from the syntax tree: whenever the expression matches a record, some l of L is a
 *   substring of the record (under MLZ_REGEX_IGNORE_CASE: of the record with A - Z folded to a - z; L is then stored folded).  At most 64 strings
 *   of 1 .. 256 bytes each, none empty, sorted bytewise; L may be empty, which means "none": an expression too rich for the limits has no literals,
 *   compiling never fails because of them.  The rule is fixed, so that L can be pinned.  Per node of the tree two values — E, the finite set of ALL
 *   strings the node matches (or unknown), and F, the best set of required factors (or none); under the case flag a byte set is first mapped to its
 *   lower-case image:
 *     byte set S (literal, class, escape, .): E = the one-byte strings if |S| <= 4, else unknown; F = E.     ^, $, an empty node: E = {""}, F = none.
 *     concatenation: left to right with a running set X = {""}.  While E(child) is known, |X| |E(child)| <= 16 and no product string exceeds 256
 *       bytes, X = X x E(child); otherwise X becomes a candidate and a new X starts from E(child) (from {""} if that is unknown).  The final X is a
 *       candidate, and so is every child's F.  E = X if the run was never closed, else unknown; F = the best candidate.
 *     alternation: E = the union of the branches' E if all are known and it has at most 16 strings; F = the union of the branches' F if every branch
 *       has one and it has at most 64 strings.
 *     a{m,n}: m = 0: F = none; E = E(a) + {""} if n = 1 and E(a) is known.  m >= 1: with E(a)^m built as m products within the same caps,
 *       F = the better of F(a) and E(a)^m, E = E(a)^m if m = n.         Several expressions of one compile: an alternation of their roots.
 *     best: a set that holds the empty string is no candidate; the larger shortest string wins, then the fewer strings, then the leftmost.
 *   "status":5[0-9][0-9] -> {"status":5};  ^(ERROR|FATAL) -> {ERROR, FATAL};  user_[0-9]+@ -> {user_};  [Ee]rror -> {Error, error};  a*, ^$, [0-9]+ -> none.
 *
 * mlz_regex_literals -> the number of literals (0: none).  lens[i] for i < min(count, lens_cap); the strings back to back in buf as far as buf_cap
 *   reaches, whole strings only.  info (may be NULL, 4 values): count, bytes of all strings, shortest length, bit 0 = folded.  -MLZ_ERR_ARG for a
 *   NULL re (or a NULL buf / lens with a capacity). */
int mlz_regex_literals(const mlz_regex* re, uint8_t* buf, size_t buf_cap, uint32_t* lens, size_t lens_cap, uint64_t* info /* may be NULL: 4 values */);

/* mlz_dev_reader_grep_regex_pruned: mlz_dev_reader_grep_regex with the same arguments and the same results — M, S, C, R, the order, d_rec_no, d_rec_kind,
 *   the cut at rec_cap, totals, MLZ_GREP_INVERT and before / after, the argument errors and the refusal of records beyond MLZ_REGEX_MAX_RECORD before
 *   anything is decoded — that decodes only the chunks the handle's search tables (inline 0x45 / 0x46 chunks or the attached sidecar) admit for the
 *   expression's literals.  Flags: MLZ_STREAM_IGNORE_CRC, MLZ_GREP_INVERT and, additionally, MLZ_SEARCH_NO_TABLES.
 *   Plan: the literals that do not hold the handle's delimiter (those cannot lie inside a record) are planned as the patterns of
 *     mlz_dev_reader_search_many, under MLZ_SEARCH_IGNORE_CASE for a folded set.  Every chunk with bytes is taken when the expression has no literals,
 *     under MLZ_SEARCH_NO_TABLES, on a set handle, when a literal is not served by the tables, and under the case flag with an ASCII letter as the
 *     delimiter.  If the expression has literals and each holds the delimiter, no record can match: nothing is decoded and M is empty.
 *   Widen: a literal found in a chunk proves only that some record touching the chunk may match, and the automaton needs that record whole.  One kernel,
 *     a lane per taken chunk, finds the start of the record that holds the chunk's first byte and the end of the one that holds its last (16 bytes
 *     per taken chunk come home); every chunk that intersects such a span is decoded as well.
 *   Decode and mark: the widened list is decoded in groups, each marked by one kernel launch however many holes it has; a record is evaluated when a
 *     run of decoded chunks holds it whole, and carries its state across a group's border as in the unpruned call.  A record cut by a run's end
 *     touches no chunk the plan took and cannot match.
 *   stats (host, may be NULL: 4 values) = data chunks, chunks decoded (after widening), chunks with a usable table as the plan reports them, chunks the
 *     plan took before widening; mlz_get_counter 10 / 11 / 14 describe the call likewise.  Decode and CRC errors are those of the first failing
 *     DECODED chunk in stream order, with nothing written: a broken chunk that the tables prune goes unnoticed, as in mlz_dev_reader_grep_records.
 *   With every chunk taken the call runs the same kernels on one run per group.  Synchronous; `stream` as for mlz_dev_reader_read. */
int64_t mlz_dev_reader_grep_regex_pruned(mlz_dev_reader* reader, void* stream, uint32_t flags, const mlz_regex* re,
                                         uint64_t before, uint64_t after, uint64_t* d_rec_no, uint8_t* d_rec_kind, size_t rec_cap,
                                         uint64_t* totals /* host, may be NULL: 4 values */, uint64_t* stats /* host, may be NULL: 4 values */);

#ifdef __cplusplus
}
#endif

#endif /* MINLZ_HIP_REGEX_PRUNE_H */
