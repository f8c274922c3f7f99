"""The contract of mlz_stream_search_batch_device (include/minlz_hip_search_batch.h) in plain Python: every stream of a batch searched on its own decoded
bytes (search_model.brute), and what the call makes of the streams' answers.  A failed stream is `None` in the place of its decoded bytes:
it brings no triple, a count of 0 and an empty presence row."""
from tests import search_model as SMod


def stream_pairs(data, patterns):
    """One stream -> its pairs (position, pattern) ascending."""
    return sorted((q, i) for i, p in enumerate(patterns) for q in SMod.brute(data, p))


def result(streams, patterns, cap=None):
    """streams: each stream's decoded bytes (or None: the stream failed); patterns: bytes objects ->
    dict(total, counts: per stream, pattern_counts: per pattern, present: per stream the set of patterns that occur in it,
    triples: the smallest min(total, cap) (stream, position, pattern) ascending; cap None: all)."""
    triples, counts, present = [], [], []
    pattern_counts = [0] * len(patterns)
    for i, d in enumerate(streams):
        pairs = [] if d is None else stream_pairs(d, patterns)
        triples += [(i, q, p) for q, p in pairs]
        counts.append(len(pairs))
        present.append({p for _, p in pairs})
        for _, p in pairs:
            pattern_counts[p] += 1
    return dict(total=len(triples), counts=counts, pattern_counts=pattern_counts, present=present, triples=triples if cap is None else triples[:cap])


def present_words(present, n_patterns):
    """The presence rows as the call packs them: per stream ceil(n_patterns / 32) words, bit (p & 31) of word p // 32."""
    words = (n_patterns + 31) // 32
    rows = []
    for s in present:
        row = [0] * words
        for p in s:
            row[p >> 5] |= 1 << (p & 31)
        rows.append(row)
    return rows
