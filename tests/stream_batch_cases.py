"""Batches of streams for tests/test_stream_batch_host.py (host) and tests/test_gpu_stream_batch.py (GPU): the small oracle stream whose
mutants both run, and streams laid into one buffer with their spans."""
import oracle as O
from minlz_amd import synth
from tests import corrupt as CM

BS = 64 << 10
_CACHE = {}

# stream_mutants of small_stream(): how many, and how many per code of the oracle's Reader (pinned as test_stream_device_host.test_mutants
# pins those of the large streams)
MUTANT_COUNT = 70
MUTANT_CODES = {0: 3, 1: 40, 2: 2, 3: 6, 5: 19}


def small_data():
    """Five 64 KiB blocks of text, two of random bytes (stored chunks), two of JSON."""
    if "d" not in _CACHE:
        _CACHE["d"] = synth.text_like(5 * BS, 21).tobytes() + synth.random_bytes(2 * BS, seed=22).tobytes() + synth.json_like(2 * BS, 23).tobytes()
    return _CACHE["d"]


def small_stream():
    if "s" not in _CACHE:
        _CACHE["s"] = O.stream_encode(small_data(), 1, BS, False)
    return _CACHE["s"]


def small_mutants():
    if "m" not in _CACHE:
        _CACHE["m"] = CM.stream_mutants(small_stream())
    return _CACHE["m"]


def back_to_back(streams, gap=0):
    """-> (buffer, [(off, len)]): the streams one behind the other, `gap` bytes of 0xA5 between two."""
    spans, parts, o = [], [], 0
    for s in streams:
        spans.append((o, len(s)))
        parts.append(s)
        o += len(s)
        if gap:
            parts.append(b"\xa5" * gap)
            o += gap
    return b"".join(parts), spans
