"""Streams for the device-resident Reader's tests (tests/test_stream_device_host.py on the host, tests/test_gpu_stream_device.py on the GPU):
the data mix of tests/test_gpu_corrupt.py's stream tests, oracle-written and hand-framed streams, and the stream of very many tiny chunks."""
import oracle as O
from minlz_amd import stream as S, synth

_CACHE = {}


def data_mix():
    if "d" not in _CACHE:
        _CACHE["d"] = synth.text_like(2 << 20, 3).tobytes() + synth.random_bytes((1 << 20) + 300_000, seed=4).tobytes() + synth.json_like(700_000, 5).tobytes()
    return _CACHE["d"]


def frame(type_, body):
    n = len(body)
    return bytes([type_, n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF]) + body


def stream_id(block_size):
    return S.MAGIC + bytes([(block_size - 1).bit_length() - 10])


def data_chunk(block, level=1):
    """[0x02][len24][crc][uvarint N][tokens], or the stored form when the block does not compress."""
    tokens = O.encode_block(block, level)
    crc = O.crc(block).to_bytes(4, "little")
    if not tokens:
        return frame(S.CHUNK_UNCOMPRESSED, crc + block)
    return frame(S.CHUNK_MINLZ, crc + S.put_uvarint(len(block)) + tokens)


def eof(n):
    return frame(S.CHUNK_EOF, S.put_uvarint(n))


def to_compcrc(stream):
    """Every 0x02 chunk as 0x03: the same body, the CRC over the token bytes (reader.go:341-344)."""
    b = bytearray(stream)
    p = 0
    while p + 4 <= len(b):
        t = b[p]
        n = b[p + 1] | b[p + 2] << 8 | b[p + 3] << 16
        if t == 0x02:
            _, hl = S.uvarint(b, p + 8)
            b[p] = 0x03
            b[p + 4:p + 8] = O.crc(bytes(b[p + 8 + hl:p + 4 + n])).to_bytes(4, "little")
        p += 4 + n
    return bytes(b)


def oracle_stream(block_size, level=1, add_index=False):
    key = ("o", block_size, level, add_index)
    if key not in _CACHE:
        _CACHE[key] = O.stream_encode(data_mix(), level, block_size, add_index)
    return _CACHE[key]


def with_skippables(block_size=64 << 10):
    """User skippable chunks and padding between the data chunks of a hand-framed stream -> (stream, data)."""
    d = data_mix()[:block_size * 9 + 123]
    out = [stream_id(block_size), frame(0x80, b"user chunk in front")]
    for i in range(0, len(d), block_size):
        out.append(data_chunk(d[i:i + block_size]))
        out.append(frame(S.CHUNK_PADDING, bytes((i >> 16) % 700)))
        if i % (3 * block_size) == 0:
            out.append(frame(0x99, b"\x02\x00\x00\x01" * 50))   # (a body that looks like chunk headers)
    out += [eof(len(d)), frame(0x81, b"behind the end")]
    return b"".join(out), d


def tiny_chunks(n_skippable=200_000, every=1_000, break_crc=False):
    """Identifier, n_skippable empty skippable chunks (type 0x80, length 0) with a small data chunk after every `every` of them, EOF
    -> (stream, data).  break_crc: the CRC of the last data chunk but two is wrong."""
    if ("t", every) not in _CACHE:
        _CACHE[("t", every)] = synth.text_like(600 * 1024, 17).tobytes()
    text = _CACHE[("t", every)]
    pad = frame(0x80, b"") * every
    out, data = [stream_id(4 << 10)], []
    k = n_skippable // every
    for i in range(k):
        blk = text[(i * 577) % (len(text) - 700):][:100 + (i * 37) % 600]
        ck = bytearray(data_chunk(blk))
        if break_crc and i == k - 3:
            ck[5] ^= 0x20
        out += [pad, bytes(ck)]
        data.append(blk)
    d = b"".join(data)
    out.append(eof(len(d)))
    return b"".join(out), d


def valid_streams_cpu():
    """(name, stream, data) that the oracle alone can make."""
    d = data_mix()
    cases = []
    for level in (1, 2, 3):
        for bs in (4 << 10, 64 << 10, 1 << 20, 8 << 20):
            for idx in (False, True):
                if level != 1 and (bs, idx) not in (((64 << 10), True), ((1 << 20), False)):
                    continue   # (every level; every size and the index at level 1: the framing does not depend on the level)
                cases.append(("oracle_L%d_bs%d_idx%d" % (level, bs, idx), oracle_stream(bs, level, idx), d))
    cases.append(("empty", O.stream_encode(b"", 1, 1 << 20), b""))
    cases.append(("no_bytes", b"", b""))
    cases.append(("one_byte", O.stream_encode(b"x", 1, 1 << 20), b"x"))
    a, b = d[:1_500_000], d[1_500_000:]
    cases.append(("two_streams", O.stream_encode(a, 1, 1 << 20) + O.stream_encode(b, 2, 64 << 10, True), d))
    s, sd = with_skippables()
    cases.append(("skippables", s, sd))
    cases.append(("compcrc", to_compcrc(oracle_stream(1 << 20)), d))
    return cases
