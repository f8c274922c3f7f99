"""Streams that the tests of mlz_dev_reader_extract_sidecar share (tests/test_sidecar_extract_host.py, tests/test_gpu_sidecar_extract.py):
framed on the host by the models, so that both files hold the same bytes against tests/sidecar_extract_model.py."""
import numpy as np

from minlz_amd import index as I
from minlz_amd import synth
from tests import search_model as SMod
from tests import sidecar_model as SM

T1 = SMod.config(1, 6)
HEADER_AND_EOF = bytes([0xFF, 6, 0, 0]) + b"MinLz" + bytes([6]) + b"\x20\x01\x00\x00\x00"


def with_fresh_index(stream, n_decoded):
    """The stream with the index a Writer under MLZ_STREAM_ADD_INDEX appends: an entry per data chunk, behind the EOF chunk."""
    idx = I.Index()
    idx.reset(SM.max_block_of(stream[:10]))
    u = 0
    for (p, n) in SM.main_chunks(stream):
        idx.add(p, u)
        u += n
    assert u == n_decoded
    return stream + idx.append_to(n_decoded, len(stream))


def hand_framed(seed=21, post_eof_table=False):
    """-> (stream, data): 4 KiB blocks under a 4 KiB header, the second and the fourth random bytes, hence stored (0x01), a short last block;
    a type 1 table in front of every block; between blocks a padding chunk and a user chunk, a gap of 300 one-byte padding chunks and a
    stray 0x47; a table with no block behind it in front of the EOF chunk; an index chunk behind it (post_eof_table: and a table behind that)."""
    bs = 4 << 10
    sizes = [bs] * 6 + [1234]
    d = bytearray(synth.text_like(sum(sizes), seed).tobytes())
    for k in (1, 3):
        d[k * bs:(k + 1) * bs] = synth.random_bytes(bs, seed=seed + k).tobytes()
    d = bytes(d)
    plain = SM.framed(d, sizes, size_byte=2)
    assert [t for _, t in SMod.data_grid(plain)] == [2, 1, 2, 1, 2, 2, 2]
    B = SMod.table_bits(bs)
    spliced, tables = SMod.splice(plain, d, T1, B, stored_too=True)
    assert all(t is not None for t in tables)
    pad = lambda n: SMod.frame(0xFE, bytes(n))
    extra = {2: pad(7) + SMod.frame(0x80, b"user chunk"), 4: pad(1) * 300, 5: SM.ref_chunk(12345, 7)}
    out, k = [], 0
    for p, t, n in SMod.chunks_of(spliced):
        raw = spliced[p:p + 4 + n]
        if t == SMod.CHUNK_TABLE:              # (a block's extras lie in front of its table)
            out.append(extra.get(k, b""))
        if t in (1, 2, 3):
            k += 1
        if t == 0x20:
            out.append(SMod.table_chunk(T1, B, b"\x55" * (1 << (B - 3)), 0))
        out.append(raw)
    stream = with_fresh_index(b"".join(out), len(d))
    if post_eof_table:
        stream += SMod.table_chunk(T1, B, b"\x33" * (1 << (B - 3)), 0)
    return stream, d


def mixed_compress_data(bs=64 << 10, seed=100):
    """8 blocks for the Writer under search_compress: JSON-like text, one block of random bytes, two of a short phrase repeated (their
    tables are nearly empty and compress)."""
    d = bytearray(synth.json_like(8 * bs + 500, seed).tobytes())
    d[bs:2 * bs] = synth.random_bytes(bs, seed=6).tobytes()
    phrase = (b"the quick brown fox jumps over the lazy dog, %d times; " * 5) % (1, 2, 3, 4, 5)
    for k in (2, 5):
        d[k * bs:(k + 1) * bs] = (phrase * (bs // len(phrase) + 1))[:bs]
    return bytes(d)


def first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n = min(len(a), len(b))
    w = np.flatnonzero(a[:n] != b[:n])
    return int(w[0]) if len(w) else n
