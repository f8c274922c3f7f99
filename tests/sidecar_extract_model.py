"""mlz_dev_reader_extract_sidecar in plain Python: the reference's ExtractSidecar (sidecar.go:557-771) restated for one stream.

    extract(stream, strip) -> (side, main or None, counts)

The source's 0x44 / 0x45 / 0x46 chunks go to the sidecar as they are, every data chunk gets one remote reference (0x47), and with `strip`
the stream is written again without its search and index chunks, with an EOF chunk that names the decoded size and a fresh seek index
(minlz_amd/index.py) behind it; the references then name the offsets in that stream, else those in the source.  counts: the fields of
mlz_sidecar_extract_result (api.SidecarExtract)."""
from minlz_amd import api
from minlz_amd import index as I
from tests import search_model as SMod
from tests import sidecar_model as SM

SEARCH, INDEX, DATA = (0x44, 0x45, 0x46), (0x40, 0x99), (0x01, 0x02, 0x03)


class ExtractError(Exception):
    """kind: "corrupt" or "unsupported" """

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def extract(stream, strip):
    stream = bytes(stream)
    cks = SMod.chunks_of(stream)
    idents = [p for p, t, n in cks if t == 0xFF]
    if not idents:
        raise ExtractError("corrupt")
    if len(idents) > 1 or sum(t == 0x20 for _, t, _ in cks) != 1:
        raise ExtractError("unsupported")
    ident = stream[idents[0]:idents[0] + 10]
    max_block = SM.max_block_of(ident)
    side, main = [ident], [ident]
    written, uncomp = 10, 0                  # newStreamWritten, newUncompWritten
    idx = I.Index()
    idx.reset(max_block)
    c = dict(blocks=0, info_chunks=0, tables=0, tables_compressed=0, passed_bytes=0, dropped_bytes=0)
    for p, t, n in cks:
        raw = stream[p:p + 4 + n]
        if t in SEARCH:
            side.append(raw)
            c["info_chunks"] += t == 0x44
            c["tables"] += t != 0x44
            c["tables_compressed"] += t == 0x46
        elif t in DATA:
            size = n - 4 if t == 0x01 else SMod.S.uvarint(stream, p + 8)[0]
            if size <= 0 or size > max_block:
                raise ExtractError("corrupt")
            ref = p
            if strip:
                ref = written
                main.append(raw)
                idx.add(written, uncomp)
                written += len(raw)
                uncomp += size
            side.append(SM.ref_chunk(ref, max_block - size))
            c["blocks"] += 1
        elif t == 0x20:
            side.append(SM.EOF_CHUNK)
            if strip:
                v = SM.uvarint(uncomp)
                main.append(bytes([0x20, len(v), 0, 0]) + v)
                main.append(idx.append_to(uncomp, -1))
        elif t in INDEX:
            c["dropped_bytes"] += len(raw) if strip else 0
        elif t == 0xFF:
            pass
        else:
            if t <= 0x3F:
                raise ExtractError("corrupt")
            if strip:
                main.append(raw)
                written += len(raw)
                c["passed_bytes"] += len(raw)
    side, main = b"".join(side), b"".join(main) if strip else None
    return side, main, api.SidecarExtract(side_len=len(side), main_len=len(main) if strip else 0, **c)
