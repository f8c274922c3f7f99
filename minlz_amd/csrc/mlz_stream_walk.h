// mlz_stream_walk.h — the Reader's framing rules (reader.go:248-543), written once for the host Reader (stream_parse in mlz_stream.hip.inc),
// the device-resident Reader and the batch calls (mlz_stream_walk.hip.inc, mlz_stream_batch.h) and their host checks (tools/stream_walk_check.cpp,
// tools/stream_batch_check.cpp): the step from chunk header to chunk header (walk_headers), the per-chunk record filled from the bytes of a
// header (walk_classify), and the Reader's running state applied to such records (WalkReader).  Plain C++: compiles for the host alone and for gfx950.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MLZ_WALK_HD __host__ __device__ inline
#else
#define MLZ_WALK_HD inline
#endif

namespace mlz {

// One chunk of the walk, as it visits the host: 32 bytes.
struct WalkChunk {
    uint64_t off;     // offset of the chunk's 4-byte header in the stream
    uint64_t val;     // 0x02 / 0x03: the uvarint decoded length; 0x20: the uvarint stream size; 0xff: the version byte
    uint32_t crc;     // 0x01 / 0x02 / 0x03: the four bytes behind the header
    uint32_t tl;      // type << 24 | chunk length
    int8_t hl;        // bytes of the uvarint (binary.Uvarint: 0 = short buffer, < 0 = overflow)
    uint8_t flags;    // kWalk*
    uint8_t pad[6];
};
static_assert(sizeof(WalkChunk) == 32, "the chunk table's record");
constexpr uint8_t kWalkStub = 1;    // fewer than 4 bytes are left at `off`: no header
constexpr uint8_t kWalkTrunc = 2;   // the chunk's length runs past the end of the stream
constexpr uint8_t kWalkHas4 = 4;    // at least 4 bytes follow the header (0x01: its CRC is there)
constexpr uint8_t kWalkMagic = 8;   // 0xff of length 6: the body starts with "MinLz"

// binary.Uvarint: bytes read (0 = short buffer, < 0 = overflow)
MLZ_WALK_HD int walk_uvarint(const uint8_t* b, size_t n, uint64_t* out) {
    uint64_t x = 0; unsigned s = 0;
    for (size_t i = 0; i < n; i++) {
        if (i == 10) return -int(i + 1);
        const uint8_t c = b[i];
        if (c < 0x80) {
            if (i == 9 && c > 1) return -int(i + 1);
            *out = x | uint64_t(c) << s;
            return int(i + 1);
        }
        x |= uint64_t(c & 0x7f) << s; s += 7;
    }
    return 0;
}

// A skippable chunk (index, padding, user chunks) that lies inside the stream changes nothing in the Reader's state: the walk steps over it
// and it never enters the table.
MLZ_WALK_HD bool walk_skippable(uint8_t type, uint64_t clen, uint64_t left /* bytes behind the header */) { return type > 0x3f && type != 0xff && left >= clen; }

// A sidecar's info, table and reference chunks: skippable, but the walk of a sidecar keeps them
MLZ_WALK_HD bool walk_search_chunk(uint8_t type) { return type == 0x44 || type == 0x45 || type == 0x46 || type == 0x47; }

// The 4-byte header of the chunk at p (p + 4 <= n): the length of what follows; *type: the chunk's type
MLZ_WALK_HD uint32_t walk_header(const uint8_t* src, uint64_t p, uint8_t* type) {
    *type = src[p];
    return uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16;
}

// The record of the chunk whose header is at p (p < n).  Reads src[p .. min(n, p + 4 + 14)) and nothing else.
MLZ_WALK_HD WalkChunk walk_classify(const uint8_t* src, uint64_t n, uint64_t p) {
    WalkChunk w{};
    w.off = p;
    if (n - p < 4) { w.flags = kWalkStub; return w; }
    uint8_t type;
    const uint32_t clen = walk_header(src, p, &type);
    w.tl = uint32_t(type) << 24 | clen;
    const uint8_t* b = src + p + 4;
    const uint64_t left = n - (p + 4);
    const bool trunc = left < clen;
    w.flags = uint8_t((trunc ? kWalkTrunc : 0) | (left >= 4 ? kWalkHas4 : 0));
    auto le32 = [](const uint8_t* q) { return uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24; };
    if (type == 0x02 || type == 0x03) {
        if (clen >= 4 && !trunc) {
            w.crc = le32(b);
            const uint32_t vn = clen - 4 < 11 ? clen - 4 : 11;   // (the eleventh byte is the overflow verdict)
            w.hl = int8_t(walk_uvarint(b + 4, vn, &w.val));
        }
    } else if (type == 0x01) {
        if (left >= 4) w.crc = le32(b);
    } else if (type == 0x20) {
        if (clen && clen <= 10 && !trunc) w.hl = int8_t(walk_uvarint(b, clen, &w.val));
    } else if (type == 0xff) {
        if (clen == 6 && left >= 6) {
            if (b[0] == 'M' && b[1] == 'i' && b[2] == 'n' && b[3] == 'L' && b[4] == 'z') w.flags |= kWalkMagic;
            w.val = b[5];
        }
    }
    return w;
}

// The chunk walk, header by header: from offset e while e < end, visit(offset) for every header that enters the table.  The stub (fewer than
// 4 bytes are left) enters the table and ends the walk; a chunk that walk_skippable accepts is stepped over — with keep_search the walk of a
// sidecar keeps its search chunks —; e += 4 + clen.  visit returns false to end the walk there (the host Reader, at its first error).
// max_steps: the most headers to step over, kWalkNoCap for no limit; returns false when the cap ended the walk.
// Reads the 4-byte headers it steps over, all inside src[0, n), and nothing else.
constexpr uint32_t kWalkNoCap = 0xffffffffu;
template <class Visit>
MLZ_WALK_HD bool walk_headers(const uint8_t* src, uint64_t n, uint64_t e, uint64_t end, bool keep_search, uint32_t max_steps, Visit visit) {
    uint32_t steps = 0;
    while (e < end) {
        if (max_steps != kWalkNoCap && steps++ == max_steps) return false;
        if (n - e < 4) { visit(e); break; }
        uint8_t type;
        const uint32_t clen = walk_header(src, e, &type);
        if ((!walk_skippable(type, clen, n - e - 4) || (keep_search && walk_search_chunk(type))) && !visit(e)) break;
        e += 4 + uint64_t(clen);
    }
    return true;
}

// Error codes as in include/minlz_hip.h (MLZ_ERR_*), negated on return.
constexpr int kWalkErrCorrupt = 1, kWalkErrTooLarge = 2, kWalkErrUnsupported = 3;

// Reader.Read's running state, chunk by chunk in stream order.  step(w, data) takes the next record: `data(type, crc, body_off, body_len, n,
// out_off, hdr_off)` is called for a data chunk that passes (hdr_off: where the chunk's 4-byte header lies, which a sidecar's remote
// references name); returns 0 or -MLZ_ERR_*, and nothing behind an error is the Reader's to see.  finish(): the decoded size, or the error
// of a stream that ends while an EOF chunk is owed.  A stub and a chunk that runs past the end of the stream are errors here.
struct WalkReader {
    uint64_t max_block_limit;
    uint64_t out = 0, max_block, stream_out = 0;
    bool read_header = false, want_eof = false;
    explicit WalkReader(uint64_t limit) : max_block_limit(limit), max_block(limit) {}

    template <class Data>
    [[gnu::always_inline]] int step(const WalkChunk& w, Data data) {   // (inlined: the loop over a table keeps the state in registers)
        if (w.flags & kWalkStub) return -kWalkErrCorrupt;
        const uint8_t type = uint8_t(w.tl >> 24);
        const uint64_t clen = w.tl & 0xffffffu, p = w.off + 4;
        const bool trunc = (w.flags & kWalkTrunc) != 0;
        const uint64_t max_enc = max_block + 2;   // mlz_max_encoded_len(max_block), max_block > 0
        if (!read_header) {
            if (type == 0xff) read_header = true;
            else if (type <= 0x3f && type != 0x20) return -kWalkErrCorrupt;   // reader.go:273-283
        }
        switch (type) {
        case 0x02: case 0x03: {
            if (clen < 4 || clen > max_enc + 4 || trunc) return -kWalkErrCorrupt;
            if (w.hl <= 0 || w.val > 0xffffffffull) return -kWalkErrCorrupt;
            if (w.val > max_block) return -kWalkErrTooLarge;
            const uint64_t body = clen - 4 - uint64_t(w.hl);
            if (w.val == 0 || w.val < body) return -kWalkErrCorrupt;   // reader.go:327
            data(type, w.crc, p + 4 + uint64_t(w.hl), body, w.val, out, w.off);
            out += w.val; stream_out += w.val;
            return 0;
        }
        case 0x01: {
            if (clen < 4 || clen > max_enc + 4 || !(w.flags & kWalkHas4)) return -kWalkErrCorrupt;
            const uint64_t nn = clen - 4;
            if (nn > max_block) return -kWalkErrTooLarge;   // (before the bytes are read: reader.go:411-464)
            if (trunc) return -kWalkErrCorrupt;
            data(type, w.crc, p + 4, nn, nn, out, w.off);
            out += nn; stream_out += nn;
            return 0;
        }
        case 0x20:
            if (clen > 10 || trunc) return -kWalkErrCorrupt;
            if (clen && (w.hl != int(clen) || w.val != stream_out)) return -kWalkErrCorrupt;   // reader.go:476-491
            want_eof = read_header = false;
            return 0;
        case 0xff: {
            if (clen != 6 || trunc) return -kWalkErrCorrupt;
            if (!(w.flags & kWalkMagic)) return -kWalkErrUnsupported;
            const uint8_t v = uint8_t(w.val);
            if (v & 0xc0) return -kWalkErrCorrupt;
            const unsigned lg = (v & 15) + 10;
            if (lg > 23) return -kWalkErrCorrupt;
            max_block = uint64_t(1) << lg;
            if (max_block > max_block_limit) return -kWalkErrTooLarge;
            stream_out = 0;
            want_eof = true;
            return 0;
        }
        default:
            if (type <= 0x3f) return -kWalkErrUnsupported;   // legacy S2/Snappy chunk (0x00) or reserved unskippable, reader.go:530-536
            return -kWalkErrCorrupt;                          // a skippable chunk that reaches the Reader is one that runs past the end
        }
    }
    int64_t finish() const { return want_eof ? -int64_t(kWalkErrCorrupt) : int64_t(out); }   // io.ErrUnexpectedEOF when an EOF chunk is owed
};

// The Reader over a table of records: the decoded size or -MLZ_ERR_*, `data` called for every data chunk in front of the first error.
// The table ends where the walk ended: at the end of the stream, at a stub or at a chunk that runs past the end.
template <class Data>
int64_t walk_parse_table(const WalkChunk* t, size_t cnt, uint64_t max_block_limit, Data data) {
    WalkReader rd(max_block_limit);
    for (size_t i = 0; i < cnt; i++)
        if (const int e = rd.step(t[i], data)) return e;
    return rd.finish();
}

}  // namespace mlz
