// mlz_stream_record_index_store.h — the rules of the stored record index (include/minlz_hip_record_index_store.h; the kernels and the calls are
// mlz_stream_record_index_store.hip.inc), shared with their host check (tools/record_index_store_check.cpp, which runs them as plain loops).
// Plain C++: compiles for the host alone and for gfx950.  tests/record_index_store_model.py is the same contract in numpy.
//
// The blob is a MinLZ stream without data (all integers little-endian):
//   ff 06 00 00 "MinLz" 0d                                   the stream identifier, block-size value 13                     [0, 10)
//   90 <len24> crc32 <fixed header, 62 B> <directory>        the header chunk; len24 = 66 + 4 nsections                      [10, 80 + 4 nsections)
//   91 <len24> crc32 <section>                               one per section; len24 = 4 + the directory's entry
//   20 01 00 00 00                                           EOF, size 0
// crc32 = the masked CRC32C (rstore_crc: the data chunks' function) of the chunk's body behind it.  62 makes every section start at a
// multiple of 4 inside the blob: 10 + 4 + 4 + 62 + 4 nsections + 8 = 88 + 4 nsections, and a section's length is a multiple of 4.
// Fixed header: "MLZRIDX1" | u32 flags (bit 0 bound, bit 1 longest known) | u8 delimiter, 3 zero bytes | u64 size | u64 k | u64 N |
//   u64 longest (all ones when unknown) | u32 stream tag | u32 data chunks | u32 nsections | u16 zero.
// A tile is 65 536 ABSOLUTE decoded positions (not the scan kernels' memory coordinates), a section 1024 consecutive tiles.
// Section: u32 number | u32 tiles | u64 rank of its first delimiter | tiles + 1 u32 cumulative counts (the first 0) | the tiles' payloads.
// Payload of a tile with c delimiters: c <= 4096: c u16 of D[j] - tile start, ascending, and one zero u16 when c is odd (sparse);
//   c > 4096: 8192 bytes, bit j & 7 of byte j >> 3 = position tile start + j is a delimiter (dense).  The choice is a rule, so the blob is a
//   function of (D, size, delimiter, binding, longest).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_record_index.h"

namespace mlz {

constexpr uint32_t kRstoreTile = 65536, kRstoreTileLog = 16, kRstoreSectionTiles = 1024, kRstoreSparseMax = 4096, kRstoreBitmap = kRstoreTile / 8;
constexpr uint32_t kRstoreIdent = 10, kRstoreFixed = 62, kRstoreFixedAt = kRstoreIdent + 8, kRstoreDirAt = kRstoreFixedAt + kRstoreFixed, kRstoreEof = 5;
constexpr uint32_t kRstoreThreads = 256;
constexpr uint8_t kRstoreChunkHeader = 0x90, kRstoreChunkSection = 0x91;
constexpr uint32_t kRstoreBound = 1u, kRstoreLongest = 2u;            // the header's flags
constexpr uint64_t kRstoreMaxSize = uint64_t(1) << 36;                // decoded bytes of a handle (the chunk walk's limit): at most 1024 sections
constexpr uint64_t kRstoreMaxBuild = (uint64_t(1) << 32) - (uint64_t(1) << 17);   // raw bytes of one build call: tile bases are 32 bits
static_assert(kRstoreDirAt == 80 && (kRstoreDirAt + 8) % 4 == 0, "sections start at multiples of 4");

// The codes of the ABI (MLZ_ERR_*), restated for the host check; mlz_stream_record_index_store.hip.inc holds them against the header
constexpr int kRstoreErrCorrupt = 1, kRstoreErrUnsupported = 3, kRstoreErrCrc = 5, kRstoreErrDstTooSmall = 6, kRstoreErrArg = 8;

// What the expand kernel reports (ORed into RstoreVerdict::bad); any bit is -MLZ_ERR_CORRUPT
constexpr uint32_t kRstoreBadSection = 1, kRstoreBadCounts = 2, kRstoreBadRank = 4, kRstoreBadOffset = 8, kRstoreBadSparse = 16, kRstoreBadDense = 32;
struct RstoreVerdict { uint32_t bad, crc_bad, last_is_delim, pad; };
static_assert(sizeof(RstoreVerdict) == 16, "a record shared with the kernels");

struct RstoreHeader {
    uint32_t flags;
    uint8_t delim;
    uint64_t size, k, N, longest;
    uint32_t tag, data_chunks, nsections;
};
// A section of the blob as the kernels see it: where its bytes (behind the CRC) lie in the blob, and how many they are
struct RstoreSection { uint64_t off, len; };

MLZ_RINDEX_HD uint64_t rstore_ntiles(uint64_t size) { return (size + kRstoreTile - 1) >> kRstoreTileLog; }
MLZ_RINDEX_HD uint64_t rstore_nsections(uint64_t size) { return (rstore_ntiles(size) + kRstoreSectionTiles - 1) / kRstoreSectionTiles; }
MLZ_RINDEX_HD uint32_t rstore_section_tiles(uint64_t ntiles, uint64_t s) {
    const uint64_t left = ntiles - s * kRstoreSectionTiles;
    return uint32_t(left < kRstoreSectionTiles ? left : kRstoreSectionTiles);
}
MLZ_RINDEX_HD bool rstore_dense(uint32_t c) { return c > kRstoreSparseMax; }
MLZ_RINDEX_HD uint32_t rstore_payload_bytes(uint32_t c) { return rstore_dense(c) ? kRstoreBitmap : ((c + 1) & ~1u) * 2; }
MLZ_RINDEX_HD uint32_t rstore_section_head(uint32_t tiles) { return 16 + 4 * (tiles + 1); }
MLZ_RINDEX_HD uint64_t rstore_frame_bytes(uint64_t nsections) { return kRstoreDirAt + 4 * nsections + 8 * nsections + kRstoreEof; }   // everything but the sections
// Bytes that always suffice for an index of k delimiters over `size` bytes
MLZ_RINDEX_HD uint64_t rstore_bound(uint64_t size, uint64_t k) {
    const uint64_t nt = rstore_ntiles(size), ns = rstore_nsections(size);
    const uint64_t sparse = 2 * k + 2 * nt, dense = uint64_t(kRstoreBitmap) * nt;
    return rstore_frame_bytes(ns) + 16 * ns + 4 * (nt + ns) + (sparse < dense ? sparse : dense);
}

// The masked CRC32C of the data chunks, a bit at a time: for the header chunk and the stream tag (a few KB at the most), on the host
inline uint32_t rstore_crc_update(uint32_t c, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
    }
    return c;
}
inline uint32_t rstore_crc_mask(uint32_t c) { c = ~c; return ((c >> 15) | (c << 17)) + 0xa282ead8u; }
inline uint32_t rstore_crc(const uint8_t* p, size_t n) { return rstore_crc_mask(rstore_crc_update(0xffffffffu, p, n)); }

// The stream tag: rstore_crc over 9 bytes per data chunk with bytes (u32 decoded length, u32 stored CRC field, u8 chunk type)
struct RstoreTag {
    uint32_t c = 0xffffffffu, chunks = 0;
    void add(uint32_t n, uint32_t crc_field, uint8_t type) {
        const uint8_t b[9] = {uint8_t(n), uint8_t(n >> 8), uint8_t(n >> 16), uint8_t(n >> 24), uint8_t(crc_field), uint8_t(crc_field >> 8), uint8_t(crc_field >> 16), uint8_t(crc_field >> 24), type};
        c = rstore_crc_update(c, b, 9);
        chunks++;
    }
    uint32_t tag() const { return rstore_crc_mask(c); }
};

MLZ_RINDEX_HD void rstore_put32(uint8_t* p, uint32_t v) { p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); p[2] = uint8_t(v >> 16); p[3] = uint8_t(v >> 24); }
MLZ_RINDEX_HD void rstore_put64(uint8_t* p, uint64_t v) { rstore_put32(p, uint32_t(v)); rstore_put32(p + 4, uint32_t(v >> 32)); }
MLZ_RINDEX_HD uint32_t rstore_get16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
MLZ_RINDEX_HD uint32_t rstore_get32(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24; }
MLZ_RINDEX_HD uint64_t rstore_get64(const uint8_t* p) { return uint64_t(rstore_get32(p)) | uint64_t(rstore_get32(p + 4)) << 32; }
MLZ_RINDEX_HD void rstore_chunk_header(uint8_t* p, uint8_t type, uint32_t len24) { p[0] = type; p[1] = uint8_t(len24); p[2] = uint8_t(len24 >> 8); p[3] = uint8_t(len24 >> 16); }

// out[0, 80 + 4 nsections): the identifier and the header chunk; dir[s] = section s's length
inline void rstore_put_head(uint8_t* out, const RstoreHeader& h, const uint32_t* dir) {
    static const uint8_t ident[kRstoreIdent] = {0xff, 0x06, 0x00, 0x00, 'M', 'i', 'n', 'L', 'z', 0x0d};
    for (uint32_t i = 0; i < kRstoreIdent; i++) out[i] = ident[i];
    rstore_chunk_header(out + kRstoreIdent, kRstoreChunkHeader, 4 + kRstoreFixed + 4 * h.nsections);
    uint8_t* f = out + kRstoreFixedAt;
    for (uint32_t i = 0; i < 8; i++) f[i] = uint8_t("MLZRIDX1"[i]);
    rstore_put32(f + 8, h.flags);
    rstore_put32(f + 12, h.delim);
    rstore_put64(f + 16, h.size); rstore_put64(f + 24, h.k); rstore_put64(f + 32, h.N); rstore_put64(f + 40, h.longest);
    rstore_put32(f + 48, h.tag); rstore_put32(f + 52, h.data_chunks); rstore_put32(f + 56, h.nsections);
    f[60] = f[61] = 0;
    for (uint32_t s = 0; s < h.nsections; s++) rstore_put32(out + kRstoreDirAt + 4 * s, dir[s]);
    rstore_put32(out + kRstoreIdent + 4, rstore_crc(f, kRstoreFixed + 4 * size_t(h.nsections)));
}
MLZ_RINDEX_HD void rstore_put_eof(uint8_t* p) { p[0] = 0x20; p[1] = 0x01; p[2] = p[3] = p[4] = 0; }

// The identifier, the header chunk's frame and the fixed header of blob[0, have) -> 0, or the (positive) code.  Everything the header says
// about itself is checked here: a header that passes asks for nothing beyond what `size` allows (k <= size, nsections from the size).
inline int rstore_parse_fixed(const uint8_t* b, size_t have, RstoreHeader* h) {
    static const uint8_t ident[kRstoreIdent] = {0xff, 0x06, 0x00, 0x00, 'M', 'i', 'n', 'L', 'z', 0x0d};
    if (have < kRstoreDirAt) return kRstoreErrCorrupt;
    for (uint32_t i = 0; i < kRstoreIdent; i++) if (b[i] != ident[i]) return kRstoreErrCorrupt;
    if (b[kRstoreIdent] != kRstoreChunkHeader) return kRstoreErrCorrupt;
    const uint8_t* f = b + kRstoreFixedAt;
    for (uint32_t i = 0; i < 8; i++) if (f[i] != uint8_t("MLZRIDX1"[i])) return kRstoreErrUnsupported;
    h->flags = rstore_get32(f + 8); h->delim = f[12];
    h->size = rstore_get64(f + 16); h->k = rstore_get64(f + 24); h->N = rstore_get64(f + 32); h->longest = rstore_get64(f + 40);
    h->tag = rstore_get32(f + 48); h->data_chunks = rstore_get32(f + 52); h->nsections = rstore_get32(f + 56);
    const uint32_t len24 = uint32_t(b[kRstoreIdent + 1]) | uint32_t(b[kRstoreIdent + 2]) << 8 | uint32_t(b[kRstoreIdent + 3]) << 16;
    if ((h->flags & ~(kRstoreBound | kRstoreLongest)) || f[13] || f[14] || f[15] || f[60] || f[61]) return kRstoreErrCorrupt;
    if (h->size > kRstoreMaxSize || h->k > h->size || !(h->N == h->k || (h->N == h->k + 1 && h->size > 0))) return kRstoreErrCorrupt;
    if (h->nsections != rstore_nsections(h->size) || len24 != 4 + kRstoreFixed + 4 * h->nsections) return kRstoreErrCorrupt;
    if ((h->flags & kRstoreLongest) ? h->longest > h->size : h->longest != ~uint64_t(0)) return kRstoreErrCorrupt;
    if (!(h->flags & kRstoreBound) && (h->tag || h->data_chunks)) return kRstoreErrCorrupt;
    return 0;
}

// The directory of a blob of `len` bytes whose first `have` are at b (have >= 80 + 4 nsections or have == len): every section's place
// (sec[s], nsections of them; may be NULL), its length within what its tiles allow, the chunks' frames adding up to exactly len, and the
// header chunk's CRC unless ignore_crc.  -> 0 or the code.
inline int rstore_parse_directory(const uint8_t* b, size_t have, uint64_t len, const RstoreHeader& h, bool ignore_crc, RstoreSection* sec) {
    const uint64_t head = uint64_t(kRstoreDirAt) + 4 * uint64_t(h.nsections);
    if (len < head + kRstoreEof || have < head) return kRstoreErrCorrupt;
    const uint64_t ntiles = rstore_ntiles(h.size);
    uint64_t at = head;
    for (uint32_t s = 0; s < h.nsections; s++) {
        const uint32_t tiles = rstore_section_tiles(ntiles, s), n = rstore_get32(b + kRstoreDirAt + 4 * s), lo = rstore_section_head(tiles);
        if (n < lo || n > lo + uint64_t(kRstoreBitmap) * tiles || (n & 3)) return kRstoreErrCorrupt;
        if (sec) sec[s] = RstoreSection{at + 8, n};
        at += 8 + uint64_t(n);
    }
    if (at + kRstoreEof != len) return kRstoreErrCorrupt;
    if (!ignore_crc && rstore_get32(b + kRstoreIdent + 4) != rstore_crc(b + kRstoreFixedAt, size_t(head - kRstoreFixedAt))) return kRstoreErrCrc;
    return 0;
}

// A blob's header against the handle it is loaded into: the size always, the tag and the data chunks of a bound blob -> 0 or the code
MLZ_RINDEX_HD int rstore_match(const RstoreHeader& h, uint64_t size, uint32_t tag, uint32_t data_chunks) {
    if (h.size != size) return kRstoreErrArg;
    if ((h.flags & kRstoreBound) && (h.tag != tag || h.data_chunks != data_chunks)) return kRstoreErrArg;
    return 0;
}

// ---- pack: what a tile's workgroup does, lane by lane ----

// The tile boundaries: first[t] = the rank of the first delimiter at or behind t * 65536, first[ntiles] = k.  at(j) = D[j].
template <class At>
MLZ_RINDEX_HD uint64_t rstore_first(At at, uint64_t k, uint64_t ntiles, uint64_t t) { return t >= ntiles ? k : rindex_number(at, k, t << kRstoreTileLog); }

// Entry j of a sparse tile (j <= c: j == c is the pad of an odd count) -> the u16 at payload + 2 j
template <class At>
MLZ_RINDEX_HD uint32_t rstore_sparse_entry(At at, uint64_t first, uint32_t c, uint64_t tile, uint32_t j) { return j < c ? uint32_t(at(first + j) - (tile << kRstoreTileLog)) : 0; }

// ---- expand: the checks of one tile, in the order the kernel makes them.  ld32(off) / ld16(off): the blob's bytes at off, read only for
// off + 4 (+ 2) <= sec.off + sec.len of the tile's own section (or the next one's first 16 bytes), which the directory has bounded by len ----

struct RstoreTilePlan {
    uint32_t bad;        // kRstoreBad*; nothing of the payload is read or written when set
    uint32_t c;          // delimiters of the tile
    uint64_t rank;       // of its first delimiter
    uint64_t payload;    // where its payload lies in the blob
};

// The payload bytes of a tile whose cumulative counts are lo and hi; 0 for a pair that its own tile's plan refuses
MLZ_RINDEX_HD uint32_t rstore_count_bytes(uint32_t lo, uint32_t hi) { return hi >= lo && hi - lo <= kRstoreTile ? rstore_payload_bytes(hi - lo) : 0; }

// Tile i of section s: the section's header against what the size says, the tile's pair of counts, the ranks against k, the payload's
// place inside the section.  off_before = the payload bytes of the section's tiles in front of i (the lanes' sum of rstore_count_bytes);
// next_first = the next section's first rank, k behind the last section.
template <class Ld32>
MLZ_RINDEX_HD RstoreTilePlan rstore_tile_plan(Ld32 ld32, const RstoreSection& sec, uint64_t s, uint32_t tiles, uint32_t i, uint64_t off_before, uint64_t next_first, uint64_t k) {
    RstoreTilePlan p{0, 0, 0, 0};
    if (ld32(sec.off) != uint32_t(s) || ld32(sec.off + 4) != tiles) p.bad |= kRstoreBadSection;
    const uint64_t first = uint64_t(ld32(sec.off + 8)) | uint64_t(ld32(sec.off + 12)) << 32;
    const uint32_t lo = ld32(sec.off + 16 + 4 * uint64_t(i)), hi = ld32(sec.off + 20 + 4 * uint64_t(i));
    if (hi < lo || hi - lo > kRstoreTile || (i == 0 && lo != 0)) p.bad |= kRstoreBadCounts;
    if ((s == 0 && first != 0) || first > k || hi > k - first) p.bad |= kRstoreBadRank;
    if (i + 1 == tiles && !(p.bad & kRstoreBadRank) && first + hi != next_first) p.bad |= kRstoreBadRank;
    if (p.bad) return p;
    p.c = hi - lo;
    p.rank = first + lo;
    const uint64_t rel = uint64_t(rstore_section_head(tiles)) + off_before, bytes = rstore_payload_bytes(p.c);
    if (rel + bytes > sec.len || (i + 1 == tiles && rel + bytes != sec.len)) { p.bad |= kRstoreBadOffset; return p; }
    p.payload = sec.off + rel;
    return p;
}

// Entry j of a sparse payload (j <= c: the pad): its value checked against its neighbour in front and the tile's end -> kRstoreBadSparse or 0;
// limit = the positions of the tile inside the stream (65536, less in the last tile)
MLZ_RINDEX_HD uint32_t rstore_sparse_check(uint32_t v, uint32_t prev, bool has_prev, bool is_pad, uint32_t limit) {
    if (is_pad) return v ? kRstoreBadSparse : 0;
    return v >= limit || (has_prev && prev >= v) ? kRstoreBadSparse : 0;
}
// A word of a dense payload (word w of 2048): bits at or beyond `limit` -> kRstoreBadDense
MLZ_RINDEX_HD uint32_t rstore_dense_check(uint32_t word, uint32_t w, uint32_t limit) {
    const uint32_t lo = w * 32;
    if (lo + 32 <= limit) return 0;
    const uint32_t keep = limit > lo ? (1u << (limit - lo)) - 1 : 0;
    return (word & ~keep) ? kRstoreBadDense : 0;
}

}  // namespace mlz
