// record_index_store_check.cpp — the rules that the stored record index shares with its kernels (minlz_amd/csrc/mlz_stream_record_index_store.h),
// run as plain loops for tests/test_record_index_store_host.py:
//   g++ -O2 -std=c++17 -o ris tools/record_index_store_check.cpp && ./ris cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 delimiter, shift, flags, tag, data chunks; u64 size, longest, k; k u64 positions D
//           -> the save path as the kernels run it — the tile boundaries by bisection (rstore_first), per section the scan of the payload
//           sizes, the host's layout, per tile a loop over the lanes' entries (rstore_sparse_entry; dense: a bitmap of 2048 words ORed bit
//           by bit), the CRCs, the frames — into a buffer of exactly the blob's bytes that lies `shift` bytes off a 4-byte boundary, then
//           the load path over it (below), whose table must be D:  "<bytes> <sections> <sparse> <dense> <the blob in hex>"
//   kind 2  u32 shift, flags (1 = ignore CRCs), tag, data chunks; u64 size, len; the blob
//           -> the load path as the kernels run it for a handle of that size, tag and data chunks: rstore_parse_fixed, the size,
//           rstore_parse_directory, rstore_match, the sections' frames and CRCs, per tile rstore_tile_plan and the payload's checks.  Every
//           read of the blob goes through a bounds check of its own (a read outside the blob ends the program with status 3, as a heap
//           overflow does under the sanitizer: the buffer holds exactly the blob):  "ok <N> <k> <delimiter> <longest> : D ..." or "error <code>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_record_index_store.h"

namespace {

using namespace mlz;

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

[[noreturn]] void fail(const char* what, uint64_t i) {
    std::fprintf(stderr, "%s (at %llu)\n", what, (unsigned long long)i);
    std::exit(3);
}

// `n` bytes that lie `shift` bytes off a 4-byte boundary and end where their allocation ends: a read or a store behind them is a heap
// overflow under the sanitizer
struct Shifted {
    uint8_t* store;
    uint8_t* p;
    Shifted(size_t n, uint32_t shift) : store(static_cast<uint8_t*>(std::malloc(shift + n + (shift + n == 0)))), p(store + shift) {
        if (!store || (reinterpret_cast<uintptr_t>(store) & 3)) fail("no buffer", n);
    }
    ~Shifted() { std::free(store); }
    Shifted(const Shifted&) = delete;
    Shifted& operator=(const Shifted&) = delete;
};

struct Store {
    uint8_t* base; uint64_t len; bool aligned;
    void check(uint64_t off, uint32_t n) const {
        if (off + n > len) fail("a store outside the blob", off);
        if (aligned && (reinterpret_cast<uintptr_t>(base + off) & (n - 1))) fail("a store that is not aligned", off);
    }
    void st32(uint64_t off, uint32_t v) const { check(off, 4); rstore_put32(base + off, v); }
    void st16(uint64_t off, uint32_t v) const { check(off, 2); base[off] = uint8_t(v); base[off + 1] = uint8_t(v >> 8); }
};

struct Load {
    const uint8_t* base; uint64_t len; bool aligned;
    void check(uint64_t off, uint32_t n) const {
        if (off + n > len) fail("a read outside the blob", off);
        if (aligned && (reinterpret_cast<uintptr_t>(base + off) & (n - 1))) fail("a read that is not aligned", off);
    }
    uint32_t ld32(uint64_t off) const { check(off, 4); return rstore_get32(base + off); }
    uint32_t ld16(uint64_t off) const { check(off, 2); return rstore_get16(base + off); }
    uint8_t ld8(uint64_t off) const { check(off, 1); return base[off]; }
};

// The save path -> the blob's bytes; *sparse, *dense: the tiles of either kind
std::vector<uint8_t> save(const std::vector<uint64_t>& D, uint64_t size, RstoreHeader h, uint32_t shift, uint64_t* sparse, uint64_t* dense) {
    const uint64_t k = D.size(), nt = rstore_ntiles(size), ns = rstore_nsections(size);
    auto at = [&](uint64_t j) { if (j >= k) fail("a table entry beyond k", j); return D[size_t(j)]; };
    std::vector<uint64_t> first(size_t(nt) + 1);
    for (uint64_t t = 0; t <= nt; t++) first[size_t(t)] = rstore_first(at, k, nt, t);
    std::vector<uint32_t> tile_off(static_cast<size_t>(nt)), dir(static_cast<size_t>(ns));
    std::vector<uint64_t> sec_off(static_cast<size_t>(ns));
    *dense = 0;
    uint64_t pos = kRstoreDirAt + 4 * ns;
    for (uint64_t s = 0; s < ns; s++) {
        const uint32_t tiles = rstore_section_tiles(nt, s);
        uint32_t run = 0;
        for (uint32_t i = 0; i < tiles; i++) {
            const uint64_t t = s * kRstoreSectionTiles + i;
            const uint32_t c = uint32_t(first[size_t(t) + 1] - first[size_t(t)]);
            tile_off[size_t(t)] = rstore_section_head(tiles) + run;
            run += rstore_payload_bytes(c);
            *dense += rstore_dense(c) ? 1 : 0;
        }
        dir[size_t(s)] = rstore_section_head(tiles) + run;
        sec_off[size_t(s)] = pos + 8;
        pos += 8 + dir[size_t(s)];
    }
    *sparse = nt - *dense;
    const uint64_t total = pos + kRstoreEof;
    if (total > rstore_bound(size, k)) fail("the blob exceeds its bound", total);
    Shifted buf(size_t(total), shift);
    std::memset(buf.p, 0xEE, size_t(total));   // (a byte that nothing writes shows against the model)
    const Store st{buf.p, total, shift == 0};
    for (uint64_t t = 0; t < nt; t++) {
        const uint64_t s = t / kRstoreSectionTiles, so = sec_off[size_t(s)], f0 = first[size_t(t)], f1 = first[size_t(t) + 1], fs = first[size_t(s * kRstoreSectionTiles)];
        const uint32_t i = uint32_t(t % kRstoreSectionTiles), tiles = rstore_section_tiles(nt, s), c = uint32_t(f1 - f0);
        if (i == 0) { st.st32(so, uint32_t(s)); st.st32(so + 4, tiles); st.st32(so + 8, uint32_t(fs)); st.st32(so + 12, uint32_t(fs >> 32)); st.st32(so + 16, 0); }
        st.st32(so + 20 + 4 * i, uint32_t(f1 - fs));
        const uint64_t out = so + tile_off[size_t(t)];
        if (!rstore_dense(c)) {
            for (uint32_t j = 0; j < c + (c & 1); j++) st.st16(out + 2 * j, rstore_sparse_entry(at, f0, c, t, j));
            continue;
        }
        std::vector<uint32_t> bitmap(kRstoreBitmap / 4, 0);
        for (uint32_t j = 0; j < c; j++) {
            const uint64_t rel = at(f0 + j) - (t << kRstoreTileLog);
            if (rel >= kRstoreTile) fail("a delimiter outside its tile", t);
            bitmap[size_t(rel >> 5)] |= 1u << (rel & 31);
        }
        for (uint32_t w = 0; w < kRstoreBitmap / 4; w++) st.st32(out + 4 * w, bitmap[w]);
    }
    h.nsections = uint32_t(ns);
    std::vector<uint8_t> head(size_t(kRstoreDirAt + 4 * ns));
    rstore_put_head(head.data(), h, dir.data());
    std::memcpy(buf.p, head.data(), head.size());
    for (uint64_t s = 0; s < ns; s++) {
        uint8_t* p = buf.p + sec_off[size_t(s)] - 8;
        rstore_chunk_header(p, kRstoreChunkSection, 4 + dir[size_t(s)]);
        rstore_put32(p + 4, rstore_crc(p + 8, dir[size_t(s)]));
    }
    rstore_put_eof(buf.p + pos);
    return std::vector<uint8_t>(buf.p, buf.p + total);
}

// The load path -> 0 and the table, or the code
int load(const uint8_t* blob, uint64_t len, bool aligned, bool ignore_crc, uint64_t size, uint32_t tag, uint32_t chunks, RstoreHeader* hout, std::vector<uint64_t>* table) {
    const uint64_t nt = rstore_ntiles(size), ns = rstore_nsections(size), head_n = kRstoreDirAt + 4 * ns, have = len < head_n ? len : head_n;
    std::vector<uint8_t> head(blob, blob + have);   // what the host fetches: nothing behind `have` is looked at by the parse
    RstoreHeader h{};
    int e = rstore_parse_fixed(head.data(), size_t(have), &h);
    if (e) return e;
    if (h.size != size) return kRstoreErrArg;
    std::vector<RstoreSection> secs(static_cast<size_t>(ns));
    if ((e = rstore_parse_directory(head.data(), size_t(have), len, h, ignore_crc, secs.data()))) return e;
    if ((e = rstore_match(h, size, tag, chunks))) return e;
    const Load L{blob, len, aligned};
    const uint64_t k = h.k;
    table->assign(static_cast<size_t>(k), ~uint64_t(0));   // exactly k entries: a rank beyond is a failure here and a heap overflow under the sanitizer
    RstoreVerdict v{0, 0, 0, 0};
    for (uint64_t s = 0; s < ns; s++) {   // rstore_frames_kernel
        const uint64_t p = secs[size_t(s)].off - 8;
        const uint32_t len24 = uint32_t(L.ld8(p + 1)) | uint32_t(L.ld8(p + 2)) << 8 | uint32_t(L.ld8(p + 3)) << 16;
        if (L.ld8(p) != kRstoreChunkSection || len24 != 4 + secs[size_t(s)].len) v.bad |= kRstoreBadSection;
        if (secs[size_t(s)].off + secs[size_t(s)].len > len) fail("a section outside the blob", s);
        if (!ignore_crc && L.ld32(p + 4) != rstore_crc(blob + secs[size_t(s)].off, size_t(secs[size_t(s)].len))) v.crc_bad = 1;
    }
    {
        const uint64_t eo = len - kRstoreEof;
        if (L.ld8(eo) != 0x20 || L.ld8(eo + 1) != 1 || L.ld8(eo + 2) || L.ld8(eo + 3) || L.ld8(eo + 4)) v.bad |= kRstoreBadSection;
    }
    auto put = [&](uint64_t rank, uint64_t pos) {
        if (rank >= k) fail("a rank beyond k", rank);
        (*table)[size_t(rank)] = pos;
        if (pos + 1 == size) v.last_is_delim = 1;
    };
    const auto ld32 = [&](uint64_t off) { return L.ld32(off); };
    for (uint64_t t = 0; t < nt; t++) {   // rstore_expand_kernel
        const uint64_t s = t / kRstoreSectionTiles;
        const uint32_t i = uint32_t(t % kRstoreSectionTiles), tiles = rstore_section_tiles(nt, s);
        const RstoreSection sec = secs[size_t(s)];
        uint32_t before = 0;
        for (uint32_t j = 0; j < i; j++) before += rstore_count_bytes(L.ld32(sec.off + 16 + 4 * uint64_t(j)), L.ld32(sec.off + 20 + 4 * uint64_t(j)));
        uint64_t next_first = k;
        if (i + 1 == tiles && s + 1 < ns) next_first = uint64_t(L.ld32(secs[size_t(s) + 1].off + 8)) | uint64_t(L.ld32(secs[size_t(s) + 1].off + 12)) << 32;
        const RstoreTilePlan p = rstore_tile_plan(ld32, sec, s, tiles, i, before, next_first, k);
        if (p.bad) { v.bad |= p.bad; continue; }
        const uint64_t t0 = t << kRstoreTileLog;
        const uint32_t limit = size - t0 < kRstoreTile ? uint32_t(size - t0) : kRstoreTile;
        if (!rstore_dense(p.c)) {
            for (uint32_t j = 0; j < p.c + (p.c & 1); j++) {
                const uint32_t val = L.ld16(p.payload + 2 * j), prev = j ? L.ld16(p.payload + 2 * j - 2) : 0;
                v.bad |= rstore_sparse_check(val, prev, j > 0, j == p.c, limit);
                if (j < p.c) put(p.rank + j, t0 + val);
            }
            continue;
        }
        uint32_t pc = 0, r = 0;
        for (uint32_t w = 0; w < kRstoreBitmap / 4; w++) {
            const uint32_t word = L.ld32(p.payload + 4 * w);
            v.bad |= rstore_dense_check(word, w, limit);
            pc += rindex_popcount(word);
        }
        if (pc != p.c) v.bad |= kRstoreBadDense;
        for (uint32_t w = 0; w < kRstoreBitmap / 4; w++)
            for (uint32_t word = L.ld32(p.payload + 4 * w), j = 0; word; j++, word >>= 1)
                if (word & 1u) { if (r < p.c) put(p.rank + r, t0 + 32 * w + j); r++; }
    }
    if (v.crc_bad) return kRstoreErrCrc;
    if (v.bad) return kRstoreErrCorrupt;
    if (h.N != rindex_records(k, size, v.last_is_delim != 0)) return kRstoreErrCorrupt;
    *hout = h;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    In in;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    in.b.resize(size_t(std::ftell(f)));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(in.b.data(), 1, in.b.size(), f) != in.b.size()) return 2;
    std::fclose(f);
    while (in.p < in.b.size()) {
        const uint32_t kind = in.get<uint32_t>();
        if (kind == 1) {
            RstoreHeader h{};
            h.delim = uint8_t(in.get<uint32_t>());
            const uint32_t shift = in.get<uint32_t>() & 3;
            h.flags = in.get<uint32_t>(); h.tag = in.get<uint32_t>(); h.data_chunks = in.get<uint32_t>();
            const uint64_t size = in.get<uint64_t>();
            h.longest = in.get<uint64_t>();
            const uint64_t k = in.get<uint64_t>();
            std::vector<uint64_t> D(static_cast<size_t>(k));
            for (uint64_t& d : D) d = in.get<uint64_t>();
            h.size = size; h.k = k; h.N = rindex_records(k, size, k && D[size_t(k - 1)] == size - 1);
            uint64_t sparse = 0, dense = 0;
            const std::vector<uint8_t> blob = save(D, size, h, shift, &sparse, &dense);
            Shifted again(blob.size(), shift);
            std::memcpy(again.p, blob.data(), blob.size());
            RstoreHeader back{};
            std::vector<uint64_t> table;
            const int e = load(again.p, blob.size(), shift == 0, false, size, h.tag, h.data_chunks, &back, &table);
            if (e) fail("the blob does not load", uint64_t(e));
            if (table != D) fail("the loaded table differs from D", 0);
            if (back.N != h.N || back.delim != h.delim || back.longest != h.longest || back.flags != h.flags) fail("the loaded header differs", 0);
            std::printf("%llu %llu %llu %llu ", (unsigned long long)blob.size(), (unsigned long long)rstore_nsections(size), (unsigned long long)sparse, (unsigned long long)dense);
            for (uint8_t b : blob) std::printf("%02x", b);
            std::printf("\n");
        } else if (kind == 2) {
            const uint32_t shift = in.get<uint32_t>() & 3, flags = in.get<uint32_t>(), tag = in.get<uint32_t>(), chunks = in.get<uint32_t>();
            const uint64_t size = in.get<uint64_t>(), len = in.get<uint64_t>();
            const uint8_t* src = in.bytes(size_t(len));
            Shifted buf(size_t(len), shift);
            std::memcpy(buf.p, src, size_t(len));
            RstoreHeader h{};
            std::vector<uint64_t> table;
            const int e = load(buf.p, len, shift == 0, (flags & 1) != 0, size, tag, chunks, &h, &table);
            if (e) { std::printf("error %d\n", e); continue; }
            std::printf("ok %llu %llu %u %llu :", (unsigned long long)h.N, (unsigned long long)h.k, unsigned(h.delim), (unsigned long long)h.longest);
            for (uint64_t d : table) std::printf(" %llu", (unsigned long long)d);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown record %u\n", kind);
            return 2;
        }
    }
    return 0;
}
