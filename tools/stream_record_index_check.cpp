// stream_record_index_check.cpp — the rules that the record index shares with its kernels (minlz_amd/csrc/mlz_stream_record_index.h), run as
// plain loops for tests/test_stream_record_index_host.py:
//   g++ -O2 -std=c++17 -o sri tools/stream_record_index_check.cpp && ./sri cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 delimiter, shift; u64 size, npos; the decoded bytes; npos u64 positions
//           -> the bytes lie `shift` bytes off a 16-byte boundary.  The count pass as the kernel runs it — per tile 256 lanes in 16 steps, a
//           16-byte block each (rindex_block_at, rindex_block_mask; a read outside the bytes or a vector read that is not aligned ends the
//           program with status 3) —, the tiles' exclusive bases, the emit pass — per step and wavefront the lower lanes' hits, the 64 slot
//           totals summed up in slot order (rindex_slot), every hit stored at its rank (rindex_emit) — compared with a plain loop over the
//           bytes; every whole block's mask compared with a compare per byte; N (rindex_records), every record's span (rindex_span), the
//           positions' numbers (rindex_number):
//           "N k tiles : D ... | off:len ... | numbers ..."
//   kind 2  no payload -> rindex_word_mask against a compare per byte for every delimiter and every word a | b << 8 | b << 16 | a << 24:
//           "words <how many> ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_record_index.h"

namespace {

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

void words() {
    uint64_t n = 0;
    for (uint32_t d = 0; d < 256; d++)
        for (uint32_t a = 0; a < 256; a++)
            for (uint32_t b = 0; b < 256; b++, n++) {
                const uint32_t w = a | b << 8 | b << 16 | a << 24;
                const uint32_t want = (a == d ? 9u : 0u) | (b == d ? 6u : 0u);
                if (mlz::rindex_word_mask(w, mlz::rindex_splat(uint8_t(d))) != want) fail("rindex_word_mask differs from a compare per byte", w);
            }
    std::printf("words %llu ok\n", (unsigned long long)n);
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
    using namespace mlz;
    while (in.p < in.b.size()) {
        const uint32_t kind = in.get<uint32_t>();
        if (kind == 2) { words(); continue; }
        if (kind != 1) { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
        const uint8_t delim = uint8_t(in.get<uint32_t>());
        const uint32_t shift = in.get<uint32_t>() & 15;
        const uint64_t size = in.get<uint64_t>(), npos = in.get<uint64_t>();
        const uint8_t* dp = in.bytes(size_t(size));
        // exactly the bytes, `shift` off a 16-byte boundary (over-aligned storage, so the shift is the misalignment; nothing behind them)
        std::vector<uint8_t> store(size_t(size) + 32);
        uint8_t* base = store.data() + ((16 - (reinterpret_cast<uintptr_t>(store.data()) & 15)) & 15) + shift;
        std::memcpy(base, dp, size_t(size));
        std::vector<uint64_t> pos(static_cast<size_t>(npos), 0);
        for (uint64_t& p : pos) p = in.get<uint64_t>();
        const int64_t mis = int64_t(reinterpret_cast<uintptr_t>(base) & 15), ylo = mis, yhi = mis + int64_t(size);
        if (uint32_t(mis) != shift) fail("the buffer is not where the case wants it", shift);
        const uint8_t* al = base - mis;
        auto byte = [&](int64_t y) {
            if (y < ylo || y >= yhi) fail("a byte read outside the bytes", uint64_t(y));
            return al[y];
        };
        auto vec = [&](int64_t y, uint32_t* v) {
            if (y < ylo || y + 16 > yhi) fail("a vector read outside the bytes", uint64_t(y));
            if ((reinterpret_cast<uintptr_t>(al + y) & 15) != 0) fail("a vector read that is not aligned", uint64_t(y));
            std::memcpy(v, al + y, 16);
            uint32_t want = 0;   // the exact mask, a compare per byte
            for (uint32_t j = 0; j < 16; j++) want |= al[y + j] == delim ? 1u << j : 0u;
            if (rindex_vec_mask(v, rindex_splat(delim)) != want) fail("a block's mask differs from a compare per byte", uint64_t(y));
        };
        const uint64_t ntiles = rindex_tiles(uint64_t(mis), size);
        // count
        const size_t nt = size_t(ntiles);
        std::vector<uint32_t> tile_count(nt), tile_base(nt);
        for (uint64_t t = 0; t < ntiles; t++) {
            uint32_t c = 0;
            for (uint32_t tid = 0; tid < kRindexThreads; tid++)
                for (uint32_t s = 0; s < kRindexSteps; s++) c += rindex_popcount(rindex_block_mask(rindex_block_at(t, s, tid), ylo, yhi, delim, vec, byte));
            tile_count[size_t(t)] = c;
        }
        // scan
        uint64_t total = 0;
        for (uint64_t t = 0; t < ntiles; t++) { tile_base[size_t(t)] = uint32_t(total); total += tile_count[size_t(t)]; }
        // emit: a table of exactly `total` entries, so that a rank beyond it is a heap overflow under the sanitizer and a failure here
        std::vector<uint64_t> table(static_cast<size_t>(total), ~uint64_t(0));
        for (uint64_t t = 0; t < ntiles; t++) {
            static uint32_t m[kRindexSteps][kRindexThreads], below[kRindexSteps][kRindexThreads];
            uint32_t slot[kRindexSlots], slot_base[kRindexSlots];
            for (uint32_t s = 0; s < kRindexSteps; s++)
                for (uint32_t w = 0; w < kRindexWaves; w++) {
                    uint32_t run = 0;   // the wavefront's scan over its 64 lanes
                    for (uint32_t lane = 0; lane < kRindexLanes; lane++) {
                        const uint32_t tid = w * kRindexLanes + lane;
                        m[s][tid] = rindex_block_mask(rindex_block_at(t, s, tid), ylo, yhi, delim, vec, byte);
                        below[s][tid] = run;
                        run += rindex_popcount(m[s][tid]);
                    }
                    slot[rindex_slot(s, w)] = run;
                }
            uint32_t run = 0;
            for (uint32_t q = 0; q < kRindexSlots; q++) { slot_base[q] = run; run += slot[q]; }
            if (run != tile_count[size_t(t)]) fail("the emit pass counts other hits than the count pass", t);
            for (uint32_t s = 0; s < kRindexSteps; s++)
                for (uint32_t tid = 0; tid < kRindexThreads; tid++)
                    rindex_emit(m[s][tid], uint64_t(tile_base[size_t(t)]) + slot_base[rindex_slot(s, tid / kRindexLanes)] + below[s][tid], total, rindex_block_at(t, s, tid),
                                [&](uint64_t rank, int64_t y) {
                                    if (table[size_t(rank)] != ~uint64_t(0)) fail("a rank is given twice", rank);
                                    table[size_t(rank)] = uint64_t(y - ylo);
                                });
        }
        // against a plain loop
        std::vector<uint64_t> plain;
        for (uint64_t x = 0; x < size; x++) if (dp[x] == delim) plain.push_back(x);
        if (plain != table) fail("the table differs from the plain loop's", 0);
        const uint64_t k = total, N = rindex_records(k, size, k && table[size_t(k - 1)] == size - 1);
        auto at = [&](uint64_t j) {
            if (j >= k) fail("a table entry beyond k", j);
            return table[size_t(j)];
        };
        std::printf("%llu %llu %llu :", (unsigned long long)N, (unsigned long long)k, (unsigned long long)ntiles);
        for (uint64_t j = 0; j < k; j++) std::printf(" %llu", (unsigned long long)table[size_t(j)]);
        std::printf(" |");
        for (uint64_t r = 0; r < N; r++) {
            const RindexSpan sp = rindex_span(at, k, size, r);
            std::printf(" %llu:%llu", (unsigned long long)sp.off, (unsigned long long)sp.len);
        }
        const RindexSpan end = rindex_span(at, k, size, N);
        if (end.off != size || end.len != 0) fail("the span one past the last record is not the empty one at the end", N);
        std::printf(" |");
        for (uint64_t p : pos) {
            if (p >= size) { std::printf(" -"); continue; }
            const uint64_t no = rindex_number(at, k, p);
            uint64_t want = 0;
            for (uint64_t x = 0; x < p; x++) want += dp[x] == delim ? 1 : 0;
            if (no != want) fail("a position's number differs from the plain count", p);
            std::printf(" %llu", (unsigned long long)no);
        }
        std::printf("\n");
    }
    return 0;
}
