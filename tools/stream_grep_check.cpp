// stream_grep_check.cpp — the rules that the grep over the record index shares with its kernels (minlz_amd/csrc/mlz_stream_grep.h), run as plain
// loops for tests/test_stream_grep_host.py:
//   g++ -O2 -std=c++17 -o sgc tools/stream_grep_check.cpp && ./sgc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 flags (16 = invert), tile; u64 size, k, npos, before, after, rec_cap; k u64 delimiter positions (D); npos u64 occurrence positions
//           -> mark: the positions are cut into tiles of `tile` start positions; per tile grep_narrow of its first and last position, per
//           occurrence grep_number_between, compared with the full bisection (rindex_number) and with a plain count of the delimiters in
//           front (a table entry beyond k, or outside a tile's two numbers, ends the program with status 3); the bit is tested before it is set.
//           select: grep_select_word in place.  Scans: as the kernel runs them — 1024 lanes, a slab of words each (grep_slab), the lanes' keys
//           scanned forwards and in reverse — compared with one plain loop over the words in either direction.  Context: grep_context_word
//           compared, record by record, with the contract's own words (the nearest selected record at or below within `after`, at or above
//           within `before`).  Compact: the popcounts' exclusive prefix, grep_emit_word into arrays of exactly min(R, rec_cap) entries (a
//           rank beyond them is a heap overflow under the sanitizer and a failure here), the two byte sums compared with rindex_span sums:
//           "R S written bytes atomics : numbers ... | kinds ..."   (atomics: how many bits the mark pass set = |M|)
//   kind 2  no payload -> grep_smear_up / grep_smear_down against an OR of single shifts for every n <= 31 and a set of words; grep_valid_bits:
//           "smear ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_grep.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
};

[[noreturn]] void fail(const char* what, uint64_t i) {
    std::fprintf(stderr, "%s (at %llu)\n", what, (unsigned long long)i);
    std::exit(3);
}

void smear() {
    using namespace mlz;
    const uint32_t words[] = {0, 1, 0x80000000u, 0x00010000u, 0x80000001u, 0xdeadbeefu, 0x00100400u, ~uint32_t(0), 0x40000002u};
    for (uint32_t x : words)
        for (uint32_t n = 0; n <= 31; n++) {
            uint32_t up = 0, down = 0;
            for (uint32_t j = 0; j <= n; j++) { up |= x << j; down |= x >> j; }
            if (grep_smear_up(x, n) != up || grep_smear_down(x, n) != down) fail("a smear differs from the OR of its shifts", n);
        }
    if (grep_valid_bits(0, 0) != 0 || grep_valid_bits(0, 1) != 1 || grep_valid_bits(0, 32) != ~uint32_t(0) || grep_valid_bits(1, 32) != 0 || grep_valid_bits(1, 33) != 1 ||
        grep_valid_bits(0, 31) != 0x7fffffffu || grep_valid_bits(2, 64) != 0)
        fail("grep_valid_bits", 0);
    std::printf("smear ok\n");
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
        if (kind == 2) { smear(); continue; }
        if (kind != 1) { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
        const uint32_t flags = in.get<uint32_t>(), tile = in.get<uint32_t>();
        const uint64_t size = in.get<uint64_t>(), k = in.get<uint64_t>(), npos = in.get<uint64_t>(), before_in = in.get<uint64_t>(), after_in = in.get<uint64_t>(),
                       rec_cap = in.get<uint64_t>();
        if (tile == 0) return 2;
        std::vector<uint64_t> D(static_cast<size_t>(k), 0), pos(static_cast<size_t>(npos), 0);
        for (uint64_t& d : D) d = in.get<uint64_t>();
        for (uint64_t& p : pos) p = in.get<uint64_t>();
        const uint64_t N = rindex_records(k, size, k && D[size_t(k - 1)] == size - 1), W = grep_words(N);
        if (N >= kGrepMaxRecords) return 2;
        const bool invert = (flags & kGrepInvert) != 0;
        const uint64_t before = grep_clamp(before_in, N), after = grep_clamp(after_in, N);
        auto at = [&](uint64_t j) {
            if (j >= k) fail("a table entry beyond k", j);
            return D[size_t(j)];
        };
        // mark
        std::vector<uint32_t> sel(static_cast<size_t>(W), 0);   // exactly W words: a bit beyond N's word is a heap overflow
        uint64_t atomics = 0, plain = 0;
        for (size_t i = 0; i < pos.size();) {
            const uint64_t t0 = pos[i] / tile * tile, t1 = t0 + tile - 1 < size - 1 ? t0 + tile - 1 : size - 1;   // the tile's first and last start position
            const GrepNarrow nr = grep_narrow(at, k, t0, t1);
            auto between = [&](uint64_t j) {
                if (j < nr.lo || j >= nr.hi) fail("a table entry outside the tile's two numbers", j);
                return at(j);
            };
            for (; i < pos.size() && pos[i] <= t1; i++) {
                const uint64_t p = pos[i];
                if (p >= size || p < t0) fail("the occurrences do not ascend inside the stream", p);
                const uint64_t r = grep_number_between(between, nr, p);
                if (r != rindex_number(at, k, p)) fail("the narrowed bisection differs from the full one", p);
                while (plain < k && D[size_t(plain)] < p) plain++;   // (the occurrences ascend: the count goes on from the one before)
                if (r != plain) fail("a position's number differs from the plain count", p);
                if (r >= N) fail("a record number beyond N", p);
                const uint32_t bit = 1u << (uint32_t(r) & 31);
                if (!(sel[size_t(r >> 5)] & bit)) { sel[size_t(r >> 5)] |= bit; atomics++; }
            }
        }
        std::vector<uint8_t> inM(static_cast<size_t>(N), 0);
        for (uint64_t r = 0; r < N; r++) inM[size_t(r)] = uint8_t((sel[size_t(r >> 5)] >> (r & 31)) & 1u);
        // select
        for (uint64_t w = 0; w < W; w++) sel[size_t(w)] = grep_select_word(sel[size_t(w)], w, N, invert);
        for (uint64_t r = 0; r < N; r++)
            if (((sel[size_t(r >> 5)] >> (r & 31)) & 1u) != (invert ? 1u - inM[size_t(r)] : inM[size_t(r)])) fail("S is not M or its complement", r);
        if (W && (sel[size_t(W - 1)] & ~grep_valid_bits(W - 1, N))) fail("a bit at or beyond N is selected", N);
        // scans, as the kernel: per lane the keys of its slab, the lanes scanned forwards and in reverse, then along the slab
        std::vector<uint32_t> below(static_cast<size_t>(W), 0), above(static_cast<size_t>(W), 0);
        {
            std::vector<uint32_t> last(kGrepScanThreads, 0), first(kGrepScanThreads, 0);
            for (uint32_t tid = 0; tid < kGrepScanThreads; tid++) {
                const GrepSlab sl = grep_slab(W, tid);
                if (sl.b > sl.e || sl.e > W || (tid + 1 == kGrepScanThreads && sl.e != W)) fail("the slabs do not cover the words", tid);
                for (uint64_t w = sl.b; w < sl.e; w++) {
                    const uint32_t lk = grep_last_key(sel[size_t(w)], w), fk = grep_first_key(sel[size_t(w)], w, N);
                    if (lk > last[tid]) last[tid] = lk;
                    if (fk > first[tid]) first[tid] = fk;
                }
            }
            uint32_t run = 0;
            for (uint32_t tid = 0; tid < kGrepScanThreads; tid++) {
                const GrepSlab sl = grep_slab(W, tid);
                uint32_t b = run;
                for (uint64_t w = sl.b; w < sl.e; w++) {
                    below[size_t(w)] = b;
                    const uint32_t lk = grep_last_key(sel[size_t(w)], w);
                    if (lk > b) b = lk;
                }
                if (last[tid] > run) run = last[tid];
            }
            run = 0;
            for (uint32_t tid = kGrepScanThreads; tid-- > 0;) {
                const GrepSlab sl = grep_slab(W, tid);
                uint32_t a = run;
                for (uint64_t w = sl.e; w > sl.b; w--) {
                    above[size_t(w - 1)] = a;
                    const uint32_t fk = grep_first_key(sel[size_t(w - 1)], w - 1, N);
                    if (fk > a) a = fk;
                }
                if (first[tid] > run) run = first[tid];
            }
            uint32_t b = 0, a = 0;   // one plain loop in either direction
            for (uint64_t w = 0; w < W; w++) {
                if (below[size_t(w)] != b) fail("the forward scan differs from the plain loop", w);
                const uint32_t lk = grep_last_key(sel[size_t(w)], w);
                if (lk > b) b = lk;
            }
            for (uint64_t w = W; w > 0; w--) {
                if (above[size_t(w - 1)] != a) fail("the backward scan differs from the plain loop", w - 1);
                const uint32_t fk = grep_first_key(sel[size_t(w - 1)], w - 1, N);
                if (fk > a) a = fk;
            }
        }
        // context, against the contract's words
        std::vector<uint32_t> ctx(static_cast<size_t>(W), 0), rank(static_cast<size_t>(W), 0);
        for (uint64_t w = 0; w < W; w++) ctx[size_t(w)] = grep_context_word(sel[size_t(w)], w, below[size_t(w)], above[size_t(w)], before, after, N);
        {
            std::vector<uint8_t> want(static_cast<size_t>(N), 0);
            bool have = false;
            uint64_t near = 0;
            for (uint64_t r = 0; r < N; r++) {   // the nearest selected record at or below
                if ((sel[size_t(r >> 5)] >> (r & 31)) & 1u) { have = true; near = r; }
                if (have && r - near <= after_in) want[size_t(r)] = 1;
            }
            have = false;
            for (uint64_t r = N; r-- > 0;) {   // ... and at or above
                if ((sel[size_t(r >> 5)] >> (r & 31)) & 1u) { have = true; near = r; }
                if (have && near - r <= before_in) want[size_t(r)] = 1;
            }
            for (uint64_t r = 0; r < N; r++)
                if (((ctx[size_t(r >> 5)] >> (r & 31)) & 1u) != want[size_t(r)]) fail("a context bit differs from the contract", r);
            if (W && (ctx[size_t(W - 1)] & ~grep_valid_bits(W - 1, N))) fail("a context bit at or beyond N", N);
        }
        // compact
        uint64_t R = 0, S = 0;
        for (uint64_t w = 0; w < W; w++) { rank[size_t(w)] = uint32_t(R); R += rindex_popcount(ctx[size_t(w)]); S += rindex_popcount(sel[size_t(w)]); }
        const uint64_t kk = R < rec_cap ? R : rec_cap;
        std::vector<uint64_t> no(static_cast<size_t>(kk), ~uint64_t(0));
        std::vector<uint8_t> kinds(static_cast<size_t>(kk), 0xff);
        uint64_t written = 0, bytes = 0;
        for (uint64_t w = 0; w < W; w++)
            grep_emit_word(ctx[size_t(w)], sel[size_t(w)], w, rank[size_t(w)], rec_cap, [&](uint64_t r) { return rindex_span(at, k, size, r).len; },
                           [&](uint64_t a, uint64_t r, uint8_t kind) {
                               if (a >= kk) fail("a rank beyond the cap", a);
                               if (no[size_t(a)] != ~uint64_t(0)) fail("a rank is given twice", a);
                               no[size_t(a)] = r; kinds[size_t(a)] = kind;
                           }, &written, &bytes);
        uint64_t want_written = 0, want_bytes = 0, seen = 0;
        for (uint64_t r = 0; r < N; r++)
            if ((ctx[size_t(r >> 5)] >> (r & 31)) & 1u) {
                const uint64_t l = rindex_span(at, k, size, r).len;
                want_bytes += l;
                if (seen < kk) {
                    want_written += l;
                    if (no[size_t(seen)] != r) fail("the written numbers are not the smallest members in ascending order", seen);
                }
                seen++;
            }
        if (written != want_written || bytes != want_bytes) fail("the byte sums differ from the spans'", R);
        std::printf("%llu %llu %llu %llu %llu :", (unsigned long long)R, (unsigned long long)S, (unsigned long long)written, (unsigned long long)bytes, (unsigned long long)atomics);
        for (uint64_t j = 0; j < kk; j++) std::printf(" %llu", (unsigned long long)no[size_t(j)]);
        std::printf(" |");
        for (uint64_t j = 0; j < kk; j++) std::printf(" %u", unsigned(kinds[size_t(j)]));
        std::printf("\n");
    }
    return 0;
}
