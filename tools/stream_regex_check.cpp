// stream_regex_check.cpp — the compiler of regular expressions (minlz_amd/csrc/mlz_regex_compile.h) and the rules that the grep for them shares
// with its kernels (minlz_amd/csrc/mlz_stream_regex.h), run as plain loops for tests/test_stream_regex_host.py:
//   g++ -O2 -std=c++17 -o src tools/stream_regex_check.cpp && ./src cases.bin
// The case file is a sequence of little-endian records, one output line each.  Both kinds begin with an expression set:
//   u32 flags (1 = ignore case), n_exprs; n_exprs u32 lengths; the expressions back to back
//   kind 1  the set; u32 has_alphabet, 4 bytes; u32 n_strings; per string u32 length and its bytes
//           -> compile; on a refusal "err <code> <expression> <offset>".  Else every string over the alphabet of length 0 .. 6 (has_alphabet; in
//           the order of a base-4 counter per length, the first byte the most significant) and then every listed string is tested three ways,
//           which must agree (else status 3): regex_test; regex_walk_blocks over a heap copy of exactly the string's bytes at each of the
//           misalignments 0, 1, 7 and 15 (a read outside the copy is a heap overflow under the sanitizer); the table's own invariants are
//           checked once (dead's row 0, matched's row C, entries below S C and multiples of C, the class map below C, the image size).
//           "ok <S> <C> <image bytes> <empty> : <one 0 / 1 per string>"
//   kind 2  the set; u32 delimiter; u64 size; the data; u32 n_cuts; n_cuts u64 group sizes (0: one group)
//           -> the record index D by a plain loop; per cut the data is cut into groups of that many bytes, each copied to a heap block of its
//           own at a misalignment that changes from group to group, and marked as the kernel's launch does it: regex_bounds, the lanes of
//           regex_slices * kRegexThreads records from regex_launch_base, regex_run_lane with regex_walk_blocks (compared with regex_walk over the
//           whole data), the carry through slots g % 2 and (g + 1) % 2, a ballot per 64 lanes, its halves ORed into a bitmap of exactly W words
//           by lanes 0 and 32.  Status 3: a word with two writers in one launch, a carry for another record, a lane that is not idle outside
//           [r_lo, r_hi], a record that no group finished or two did.
//           "<N> <longest> | <one 0 / 1 per record> | ..."  (one bitmap per cut; longest = regex_longest)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_regex_compile.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    std::vector<uint8_t> bytes(size_t n) {
        if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
        std::vector<uint8_t> v(b.begin() + p, b.begin() + p + n);
        p += n;
        return v;
    }
};

[[noreturn]] void fail(const char* what, uint64_t i) {
    std::fprintf(stderr, "%s (at %llu)\n", what, (unsigned long long)i);
    std::exit(3);
}

// The bytes [0, n) of `data` as a region of memory whose first byte is `mis` bytes behind a 16-byte boundary: a heap block of exactly n bytes
struct Region {
    std::vector<uint8_t> heap;
    int64_t mis;
    Region(const uint8_t* data, size_t n, uint32_t mis_) : heap(data, data + n), mis(mis_) {}
    int64_t ylo() const { return mis; }
    int64_t yhi() const { return mis + int64_t(heap.size()); }
    uint32_t walk(const mlz::RegexProgram& pr, uint64_t from, uint64_t to, uint32_t state) const {   // over the region's bytes [from, to)
        const uint8_t* base = heap.data();
        const int64_t m = mis;
        return mlz::regex_walk_blocks(pr.next.data(), pr.cmap, pr.C,
                                      [&](int64_t y, uint32_t* v) { std::memcpy(v, base + (y - m), 16); },
                                      [&](int64_t y) { return base[y - m]; }, ylo(), yhi(), int64_t(from) + m, int64_t(to) + m, state);
    }
};

void invariants(const mlz::RegexProgram& pr) {
    const uint32_t S = pr.S, C = pr.C;
    if (S < 2 || S > mlz::kRegexMaxStates || C < 1 || C > 256 || pr.next.size() != size_t(S) * C) fail("the table's shape", S);
    if (pr.image_bytes() > mlz::kRegexLdsMax || pr.image_bytes() % 16 || pr.image_bytes() < 256 + S * C * 2) fail("the image size", pr.image_bytes());
    for (uint32_t b = 0; b < 256; b++) if (pr.cmap[b] >= C) fail("a class beyond C", b);
    for (size_t i = 0; i < pr.next.size(); i++) if (pr.next[i] % C || pr.next[i] >= S * C) fail("an entry that is no state", i);
    for (uint32_t c = 0; c < C; c++) if (pr.next[c] != 0 || pr.next[C + c] != C) fail("dead or matched leaves", c);
    if (pr.start % C || pr.start >= S * C || pr.end_hi != (2 + pr.n_end) * C || pr.end_hi > S * C) fail("the start or the end-accepting range", pr.start);
    if (pr.empty_ok != (mlz::regex_verdict(pr.start, true, C, pr.end_hi) != 0)) fail("empty_ok", 0);
}

int test_string(const mlz::RegexProgram& pr, const uint8_t* s, size_t n, uint64_t which) {
    const int v = mlz::regex_test(pr, s, n);
    for (uint32_t mis : {0u, 1u, 7u, 15u}) {
        const Region rg(s, n, mis);
        if (int(mlz::regex_verdict(rg.walk(pr, 0, n, pr.start), true, pr.C, pr.end_hi)) != v) fail("the block walk differs from the byte walk", which);
    }
    return v;
}

bool compile(In& in, mlz::RegexProgram* pr) {
    const uint32_t flags = in.get<uint32_t>(), n = in.get<uint32_t>();
    std::vector<uint32_t> len(n);
    size_t total = 0;
    for (uint32_t& l : len) { l = in.get<uint32_t>(); total += l; }
    const std::vector<uint8_t> exprs = in.bytes(total);
    uint64_t where[2] = {77, 77};
    const int r = mlz::regex_compile(exprs.data(), len.data(), n, flags, pr, where);
    if (r) { std::printf("err %d %llu %llu", -r, (unsigned long long)where[0], (unsigned long long)where[1]); return false; }
    invariants(*pr);
    return true;
}

void strings(In& in) {
    mlz::RegexProgram pr;
    const bool ok = compile(in, &pr);
    const uint32_t has_alphabet = in.get<uint32_t>();
    const std::vector<uint8_t> alphabet = in.bytes(4);
    const uint32_t n = in.get<uint32_t>();
    std::vector<std::vector<uint8_t>> listed(n);
    for (auto& s : listed) { const uint32_t l = in.get<uint32_t>(); s = in.bytes(l); }
    if (!ok) { std::printf("\n"); return; }
    std::printf("ok %u %u %u %d : ", pr.S, pr.C, pr.image_bytes(), int(pr.empty_ok));
    uint64_t which = 0;
    if (has_alphabet)
        for (uint32_t l = 0; l <= 6; l++)
            for (uint32_t v = 0; v < (1u << (2 * l)); v++) {
                uint8_t s[6] = {0, 0, 0, 0, 0, 0};
                for (uint32_t i = 0; i < l; i++) s[i] = alphabet[(v >> (2 * (l - 1 - i))) & 3];
                std::putchar('0' + test_string(pr, s, l, which++));
            }
    for (const auto& s : listed) std::putchar('0' + test_string(pr, s.data(), s.size(), which++));
    std::printf("\n");
}

void groups(In& in) {
    using namespace mlz;
    RegexProgram pr;
    const bool ok = compile(in, &pr);
    const uint8_t delim = uint8_t(in.get<uint32_t>());
    const uint64_t size = in.get<uint64_t>();
    const std::vector<uint8_t> data = in.bytes(size_t(size));
    const uint32_t n_cuts = in.get<uint32_t>();
    std::vector<uint64_t> cuts(n_cuts);
    for (uint64_t& c : cuts) c = in.get<uint64_t>();
    if (!ok) { std::printf("\n"); return; }
    std::vector<uint64_t> D;
    for (uint64_t p = 0; p < size; p++) if (data[size_t(p)] == delim) D.push_back(p);
    const uint64_t k = D.size(), N = rindex_records(k, size, k && D[size_t(k - 1)] == size - 1), W = grep_words(N);
    auto at = [&](uint64_t j) {
        if (j >= k) fail("a table entry beyond k", j);
        return D[size_t(j)];
    };
    uint64_t longest = 0;
    for (uint64_t r = 0; r < N; r++) longest = std::max(longest, rindex_span(at, k, size, r).len);
    if (regex_longest(at, k, size) != longest) fail("regex_longest", longest);
    std::printf("%llu %llu", (unsigned long long)N, (unsigned long long)longest);
    for (uint64_t cut : cuts) {
        std::vector<uint32_t> sel(static_cast<size_t>(W), 0);   // exactly W words
        std::vector<uint32_t> finished(static_cast<size_t>(N), 0);
        RegexCarry slot[2] = {{~uint64_t(0), 0, 0}, {~uint64_t(0), 0, 0}};
        uint64_t g = 0;
        for (uint64_t first = 0; first < size; g++) {
            const RegexGroup gr{first, cut && cut < size - first ? cut : size - first};
            const Region rg(data.data() + first, size_t(gr.n), uint32_t((g * 5 + 3) & 15));
            const RegexBounds b = regex_bounds(at, k, gr);
            if (b.r_lo > b.r_hi || b.r_hi >= N) fail("a group's records", g);
            const RegexCarry in_slot = slot[g & 1];
            std::vector<uint32_t> writers(static_cast<size_t>(W), 0);
            const uint64_t lanes = regex_slices(b) * kRegexThreads;
            if (regex_lane_record(b, lanes - 1) < b.r_hi || regex_lane_record(b, 0) > b.r_lo) fail("the launch does not cover the group's records", g);
            for (uint64_t w0 = 0; w0 < lanes; w0 += kRegexLanes) {   // a wavefront
                uint64_t ballot = 0;
                for (uint32_t lane = 0; lane < kRegexLanes; lane++) {
                    const uint64_t r = regex_lane_record(b, w0 + lane);
                    if (r < b.r_lo || r > b.r_hi) continue;   // an idle lane
                    const RegexLane ln = regex_lane(at, k, size, gr, r);
                    if (ln.crossed_in && in_slot.rec != r) fail("a carry for another record", r);
                    if (ln.from < gr.first || ln.to > gr.first + gr.n || ln.from > ln.to) fail("a lane leaves its group", r);
                    const RegexLaneOut out = regex_run_lane(at, k, size, gr, r, in_slot, pr.start, pr.C, pr.end_hi,
                                                            [&](uint64_t from, uint64_t to, uint32_t st) { return rg.walk(pr, from - gr.first, to - gr.first, st); });
                    const RegexLaneOut plain = regex_run_lane(at, k, size, gr, r, in_slot, pr.start, pr.C, pr.end_hi, [&](uint64_t from, uint64_t to, uint32_t st) {
                        return regex_walk(pr.next.data(), pr.cmap, pr.C, [&](uint64_t p) { return data[size_t(p)]; }, from, to, st);
                    });
                    if (out.finished != plain.finished || out.verdict != plain.verdict || out.carry.state != plain.carry.state) fail("the block walk differs from the byte walk", r);
                    if (out.finished) {
                        finished[size_t(r)]++;
                        if (out.verdict) ballot |= uint64_t(1) << lane;
                    } else {
                        if (r != b.r_hi) fail("a record in front of the group's last goes on", r);
                        slot[(g + 1) & 1] = out.carry;
                    }
                }
                const uint64_t wave_first = regex_lane_record(b, w0);
                for (uint32_t half = 0; half < 2; half++) {
                    const uint32_t bits = uint32_t(ballot >> (32 * half));
                    const uint64_t w = regex_word(wave_first, half);
                    if (!bits) continue;
                    if (w >= W) fail("a word beyond the bitmap", w);
                    sel[size_t(w)] |= bits;
                    if (++writers[size_t(w)] > 1) fail("a word with two writers in one launch", w);
                }
            }
            first += gr.n;
        }
        std::printf(" | ");
        for (uint64_t r = 0; r < N; r++) {
            if (finished[size_t(r)] != 1) fail("a record that no group finished, or two did", r);
            std::putchar('0' + ((sel[size_t(r / 32)] >> (r % 32)) & 1));
        }
    }
    std::printf("\n");
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
        if (kind == 1) strings(in);
        else if (kind == 2) groups(in);
        else { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
    }
    return 0;
}
