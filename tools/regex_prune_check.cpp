// regex_prune_check.cpp — the required literals of the regex compiler (minlz_amd/csrc/mlz_regex_compile.h) and the rules that the pruned regex grep
// shares with its kernels (minlz_amd/csrc/mlz_stream_regex_prune.h: widen, the run table, the lanes), run as plain loops for
// tests/test_regex_prune_host.py:
//   g++ -O2 -std=c++17 -o check tools/regex_prune_check.cpp && ./check cases.bin
// The case file is a sequence of little-endian records, one output line each.  Both kinds begin with an expression set:
//   u32 flags (1 = ignore case), n_exprs; n_exprs u32 lengths; the expressions back to back
//   kind 1  the set -> compile; on a refusal "err <code> <expression> <offset>", else the literals with their invariants checked (at most
//           kRegexMaxLiterals, 1 .. kRegexMaxLiteralLen bytes, sorted, none twice, folded under the flag; status 3 otherwise):
//           "lits <folded> <count> : <hex> <hex> ..."
//   kind 2  the set; u32 delimiter; u64 size; the data; u32 chunk bytes; u32 n_groupings, that many u32 chunks per decode group (0: one group);
//           u32 n_takes, per take one byte per chunk (the plan's answer)
//           -> the record index D by a plain loop; per take: regex_widen per taken chunk and regex_widen_take (compared with a plain loop over
//           all pairs); per grouping the widened list is cut into groups, regex_run_table is built and every group's pieces are copied side by
//           side into a heap block of exactly the group's bytes at a misalignment that changes from group to group; the group is marked as
//           regex_mark_runs_kernel's launch does it: regex_bounds over the pieces' extent, the lanes of regex_slices * kRegexThreads records,
//           regex_run_lane_of, regex_lane_result with regex_walk_blocks over the block (compared with regex_walk over the data), the carry
//           through slots g % 2 and (g + 1) % 2, a ballot per 64 lanes ORed into a bitmap of exactly W words by lanes 0 and 32.  Status 3: a
//           word with two writers in one launch, a carry for another record, a piece outside its block, a record that some run holds whole and
//           that no group or more than one finished, a record that no run holds whole and that a lane evaluated, groupings that disagree.
//           "<N> <chunks> | <one 0 / 1 per chunk: the widened set> <one 0 / 1 per record: the bitmap> | ..."  (one pair per take)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

bool compile(In& in, mlz::RegexProgram* pr) {
    const uint32_t flags = in.get<uint32_t>(), n = in.get<uint32_t>();
    std::vector<uint32_t> len(n);
    size_t total = 0;
    for (uint32_t& l : len) { l = in.get<uint32_t>(); total += l; }
    const std::vector<uint8_t> exprs = in.bytes(total);
    uint64_t where[2] = {77, 77};
    const int r = mlz::regex_compile(exprs.data(), len.data(), n, flags, pr, where);
    if (r) { std::printf("err %d %llu %llu", -r, (unsigned long long)where[0], (unsigned long long)where[1]); return false; }
    return true;
}

void literals(In& in) {
    mlz::RegexProgram pr;
    if (!compile(in, &pr)) { std::printf("\n"); return; }
    const std::vector<std::string>& L = pr.literals;
    const bool fold = (pr.flags & mlz::kRegexIgnoreCase) != 0;
    if (L.size() > mlz::kRegexMaxLiterals) fail("too many literals", L.size());
    for (size_t i = 0; i < L.size(); i++) {
        if (L[i].empty() || L[i].size() > mlz::kRegexMaxLiteralLen) fail("a literal's length", i);
        if (i && !(L[i - 1] < L[i])) fail("the literals are not sorted", i);
        if (fold) for (char ch : L[i]) if (mlz::regex_lit_fold(uint8_t(ch)) != uint8_t(ch)) fail("a literal that is not folded", i);
    }
    std::printf("lits %d %zu :", int(fold), L.size());
    for (const std::string& l : L) {
        std::printf(" ");
        for (char ch : l) std::printf("%02x", unsigned(uint8_t(ch)));
    }
    std::printf("\n");
}

// A group's bytes as a region of memory whose first byte is `mis` bytes behind a 16-byte boundary: a heap block of exactly `used` bytes
struct Block {
    std::vector<uint8_t> heap;
    int64_t mis;
    uint32_t walk(const mlz::RegexProgram& pr, uint64_t from, uint64_t to, uint32_t state) const {   // over the block's bytes [from, to)
        const uint8_t* base = heap.data();
        const int64_t m = mis;
        return mlz::regex_walk_blocks(pr.next.data(), pr.cmap, pr.C,
                                      [&](int64_t y, uint32_t* v) { std::memcpy(v, base + (y - m), 16); },
                                      [&](int64_t y) { return base[y - m]; }, m, m + int64_t(heap.size()), int64_t(from) + m, int64_t(to) + m, state);
    }
};

void marks(In& in) {
    using namespace mlz;
    RegexProgram pr;
    const bool ok = compile(in, &pr);
    const uint8_t delim = uint8_t(in.get<uint32_t>());
    const uint64_t size = in.get<uint64_t>();
    const std::vector<uint8_t> data = in.bytes(size_t(size));
    const uint32_t cbytes = in.get<uint32_t>(), n_groupings = in.get<uint32_t>();
    std::vector<uint32_t> groupings(n_groupings);
    for (uint32_t& g : groupings) g = in.get<uint32_t>();
    const size_t nck = cbytes ? size_t((size + cbytes - 1) / cbytes) : 0;
    const uint32_t n_takes = in.get<uint32_t>();
    std::vector<std::vector<uint8_t>> takes(n_takes);
    for (auto& t : takes) t = in.bytes(nck);
    if (!ok) { std::printf("\n"); return; }
    auto off_of = [&](size_t c) { return uint64_t(c) * cbytes; };
    auto n_of = [&](size_t c) { return std::min<uint64_t>(cbytes, size - off_of(c)); };
    std::vector<uint64_t> D;
    for (uint64_t p = 0; p < size; p++) if (data[size_t(p)] == delim) D.push_back(p);
    const uint64_t k = D.size(), N = rindex_records(k, size, k && D[size_t(k - 1)] == size - 1), W = grep_words(N);
    auto at = [&](uint64_t j) {
        if (j >= k) fail("a table entry beyond k", j);
        return D[size_t(j)];
    };
    std::printf("%llu %zu", (unsigned long long)N, nck);
    for (const std::vector<uint8_t>& plan : takes) {
        // widen: the rule per taken chunk, the one pass of regex_widen_take against all pairs
        std::vector<uint8_t> take = plan, pairs = plan;
        std::vector<RegexWiden> spans;
        for (size_t c = 0; c < nck; c++) {
            if (!plan[c]) continue;
            const RegexWiden w = regex_widen(at, k, size, RegexTaken{off_of(c), off_of(c) + n_of(c) - 1});
            if (w.start > off_of(c) || w.end > size || w.start > w.end) fail("a widened span", c);
            spans.push_back(w);
            for (size_t j = 0; j < nck; j++) if (off_of(j) < w.end && off_of(j) + n_of(j) > w.start) pairs[j] = 1;
        }
        size_t n_wide = regex_widen_take(nck, off_of, n_of, spans.data(), spans.size(), &take), n_pairs = 0;
        for (size_t j = 0; j < nck; j++) n_pairs += pairs[j] ? 1 : 0;
        if (take != pairs || n_wide != n_pairs) fail("regex_widen_take differs from all pairs", n_wide);
        std::vector<size_t> list;
        for (size_t c = 0; c < nck; c++) if (take[c]) list.push_back(c);
        // which records some run holds whole, by a plain loop over the maximal runs
        std::vector<uint8_t> whole(size_t(N), 0);
        for (size_t i = 0; i < list.size();) {
            size_t j = i;
            while (j + 1 < list.size() && list[j + 1] == list[j] + 1) j++;
            const uint64_t first = off_of(list[i]), end = off_of(list[j]) + n_of(list[j]);
            for (uint64_t r = 0; r < N; r++) {
                const RindexSpan sp = rindex_span(at, k, size, r);
                if (first <= sp.off && sp.off < end && sp.off + sp.len <= end) whole[size_t(r)] = 1;
            }
            i = j + 1;
        }
        std::string bitmap_of_first;
        for (size_t gi = 0; gi < groupings.size(); gi++) {
            std::vector<size_t> gend;
            for (size_t i = 0; i < list.size();) { i = groupings[gi] ? std::min(list.size(), i + groupings[gi]) : list.size(); gend.push_back(i); }
            const RegexRunTable rt = regex_run_table(list.size(), gend, [&](size_t i) { return off_of(list[i]); }, [&](size_t i) { return n_of(list[i]); });
            if (rt.groups.size() != gend.size()) fail("the run table's groups", gi);
            std::vector<uint32_t> sel(static_cast<size_t>(W), 0);   // exactly W words
            std::vector<uint32_t> finished(static_cast<size_t>(N), 0);
            RegexCarry slot[2] = {{~uint64_t(0), 0, 0}, {~uint64_t(0), 0, 0}};
            uint64_t prev_hi = 0;
            for (size_t g = 0, i0 = 0; g < gend.size(); i0 = gend[g++]) {
                const RegexRunGroup& gr = rt.groups[g];
                if (gr.r1 <= gr.r0) fail("a group without a piece", g);
                const uint32_t n_runs = uint32_t(gr.r1 - gr.r0);
                auto run_at = [&](uint32_t j) {
                    if (j >= n_runs) fail("a piece beyond the group's table", j);
                    return rt.runs[gr.r0 + j];
                };
                Block blk{std::vector<uint8_t>(size_t(gr.used)), int64_t((g * 5 + 3) & 15)};
                for (size_t i = i0; i < gend[g]; i++) {
                    if (rt.at[i] + n_of(list[i]) > gr.used) fail("a chunk outside its group's bytes", i);
                    std::memcpy(blk.heap.data() + rt.at[i], data.data() + off_of(list[i]), size_t(n_of(list[i])));
                }
                for (uint32_t j = 0; j < n_runs; j++) {
                    const RegexRun p = run_at(j);
                    if (p.first >= p.end || p.at + (p.end - p.first) > gr.used || (j && run_at(j - 1).end >= p.first)) fail("a piece of a run", j);
                    if (std::memcmp(blk.heap.data() + p.at, data.data() + p.first, size_t(p.end - p.first))) fail("a piece's bytes are not where the table says", j);
                }
                if (gr.head_first > run_at(0).first || gr.tail_end < run_at(n_runs - 1).end) fail("the group's head or tail", g);
                const RegexGroup extent{run_at(0).first, run_at(n_runs - 1).end - run_at(0).first};
                const RegexBounds b = regex_bounds(at, k, extent);
                if (b.r_lo > b.r_hi || b.r_hi >= N || (g && b.r_lo < prev_hi)) fail("a group's records", g);
                prev_hi = b.r_hi;
                const RegexCarry in_slot = slot[g & 1];
                std::vector<uint32_t> writers(static_cast<size_t>(W), 0);
                const uint64_t lanes = regex_slices(b) * kRegexThreads;
                if (regex_lane_record(b, lanes - 1) < b.r_hi || regex_lane_record(b, 0) > b.r_lo) fail("the launch does not cover the group's records", g);
                for (uint64_t w0 = 0; w0 < lanes; w0 += kRegexLanes) {   // a wavefront
                    uint64_t ballot = 0;
                    for (uint32_t lane = 0; lane < kRegexLanes; lane++) {
                        const uint64_t r = regex_lane_record(b, w0 + lane);
                        if (r < b.r_lo || r > b.r_hi) continue;   // an idle lane
                        const RindexSpan sp = rindex_span(at, k, size, r);
                        const RegexRunLane rl = regex_run_lane_of(run_at, n_runs, gr.head_first, gr.tail_end, sp.off, sp.off + sp.len);
                        if (!rl.active) continue;
                        if (!whole[size_t(r)]) fail("a lane evaluates a record that no run holds whole", r);
                        const RegexRun p = run_at(rl.piece);
                        const RegexLane ln = rl.lane;
                        if (ln.crossed_in && in_slot.rec != r) fail("a carry for another record", r);
                        if (ln.from < p.first || ln.to > p.end || ln.from > ln.to) fail("a lane leaves its piece", r);
                        const RegexLaneOut out = regex_lane_result(ln, r, in_slot, pr.start, pr.C, pr.end_hi,
                                                                   [&](uint64_t from, uint64_t to, uint32_t st) { return blk.walk(pr, p.at + (from - p.first), p.at + (to - p.first), st); });
                        const RegexLaneOut plain = regex_lane_result(ln, r, in_slot, pr.start, pr.C, pr.end_hi, [&](uint64_t from, uint64_t to, uint32_t st) {
                            return regex_walk(pr.next.data(), pr.cmap, pr.C, [&](uint64_t q) { return data[size_t(q)]; }, from, to, st);
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
            }
            std::string bitmap;
            for (uint64_t r = 0; r < N; r++) {
                if (finished[size_t(r)] != (whole[size_t(r)] ? 1u : 0u)) fail("a record that a run holds whole was finished by no group or by two", r);
                bitmap.push_back(char('0' + ((sel[size_t(r / 32)] >> (r % 32)) & 1)));
            }
            if (gi == 0) bitmap_of_first = bitmap;
            else if (bitmap != bitmap_of_first) fail("two groupings disagree", gi);
        }
        std::printf(" | ");
        for (size_t c = 0; c < nck; c++) std::putchar('0' + take[c]);
        std::printf(" %s", bitmap_of_first.c_str());
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
        if (kind == 1) literals(in);
        else if (kind == 2) marks(in);
        else { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
    }
    return 0;
}
