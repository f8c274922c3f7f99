// stream_ranges_check.cpp — the plan of the device-resident ReadSeeker's range read, on the host (no GPU): runs the library's own planner
// (minlz_amd/csrc/mlz_stream_ranges.h) and EXECUTES the plan with memcpy: every touched compressed chunk's bytes to its planned place (the
// destination image, or a scratch image of the planned size that is overwritten with garbage between two groups), then the group's
// segments.  tests/test_stream_ranges_host.py compares the result with a brute-force model.
//
//   g++ -O2 -std=c++17 -o src tools/stream_ranges_check.cpp && ./src cases.bin
// cases.bin, per case, little-endian u64s: n_chunks, n_ranges, dst_cap, flags (1 = plan only: no byte images; 2 = the chunks and bytes of the
// case before, none follow), then per chunk (decoded length, type), per range (off, len, dst_off), and unless flags & 1 the decoded bytes of the
// stream (the sum of the lengths).
// One line per case: `<rc> <touched chunks> <scratch bytes> <largest scratch extent> <groups> <segments> <crc32 of the destination image>`;
// the image starts as dst_cap bytes of 0xa5 (plan only: the last three are the planner's figures and 0).  rc < 0: the planner's refusal.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_ranges.h"

using namespace mlz;

namespace {

uint32_t crc32_ieee(const uint8_t* p, size_t n) {   // zlib.crc32
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
            tab[i] = c;
        }
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

bool get(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t head[4];
    std::vector<uint64_t> raw;
    std::vector<RdevChunk> ck;
    std::vector<ByteRange> rg;
    std::vector<uint8_t> data, dst, scratch;
    RangePlan plan;
    uint64_t size = 0;
    while (std::fread(head, 8, 4, f) == 4) {
        const uint64_t nck = head[0], nr = head[1], dst_cap = head[2];
        const bool plan_only = (head[3] & 1) != 0;
        const bool reuse = (head[3] & 2) != 0;
        if (!reuse) {
            raw.resize(size_t(nck) * 2);
            if (!get(f, raw.data(), raw.size() * 8)) { std::fprintf(stderr, "short file\n"); return 2; }
            ck.resize(size_t(nck));
            size = 0;
            for (size_t i = 0; i < nck; i++) { ck[i] = RdevChunk{size, size, uint32_t(raw[2 * i]), uint32_t(raw[2 * i + 1])}; size += raw[2 * i]; }
        }
        rg.resize(size_t(nr));
        static_assert(sizeof(ByteRange) == 24, "three u64s");
        if (!get(f, rg.data(), rg.size() * 24)) { std::fprintf(stderr, "short file\n"); return 2; }
        if (!reuse) data.clear();
        if (!plan_only && !reuse) {
            data.resize(size_t(size));
            if (!get(f, data.data(), data.size())) { std::fprintf(stderr, "short file\n"); return 2; }
        }
        const int rc = plan_ranges(ck.data(), ck.size(), size, rg.data(), rg.size(), dst_cap, &plan);
        if (rc < 0) { std::printf("%d 0 0 0 0 0 0\n", rc); continue; }
        uint64_t extent = 0;
        uint32_t sum = 0;
        if (plan_only) {
            for (const RangeGroup& g : plan.groups)
                for (size_t t = g.t0; t < g.t1; t++)
                    if (plan.touched[t].where == kRangeScratch) extent = std::max(extent, plan.touched[t].at + ck[plan.touched[t].chunk].n);
        } else {
            dst.assign(size_t(dst_cap), 0xa5);
            scratch.assign(size_t(plan.scratch_max), 0xee);
            bool bad = false;
            for (const RangeGroup& g : plan.groups) {
                for (size_t t = g.t0; t < g.t1; t++) {
                    const RangeTouched& tc = plan.touched[t];
                    const RdevChunk& c = ck[tc.chunk];
                    if (tc.where == kRangeDirect) {
                        if (tc.at + c.n > dst.size()) { bad = true; continue; }
                        std::memcpy(dst.data() + tc.at, data.data() + c.out_off, size_t(c.n));
                    } else if (tc.where == kRangeScratch) {
                        if (tc.at + c.n > scratch.size()) { bad = true; continue; }
                        std::memcpy(scratch.data() + tc.at, data.data() + c.out_off, size_t(c.n));
                        extent = std::max(extent, tc.at + c.n);
                    }
                }
                for (size_t s = g.s0; s < g.s1; s++) {
                    const RangeSeg& sg = plan.segs[s];
                    const RangeTouched& tc = plan.touched[sg.touched];
                    const RdevChunk& c = ck[tc.chunk];
                    // (a segment of another group's chunk, or of a direct one, would be a planner's fault)
                    if (sg.touched < g.t0 || sg.touched >= g.t1 || tc.where == kRangeDirect || sg.rel + sg.len > c.n || sg.dst_off + sg.len > dst.size()) { bad = true; continue; }
                    const uint8_t* from = tc.where == kRangeStored ? data.data() + c.out_off + sg.rel : scratch.data() + tc.at + sg.rel;
                    std::memcpy(dst.data() + sg.dst_off, from, size_t(sg.len));
                }
                std::fill(scratch.begin(), scratch.end(), uint8_t(0xee));   // the next group reuses it
            }
            if (bad) { std::printf("-99 0 0 0 0 0 0\n"); continue; }
            sum = crc32_ieee(dst.data(), dst.size());
        }
        std::printf("%d %zu %llu %llu %zu %zu %u\n", rc, plan.touched.size(), (unsigned long long)plan.scratch_total, (unsigned long long)extent, plan.groups.size(),
                    plan.segs.size(), sum);
    }
    std::fclose(f);
    return 0;
}
