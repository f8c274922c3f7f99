// stream_records_check.cpp — the rules that mlz_dev_reader_search_records shares with its kernels (minlz_amd/csrc/mlz_stream_records.h), run
// as plain loops for tests/test_stream_records_host.py:
//   g++ -O2 -std=c++17 -o src tools/stream_records_check.cpp && ./src cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 L, W, delimiter, shift; u64 rec_cap, dst_cap, size; the pattern; the decoded bytes
//           -> the occurrences by a plain compare; their windows and the merge (records_window, records_window_opens) compacted into offsets,
//           lengths and starts; a window buffer of exactly the windows' bytes, `shift` bytes off a 16-byte boundary; per occurrence the bounds
//           as a wavefront finds them — 64 lanes in a loop, a step at a time, the highest lane backwards and the lowest forwards
//           (records_back_block, records_fwd_block, records_block_mask; a read outside [lo, p) and [p + L, hi) ends the program with status 3)
//           — compared with the plain loop records_bounds; the opening rule, the records, the cut at the caps:
//           "R bytes occurrences flagged k written windows window_bytes :" the records as s:e:flags "|" the windows as lo:len
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_records.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

[[noreturn]] void fail(const char* what, uint64_t i) {
    std::fprintf(stderr, "%s (occurrence %llu)\n", what, (unsigned long long)i);
    std::exit(3);
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
        if (kind != 1) { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
        const uint32_t L = in.get<uint32_t>(), W = in.get<uint32_t>(), delim32 = in.get<uint32_t>(), shift = in.get<uint32_t>() & 15;
        const uint64_t rec_cap = in.get<uint64_t>(), dst_cap = in.get<uint64_t>(), size = in.get<uint64_t>();
        const uint8_t delim = uint8_t(delim32);
        const uint8_t* pp = in.bytes(L);
        const std::vector<uint8_t> pat(pp, pp + L);
        const uint8_t* dp = in.bytes(size_t(size));
        const std::vector<uint8_t> data(dp, dp + size);
        std::vector<uint64_t> off;
        for (uint64_t p = 0; p + L <= size; p++) if (std::memcmp(data.data() + p, pat.data(), L) == 0) off.push_back(p);
        const uint64_t n = off.size();
        // windows
        std::vector<uint32_t> win_of(n);
        std::vector<uint64_t> woff, wlen, wstart;
        for (uint64_t i = 0; i < n; i++) {
            const mlz::RecordsWindow w = mlz::records_window(off[i], L, W, size);
            if (i == 0 || mlz::records_window_opens(w.lo, mlz::records_window(off[i - 1], L, W, size).hi)) { woff.push_back(w.lo); wlen.push_back(0); }
            wlen.back() = w.hi - woff.back();
            win_of[i] = uint32_t(woff.size() - 1);
        }
        uint64_t wbytes = 0;
        for (size_t w = 0; w < woff.size(); w++) {
            if (w && woff[w] <= woff[w - 1] + wlen[w - 1]) fail("merged windows touch or overlap", w);
            wstart.push_back(wbytes);
            wbytes += wlen[w];
        }
        if (wbytes > size) fail("the windows hold more than the stream", 0);
        // the window buffer: exactly the windows' bytes, `shift` off a 16-byte boundary (over-aligned storage, so the shift is the misalignment)
        std::vector<uint8_t> store(size_t(wbytes) + 32);
        uint8_t* win = store.data() + ((16 - (reinterpret_cast<uintptr_t>(store.data()) & 15)) & 15) + shift;
        for (size_t w = 0; w < woff.size(); w++) std::memcpy(win + wstart[w], data.data() + woff[w], size_t(wlen[w]));
        // bounds
        std::vector<uint64_t> s(n), e(n);
        std::vector<uint8_t> cut(n);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t p = off[i];
            const uint32_t w = win_of[i];
            const mlz::RecordsWindow wd = mlz::records_window(p, L, W, size);
            if (wd.lo < woff[w] || wd.hi > woff[w] + wlen[w]) fail("an occurrence's window leaves its merged window", i);
            const int64_t x0 = int64_t(wstart[w]) - int64_t(woff[w]);
            const int64_t mis = int64_t((reinterpret_cast<uintptr_t>(win) + uintptr_t(x0)) & 15);
            int64_t rlo = 0, rhi = 0;   // the region the look-around may read, in positions of the stream
            auto byte = [&](int64_t y) {
                const int64_t x = y - mis;
                if (x < rlo || x >= rhi) fail("a byte read outside the region", i);
                return win[x0 + x];
            };
            auto vec = [&](int64_t y, uint32_t* v) {
                const int64_t x = y - mis;
                if (x < rlo || x + 16 > rhi) fail("a vector read outside the region", i);
                if ((reinterpret_cast<uintptr_t>(win + x0 + x) & 15) != 0) fail("a vector read that is not aligned", i);
                std::memcpy(v, win + x0 + x, 16);
            };
            uint8_t c = 0;
            bool found = false;
            uint64_t at = 0;
            {
                rlo = int64_t(wd.lo); rhi = int64_t(p);
                const int64_t ylo = int64_t(wd.lo) + mis, yp = int64_t(p) + mis, ytop = (yp + 15) & ~int64_t(15);
                for (uint32_t step = 0; !found && ytop - int64_t(step) * mlz::kRecordsStep > ylo; step++) {
                    for (uint32_t lane = mlz::kRecordsLanes; lane-- > 0 && !found;) {   // the highest lane with a hit, its highest bit
                        const uint32_t m = mlz::records_block_mask(mlz::records_back_block(ytop, step, lane), ylo, yp, delim, vec, byte);
                        if (!m) continue;
                        uint32_t hb = 15;
                        while (!(m >> hb & 1)) hb--;
                        at = uint64_t(mlz::records_back_block(ytop, step, lane) + hb - mis);
                        found = true;
                    }
                }
            }
            s[i] = mlz::records_left(found, at, wd.lo, &c);
            found = false;
            {
                rlo = int64_t(p + L); rhi = int64_t(wd.hi);
                const int64_t yq = int64_t(p + L) + mis, yhi = int64_t(wd.hi) + mis, ybot = yq & ~int64_t(15);
                for (uint32_t step = 0; !found && ybot + int64_t(step) * mlz::kRecordsStep < yhi; step++) {
                    for (uint32_t lane = 0; lane < mlz::kRecordsLanes && !found; lane++) {   // the lowest lane with a hit, its lowest bit
                        const uint32_t m = mlz::records_block_mask(mlz::records_fwd_block(ybot, step, lane), yq, yhi, delim, vec, byte);
                        if (!m) continue;
                        uint32_t lb = 0;
                        while (!(m >> lb & 1)) lb++;
                        at = uint64_t(mlz::records_fwd_block(ybot, step, lane) + lb - mis);
                        found = true;
                    }
                }
            }
            e[i] = mlz::records_right(found, at, wd.hi, size, &c);
            cut[i] = c;
            const mlz::RecordsBounds plain = mlz::records_bounds([&](uint64_t x) { return data[size_t(x)]; }, p, L, wd, size, delim);
            if (plain.s != s[i] || plain.e != e[i] || plain.cut != c) fail("the wavefront's bounds differ from the plain loop's", i);
        }
        // records, caps
        std::vector<uint64_t> rs, re;
        std::vector<uint8_t> rf;
        for (uint64_t i = 0; i < n; i++) {
            if (mlz::records_opens(i, s[i], i ? s[i - 1] : 0)) { rs.push_back(s[i]); re.push_back(0); rf.push_back(cut[i] & mlz::kRecordCutLeft); }
            re.back() = e[i];
            rf.back() = uint8_t((rf.back() & mlz::kRecordCutLeft) | (cut[i] & mlz::kRecordCutRight));
        }
        uint64_t bytes = 0, flagged = 0, k = 0, written = 0;
        for (size_t r = 0; r < rs.size(); r++) {
            if (rs[r] < woff[0] || re[r] <= rs[r]) fail("a record without bytes", r);
            bytes += re[r] - rs[r];
            flagged += rf[r] ? 1 : 0;
            if (mlz::records_fits(r, bytes, rec_cap, dst_cap)) { k++; written = bytes; }
        }
        std::printf("%zu %llu %llu %llu %llu %llu %zu %llu :", rs.size(), (unsigned long long)bytes, (unsigned long long)n, (unsigned long long)flagged, (unsigned long long)k,
                    (unsigned long long)written, woff.size(), (unsigned long long)wbytes);
        for (size_t r = 0; r < rs.size(); r++) std::printf(" %llu:%llu:%u", (unsigned long long)rs[r], (unsigned long long)re[r], rf[r]);
        std::printf(" |");
        for (size_t w = 0; w < woff.size(); w++) std::printf(" %llu:%llu", (unsigned long long)woff[w], (unsigned long long)wlen[w]);
        std::printf("\n");
    }
    return 0;
}
