// stream_walk_check.cpp — the device-resident Reader's chunk walk, on the host (no GPU): the region algorithm of
// minlz_amd/csrc/mlz_stream_walk.hip.inc restated in plain C++ (exits of every offset from its 4 KiB region, lifted to 256 KiB regions, the
// entries followed top-down; the chunk headers of every entered region listed by the library's own step, walk_headers), then the SAME record
// and running-state code the library uses (mlz_stream_walk.h).  Beside it the host Reader's walk as stream_parse runs it: the same step,
// record and state from offset 0, stopping at the first error.  tests/test_stream_device_host.py compares both with the library's host
// Reader and with the oracle; under the sanitizers the exact-size buffer shows that neither reads a byte past the stream's end.
//
//   g++ -O2 -std=c++17 -o swc tools/stream_walk_check.cpp && ./swc streams.bin
// streams.bin: for every stream a little-endian u64 length and its bytes.  One line per stream: `<result> <prefix_len> <table entries>
// <host result> <host prefix_len>`, result as mlz_stream_decoded_len, prefix_len as mlz_stream_decoded_prefix_len; the first three from the
// region walk, the last two from the host Reader's walk.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_walk.h"

using namespace mlz;

namespace {

constexpr int kR0Log = 12, kR1Log = 18;
constexpr uint32_t kR0 = 1u << kR0Log, kR1 = 1u << kR1Log, kStop = 0xffffffffu, kNone = 0xffffffffu;

void walk(const uint8_t* src, uint64_t n, std::vector<WalkChunk>* table) {
    table->clear();
    if (n == 0) return;
    const uint64_t nreg0 = (n + kR0 - 1) >> kR0Log, nreg1 = (n + kR1 - 1) >> kR1Log;
    std::vector<uint32_t> x0(n), x1(n), entry0(nreg0, kNone);
    std::vector<uint64_t> entry1(nreg1, ~uint64_t(0));
    // W1: exit of every offset from its 4 KiB region (the kernel jumps pointers; right to left gives the same fixed point)
    for (uint64_t r = 0; r < nreg0; r++) {
        const uint64_t base = r << kR0Log;
        const uint32_t own = uint32_t(n - base < kR0 ? n - base : kR0);
        for (uint32_t i = own; i-- > 0;) {
            const uint64_t p = base + i;
            uint32_t v = kStop;
            if (n - p >= 4) v = i + 4 + (uint32_t(src[p + 1]) | uint32_t(src[p + 2]) << 8 | uint32_t(src[p + 3]) << 16);
            if (v < kR0) v = v < own ? x0[base + v] : kStop;   // (at or behind the end of the stream: the kernel's table says stop there)
            x0[p] = v;
        }
    }
    // W2
    for (uint64_t p = 0; p < n; p++) {
        const uint64_t base1 = p & ~uint64_t(kR1 - 1), end1 = base1 + kR1;
        uint64_t base0 = p & ~uint64_t(kR0 - 1);
        uint32_t x = x0[p];
        for (;;) {
            if (x == kStop) break;
            const uint64_t e = base0 + x;
            if (e >= end1 || e >= n) { x = uint32_t(e - base1); break; }
            base0 = e & ~uint64_t(kR0 - 1);
            x = x0[e];
        }
        x1[p] = x;
    }
    // W3
    for (uint64_t e = 0; e < n;) {
        const uint64_t r1 = e >> kR1Log;
        entry1[r1] = e;
        if (x1[e] == kStop) break;
        e = (r1 << kR1Log) + x1[e];
    }
    // W4
    for (uint64_t r1 = 0; r1 < nreg1; r1++) {
        uint64_t e = entry1[r1];
        if (e == ~uint64_t(0)) continue;
        const uint64_t end1 = (r1 + 1) << kR1Log;
        while (e < end1 && e < n) {
            const uint64_t r0 = e >> kR0Log;
            entry0[r0] = uint32_t(e & (kR0 - 1));
            if (x0[e] == kStop) break;
            e = (r0 << kR0Log) + x0[e];
        }
    }
    // W5
    for (uint64_t r0 = 0; r0 < nreg0; r0++) {
        if (entry0[r0] == kNone) continue;
        const uint64_t base = r0 << kR0Log, end = base + kR0 < n ? base + kR0 : n;
        walk_headers(src, n, base + entry0[r0], end, false, kWalkNoCap, [&](uint64_t e) { table->push_back(walk_classify(src, n, e)); return true; });
    }
}

// The host Reader's walk (stream_parse in mlz_stream.hip.inc): the headers from offset 0, a record and a step of the running state for each
// that enters, up to the first error and not a byte further
int64_t host_reader(const uint8_t* src, uint64_t n, uint64_t* prefix) {
    WalkReader rd(uint64_t(8) << 20);
    int err = 0;
    *prefix = 0;
    walk_headers(src, n, 0, n, false, kWalkNoCap, [&](uint64_t e) {
        err = rd.step(walk_classify(src, n, e), [&](uint8_t, uint32_t, uint64_t, uint64_t, uint64_t nn, uint64_t out_off, uint64_t) { *prefix = out_off + nn; });
        return err == 0;
    });
    const int64_t r = err ? err : rd.finish();
    if (r >= 0) *prefix = uint64_t(r);
    return r;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<uint8_t> buf;
    std::vector<WalkChunk> table;
    uint64_t len;
    while (std::fread(&len, 8, 1, f) == 1) {
        // the bytes behind the stream's end must not matter: the copy is exact, so a read past it is caught by a sanitizer build
        buf.resize(len);
        if (len && std::fread(buf.data(), 1, len, f) != len) { std::fprintf(stderr, "short file\n"); return 2; }
        walk(buf.data(), len, &table);
        uint64_t prefix = 0;
        const int64_t r = walk_parse_table(table.data(), table.size(), uint64_t(8) << 20,
                                           [&](uint8_t, uint32_t, uint64_t, uint64_t, uint64_t nn, uint64_t out_off, uint64_t) { prefix = out_off + nn; });
        uint64_t host_prefix = 0;
        const int64_t host = host_reader(buf.data(), len, &host_prefix);
        std::printf("%lld %llu %zu %lld %llu\n", (long long)r, (unsigned long long)(r >= 0 ? uint64_t(r) : prefix), table.size(), (long long)host, (unsigned long long)host_prefix);
    }
    std::fclose(f);
    return 0;
}
