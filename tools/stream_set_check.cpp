// stream_set_check.cpp — the host code that a set of streams behind one handle (mlz_stream_open_batch_device and the calls of
// minlz_amd/csrc/mlz_stream_set.hip.inc) shares with its kernels (minlz_amd/csrc/mlz_stream_set.h: set_bases, set_locate, set_range_ok,
// set_first, set_joined, set_locate_record), for tests/test_stream_set_host.py:
//   g++ -O2 -std=c++17 -o ssc tools/stream_set_check.cpp && ./ssc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   u32 n_streams; n x u64 sizes (0 for a failed stream); u32 delimiter; the handle's bytes (the sum of the sizes);
//   u32 n_pos, n_pos x u64 positions; u32 n_rng, n_rng x (u32 which, u64 off, u64 len); u32 n_rec, n_rec x u64 record numbers
//   -> the kernels' rules as plain loops, a lane's work per item, over the delimiter table the record index would hold:
//      "bases | which:local per position | the global offset or - per range | first[0 .. n] | joined records | which:local_no per record number"
// Every array is a copy of exactly its size, so that a read beyond one is a finding for the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_set.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

typedef unsigned long long ull;

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
        const uint32_t n = in.get<uint32_t>();
        std::vector<uint64_t> size(n), bases(size_t(n) + 1);
        for (auto& v : size) v = in.get<uint64_t>();
        const uint8_t delim = uint8_t(in.get<uint32_t>());
        mlz::set_bases(size.data(), n, bases.data());
        const uint64_t total = bases[n];
        const uint8_t* d = in.bytes(size_t(total));
        const std::vector<uint8_t> data(d, d + total);
        // the record index: the positions of all delimiters, and N
        std::vector<uint64_t> D;
        for (uint64_t p = 0; p < total; p++) if (data[size_t(p)] == delim) D.push_back(p);
        const uint64_t k = D.size(), N = mlz::rindex_records(k, total, k && D[size_t(k - 1)] == total - 1);
        auto at = [&](uint64_t j) { if (j >= k) { std::fprintf(stderr, "a read beyond the delimiter table\n"); std::exit(3); } return D[size_t(j)]; };

        for (uint32_t i = 0; i <= n; i++) std::printf(" %llu", ull(bases[i]));
        std::printf(" |");
        for (uint32_t q = in.get<uint32_t>(); q; q--) {
            uint32_t w;
            uint64_t l;
            mlz::set_locate(bases.data(), n, in.get<uint64_t>(), &w, &l);
            std::printf(" %u:%llu", w, ull(l));
        }
        std::printf(" |");
        for (uint32_t q = in.get<uint32_t>(); q; q--) {
            const uint32_t which = in.get<uint32_t>();
            const uint64_t off = in.get<uint64_t>(), len = in.get<uint64_t>();
            uint64_t g;
            if (mlz::set_range_ok(bases.data(), n, which, off, len, &g)) std::printf(" %llu", ull(g));
            else std::printf(" -");
        }
        std::printf(" |");
        for (uint32_t i = 0; i <= n; i++) std::printf(" %llu", ull(mlz::set_first(at, k, N, bases[i])));
        uint64_t joined = 0;
        for (uint32_t i = 0; i < n; i++) joined += mlz::set_joined(at, k, bases.data(), n, i) ? 1 : 0;
        std::printf(" | %llu %llu |", ull(joined), ull(N));
        for (uint32_t q = in.get<uint32_t>(); q; q--) {
            uint32_t w;
            uint64_t l;
            mlz::set_locate_record(at, k, N, bases.data(), n, in.get<uint64_t>(), &w, &l);
            std::printf(" %u:%llu", w, ull(l));
        }
        std::printf("\n");
    }
    return 0;
}
