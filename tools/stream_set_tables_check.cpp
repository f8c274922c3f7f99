// stream_set_tables_check.cpp — the host code that a set of streams which keeps its streams' search tables (mlz_stream_open_batch_device_tables,
// minlz_amd/csrc/mlz_stream_set_tables.hip.inc) shares with its kernels (minlz_amd/csrc/mlz_stream_set_tables.h: set_tables_cross,
// set_tables_cross_records, set_tables_tail, set_tables_mark_from, set_tables_plan_mark; the classes are batch_assign_classes), for
// tests/test_stream_set_tables_host.py:
//   g++ -O2 -std=c++17 -o sstc tools/stream_set_tables_check.cpp && ./sstc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   u32 n_streams; u32 records (1: the record-bound form of cross); u32 nw, L, t_min of the one pattern;
//   per stream: u8 T, M, B, ok, part; u16 flen; u64 hash (its info key; part = 0: left out of the set); u32 mode (0 skipped, 1 whole, 2 pruned);
//               u32 last_is_delim; u32 n_chunks; per chunk u64 decoded bytes, u32 a, u32 s (its table's probe: leading and trailing groups)
//   -> "class per stream (255: none) and the classes found | cross per stream | tail per chunk | the chunks taken", a lane's work per
//      (chunk, pattern) as plain loops over the handle's chunk list.  The record index holds a delimiter at the last byte of every stream
//      that says so, which is all set_joined looks at.
// Every array is a copy of exactly its size, so that a read beyond one is a finding for the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_set_tables.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
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
        const uint32_t n = in.get<uint32_t>(), records = in.get<uint32_t>();
        mlz::SearchManyPat pt{0, in.get<uint32_t>(), 1, 0, 0, 0};
        pt.L = in.get<uint32_t>();
        pt.t_min = in.get<uint32_t>();
        std::vector<mlz::BatchInfoKey> keys(n);
        std::vector<uint8_t> part(n), cls(n);
        std::vector<mlz::BatchPlanStream> st(n);
        std::vector<uint32_t> ends_delim(n), a, s;
        std::vector<uint64_t> size(n, 0), bases(size_t(n) + 1);
        std::vector<mlz::SetTabChunk> ck;
        for (uint32_t i = 0; i < n; i++) {
            keys[i].T = in.get<uint8_t>(); keys[i].M = in.get<uint8_t>(); keys[i].B = in.get<uint8_t>(); keys[i].ok = in.get<uint8_t>();
            part[i] = in.get<uint8_t>();
            keys[i].flen = in.get<uint16_t>(); keys[i].pad = 0;
            keys[i].hash = in.get<uint64_t>();
            const uint32_t mode = in.get<uint32_t>();
            ends_delim[i] = in.get<uint32_t>();
            const uint32_t nc = in.get<uint32_t>();
            st[i] = mlz::BatchPlanStream{0, 0, uint32_t(ck.size()), uint32_t(ck.size()) + nc, mode, 0};
            for (uint32_t k = 0; k < nc; k++) {
                ck.push_back(mlz::SetTabChunk{in.get<uint64_t>(), 0, i, 0});
                a.push_back(in.get<uint32_t>());
                s.push_back(in.get<uint32_t>());
                size[i] += ck.back().n;
            }
            uint64_t behind = 0;
            for (size_t k = st[i].c1; k-- > st[i].c0;) { ck[k].behind = behind; behind += ck[k].n; }
        }
        const size_t nck = ck.size();
        mlz::set_bases(size.data(), n, bases.data());
        std::vector<uint64_t> D;
        for (uint32_t i = 0; i < n; i++) if (size[i] && ends_delim[i]) D.push_back(bases[i + 1] - 1);
        const uint64_t k = D.size();
        auto at = [&](uint64_t j) { if (j >= k) { std::fprintf(stderr, "a read beyond the delimiter table\n"); std::exit(3); } return D[size_t(j)]; };

        size_t rep[mlz::kSidecarMaxConfigs] = {};
        const uint32_t classes = mlz::batch_assign_classes(keys.data(), part.data(), n, cls.data(), rep);
        for (uint32_t i = 0; i < n; i++) std::printf(" %u", unsigned(cls[i]));
        std::printf(" %u |", classes);
        std::vector<uint8_t> cross(n);
        for (uint32_t i = 0; i < n; i++) {
            cross[i] = (records ? mlz::set_tables_cross_records(at, k, bases.data(), n, i) : mlz::set_tables_cross(bases.data(), n, i)) ? 1 : 0;
            std::printf(" %u", unsigned(cross[i]));
        }
        std::printf(" |");
        for (size_t j = 0; j < nck; j++) std::printf(" %u", mlz::set_tables_tail(ck[j].n, ck[j].behind, pt.L) ? 1u : 0u);
        std::printf(" |");
        std::vector<uint8_t> take(nck, 0);
        auto chunk = [&](size_t j) { if (j >= nck) { std::fprintf(stderr, "a read beyond the chunk list\n"); std::exit(3); } return ck[j]; };
        auto cross_of = [&](uint32_t i) { if (i >= n) { std::fprintf(stderr, "a read beyond the streams\n"); std::exit(3); } return cross[i] != 0; };
        auto probe = [&](size_t j, bool lead) { if (j >= nck) { std::fprintf(stderr, "a probe beyond the chunk list\n"); std::exit(3); } return lead ? a[j] : s[j]; };
        for (size_t j = 0; j < nck; j++) mlz::set_tables_plan_mark(j, nck, st[ck[j].stream], pt, probe, chunk, cross_of, take.data());
        for (size_t j = 0; j < nck; j++) if (take[j]) std::printf(" %llu", ull(j));
        std::printf("\n");
    }
    return 0;
}
