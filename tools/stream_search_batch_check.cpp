// stream_search_batch_check.cpp — the host code that mlz_stream_search_batch_device shares with its kernels (minlz_amd/csrc/mlz_stream_search_batch.h:
// batch_vbases, batch_stream_of, batch_tile_streams, batch_stream_count; mlz_stream_search.h: search_layout, search_many_index,
// search_many_tile_pairs), for tests/test_stream_search_batch_host.py:
//   g++ -O2 -std=c++17 -o ssb tools/stream_search_batch_check.cpp && ./ssb cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   u32 n_streams, npat; u64 group bytes; per stream u32 nck and nck x u64 chunk sizes; npat x u32 len; the patterns; every stream's data
//   -> the call's host side and its kernels' rules as plain loops: the virtual positions; one job list of the chunks that have bytes, in
//      descriptor order, cut into groups of the record's size; search_layout over the virtual positions; every group's chunks copied to their
//      places in ONE reused scratch (poisoned between groups, the carried bytes kept), every tile walked by search_many_tile_pairs over a copy
//      of exactly the bytes the kernel stages, its pairs appended as (virtual position, pattern) and its count added to the running prefix,
//      presence marked by tile_stream; then the finish rule: every stream's count from the prefix at tile_first, every pair's stream and
//      position by batch_stream_of:
//      "total tiles groups bad_tiles : stream:position:pattern ... | count per stream | presence row per stream (hex words joined by ,)"
//      bad_tiles: tiles whose [gpos, gpos + hi_end) holds a hole byte or leaves its stream (0 for a correct layout).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_search_batch.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

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
        const uint32_t n = in.get<uint32_t>(), npat = in.get<uint32_t>();
        const uint64_t group_bytes = in.get<uint64_t>();
        if (n == 0 || npat == 0) { std::fprintf(stderr, "an empty record\n"); return 2; }
        std::vector<std::vector<uint64_t>> ck(n);
        std::vector<uint64_t> size(n, 0), vbase(n + 1);
        for (uint32_t i = 0; i < n; i++) {
            ck[i].resize(in.get<uint32_t>());
            for (auto& v : ck[i]) { v = in.get<uint64_t>(); size[i] += v; }
        }
        std::vector<uint32_t> len(npat), off(npat + 1, 0);
        for (uint32_t i = 0; i < npat; i++) { len[i] = in.get<uint32_t>(); off[i + 1] = off[i] + len[i]; }
        const uint8_t* pb = in.bytes(off[npat]);
        const std::vector<uint8_t> blob(pb, pb + off[npat]);   // (copies of their own size: a read beyond one is a finding for the sanitizer)
        std::vector<std::vector<uint8_t>> data(n);
        for (uint32_t i = 0; i < n; i++) { const uint8_t* d = in.bytes(size_t(size[i])); data[i].assign(d, d + size[i]); }

        mlz::batch_vbases(size.data(), n, vbase.data());
        // the job list: (stream, offset inside it, bytes), chunks that have bytes only
        struct Job { uint32_t s; uint64_t o, n; };
        std::vector<Job> jobs;
        for (uint32_t i = 0; i < n; i++) {
            uint64_t o = 0;
            for (uint64_t v : ck[i]) { if (v) jobs.push_back(Job{i, o, v}); o += v; }
        }
        std::vector<size_t> gend;
        for (size_t i = 0; i < jobs.size();) {   // range_group_ends with the record's group size
            uint64_t acc = 0;
            while (i < jobs.size() && acc < group_bytes) acc += jobs[i++].n;
            gend.push_back(i);
        }
        mlz::SearchManyIndex ix;
        mlz::search_many_index(blob.data(), len.data(), npat, &ix);
        mlz::SearchLayout lay;
        mlz::search_layout(jobs.size(), gend, [&](size_t j) { return vbase[jobs[j].s] + jobs[j].o; }, [&](size_t j) { return jobs[j].n; }, ix.lmin, ix.lmax, mlz::kSearchManyTile, &lay);
        const size_t nt = lay.tiles.size();
        std::vector<uint32_t> tile_stream(nt), tile_first(n + 1);
        const bool ascending = mlz::batch_tile_streams(lay.tiles.data(), nt, vbase.data(), n, tile_stream.data(), tile_first.data());
        size_t bad_tiles = ascending ? 0 : 1;
        for (size_t t = 0; t < nt; t++) {   // no tile's bytes hold a hole or another stream's byte (checked on its own, hole by hole)
            const mlz::SearchTile& tl = lay.tiles[t];
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t hole = vbase[i + 1] - 1;
                if (hole >= tl.gpos && hole < tl.gpos + tl.hi_end) bad_tiles++;
            }
        }

        const size_t words = (npat + 31) / 32;
        std::vector<uint32_t> present(size_t(n) * words, 0);
        std::vector<uint64_t> prefix(nt, 0), vpos;
        std::vector<uint32_t> which;
        uint64_t total = 0;
        std::vector<uint8_t> keep(mlz::kSearchMaxPattern), scratch(size_t(lay.scratch_max) + 1, 0xEE);
        for (size_t g = 0, j0 = 0; g < gend.size(); j0 = gend[g++]) {
            for (size_t j = j0; j < gend[g]; j++) std::memcpy(scratch.data() + lay.at[j], data[jobs[j].s].data() + jobs[j].o, size_t(jobs[j].n));
            for (size_t t = g ? lay.tile_end[g - 1] : 0; t < lay.tile_end[g]; t++) {
                const mlz::SearchTile& tl = lay.tiles[t];
                if (tl.src_off < 1 || tl.count < 1 || tl.count > mlz::kSearchManyTile || uint64_t(tl.src_off) + tl.hi_end > lay.used[g] || tl.count - 1 + ix.lmin > tl.hi_end) {
                    std::fprintf(stderr, "a tile reads outside the group's bytes\n");
                    return 3;
                }
                uint32_t avail = tl.count - 1 + ix.lmax;
                if (avail > tl.hi_end) avail = tl.hi_end;
                const std::vector<uint8_t> staged(scratch.begin() + tl.src_off, scratch.begin() + tl.src_off + avail);
                prefix[t] = total;
                uint32_t* row = present.data() + size_t(tile_stream[t]) * words;
                mlz::search_many_tile_pairs(staged.data(), tl, ix, blob.data(), [&](uint32_t i, uint32_t p) {
                    vpos.push_back(tl.gpos + i); which.push_back(p);
                    row[p >> 5] |= 1u << (p & 31);
                    total++;
                });
            }
            if (lay.carry[g]) std::memcpy(keep.data(), scratch.data() + lay.used[g] - lay.carry[g], lay.carry[g]);
            std::memset(scratch.data(), 0xEE, scratch.size());   // (the next group overwrites the scratch)
            if (lay.carry[g]) std::memcpy(scratch.data() + mlz::kSearchPad - lay.carry[g], keep.data(), lay.carry[g]);
        }
        // the finish rule
        std::printf("%llu %zu %zu %zu :", (unsigned long long)total, nt, gend.size(), bad_tiles);
        for (size_t k = 0; k < vpos.size(); k++) {
            const size_t s = mlz::batch_stream_of(vbase.data(), n, vpos[k]);
            std::printf(" %zu:%llu:%u", s, (unsigned long long)(vpos[k] - vbase[s]), which[k]);
        }
        std::printf(" |");
        for (uint32_t i = 0; i < n; i++)
            std::printf(" %llu", (unsigned long long)mlz::batch_stream_count([&](size_t t) { return prefix[t]; }, nt, total, tile_first.data(), i));
        std::printf(" |");
        for (uint32_t i = 0; i < n; i++) {
            std::printf(" ");
            for (size_t w = 0; w < words; w++) std::printf(w ? ",%x" : "%x", present[size_t(i) * words + w]);
        }
        std::printf("\n");
    }
    return 0;
}
