// stream_search_many_check.cpp — the host code that mlz_dev_reader_search_many shares with its kernels (minlz_amd/csrc/mlz_stream_search.h:
// search_pattern_hashes, search_decoded_mark, search_layout, search_many_index, search_many_tile_pairs), for tests/test_stream_search_many_host.py:
//   g++ -O2 -std=c++17 -o ssm tools/stream_search_many_check.cpp && ./ssm cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 T, M, B, field bytes, nck, npat; the field; nck x u64 n; nck x (u32 R or 0xffffffff, u32 table bytes, the table); npat x u32 len; the patterns
//           -> "served unserved :" and the union of the patterns' decoded sets as the plan kernel marks it: search_pattern_hashes and
//           search_probe per pattern, search_decoded_mark over every (chunk, pattern) on one array (an unserved pattern: every non-empty chunk)
//   kind 2  u32 nck, n_take, npat; u64 group bytes, data bytes; nck x u64 n; n_take x u32 chunk; npat x u32 len; the patterns; data
//           -> the pairs found by search_layout's tiles (lmin .. lmax, tiles of kSearchManyTile), executed as the search executes them: the taken chunks of a group copied to
//           their places in ONE reused scratch, every tile walked by search_many_tile_pairs (the index look-up and the verify as far as
//           the run holds a pattern's bytes), its pairs appended in the order found (the write rule), the carried bytes copied in front of the next group:
//           "count tiles groups scratch_max :" and the pairs as position:pattern
//   kind 3  u32 npat; npat x u32 len; the patterns -> "m hb lmin lmax : heads | order" (search_many_index)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_search.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

struct Pats { std::vector<uint32_t> len, off; std::vector<uint8_t> blob; };
Pats read_patterns(In& in, uint32_t npat) {
    Pats p;
    p.len.resize(npat); p.off.assign(npat + 1, 0);
    for (uint32_t i = 0; i < npat; i++) { p.len[i] = in.get<uint32_t>(); p.off[i + 1] = p.off[i] + p.len[i]; }
    const uint8_t* b = in.bytes(p.off[npat]);
    p.blob.assign(b, b + p.off[npat]);   // (a copy of its own size: a read beyond it is a finding for the sanitizer)
    return p;
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
        if (kind == 1) {
            const uint32_t T = in.get<uint32_t>(), M = in.get<uint32_t>(), B = in.get<uint32_t>(), flen = in.get<uint32_t>(), nck = in.get<uint32_t>(), npat = in.get<uint32_t>();
            uint8_t field[mlz::kSearchMaxField + 2] = {};
            std::memcpy(field, in.bytes(flen), flen);
            std::vector<uint64_t> n(nck);
            for (auto& v : n) v = in.get<uint64_t>();
            std::vector<uint32_t> R(nck);
            std::vector<std::vector<uint8_t>> tab(nck);
            for (uint32_t k = 0; k < nck; k++) {
                R[k] = in.get<uint32_t>();
                const uint32_t tb = in.get<uint32_t>();
                const uint8_t* t = in.bytes(tb);
                tab[k].assign(t, t + tb);
            }
            const Pats ps = read_patterns(in, npat);
            std::vector<uint8_t> take(nck, 0);
            std::vector<uint32_t> win(mlz::kSearchMaxWindows);
            uint32_t served = 0;
            for (uint32_t i = 0; i < npat; i++) {
                std::vector<uint32_t> h;
                mlz::SearchManyPat pt;
                if (!mlz::search_pattern_hashes(ps.blob.data() + ps.off[i], ps.len[i], T, M, B, field, win.data(), &h, &pt)) {
                    for (uint32_t k = 0; k < nck; k++) if (n[k]) take[k] = 1;
                    continue;
                }
                served++;
                const uint32_t nw = pt.nw, gsize = pt.gsize, t_min = pt.t_min, L = pt.L;
                auto probe = [&](size_t k, bool lead) {
                    uint32_t a = nw, s = nw;
                    if (R[k] != mlz::kSearchNoTable) mlz::search_probe(tab[k].data(), B - R[k], h.data(), nw, &a, &s, gsize);
                    return lead ? a : s;
                };
                for (uint32_t k = 0; k < nck; k++)
                    mlz::search_decoded_mark(k, nck, [&](size_t j) { return probe(j, true); }, [&](size_t j) { return probe(j, false); }, [&](size_t j) { return n[j]; }, nw, L,
                                             take.data(), t_min);
            }
            std::printf("%u %u :", served, npat - served);
            for (uint32_t k = 0; k < nck; k++) if (take[k]) std::printf(" %u", k);
            std::printf("\n");
        } else if (kind == 2) {
            const uint32_t nck = in.get<uint32_t>(), n_take = in.get<uint32_t>(), npat = in.get<uint32_t>();
            const uint64_t group_bytes = in.get<uint64_t>(), dlen = in.get<uint64_t>();
            std::vector<uint64_t> n(nck), off(nck);
            for (auto& v : n) v = in.get<uint64_t>();
            for (uint32_t k = 1; k < nck; k++) off[k] = off[k - 1] + n[k - 1];
            std::vector<uint32_t> jobs(n_take);
            for (auto& v : jobs) v = in.get<uint32_t>();
            const Pats ps = read_patterns(in, npat);
            const uint8_t* d = in.bytes(size_t(dlen));
            std::vector<size_t> gend;
            for (size_t i = 0; i < n_take;) {   // range_group_ends with the record's group size
                uint64_t acc = 0;
                while (i < n_take && acc < group_bytes) acc += n[jobs[i++]];
                gend.push_back(i);
            }
            mlz::SearchManyIndex ix;
            mlz::search_many_index(ps.blob.data(), ps.len.data(), npat, &ix);
            mlz::SearchLayout lay;
            mlz::search_layout(n_take, gend, [&](size_t i) { return off[jobs[i]]; }, [&](size_t i) { return n[jobs[i]]; }, ix.lmin, ix.lmax, mlz::kSearchManyTile, &lay);
            std::vector<uint8_t> keep(mlz::kSearchMaxPattern);
            std::vector<uint64_t> pos;
            std::vector<uint32_t> which;
            std::vector<uint8_t> scratch(size_t(lay.scratch_max), 0xEE);
            for (size_t g = 0, j0 = 0; g < gend.size(); j0 = gend[g++]) {
                for (size_t i = j0; i < gend[g]; i++) std::memcpy(scratch.data() + lay.at[i], d + off[jobs[i]], size_t(n[jobs[i]]));
                for (size_t t = g ? lay.tile_end[g - 1] : 0; t < lay.tile_end[g]; t++) {
                    const mlz::SearchTile& tl = lay.tiles[t];
                    if (tl.src_off < 1 || tl.count < 1 || tl.count > mlz::kSearchManyTile ||
                        uint64_t(tl.src_off) + tl.hi_end > lay.used[g] || tl.count - 1 + ix.lmin > tl.hi_end) {
                        std::fprintf(stderr, "a tile reads outside the group's bytes\n");
                        return 3;
                    }
                    // the tile's bytes as the kernel stages them: count - 1 + lmax, as far as the run has them (a copy of exactly that size)
                    uint32_t avail = tl.count - 1 + ix.lmax;
                    if (avail > tl.hi_end) avail = tl.hi_end;
                    const std::vector<uint8_t> staged(scratch.begin() + tl.src_off, scratch.begin() + tl.src_off + avail);
                    mlz::search_many_tile_pairs(staged.data(), tl, ix, ps.blob.data(), [&](uint32_t i, uint32_t p) { pos.push_back(tl.gpos + i); which.push_back(p); });
                }
                if (lay.carry[g]) std::memcpy(keep.data(), scratch.data() + lay.used[g] - lay.carry[g], lay.carry[g]);
                std::memset(scratch.data(), 0xEE, scratch.size());   // (the next group overwrites the scratch)
                if (lay.carry[g]) std::memcpy(scratch.data() + mlz::kSearchPad - lay.carry[g], keep.data(), lay.carry[g]);
            }
            std::printf("%zu %zu %zu %llu :", pos.size(), lay.tiles.size(), gend.size(), (unsigned long long)lay.scratch_max);
            for (size_t i = 0; i < pos.size(); i++) std::printf(" %llu:%u", (unsigned long long)pos[i], which[i]);
            std::printf("\n");
        } else if (kind == 3) {
            const uint32_t npat = in.get<uint32_t>();
            const Pats ps = read_patterns(in, npat);
            mlz::SearchManyIndex ix;
            mlz::search_many_index(ps.blob.data(), ps.len.data(), npat, &ix);
            std::printf("%u %u %u %u :", ix.m, ix.hb, ix.lmin, ix.lmax);
            for (uint16_t v : ix.heads) std::printf(" %u", v);
            std::printf(" |");
            for (uint16_t v : ix.order) std::printf(" %u", v);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown record %u\n", kind);
            return 2;
        }
    }
    return 0;
}
