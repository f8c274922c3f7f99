// stream_search_fold_check.cpp — the host code of MLZ_SEARCH_IGNORE_CASE that the searches share with their kernels
// (minlz_amd/csrc/mlz_stream_search.h: search_fold, search_fold4, search_windows_fold, search_pattern_hashes_fold, search_probe_fold, and
// search_many_index / search_many_tile_pairs over folded patterns), for tests/test_stream_search_fold_host.py:
//   g++ -O2 -std=c++17 -o ssf tools/stream_search_fold_check.cpp && ./ssf cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  nothing -> search_fold4 of every byte value in each of the four byte positions between neighbours of 0x00 and of 0xFF, as
//           2048 hex words (position, neighbour, value ascending), then "|" and search_fold of the 256 byte values
//   kind 2  u32 T, M, B, field bytes, L, budget; the field; the pattern (as the caller gives it, not folded)
//           -> "nw gsize t_min served over :" the window starts of search_windows_fold "|" per window its variant hashes joined by ","
//           ("-": the window abstains) as search_pattern_hashes_fold lays them out; nothing behind "|" when it returns false
//   kind 3  u32 T, M, B, field bytes, nck, npat, budget; the field; nck x u64 n; nck x (u32 R or 0xffffffff, u32 table bytes, the table);
//           npat x u32 len; the patterns -> "served unserved :" and the union of the decoded sets as the plan marks it: the patterns folded,
//           search_pattern_hashes_fold in order against the budget, search_probe_fold and search_decoded_mark over every (chunk, pattern)
//   kind 4  u32 npat, fold, data bytes; npat x u32 len; the patterns; the data (at most kSearchManyTile + 255 bytes)
//           -> "m hb : order |" and the pairs position:pattern of ONE tile over the data, by search_many_index over the patterns (folded
//           first when fold is set) and search_many_tile_pairs
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
    std::vector<uint8_t> bytes(size_t n) {   // (a copy of its own size: a read beyond it is a finding for the sanitizer)
        if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
        std::vector<uint8_t> v(b.begin() + p, b.begin() + p + n);
        p += n;
        return v;
    }
};

struct Pats { std::vector<uint32_t> len, off; std::vector<uint8_t> blob; };
Pats read_patterns(In& in, uint32_t npat, bool fold) {
    Pats p;
    p.len.resize(npat); p.off.assign(npat + 1, 0);
    for (uint32_t i = 0; i < npat; i++) { p.len[i] = in.get<uint32_t>(); p.off[i + 1] = p.off[i] + p.len[i]; }
    p.blob = in.bytes(p.off[npat]);
    if (fold) for (auto& v : p.blob) v = mlz::search_fold(v);   // as the calls fold them, once
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
            for (uint32_t pos = 0; pos < 4; pos++)
                for (uint32_t nb = 0; nb < 2; nb++)
                    for (uint32_t v = 0; v < 256; v++) {
                        const uint32_t x = ((nb ? 0xffffffffu : 0u) & ~(0xffu << (8 * pos))) | (v << (8 * pos));
                        std::printf("%08x ", mlz::search_fold4(x));
                    }
            std::printf("|");
            for (uint32_t v = 0; v < 256; v++) std::printf(" %02x", mlz::search_fold(uint8_t(v)));
            std::printf("\n");
        } else if (kind == 2) {
            const uint32_t T = in.get<uint32_t>(), M = in.get<uint32_t>(), B = in.get<uint32_t>(), flen = in.get<uint32_t>(), L = in.get<uint32_t>(), budget = in.get<uint32_t>();
            uint8_t field[mlz::kSearchMaxField + 2] = {};
            const std::vector<uint8_t> fb = in.bytes(flen), pat = in.bytes(L);
            if (flen) std::memcpy(field, fb.data(), flen);
            std::vector<uint32_t> win(mlz::kSearchMaxWindows), voff{7, 7}, hs{9};   // (something in front: the offsets are absolute)
            uint32_t t_min = 9, gsize = 9;
            const uint32_t nw = mlz::search_windows_fold(pat.data(), L, T, M, field, win.data(), &t_min, &gsize);
            mlz::SearchManyPat pt{};
            bool over = false;
            const bool ok = mlz::search_pattern_hashes_fold(pat.data(), L, T, M, B, field, win.data(), &voff, &hs, &pt, budget, &over);
            std::printf("%u %u %u %d %d :", nw, gsize, t_min, ok ? 1 : 0, over ? 1 : 0);
            for (uint32_t w = 0; w < nw * gsize; w++) std::printf(" %u", win[w]);
            std::printf(" |");
            if (ok) {
                if (pt.h_off != 2 || pt.nw != nw || pt.gsize != gsize || pt.t_min != t_min || pt.L != L || voff.size() != 2 + size_t(nw) * gsize + 1 || voff.back() != hs.size()) {
                    std::fprintf(stderr, "the pattern's record does not fit its windows\n");
                    return 3;
                }
                for (uint32_t w = 0; w < nw * gsize; w++) {
                    std::printf(" ");
                    if (voff[2 + w] == voff[3 + w]) std::printf("-");
                    for (uint32_t e = voff[2 + w]; e < voff[3 + w]; e++) std::printf(e == voff[2 + w] ? "%u" : ",%u", hs[e]);
                }
            } else if (voff.size() != 2 || hs.size() != 1) {
                std::fprintf(stderr, "a pattern that is not served left something behind\n");
                return 3;
            }
            std::printf("\n");
        } else if (kind == 3) {
            const uint32_t T = in.get<uint32_t>(), M = in.get<uint32_t>(), B = in.get<uint32_t>(), flen = in.get<uint32_t>(), nck = in.get<uint32_t>(), npat = in.get<uint32_t>(),
                           budget = in.get<uint32_t>();
            uint8_t field[mlz::kSearchMaxField + 2] = {};
            const std::vector<uint8_t> fb = in.bytes(flen);
            if (flen) std::memcpy(field, fb.data(), flen);
            std::vector<uint64_t> n(nck);
            for (auto& v : n) v = in.get<uint64_t>();
            std::vector<uint32_t> R(nck);
            std::vector<std::vector<uint8_t>> tab(nck);
            for (uint32_t k = 0; k < nck; k++) {
                R[k] = in.get<uint32_t>();
                const uint32_t tb = in.get<uint32_t>();
                tab[k] = in.bytes(tb);
            }
            const Pats ps = read_patterns(in, npat, true);
            std::vector<uint8_t> take(nck, 0);
            std::vector<uint32_t> win(mlz::kSearchMaxWindows), voff, hs;
            uint32_t served = 0;
            for (uint32_t i = 0; i < npat; i++) {
                mlz::SearchManyPat pt;
                if (!mlz::search_pattern_hashes_fold(ps.blob.data() + ps.off[i], ps.len[i], T, M, B, field, win.data(), &voff, &hs, &pt, uint32_t(budget - hs.size()))) {
                    for (uint32_t k = 0; k < nck; k++) if (n[k]) take[k] = 1;
                    continue;
                }
                served++;
                auto probe = [&](size_t k, bool lead) {
                    uint32_t a = pt.nw, s = pt.nw;
                    if (R[k] != mlz::kSearchNoTable) mlz::search_probe_fold(tab[k].data(), B - R[k], voff.data() + pt.h_off, hs.data(), pt.nw, &a, &s, pt.gsize);
                    return lead ? a : s;
                };
                for (uint32_t k = 0; k < nck; k++)
                    mlz::search_decoded_mark(k, nck, [&](size_t j) { return probe(j, true); }, [&](size_t j) { return probe(j, false); }, [&](size_t j) { return n[j]; }, pt.nw, pt.L,
                                             take.data(), pt.t_min);
            }
            std::printf("%u %u :", served, npat - served);
            for (uint32_t k = 0; k < nck; k++) if (take[k]) std::printf(" %u", k);
            std::printf("\n");
        } else if (kind == 4) {
            const uint32_t npat = in.get<uint32_t>(), fold = in.get<uint32_t>(), dlen = in.get<uint32_t>();
            const Pats ps = read_patterns(in, npat, fold != 0);
            const std::vector<uint8_t> d = in.bytes(dlen);
            mlz::SearchManyIndex ix;
            mlz::search_many_index(ps.blob.data(), ps.len.data(), npat, &ix);
            if (dlen < ix.lmin || dlen - ix.lmin + 1 > mlz::kSearchManyTile) { std::fprintf(stderr, "the data is no single tile\n"); return 2; }
            const mlz::SearchTile tl{0, 0, dlen - ix.lmin + 1, dlen};
            std::printf("%u %u :", ix.m, ix.hb);
            for (uint16_t v : ix.order) std::printf(" %u", v);
            std::printf(" |");
            mlz::search_many_tile_pairs(d.data(), tl, ix, ps.blob.data(), [&](uint32_t i, uint32_t p) { std::printf(" %u:%u", i, p); }, fold != 0);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown record %u\n", kind);
            return 2;
        }
    }
    return 0;
}
