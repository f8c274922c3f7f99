// stream_search_check.cpp — the rules of minlz_amd/csrc/mlz_stream_search.h on the host, for tests/test_stream_search_host.py:
//   g++ -O2 -std=c++17 -o ssc tools/stream_search_check.cpp && ./ssc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 count, count x (u64 val, u32 B, u32 M)               -> the hashes (search_hash)
//   kind 2  u32 nck, nw, L; nck x u32 a; nck x u32 s; nck x u64 n    -> the decoded set (search_decoded_set)
//   kind 3  u64 stream bytes, u32 L, u32 flags; the stream; pattern  -> "M B usable :" and the decoded set of a search over that stream, with the
//           tables found as search_info_kernel and search_locate_kernel find them (the same hops, search_info, search_table_reductions, the
//           CRC of the table bytes), probed by search_probe.  flags: 1 = MLZ_SEARCH_NO_TABLES, 2 = MLZ_STREAM_IGNORE_CRC
//   kind 4  u32 B; (B - 8 + 1) x u32 pop                             -> table bytes and R (search_reduce_rule)
//   kind 5  u32 nck, n_take, L; u64 group bytes, data bytes; nck x u64 n; n_take x u32 chunk; pattern; data
//           -> the occurrences found by search_layout's tiles (lmin = lmax = L, tiles of kSearchTile), executed as the search executes them: the taken chunks of a group copied to
//           their places in ONE reused scratch, every tile compared position by position, the carried bytes copied in front of the next
//           group: "count tiles groups scratch_max :" and the positions
// The prefix tables' rules (table types 2 and 3), for tests/test_stream_search_prefix_host.py:
//   kind 6  as kind 3, over a stream of any table type 1 .. 3                  -> "T M B usable nw t_min :" and the decoded set (usable, nw = 0: the tables
//           were not used)
//   kind 7  u32 nck, nw, L, t_min; nck x u32 a; nck x u32 s; nck x u64 n       -> the decoded set (search_decoded_set with t_min)
//   kind 8  u32 B, limit; (B - 8 + 1) x u32 pop                                -> table bytes and R (search_reduce_rule with the fold limit in per cent)
//   kind 9  u32 T, M, L; 32 bytes of prefix field; pattern                     -> "t_min :" and the starts of the checkable windows (search_windows)
// The long-prefix tables' rules (table type 4), for tests/test_stream_search_long_prefix_host.py:
//   kind 10 as kind 3, over a stream of any table type 1 .. 4                  -> "T M B usable ng t_min gsize :" and the decoded set (ng = the pattern's
//           groups of gsize windows; usable, ng = 0: the tables were not used)
//   kind 11 u32 M, L, field bytes; the field (K-1 | E | pfx); pattern          -> "t_min gsize :" and the start of every group's first window
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_search.h"
#include "../minlz_amd/csrc/mlz_search_compressed.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

uint32_t masked_crc(const uint8_t* p, size_t n) {   // minlz.go:133-140
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (c & 1 ? 0x82f63b78u : 0); tab[i] = c; }
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    c = ~c;
    return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

struct Data { uint64_t prev_end, body_off, n; };

void print_set(const std::vector<uint8_t>& take) {
    for (size_t k = 0; k < take.size(); k++) if (take[k]) std::printf(" %zu", k);
    std::printf("\n");
}

void run_stream(const uint8_t* s, uint64_t slen, const uint8_t* pat, uint32_t L, uint32_t flags, bool prefix_kind = false, bool long_kind = false) {
    // the data chunks (a valid stream: the walk's table)
    std::vector<Data> ck;
    uint64_t end = 0;
    for (uint64_t p = 0; p + 4 <= slen;) {
        const uint8_t type = s[p];
        const uint32_t clen = uint32_t(s[p + 1]) | uint32_t(s[p + 2]) << 8 | uint32_t(s[p + 3]) << 16;
        if (type == 1) ck.push_back(Data{end, p + 8, clen - 4});
        else if (type == 2 || type == 3) {
            uint64_t v = 0; unsigned sh = 0; uint64_t q = p + 8;
            for (;; q++) { v |= uint64_t(s[q] & 0x7f) << sh; sh += 7; if (s[q] < 0x80) { q++; break; } }
            ck.push_back(Data{end, q, v});
        }
        p += 4 + uint64_t(clen);
        if (type >= 1 && type <= 3) end = p;
    }
    const size_t nck = ck.size();
    auto is_data = [](uint8_t t) { return t >= 1 && t <= 3; };
    // search_info_kernel
    uint32_t M = 0, B = 0, T = 0;
    uint8_t field[mlz::kSearchMaxField] = {};
    bool ok = false, seen_id = false;
    const uint64_t limit0 = nck ? ck[0].body_off : slen;
    for (uint64_t p = 0; p + 4 <= limit0;) {
        const uint8_t type = s[p];
        const uint32_t clen = uint32_t(s[p + 1]) | uint32_t(s[p + 2]) << 8 | uint32_t(s[p + 3]) << 16;
        if (is_data(type)) break;
        if (type == 0xff) seen_id = true;
        else if (type == mlz::kChunkSearchInfo && seen_id) { if (p + 4 + clen <= limit0) ok = mlz::search_info(s + p + 4, clen, &T, &M, &B, field); break; }
        p += 4 + uint64_t(clen);
    }
    // search_locate_kernel and the CRC rounds
    std::vector<mlz::SearchTab> tabs(nck, mlz::SearchTab{0, 0, mlz::kSearchNoTable, 0, 0});
    std::vector<std::vector<uint8_t>> expanded(nck);   // the bitmaps of compressed tables (the handle's arena)
    size_t usable = 0;
    if (ok)
        for (size_t k = 0; k < nck; k++) {
            const uint64_t limit = ck[k].body_off;
            for (uint64_t p = ck[k].prev_end; p + 4 <= limit;) {
                const uint8_t type = s[p];
                const uint32_t clen = uint32_t(s[p + 1]) | uint32_t(s[p + 2]) << 8 | uint32_t(s[p + 3]) << 16;
                if (is_data(type)) break;
                if (type == mlz::kChunkSearchTable && p + 4 + clen <= limit) {
                    const int R = mlz::search_table_reductions(s + p + 4, clen, M, B, T, field);
                    const uint32_t f = mlz::search_field_len(T, field);
                    uint32_t crc = 0;
                    if (R >= 0) std::memcpy(&crc, s + p + 8 + f, 4);
                    if (R >= 0 && ((flags & 2) || masked_crc(s + p + 12 + f, clen - 8 - f) == crc)) { tabs[k] = mlz::SearchTab{p + 12 + f, clen - 8 - f, uint32_t(R), crc, 0}; usable++; break; }
                } else if (type == mlz::kChunkSearchTableCompressed && p + 4 + clen <= limit) {
                    // a compressed table: a candidate that cst_settle turns into a table in the arena, into no table (flags & 4: the arena
                    // could not be allocated) or into one that is passed over (cst_resolve's rounds: the same choice, made on the spot)
                    const int R = mlz::cst_fixed_fields(s + p + 4, clen, M, B, T, field);
                    if (R >= 0) {
                        mlz::CstPlan plan;
                        std::vector<uint8_t> bm(size_t(1) << (B - uint32_t(R) - 3));
                        const uint32_t f = mlz::search_field_len(T, field);
                        uint32_t stated = 0;
                        std::memcpy(&stated, s + p + 8 + f, 4);
                        tabs[k] = mlz::SearchTab{p + 4, clen, uint32_t(R), stated, mlz::kSearchTabArena};
                        const uint32_t good = mlz::cst_expand_host(s + p + 4, clen, bm.data(), bm.size(), &plan) == int64_t(bm.size()) ? 1 : 0;
                        const uint32_t crc = good ? masked_crc(bm.data(), bm.size()) : 0;
                        const uint64_t at = 0, size = bm.size();
                        std::vector<uint32_t> skip(nck, 0);
                        const bool again = mlz::cst_settle(&tabs, std::vector<size_t>{k}, &at, &size, (flags & 4) ? nullptr : &good, (flags & 2) ? nullptr : &crc, &skip);
                        if (again) tabs[k] = mlz::SearchTab{0, 0, mlz::kSearchNoTable, 0, 0};
                        else {
                            if (tabs[k].R != mlz::kSearchNoTable) { expanded[k] = std::move(bm); usable++; }
                            break;
                        }
                    }
                }
                p += 4 + uint64_t(clen);
            }
        }
    std::vector<uint8_t> take(nck, 0);
    std::vector<uint32_t> win(mlz::kSearchMaxWindows);
    uint32_t t_min = 1, gsize = 1;
    const uint32_t nw = !(flags & 1) && ok && usable ? mlz::search_windows(pat, L, T, M, field, win.data(), &t_min, &gsize) : 0;
    if (!nw) {
        for (size_t k = 0; k < nck; k++) take[k] = ck[k].n ? 1 : 0;
        if (long_kind) std::printf("%u %u %u 0 0 %u %u :", T, M, B, t_min, gsize);
        else if (prefix_kind) std::printf("%u %u %u 0 0 %u :", T, M, B, t_min);
        else std::printf("%u %u 0 :", M, B);
        print_set(take);
        return;
    }
    std::vector<uint32_t> h(nw * gsize), a(nck, nw), sv(nck, nw);
    for (uint32_t i = 0; i < nw * gsize; i++) {
        uint64_t v = 0;
        for (uint32_t j = 0; j < M; j++) v |= uint64_t(pat[win[i] + j]) << (8 * j);
        h[i] = mlz::search_hash(v, B, M);
    }
    for (size_t k = 0; k < nck; k++)
        if (tabs[k].R != mlz::kSearchNoTable) mlz::search_probe(tabs[k].pad ? expanded[k].data() : s + tabs[k].off, B - tabs[k].R, h.data(), nw, &a[k], &sv[k], gsize);
    mlz::search_decoded_set(nck, [&](size_t k) { return a[k]; }, [&](size_t k) { return sv[k]; }, [&](size_t k) { return ck[k].n; }, nw, L, take.data(), t_min);
    if (long_kind) std::printf("%u %u %u %zu %u %u %u :", T, M, B, usable, nw, t_min, gsize);
    else if (prefix_kind) std::printf("%u %u %u %zu %u %u :", T, M, B, usable, nw, t_min);
    else std::printf("%u %u %zu :", M, B, usable);
    print_set(take);
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
            const uint32_t count = in.get<uint32_t>();
            for (uint32_t i = 0; i < count; i++) {
                const uint64_t v = in.get<uint64_t>();
                const uint32_t B = in.get<uint32_t>(), M = in.get<uint32_t>();
                std::printf(" %u", mlz::search_hash(v, B, M));
            }
            std::printf("\n");
        } else if (kind == 2) {
            const uint32_t nck = in.get<uint32_t>(), nw = in.get<uint32_t>(), L = in.get<uint32_t>();
            std::vector<uint32_t> a(nck), s(nck);
            std::vector<uint64_t> n(nck);
            for (auto& v : a) v = in.get<uint32_t>();
            for (auto& v : s) v = in.get<uint32_t>();
            for (auto& v : n) v = in.get<uint64_t>();
            std::vector<uint8_t> take(nck);
            mlz::search_decoded_set(nck, [&](size_t k) { return a[k]; }, [&](size_t k) { return s[k]; }, [&](size_t k) { return n[k]; }, nw, L, take.data());
            print_set(take);
        } else if (kind == 3) {
            const uint64_t slen = in.get<uint64_t>();
            const uint32_t L = in.get<uint32_t>(), flags = in.get<uint32_t>();
            const uint8_t* s = in.bytes(size_t(slen));
            const uint8_t* pat = in.bytes(L);
            run_stream(s, slen, pat, L, flags);
        } else if (kind == 4) {
            const uint32_t B = in.get<uint32_t>();
            std::vector<uint32_t> pop(B - 8 + 1);
            for (auto& v : pop) v = in.get<uint32_t>();
            uint32_t R = 0;
            const uint32_t bytes = mlz::search_reduce_rule(pop.data(), B, &R);
            std::printf(" %u %u\n", bytes, R);
        } else if (kind == 5) {
            const uint32_t nck = in.get<uint32_t>(), n_take = in.get<uint32_t>(), L = in.get<uint32_t>();
            const uint64_t group_bytes = in.get<uint64_t>(), dlen = in.get<uint64_t>();
            std::vector<uint64_t> n(nck), off(nck);
            for (auto& v : n) v = in.get<uint64_t>();
            for (uint32_t k = 1; k < nck; k++) off[k] = off[k - 1] + n[k - 1];
            std::vector<uint32_t> jobs(n_take);
            for (auto& v : jobs) v = in.get<uint32_t>();
            const uint8_t* pat = in.bytes(L);
            const uint8_t* d = in.bytes(size_t(dlen));
            std::vector<size_t> gend;
            for (size_t i = 0; i < n_take;) {   // range_group_ends with the record's group size
                uint64_t acc = 0;
                while (i < n_take && acc < group_bytes) acc += n[jobs[i++]];
                gend.push_back(i);
            }
            mlz::SearchLayout lay;
            mlz::search_layout(n_take, gend, [&](size_t i) { return off[jobs[i]]; }, [&](size_t i) { return n[jobs[i]]; }, L, L, mlz::kSearchTile, &lay);
            std::vector<uint8_t> scratch(size_t(lay.scratch_max), 0xEE), keep(mlz::kSearchMaxPattern);
            std::vector<uint64_t> found;
            for (size_t g = 0, j0 = 0; g < gend.size(); j0 = gend[g++]) {
                for (size_t i = j0; i < gend[g]; i++) std::memcpy(scratch.data() + lay.at[i], d + off[jobs[i]], size_t(n[jobs[i]]));
                for (size_t t = g ? lay.tile_end[g - 1] : 0; t < lay.tile_end[g]; t++) {
                    const mlz::SearchTile& tl = lay.tiles[t];
                    if (tl.src_off < 1 || uint64_t(tl.src_off) + tl.count - 1 + L > lay.used[g]) { std::fprintf(stderr, "a tile reads outside the group's bytes\n"); return 3; }
                    for (uint32_t i = 0; i < tl.count; i++)
                        if (!std::memcmp(scratch.data() + tl.src_off + i, pat, L)) found.push_back(tl.gpos + i);
                }
                if (lay.carry[g]) {
                    std::memcpy(keep.data(), scratch.data() + lay.used[g] - lay.carry[g], lay.carry[g]);
                    std::memset(scratch.data(), 0xEE, scratch.size());   // (the next group overwrites the scratch)
                    std::memcpy(scratch.data() + mlz::kSearchPad - lay.carry[g], keep.data(), lay.carry[g]);
                } else std::memset(scratch.data(), 0xEE, scratch.size());
            }
            std::printf("%zu %zu %zu %llu :", found.size(), lay.tiles.size(), gend.size(), (unsigned long long)lay.scratch_max);
            for (uint64_t p : found) std::printf(" %llu", (unsigned long long)p);
            std::printf("\n");
        } else if (kind == 6) {
            const uint64_t slen = in.get<uint64_t>();
            const uint32_t L = in.get<uint32_t>(), flags = in.get<uint32_t>();
            const uint8_t* s = in.bytes(size_t(slen));
            const uint8_t* pat = in.bytes(L);
            run_stream(s, slen, pat, L, flags, true);
        } else if (kind == 7) {
            const uint32_t nck = in.get<uint32_t>(), nw = in.get<uint32_t>(), L = in.get<uint32_t>(), t_min = in.get<uint32_t>();
            std::vector<uint32_t> a(nck), s(nck);
            std::vector<uint64_t> n(nck);
            for (auto& v : a) v = in.get<uint32_t>();
            for (auto& v : s) v = in.get<uint32_t>();
            for (auto& v : n) v = in.get<uint64_t>();
            std::vector<uint8_t> take(nck);
            mlz::search_decoded_set(nck, [&](size_t k) { return a[k]; }, [&](size_t k) { return s[k]; }, [&](size_t k) { return n[k]; }, nw, L, take.data(), t_min);
            print_set(take);
        } else if (kind == 8) {
            const uint32_t B = in.get<uint32_t>(), limit = in.get<uint32_t>();
            std::vector<uint32_t> pop(B - 8 + 1);
            for (auto& v : pop) v = in.get<uint32_t>();
            uint32_t R = 0;
            const uint32_t bytes = mlz::search_reduce_rule(pop.data(), B, &R, limit);
            std::printf(" %u %u\n", bytes, R);
        } else if (kind == 9) {
            const uint32_t T = in.get<uint32_t>(), M = in.get<uint32_t>(), L = in.get<uint32_t>();
            const uint8_t* field = in.bytes(32);
            const uint8_t* pat = in.bytes(L);
            uint32_t win[mlz::kSearchMaxPattern], t_min = 0;
            const uint32_t nw = mlz::search_windows(pat, L, T, M, field, win, &t_min);
            std::printf("%u :", t_min);
            for (uint32_t i = 0; i < nw; i++) std::printf(" %u", win[i]);
            std::printf("\n");
        } else if (kind == 10) {
            const uint64_t slen = in.get<uint64_t>();
            const uint32_t L = in.get<uint32_t>(), flags = in.get<uint32_t>();
            const uint8_t* s = in.bytes(size_t(slen));
            const uint8_t* pat = in.bytes(L);
            run_stream(s, slen, pat, L, flags, true, true);
        } else if (kind == 11) {
            const uint32_t M = in.get<uint32_t>(), L = in.get<uint32_t>(), flen = in.get<uint32_t>();
            const uint8_t* field = in.bytes(flen);
            const uint8_t* pat = in.bytes(L);
            std::vector<uint32_t> win(mlz::kSearchMaxWindows);
            uint32_t t_min = 0, gsize = 0;
            const uint32_t ng = mlz::search_windows(pat, L, 4, M, field, win.data(), &t_min, &gsize);
            std::printf("%u %u :", t_min, gsize);
            for (uint32_t g = 0; g < ng; g++) std::printf(" %u", win[g * gsize]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown record %u\n", kind);
            return 2;
        }
    }
    return 0;
}
