// search_prefold_check.cpp — the pre-fold rule of minlz_amd/csrc/mlz_stream_search.h (search_prefold, search_table_marks) on the host, for
// tests/test_stream_encode_batch_tables_host.py:
//   g++ -O2 -std=c++17 -o spc tools/search_prefold_check.cpp && ./spc cases.bin
// A block's table is built twice: in full (2^B bits, then search_reduce_rule over the counts of every fold, as stab_build_kernel and
// stab_reduce_kernel do it) and pre-folded (2^(B - r0) bits, bit h & (2^(B - r0) - 1), then the fold rule from R = r0, as the pre-folded
// kernels do it).  The two must be the same (table, R); a pre-folded table must never meet the 70 % rule, and every fold up to r0 must be one
// the full rule accepts.  The program first runs its own blocks — designed ones (empty, shorter than a window, all one byte, every byte a
// prefix byte, lengths around the thresholds where r0 changes) and pseudo-random ones — and then the case file's records, little-endian:
//   u32 T, M, B, n, follow (0xffffffff: the stream's last block, else the bytes that follow it), field bytes; the field; n bytes; the follow bytes
// with one output line each: "r0 R bytes crc" (crc: the masked CRC of the table, as its chunk would carry it; "r0 0 0 0" for a dropped table).
// An exit status other than 0 says what differed.
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

uint32_t masked_crc(const uint8_t* p, size_t n) {   // minlz.go:133-140
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (c & 1 ? 0x82f63b78u : 0); tab[i] = c; }
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    c = ~c;
    return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

constexpr uint32_t kLast = 0xffffffffu;

struct Block {
    uint32_t T, M, B;
    std::vector<uint8_t> field, data, follow;
    bool last;   // the stream's last block: `follow` is empty and nothing behind the block is indexed
};

// hit(h) for every hash the block's table holds (SPEC_SEARCH.md 3.3; the kernels' positions): the block's bytes, then the stream's bytes that
// follow it (the overlap's at the most), then zeros; a long prefix lies inside the stream's bytes
template <class Hit>
void indexed(const Block& k, Hit hit) {
    const uint32_t ov = mlz::search_overlap(k.T, k.M, k.field.data());
    const size_t n = k.data.size(), real = n + (k.last ? 0 : std::min<size_t>(ov, k.follow.size()));
    auto at = [&](size_t q) -> uint64_t { return q < n ? k.data[q] : q < real ? k.follow[q - n] : 0; };
    auto window = [&](size_t q) {
        uint64_t v = 0;
        if (q + 8 <= n) std::memcpy(&v, k.data.data() + q, 8);   // (a little-endian host)
        else for (uint32_t j = 0; j < 8; j++) v |= at(q + j) << (8 * j);
        return mlz::search_hash(v, k.B, k.M);
    };
    if (k.T == 1) {
        const size_t npos = k.last ? (n + 1 >= k.M ? n + 1 - k.M : 0) : n;
        for (size_t q = 0; q < npos; q++) hit(window(q));
    } else if (k.T != 4) {
        uint32_t mask[8];
        mlz::search_prefix_mask(k.T, k.field.data(), mask);
        const size_t hi = k.last ? (n >= k.M ? n - k.M : 0) : n;
        for (size_t q = 1; q <= hi; q++) if (mlz::search_is_prefix(mask, uint8_t(at(q - 1)))) hit(window(q));
    } else {
        const uint32_t K = mlz::search_long_k(k.field.data()), E = mlz::search_long_e(k.field.data());
        const uint8_t* pfx = mlz::search_long_prefix(k.field.data());
        const size_t starts = k.last ? (n >= size_t(K) + k.M + E ? n - K - k.M - E + 1 : 0) : n;
        for (size_t p = 0; p < starts; p++) {
            if (p + K > real) break;
            uint32_t j = 0;
            while (j < K && at(p + j) == pfx[j]) j++;
            if (j == K) for (uint32_t e = 0; e <= E; e++) hit(window(p + K + e));
        }
    }
}

// A table: 64-bit words, bit h at word h >> 6 (on a little-endian host the table's bytes as a chunk carries them)
using Table = std::vector<uint64_t>;
void set_bit(Table& t, uint32_t h) { t[h >> 6] |= uint64_t(1) << (h & 63); }
uint32_t popcount(const Table& t) { uint32_t s = 0; for (uint64_t v : t) s += uint32_t(__builtin_popcountll(v)); return s; }
Table folded(const Table& t) {
    Table h(t.size() / 2);
    for (size_t i = 0; i < h.size(); i++) h[i] = t[i] | t[h.size() + i];
    return h;
}

struct Result { uint32_t r0, R; Table table; };   // an empty table: dropped

// Both builds of one block; exits when they differ
Result check(const Block& k, const char* what) {
    const uint32_t B = k.B, limit = mlz::search_fold_limit(k.T);
    // in full: every fold's count, then the rule
    std::vector<Table> t(1, Table(size_t(1) << (B - 6), 0));
    indexed(k, [&](uint32_t h) { set_bit(t[0], h); });
    std::vector<uint32_t> pop{popcount(t[0])};
    for (uint32_t r = 1; r <= B - 8; r++) { t.push_back(folded(t.back())); pop.push_back(popcount(t.back())); }
    uint32_t R = 0;
    const uint32_t bytes = mlz::search_reduce_rule(pop.data(), B, &R, limit);
    // pre-folded
    const uint64_t marks = mlz::search_table_marks(k.T, k.M, k.field.data(), k.data.size(), !k.last);
    const uint32_t r0 = mlz::search_prefold(marks, B, limit);
    if (pop[0] > marks) { std::fprintf(stderr, "%s: %u bits set by %llu positions\n", what, pop[0], (unsigned long long)marks); std::exit(1); }
    Table f(size_t(1) << (B - r0 - 6), 0);
    const uint32_t fmask = (1u << (B - r0)) - 1;
    indexed(k, [&](uint32_t h) { set_bit(f, h & fmask); });
    uint32_t Rf = r0;
    if (r0 && mlz::search_table_dropped(popcount(f), B)) { std::fprintf(stderr, "%s: a pre-folded table met the 70 %% rule\n", what); std::exit(1); }
    if (!r0 && mlz::search_table_dropped(popcount(f), B)) f.clear();
    while (f.size() * 8 >= 64) {
        Table h = folded(f);
        if (!mlz::search_fold_accepted(popcount(h), uint64_t(h.size()) * 64, limit)) break;
        f.swap(h); Rf++;
    }
    if (r0 > R && bytes) { std::fprintf(stderr, "%s: r0 = %u, the full rule stops at R = %u\n", what, r0, R); std::exit(1); }
    const Table none;
    const Table& full = bytes ? t[R] : none;
    if (full.size() * 8 != bytes || f != full || (bytes && Rf != R)) {
        std::fprintf(stderr, "%s: T %u M %u B %u n %zu last %d: full (%u bytes, R %u), pre-folded from %u (%zu bytes, R %u)\n", what, k.T, k.M, B, k.data.size(), int(k.last), bytes, R, r0, f.size() * 8, Rf);
        std::exit(1);
    }
    return Result{r0, bytes ? R : 0, f};
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return uint32_t(rng_state >> 32); }

std::vector<uint8_t> field_of(uint32_t T, const char* pfx, uint32_t E) {
    std::vector<uint8_t> f(mlz::kSearchMaxField + 2, 0);
    const size_t n = std::strlen(pfx);
    if (T == 2) for (uint32_t i = 0; i < 8; i++) f[i] = uint8_t(pfx[i < n ? i : n - 1]);
    if (T == 3) for (size_t i = 0; i < n; i++) f[uint8_t(pfx[i]) >> 3] |= uint8_t(1u << (pfx[i] & 7));
    if (T == 4) { f[0] = uint8_t(n - 1); f[1] = uint8_t(E); std::memcpy(f.data() + 2, pfx, n); }
    return f;
}

// text-like bytes with the prefixes of the configurations in them, or noise
std::vector<uint8_t> bytes_of(size_t n, int kind) {
    static const char* words[] = {"\"user\":\"", "alpha", "\":, ", "{\"id\":", "12345", " ", "beta\n", "\"", ","};
    std::vector<uint8_t> d;
    d.reserve(n + 16);
    while (d.size() < n) {
        if (kind == 0) d.push_back(uint8_t(rnd()));
        else if (kind == 1) { const char* w = words[rnd() % 9]; d.insert(d.end(), w, w + std::strlen(w)); }
        else d.push_back(uint8_t('a' + rnd() % 3));
    }
    d.resize(n);
    return d;
}

size_t self_check() {
    struct Cfg { uint32_t T, M; const char* pfx; uint32_t E; };
    const Cfg cfgs[] = {{1, 6, "", 0}, {1, 1, "", 0}, {1, 2, "", 0}, {1, 8, "", 0}, {2, 6, "\":, ", 0}, {2, 1, "\"", 0}, {3, 6, "\":,{}[] \n-_", 0},
                        {4, 4, "\"user\":\"", 3}, {4, 1, "\"", 15}};
    const uint32_t Bs[] = {12, 16, 20, 22};
    size_t done = 0;
    for (const Cfg& c : cfgs)
        for (uint32_t B : Bs) {
            Block k{c.T, c.M, B, field_of(c.T, c.pfx, c.E), {}, {}, false};
            const uint32_t limit = mlz::search_fold_limit(c.T);
            // designed lengths: nothing, shorter than a window, and the lengths around which r0 changes (marks * 100 = 2^(B - r) * limit)
            std::vector<size_t> ns{0, 1, size_t(c.M - 1), size_t(c.M), 7, 8, 31, 100, 4095, 4096, 4097, size_t(1) << B};
            if (B < 20) { ns.push_back(size_t(1) << (B - 1)); ns.push_back((size_t(1) << B) - 1); }
            for (uint32_t r = 1; r <= B - 8; r += 3) {
                const size_t edge = size_t((uint64_t(1) << (B - r)) * limit / 100);
                for (size_t d = 0; d < 3; d++) ns.push_back(edge + d > 0 ? edge + d - 1 : 0);
            }
            const bool big = B >= 20;   // (tables of 128 KiB and more, and blocks of 8 KiB and more: fewer forms, for time)
            size_t turn = 0;
            for (size_t n : ns) {
                if (n > (size_t(1) << B)) continue;
                for (int kind = 0; kind < 4; kind++) {
                    // kind 3: all one byte, and that byte a prefix byte of the types that have one (every position is indexed, into one bit)
                    k.data = kind == 3 ? std::vector<uint8_t>(n, uint8_t('"')) : bytes_of(n, kind);
                    for (int fol = 0; fol < 4; fol++) {
                        if ((big || n >= 8192) && turn++ % 16 != (n + B) % 16) continue;   // one (kind, follow) form per length, a different one from length to length
                        k.last = fol == 0;
                        k.follow = fol <= 1 ? std::vector<uint8_t>() : bytes_of(fol == 2 ? 2 : 300, 1);
                        check(k, "self check");
                        done++;
                    }
                }
            }
            // pseudo-random lengths
            for (int i = 0; i < (big ? 4 : 24); i++) {
                k.data = bytes_of(rnd() % (std::min<size_t>(size_t(1) << B, 20000) + 1), int(rnd() % 3));
                k.last = rnd() & 1;
                k.follow = k.last ? std::vector<uint8_t>() : bytes_of(rnd() % 400, 1);
                check(k, "self check, random");
                done++;
            }
        }
    return done;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    In in;
    {
        FILE* f = std::fopen(argv[argc - 1], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[argc - 1]); return 2; }
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.b.insert(in.b.end(), buf, buf + n);
        std::fclose(f);
    }
    std::printf("self %zu\n", self_check());
    while (in.p < in.b.size()) {
        Block k{};
        k.T = in.get<uint32_t>(); k.M = in.get<uint32_t>(); k.B = in.get<uint32_t>();
        const uint32_t n = in.get<uint32_t>(), fol = in.get<uint32_t>(), flen = in.get<uint32_t>();
        if (k.T < 1 || k.T > 4 || k.M < 1 || k.M > 8 || k.B < 8 || k.B > 23 || flen > mlz::kSearchMaxField) { std::fprintf(stderr, "bad record\n"); return 2; }
        const uint8_t* f = in.bytes(flen);
        k.field.assign(mlz::kSearchMaxField + 2, 0);
        std::memcpy(k.field.data(), f, flen);
        const uint8_t* d = in.bytes(n);
        k.data.assign(d, d + n);
        k.last = fol == kLast;
        if (!k.last) { const uint8_t* q = in.bytes(fol); k.follow.assign(q, q + fol); }
        const Result r = check(k, "record");
        std::printf("%u %u %zu %u\n", r.r0, r.R, r.table.size() * 8, r.table.empty() ? 0u : masked_crc(reinterpret_cast<const uint8_t*>(r.table.data()), r.table.size() * 8));
    }
    return 0;
}
