// stream_search_batch_prune_check.cpp — the host code that mlz_stream_search_batch_device_pruned shares with its kernels
// (minlz_amd/csrc/mlz_stream_search_batch_prune.h: the info key, the classes, the class check, the hop to a chunk's table, a class's pattern
// records, the plan rule inside a chunk's own stream, the stats rule; mlz_stream_search.h: the probes and the rule), for
// tests/test_stream_search_batch_prune_host.py:
//   g++ -O2 -std=c++17 -o ssbp tools/stream_search_batch_prune_check.cpp && ./ssbp cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   u32 n_streams, npat, flags (2 = MLZ_STREAM_IGNORE_CRC, 32 = MLZ_SEARCH_IGNORE_CASE); n_streams x u64 stream bytes; npat x u32 len; the patterns;
//   the streams (valid ones), which the program lays back to back with three bytes between two
//   -> the call's plan as plain loops over what its kernels run lane by lane: every stream's key (batch_info_key), the classes
//      (batch_assign_classes), every stream against its class (batch_class_same), every class's pattern records (batch_class_patterns),
//      every data chunk's table (batch_locate, with the CRC rounds), every (chunk, pattern) through batch_plan_mark, batch_prune_stats:
//      "classes whole skipped tabbed decoded bad_keys home : the chunks taken of stream 0 | of stream 1 | ..." (chunk numbers inside the stream)
//      bad_keys: streams whose key disagrees with search_info on the same payload (0 for correct code); home: the bytes the call's plan
//      brings to the host by its own count (keys, class verdicts, a word per CRC round, a byte per chunk), which the test holds to batch_plan_bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_search_batch_prune.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

uint32_t masked_crc(const uint8_t* p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (c & 1 ? 0x82f63b78u : 0); tab[i] = c; }
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    c = ~c;
    return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

struct Data { uint64_t prev_end, body_off, n; };

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
        const uint32_t n = in.get<uint32_t>(), npat = in.get<uint32_t>(), flags = in.get<uint32_t>();
        if (n == 0 || npat == 0) { std::fprintf(stderr, "an empty record\n"); return 2; }
        const bool ignore_crc = (flags & 2) != 0, fold = (flags & 32) != 0;
        std::vector<uint64_t> slen(n), soff(n);
        for (auto& v : slen) v = in.get<uint64_t>();
        std::vector<uint32_t> off(npat + 1, 0);
        for (uint32_t i = 0; i < npat; i++) off[i + 1] = off[i] + in.get<uint32_t>();
        const uint8_t* pb = in.bytes(off[npat]);
        std::vector<uint8_t> blob(pb, pb + off[npat]);
        if (fold) for (auto& v : blob) v = mlz::search_fold(v);
        std::vector<uint8_t> src;   // (a buffer of exactly the batch's size: a read beyond it is a finding for the sanitizer)
        for (uint32_t i = 0; i < n; i++) {
            if (i) src.insert(src.end(), 3, 0xA5);
            soff[i] = src.size();
            const uint8_t* d = in.bytes(size_t(slen[i]));
            src.insert(src.end(), d, d + slen[i]);
        }
        const uint8_t* s = src.data();

        // the walk's table: every stream's data chunks, offsets counted from the batch's base
        std::vector<Data> ck;
        std::vector<mlz::BatchPlanStream> st(n);
        std::vector<uint32_t> chunk_stream;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c0 = uint32_t(ck.size());
            uint64_t end = soff[i];
            for (uint64_t p = soff[i]; p + 4 <= soff[i] + slen[i];) {
                const uint8_t type = s[p];
                const uint32_t clen = uint32_t(s[p + 1]) | uint32_t(s[p + 2]) << 8 | uint32_t(s[p + 3]) << 16;
                if (type == 1) ck.push_back(Data{end, p + 8, clen - 4});
                else if (type == 2 || type == 3) {
                    uint64_t v = 0; unsigned sh = 0; uint64_t q = p + 8;
                    for (;; q++) { v |= uint64_t(s[q] & 0x7f) << sh; sh += 7; if (s[q] < 0x80) { q++; break; } }
                    ck.push_back(Data{end, q, v});
                }
                p += 4 + uint64_t(clen);
                if (type >= 1 && type <= 3) { end = p; chunk_stream.push_back(i); }
            }
            const uint32_t c1 = uint32_t(ck.size());
            st[i] = mlz::BatchPlanStream{soff[i], c1 > c0 ? ck[c0].body_off : soff[i] + slen[i], c0, c1, mlz::kBatchPlanWhole, 0};
        }
        const size_t nck = ck.size();
        auto n_of = [&](size_t k) { return ck[k].n; };

        // search_batch_info_kernel, the classes, search_batch_class_kernel
        std::vector<mlz::BatchInfoKey> keys(n);
        std::vector<uint64_t> at(n, 0);
        uint64_t home = 0;
        std::vector<uint8_t> part(n, 1), cls(n);
        size_t bad_keys = 0;
        for (uint32_t i = 0; i < n; i++) {
            keys[i] = mlz::batch_info_key(s, st[i].start, st[i].limit, &at[i]);
            if (keys[i].ok) {
                mlz::SearchConfig cf{};
                const bool ok = mlz::search_info(s + at[i], 3u + keys[i].flen, &cf.T, &cf.M, &cf.B, cf.field);
                if (!ok || cf.T != keys[i].T || cf.M != keys[i].M || cf.B != keys[i].B || mlz::search_field_len(cf.T, cf.field) != keys[i].flen) bad_keys++;
            }
        }
        size_t rep[mlz::kSidecarMaxConfigs] = {};
        const uint32_t classes = mlz::batch_assign_classes(keys.data(), part.data(), n, cls.data(), rep);
        const uint32_t ncls = classes < mlz::kSidecarMaxConfigs ? classes : mlz::kSidecarMaxConfigs;
        std::vector<mlz::SearchConfig> cfg(mlz::kSidecarMaxConfigs);
        for (uint32_t c = 0; c < ncls; c++) {
            std::memset(&cfg[c], 0, sizeof(mlz::SearchConfig));
            cfg[c].ok = mlz::search_info(s + at[rep[c]], 3u + keys[rep[c]].flen, &cfg[c].T, &cfg[c].M, &cfg[c].B, cfg[c].field) ? 1 : 0;
        }
        std::vector<uint32_t> hs, voff;
        std::vector<mlz::SearchManyPat> pats(size_t(ncls ? ncls : 1) * npat);
        bool served[mlz::kSidecarMaxConfigs] = {};
        for (uint32_t c = 0; c < ncls; c++)
            served[c] = cfg[c].ok && mlz::batch_class_patterns(cfg[c], blob.data(), off.data(), npat, fold, pats.data() + size_t(c) * npat, &hs, &voff);
        for (uint32_t i = 0; i < n; i++)
            if (cls[i] != mlz::kBatchNoClass && mlz::batch_class_same(s + at[i], keys[i].flen, cfg[cls[i]]) && served[cls[i]]) { st[i].mode = mlz::kBatchPlanPrune; st[i].cls = cls[i]; }

        // the call's traffic so far: the keys, and the class verdicts when there is a class
        home += n * sizeof(mlz::BatchInfoKey) + (ncls ? n : 0);
        bool any_prune = false;
        for (uint32_t i = 0; i < n; i++) any_prune = any_prune || st[i].mode == mlz::kBatchPlanPrune;

        // search_batch_locate_kernel and the CRC rounds (search_batch_crc_desc_kernel's count, search_batch_crc_settle_kernel's rule)
        std::vector<mlz::SearchTab> tabs(nck, mlz::SearchTab{0, 0, mlz::kSearchNoTable, 0, 0});
        std::vector<uint32_t> skip(nck, 0);
        std::vector<uint8_t> redo(nck, 1);
        const uint64_t rounds = mlz::batch_crc_rounds(n) ? mlz::batch_crc_rounds(n) : 1;
        for (uint64_t round = 1; any_prune; round++) {
            for (size_t k = 0; k < nck; k++) {
                if (!redo[k]) continue;
                const mlz::BatchPlanStream& S = st[chunk_stream[k]];
                tabs[k] = S.mode == mlz::kBatchPlanPrune ? mlz::batch_locate(s, ck[k].prev_end, ck[k].body_off, skip[k], cfg[S.cls]) : mlz::SearchTab{0, 0, mlz::kSearchNoTable, 0, 0};
            }
            if (ignore_crc) break;
            uint64_t tiles = 0;
            for (size_t k = 0; k < nck; k++) if (redo[k] && tabs[k].R != mlz::kSearchNoTable) tiles += (tabs[k].bytes + 32767) >> 15;
            home += mlz::kBatchHomePerRound;
            if (!tiles) break;
            const bool last = round >= rounds;
            for (size_t k = 0; k < nck; k++) {
                if (!redo[k]) continue;
                const bool bad = tabs[k].R != mlz::kSearchNoTable && masked_crc(s + tabs[k].off, tabs[k].bytes) != tabs[k].crc;
                redo[k] = bad && !last;
                if (bad && !last) skip[k]++;
                if (bad && last) tabs[k].R = mlz::kSearchNoTable;
            }
            if (last) break;
        }
        if (any_prune) home += nck;
        if (nck == 0) home = 0;   // (the call plans nothing for a batch without data chunks)

        // search_batch_plan_kernel, lane by lane
        std::vector<uint8_t> take(nck, 0), tabbed(nck, 0);
        for (size_t k = 0; k < nck; k++) {
            tabbed[k] = tabs[k].R != mlz::kSearchNoTable;
            const mlz::BatchPlanStream& S = st[chunk_stream[k]];
            for (uint32_t p = 0; p < npat; p++) {
                if (S.mode != mlz::kBatchPlanPrune) {
                    if (p == 0) mlz::batch_plan_mark(k, S, mlz::SearchManyPat{0, 0, 1, 1, 1, 0}, [](size_t, bool) { return 0u; }, n_of, take.data());
                    continue;
                }
                const mlz::SearchManyPat pt = pats[size_t(S.cls) * npat + p];
                const uint32_t B = cfg[S.cls].B;
                auto probe = [&](size_t j, bool lead) {
                    const mlz::SearchTab t = tabs[j];
                    uint32_t a = pt.nw, sv = pt.nw;
                    if (t.R != mlz::kSearchNoTable) {
                        if (fold) mlz::search_probe_fold(s + t.off, B - t.R, voff.data() + pt.h_off, hs.data(), pt.nw, &a, &sv, pt.gsize);
                        else mlz::search_probe(s + t.off, B - t.R, hs.data() + pt.h_off, pt.nw, &a, &sv, pt.gsize);
                    }
                    return lead ? a : sv;
                };
                mlz::batch_plan_mark(k, S, pt, probe, n_of, take.data());
            }
        }
        uint64_t s4 = 0, s5 = 0, s7 = 0, decoded = 0;
        mlz::batch_prune_stats(st.data(), n, take.data(), tabbed.data(), n_of, &s4, &s5, &s7);
        for (size_t k = 0; k < nck; k++) decoded += take[k];
        std::printf("%u %llu %llu %llu %llu %zu %llu :", classes, (unsigned long long)s7, (unsigned long long)s5, (unsigned long long)s4, (unsigned long long)decoded, bad_keys,
                    (unsigned long long)home);
        for (uint32_t i = 0; i < n; i++) {
            if (i) std::printf(" |");
            for (uint32_t k = st[i].c0; k < st[i].c1; k++) if (take[k]) std::printf(" %u", k - st[i].c0);
        }
        std::printf("\n");
    }
    return 0;
}
