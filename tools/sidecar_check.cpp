// sidecar_check.cpp — the sidecar rules of minlz_amd/csrc/mlz_stream_search.h on the host, for tests/test_sidecar_host.py:
//   g++ -O2 -std=c++17 -o sc tools/sidecar_check.cpp && ./sc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 nck, n_sets, L; per set: u32 nw (0 = the set cannot vote), t_min, ov (the set's overlap), nck x u32 a, nck x u32 s; nck x u64 n
//           -> the decoded set over several table sets (search_chunk_candidate per set, search_decoded_mark_all)
//   kind 2  u64 offset, max - actual                      -> the bytes of the 0x47 chunk in hex (sidecar_put_ref; sidecar_ref_bytes must agree)
//   kind 3  u32 payload bytes; u64 max block; the payload -> "-1" or the references `offset:size` (sidecar_parse_refs)
//   kind 4  u64 sidecar bytes, main stream bytes; u32 L, flags; the sidecar; the main stream; the pattern
//           -> "error" for a sidecar the attach refuses, else "n_sets usable :" and the decoded set of a search for the pattern, with
//           the attach done as sidecar_info_kernel and sidecar_attach_kernel do it (the configurations from the head of the chunk list,
//           sidecar_check_refs per 0x47 against the main stream's data chunks, per configuration the first fitting 0x45 or 0x46 in front of it
//           with a good CRC, a 0x46 table expanded by the rules of mlz_search_compressed.h) and the plan as search_plan_kernel does it.  flags: 2 = MLZ_STREAM_IGNORE_CRC.  Both streams are well framed (the
//           walk's own errors are the walk's to check: tools/stream_walk_check.cpp).
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

void print_set(const std::vector<uint8_t>& take) {
    for (size_t k = 0; k < take.size(); k++) if (take[k]) std::printf(" %zu", k);
    std::printf("\n");
}

struct Chunk { uint64_t off; uint8_t type; uint32_t clen; };
std::vector<Chunk> chunks_of(const uint8_t* s, uint64_t n) {
    std::vector<Chunk> out;
    for (uint64_t p = 0; p + 4 <= n;) {
        const uint32_t clen = uint32_t(s[p + 1]) | uint32_t(s[p + 2]) << 8 | uint32_t(s[p + 3]) << 16;
        out.push_back(Chunk{p, s[p], clen});
        p += 4 + uint64_t(clen);
    }
    return out;
}

struct Set { uint32_t nw, t_min, gsize, ov; std::vector<uint32_t> a, s; };

// The rule over several table sets, as search_plan_kernel applies it
void decoded_set_all(const std::vector<Set>& sets, const std::vector<uint64_t>& n, uint32_t L, std::vector<uint8_t>* take) {
    const size_t nck = n.size();
    take->assign(nck, 0);
    auto sizes = [&](size_t j) { return n[j]; };
    for (size_t k = 0; k < nck; k++) {
        auto admits = [&](uint32_t c) {
            const Set& st = sets[c];
            if (!st.nw) return true;
            return mlz::search_chunk_candidate(k, nck, [&](size_t j) { return st.a[j]; }, [&](size_t j) { return st.s[j]; }, sizes, st.nw, L, st.t_min, st.ov);
        };
        mlz::search_decoded_mark_all(k, nck, uint32_t(sets.size()), admits, sizes, L, take->data());
    }
}

void run_attach(const uint8_t* side, uint64_t ns, const uint8_t* mainb, uint64_t nm, const uint8_t* pat, uint32_t L, uint32_t flags) {
    // the main stream's data chunks: header offset and decoded bytes
    std::vector<uint64_t> hdr, n;
    for (const Chunk& c : chunks_of(mainb, nm)) {
        if (c.type == 1) { hdr.push_back(c.off); n.push_back(c.clen - 4); }
        else if (c.type == 2 || c.type == 3) {
            uint64_t v = 0;
            mlz::walk_uvarint(mainb + c.off + 8, c.clen - 4, &v);
            hdr.push_back(c.off); n.push_back(v);
        }
    }
    const size_t nck = hdr.size();
    const std::vector<Chunk> rec = chunks_of(side, ns);
    uint64_t max_block = 0;
    for (const Chunk& c : rec) if (c.type == 0xff) { max_block = uint64_t(1) << ((side[c.off + 9] & 15) + 10); break; }
    // sidecar_info_kernel
    std::vector<mlz::SearchConfig> cfg;
    for (const Chunk& c : rec) {
        if (c.type == mlz::kChunkSearchTable || c.type == mlz::kChunkSearchTableCompressed || c.type == mlz::kChunkRemoteRef || cfg.size() == mlz::kSidecarMaxConfigs) break;
        if (c.type != mlz::kChunkSearchInfo) continue;
        mlz::SearchConfig o{};
        if (mlz::search_info(side + c.off + 4, c.clen, &o.T, &o.M, &o.B, o.field)) cfg.push_back(o);
    }
    // sidecar_attach_kernel, with the CRC decided on the spot (the kernel's rounds pass over broken tables one by one: the same choice)
    const mlz::SearchTab none{0, 0, mlz::kSearchNoTable, 0, 0};
    std::vector<std::vector<mlz::SearchTab>> tabs(cfg.size(), std::vector<mlz::SearchTab>(nck, none));
    std::vector<std::vector<std::vector<uint8_t>>> expanded(cfg.size(), std::vector<std::vector<uint8_t>>(nck));   // the bitmaps of 0x46 tables (the arena)
    bool bad = false;
    for (size_t i = 0; i < rec.size() && !bad; i++) {
        if (rec[i].type != mlz::kChunkRemoteRef) continue;
        size_t j = i;
        while (j > 0 && rec[j - 1].type != mlz::kChunkRemoteRef) j--;
        bool have_floor = false;
        uint64_t floor = 0, last = 0;
        if (j > 0) have_floor = mlz::sidecar_parse_refs(side + rec[j - 1].off + 4, rec[j - 1].clen, max_block, [&](uint64_t off, uint64_t) { floor = off; }) > 0;
        const int64_t k = mlz::sidecar_check_refs(side + rec[i].off + 4, rec[i].clen, max_block, nck, [&](size_t q) { return hdr[q]; }, [&](size_t q) { return n[q]; },
                                                  have_floor, floor, &last);
        if (k < 0) { bad = true; break; }
        for (size_t c = 0; c < cfg.size(); c++)
            for (size_t t = j; t < i; t++) {
                if (rec[t].type != mlz::kChunkSearchTable && rec[t].type != mlz::kChunkSearchTableCompressed) continue;
                const uint8_t* p = side + rec[t].off + 4;
                if (rec[t].type == mlz::kChunkSearchTableCompressed) {   // a candidate: expanded, or passed over (cst_settle)
                    const int R = mlz::cst_fixed_fields(p, rec[t].clen, cfg[c].M, cfg[c].B, cfg[c].T, cfg[c].field);
                    if (R < 0) continue;
                    mlz::CstPlan plan;
                    std::vector<uint8_t> bm(size_t(1) << (cfg[c].B - uint32_t(R) - 3));
                    uint32_t stated = 0;
                    std::memcpy(&stated, p + 4 + mlz::search_field_len(cfg[c].T, cfg[c].field), 4);
                    std::vector<mlz::SearchTab> one{mlz::SearchTab{rec[t].off + 4, rec[t].clen, uint32_t(R), stated, mlz::kSearchTabArena}};
                    const uint32_t good = mlz::cst_expand_host(p, rec[t].clen, bm.data(), bm.size(), &plan) == int64_t(bm.size()) ? 1 : 0;
                    const uint32_t crc = good ? masked_crc(bm.data(), bm.size()) : 0;
                    const uint64_t at = 0, size = bm.size();
                    std::vector<uint32_t> skip(1, 0);
                    if (mlz::cst_settle(&one, std::vector<size_t>{0}, &at, &size, &good, (flags & 2) ? nullptr : &crc, &skip)) continue;
                    tabs[c][size_t(k)] = one[0];
                    expanded[c][size_t(k)] = std::move(bm);
                    break;
                }
                const int R = mlz::search_table_reductions(p, rec[t].clen, cfg[c].M, cfg[c].B, cfg[c].T, cfg[c].field);
                if (R < 0) continue;
                const uint32_t f = mlz::search_field_len(cfg[c].T, cfg[c].field);
                uint32_t crc = 0;
                std::memcpy(&crc, p + 4 + f, 4);
                if (!(flags & 2) && masked_crc(p + 8 + f, rec[t].clen - 8 - f) != crc) continue;
                tabs[c][size_t(k)] = mlz::SearchTab{rec[t].off + 12 + f, rec[t].clen - 8 - f, uint32_t(R), crc, 0};
                break;
            }
    }
    if (bad) { std::printf("error\n"); return; }
    // the plan
    std::vector<Set> sets(cfg.size());
    std::vector<uint32_t> win(mlz::kSearchMaxWindows);
    bool any_table = false;
    for (size_t c = 0; c < cfg.size(); c++) for (size_t k = 0; k < nck; k++) any_table = any_table || tabs[c][k].R != mlz::kSearchNoTable;
    uint32_t serving = 0;
    for (size_t c = 0; c < cfg.size() && any_table; c++) {
        std::vector<uint32_t> hs;
        mlz::SearchManyPat pt{0, 0, 1, 1, L, 0};
        Set& st = sets[c];
        st.nw = 0;
        st.ov = mlz::search_overlap(cfg[c].T, cfg[c].M, cfg[c].field);
        if (!mlz::search_pattern_hashes(pat, L, cfg[c].T, cfg[c].M, cfg[c].B, cfg[c].field, win.data(), &hs, &pt)) continue;
        serving |= 1u << c;
        st.nw = pt.nw; st.t_min = pt.t_min; st.gsize = pt.gsize;
        st.a.assign(nck, pt.nw); st.s.assign(nck, pt.nw);
        for (size_t k = 0; k < nck; k++)
            if (tabs[c][k].R != mlz::kSearchNoTable) mlz::search_probe(tabs[c][k].pad ? expanded[c][k].data() : side + tabs[c][k].off, cfg[c].B - tabs[c][k].R, hs.data(), pt.nw, &st.a[k], &st.s[k], pt.gsize);
    }
    size_t usable = 0;
    for (size_t k = 0; k < nck; k++) {
        bool any = false;
        for (size_t c = 0; c < cfg.size(); c++) any = any || (((serving >> c) & 1) && tabs[c][k].R != mlz::kSearchNoTable);
        usable += any ? 1 : 0;
    }
    if (!usable) for (Set& st : sets) st.nw = 0;   // (no table that serves: every chunk)
    std::vector<uint8_t> take;
    decoded_set_all(sets, n, L, &take);
    std::printf("%zu %zu :", cfg.size(), usable);
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
            const uint32_t nck = in.get<uint32_t>(), n_sets = in.get<uint32_t>(), L = in.get<uint32_t>();
            std::vector<Set> sets(n_sets);
            for (Set& st : sets) {
                st.nw = in.get<uint32_t>(); st.t_min = in.get<uint32_t>(); st.ov = in.get<uint32_t>(); st.gsize = 1;
                st.a.resize(nck); st.s.resize(nck);
                for (auto& v : st.a) v = in.get<uint32_t>();
                for (auto& v : st.s) v = in.get<uint32_t>();
            }
            std::vector<uint64_t> n(nck);
            for (auto& v : n) v = in.get<uint64_t>();
            std::vector<uint8_t> take;
            decoded_set_all(sets, n, L, &take);
            print_set(take);
        } else if (kind == 2) {
            const uint64_t off = in.get<uint64_t>(), mma = in.get<uint64_t>();
            uint8_t b[mlz::kSidecarRefBound];
            const uint32_t nb = mlz::sidecar_put_ref(b, off, mma);
            if (nb != mlz::sidecar_ref_bytes(off, mma) || nb > mlz::kSidecarRefBound) { std::fprintf(stderr, "sidecar_ref_bytes disagrees\n"); return 3; }
            for (uint32_t i = 0; i < nb; i++) std::printf("%02x", b[i]);
            std::printf("\n");
        } else if (kind == 3) {
            const uint32_t clen = in.get<uint32_t>();
            const uint64_t max_block = in.get<uint64_t>();
            const uint8_t* q = in.bytes(clen);
            const std::vector<uint8_t> payload(q, q + clen);   // (a copy of exactly clen bytes: a read beyond it is a sanitizer's finding)
            std::vector<std::pair<uint64_t, uint64_t>> refs;
            const int cnt = mlz::sidecar_parse_refs(payload.data(), clen, max_block, [&](uint64_t off, uint64_t size) { refs.push_back({off, size}); });
            if (cnt < 0) std::printf("-1\n");
            else {
                for (auto& r : refs) std::printf(" %llu:%llu", (unsigned long long)r.first, (unsigned long long)r.second);
                std::printf("\n");
            }
        } else if (kind == 4) {
            const uint64_t ns = in.get<uint64_t>(), nm = in.get<uint64_t>();
            const uint32_t L = in.get<uint32_t>(), flags = in.get<uint32_t>();
            const uint8_t* side = in.bytes(size_t(ns));
            const uint8_t* mainb = in.bytes(size_t(nm));
            const uint8_t* pat = in.bytes(L);
            run_attach(side, ns, mainb, nm, pat, L, flags);
        } else {
            std::fprintf(stderr, "unknown record %u\n", kind);
            return 2;
        }
    }
    return 0;
}
