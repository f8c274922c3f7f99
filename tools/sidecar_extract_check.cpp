// sidecar_extract_check.cpp — the rules of minlz_amd/csrc/mlz_stream_sidecar_extract.h on the host, for tests/test_sidecar_extract_host.py:
// extract_classify, extract_gap_scan, extract_pieces, extract_layout and extract_emit_gap against a serial restatement of the reference's
// ExtractSidecar that walks the chunks in order and knows nothing of gaps.  Stand-alone: g++ -std=c++17, also with -fsanitize=address,undefined.
//
//   sidecar_extract_check <case file>        records back to back; one line per record, exit status 1 at the first disagreement
//     kind 1: u32 seed, u32 count             `count` pseudo-random streams, whole in memory, both modes: layout, emit, the descriptors
//                                             run as memcpy (every output byte written exactly once), bytes equal to the restatement's
//     kind 2: u32 seed                        designed and pseudo-random VIRTUAL streams (data chunks without bytes, gaps with): offsets on
//                                             both sides of 2^14, 2^21, 2^28, 2^35, max - actual of 0, 127, 128: the layout alone
//     kind 3: u32 strip, u32 foot, u64 n,     one real stream through scan, layout and emit -> `side <hex> main <hex> counts`, which the
//             the foot's bytes, the stream    test holds against tests/sidecar_extract_model.py
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_sidecar_extract.h"

using namespace mlz;

static uint64_t rng_state = 1;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint64_t below(uint64_t n) { return rnd() % n; }

[[noreturn]] static void fail(const char* what, long a = 0, long b = 0) { std::fprintf(stderr, "disagreement: %s (%ld, %ld)\n", what, a, b); std::exit(1); }

// One chunk of a stream as the restatement sees it; virt: a data chunk without bytes
struct Item { uint8_t type; uint64_t clen, decoded; };
static bool is_data(uint8_t t) { return t == 1 || t == 2 || t == 3; }
static uint32_t uvarint_len(uint64_t v) { uint32_t n = 1; while (v >= 0x80) { v >>= 7; n++; } return n; }
static void put_uvarint(std::vector<uint8_t>& o, uint64_t v) { while (v >= 0x80) { o.push_back(uint8_t(v) | 0x80); v >>= 7; } o.push_back(uint8_t(v)); }
static void pieces_of(uint64_t len, uint32_t* nl, uint32_t* ns) {
    for (uint64_t o = 0; o < len; o += 65536) (len - o <= 1024 ? *ns : *nl)++;
}

// ExtractSidecar, chunk by chunk (sidecar.go:600-770) over items whose offsets are the running sum; src may be null (a virtual stream)
struct Serial {
    uint64_t side_len = 10, main_len = 10, blocks = 0, info = 0, tables = 0, tables46 = 0, passed = 0, dropped = 0;
    uint32_t n_long = 0, n_short = 0;
    std::vector<uint64_t> new_hdr, gap_side, gap_main;   // per data chunk; per gap: where its first byte goes
    std::vector<uint8_t> side, main;
};
static Serial serial(const std::vector<Item>& items, const uint8_t* src, uint64_t max_block, bool strip, const std::vector<uint8_t>& foot, const uint8_t ident[10]) {
    Serial s;
    if (src) { s.side.assign(ident, ident + 10); if (strip) s.main.assign(ident, ident + 10); }
    uint64_t p = 0;
    s.gap_side.push_back(10); s.gap_main.push_back(10);
    for (const Item& it : items) {
        const uint64_t len = 4 + it.clen;
        if (it.type == 0x44 || it.type == 0x45 || it.type == 0x46) {
            if (src) s.side.insert(s.side.end(), src + p, src + p + len);
            s.side_len += len;
            pieces_of(len, &s.n_long, &s.n_short);
            if (it.type == 0x44) s.info++; else s.tables++;
            if (it.type == 0x46) s.tables46++;
        } else if (is_data(it.type)) {
            const uint64_t ref = strip ? s.main_len : p;
            s.new_hdr.push_back(ref);
            if (strip) {
                if (src) s.main.insert(s.main.end(), src + p, src + p + len);
                s.main_len += len;
                pieces_of(len, &s.n_long, &s.n_short);
            }
            const uint32_t rl = uvarint_len(ref) + uvarint_len(max_block - it.decoded);
            if (src) {
                s.side.push_back(0x47); s.side.push_back(uint8_t(rl)); s.side.push_back(0); s.side.push_back(0);
                put_uvarint(s.side, ref); put_uvarint(s.side, max_block - it.decoded);
            }
            s.side_len += 4 + rl;
            s.blocks++;
            s.gap_side.push_back(s.side_len); s.gap_main.push_back(s.main_len);
        } else if (it.type == 0x20) {
            const uint8_t eof[5] = {0x20, 1, 0, 0, 0};
            if (src) s.side.insert(s.side.end(), eof, eof + 5);
            s.side_len += 5;
            if (strip) {
                if (src) s.main.insert(s.main.end(), foot.begin(), foot.end());
                s.main_len += foot.size();
                pieces_of(foot.size(), &s.n_long, &s.n_short);
            }
        } else if (it.type == 0x40 || it.type == 0x99) {
            if (strip) s.dropped += len;
        } else if (it.type == 0xff) {
        } else {
            if (it.type <= 0x3f) fail("the restatement met an unskippable chunk", it.type);
            if (strip) {
                if (src) s.main.insert(s.main.end(), src + p, src + p + len);
                s.main_len += len; s.passed += len;
                pieces_of(len, &s.n_long, &s.n_short);
            }
        }
        p += len;
    }
    if (!strip) s.main_len = 0;
    return s;
}

// The gaps' bytes alone, gap after gap (what a virtual stream has of bytes), and the data chunks' table
struct Tables {
    std::vector<uint64_t> hdr, bytes, decoded;   // per data chunk
    std::vector<ExtractSpan> span;               // per gap, in the stream
    std::vector<std::vector<uint8_t>> gap_bytes; // per gap (virtual streams)
};
static void put_header(std::vector<uint8_t>& o, uint8_t type, uint64_t clen) { o.push_back(type); o.push_back(uint8_t(clen)); o.push_back(uint8_t(clen >> 8)); o.push_back(uint8_t(clen >> 16)); }
static Tables tables_of(const std::vector<Item>& items, bool fill) {
    Tables t;
    uint64_t p = 0, begin = 0;
    t.gap_bytes.emplace_back();
    for (const Item& it : items) {
        if (is_data(it.type)) {
            t.hdr.push_back(p); t.bytes.push_back(4 + it.clen); t.decoded.push_back(it.decoded);
            t.span.push_back(ExtractSpan{begin, p});
            begin = p + 4 + it.clen;
            t.gap_bytes.emplace_back();
        } else if (fill) {
            std::vector<uint8_t>& g = t.gap_bytes.back();
            put_header(g, it.type, it.clen);
            g.resize(g.size() + it.clen, uint8_t(0xa5));
        }
        p += 4 + it.clen;
    }
    t.span.push_back(ExtractSpan{begin, p});
    return t;
}

static void same(const char* what, uint64_t a, uint64_t b) { if (a != b) fail(what, long(a), long(b)); }

static ExtractLayout layout_of(const Tables& t, const std::vector<ExtractGap>& gaps, uint64_t max_block, bool strip, uint64_t foot_n) {
    return extract_layout(t.hdr.size(), max_block, strip, [&](size_t g) -> const ExtractGap& { return gaps[g]; }, [&](size_t k) { return t.hdr[k]; },
                          [&](size_t k) { return t.bytes[k]; }, [&](size_t k) { return t.decoded[k]; }, [&](const ExtractLayout&) { return foot_n; });
}

static void compare_layout(const ExtractLayout& L, const Serial& s, bool strip) {
    same("status", L.status, kExtractOk);
    same("side_len", L.side_len, s.side_len); same("main_len", L.main_len, s.main_len);
    same("blocks", L.blocks, s.blocks); same("info", L.info, s.info); same("tables", L.tables, s.tables); same("tables46", L.tables46, s.tables46);
    same("passed", L.passed, s.passed); same("dropped", L.dropped, s.dropped);
    same("n_long", L.n_long, s.n_long); same("n_short", L.n_short, s.n_short);
    for (size_t k = 0; k < s.new_hdr.size(); k++) same("new_hdr", L.new_hdr[k], s.new_hdr[k]);
    for (size_t g = 0; g < L.base.size(); g++) {
        same("gap side_off", L.base[g].side_off, s.gap_side[g]);
        if (strip) same("gap main_off", L.base[g].main_off, s.gap_main[g]);
    }
}

// A virtual stream: every gap scanned over its own bytes (a gap's record does not depend on where the gap lies)
static void check_virtual(const std::vector<Item>& items, uint64_t max_block, uint64_t foot_n) {
    const Tables t = tables_of(items, true);
    std::vector<ExtractGap> gaps;
    for (const auto& g : t.gap_bytes) gaps.push_back(extract_gap_scan(g.data(), 0, g.size()));
    const uint8_t ident[10] = {};
    for (int strip = 0; strip < 2; strip++) {
        const Serial s = serial(items, nullptr, max_block, strip != 0, std::vector<uint8_t>(foot_n), ident);
        compare_layout(layout_of(t, gaps, max_block, strip != 0, foot_n), s, strip != 0);
    }
}

static void add(std::vector<Item>& v, uint8_t type, uint64_t clen, uint64_t decoded = 0) { v.push_back(Item{type, clen, decoded}); }
static uint64_t end_of(const std::vector<Item>& v) { uint64_t p = 0; for (const Item& it : v) p += 4 + it.clen; return p; }
// Data chunks up to exactly `target`, then one whose header lies there
static void reach(std::vector<Item>& v, uint64_t target, uint64_t max_block, uint64_t mma) {
    uint64_t p = end_of(v);
    while (p < target) {
        uint64_t len = target - p;
        if (len > 4 + 0xffffffull) { len = 4 + 0xffffffull; if (target - p - len < 16) len -= 16; }
        if (len < 9) fail("reach: no room", long(target), long(p));
        add(v, 2, len - 4, max_block);
        p += len;
    }
    add(v, 1 + below(3), 100 + below(1000), max_block - mma);
}

static void designed(uint64_t max_block) {
    const int ks[4] = {14, 21, 28, 35};
    const uint64_t mmas[3] = {0, 127, 128};
    for (int side = 0; side < 2; side++) {         // headers at 2^k - 1, then at 2^k: a reference one byte longer
        std::vector<Item> v;
        add(v, 0xff, 6);
        for (int i = 0; i < 4; i++) reach(v, (uint64_t(1) << ks[i]) - (side ? 0 : 1), max_block, mmas[i % 3]);
        add(v, 0x20, 1);
        check_virtual(v, max_block, 40);
        const Tables t = tables_of(v, false);      // (no gap holds a byte beside identifier and EOF: new offsets are the old ones)
        size_t hit = 0;
        for (size_t k = 0; k < t.hdr.size(); k++)
            for (int i = 0; i < 4; i++)
                if (t.hdr[k] == (uint64_t(1) << ks[i]) - (side ? 0 : 1)) {
                    same("reference bytes at 2^k", sidecar_ref_bytes(t.hdr[k], max_block - t.decoded[k]), 4 + uint32_t(ks[i] / 7 + side) + (mmas[i % 3] == 128 ? 2 : 1));
                    hit++;
                }
        same("designed offsets met", hit, 4);
    }
    {   // an empty gap, a gap of 300 padding chunks, two tables in front of one block, a table with no data chunk behind it, an index
        std::vector<Item> v;
        add(v, 0xff, 6); add(v, 0x44, 3);
        add(v, 0x45, 520); add(v, 2, 900, max_block);
        add(v, 1, 4 + 77, 77);                                                  // (an empty gap in front of it)
        for (int i = 0; i < 300; i++) add(v, 0xfe, 1);
        add(v, 0x45, 520); add(v, 0x46, 300); add(v, 3, 5000, max_block - 127);
        add(v, 0x47, 3); add(v, 0x80, 70000); add(v, 0x45, 65536 - 4); add(v, 0x45, 65536 - 4 + 1024); add(v, 0x45, 65536 - 4 + 1025);
        add(v, 2, 60, max_block - 128);
        add(v, 0x45, 264); add(v, 0x20, 2); add(v, 0x40, 30); add(v, 0x99, 12); add(v, 0xfe, 0); add(v, 0x45, 40);
        check_virtual(v, max_block, 33);
        check_virtual(v, max_block, 70000);
    }
    {   // no data chunk at all
        std::vector<Item> v;
        add(v, 0xff, 6); add(v, 0x20, 1);
        check_virtual(v, max_block, 20);
    }
}

static std::vector<Item> random_items(uint64_t max_block, bool small, bool huge) {
    std::vector<Item> v;
    add(v, 0xff, 6);
    const size_t blocks = below(small ? 12 : 400);
    auto gap = [&]() {
        const uint64_t r = below(10);
        const size_t n = r < 3 ? 0 : r < 8 ? 1 + below(3) : below(40);
        for (size_t i = 0; i < n; i++) {
            static const uint8_t types[] = {0x44, 0x45, 0x45, 0x45, 0x46, 0x40, 0x99, 0xfe, 0xfe, 0x80, 0x47, 0x45};
            const uint64_t pick = below(8);
            const uint64_t clen = pick == 0 ? 0 : pick < 4 ? below(64) : pick < 6 ? below(3000) : pick == 6 ? 65536 * below(3) + below(2200) : (small ? below(5000) : below(200000));
            add(v, types[below(sizeof types)], clen);
        }
    };
    for (size_t b = 0; b < blocks; b++) {
        gap();
        const uint64_t mma = below(4) == 0 ? (below(3) == 0 ? 0 : 126 + below(4)) : below(max_block - 1);
        add(v, 1 + below(3), huge ? 0xffffffull - below(1 << 20) : 10 + below(small ? 3000 : 70000), max_block - mma);
    }
    gap(); add(v, 0x20, below(3)); gap();
    return v;
}

// A stream that is whole in memory: the scan over the real spans, the layout, every gap's emit (last gap first), the descriptors run as memcpy
static void run_real(const std::vector<uint8_t>& src, const std::vector<Item>& items, uint64_t max_block, bool strip, const std::vector<uint8_t>& foot,
                     std::vector<uint8_t>* side_out, std::vector<uint8_t>* main_out, ExtractLayout* L_out) {
    const Tables t = tables_of(items, false);
    const size_t ng = t.span.size();
    std::vector<ExtractGap> gaps(ng);
    for (size_t g = 0; g < ng; g++) gaps[g] = extract_gap_scan(src.data(), t.span[g].begin, t.span[g].end);
    const ExtractLayout L = layout_of(t, gaps, max_block, strip, foot.size());
    same("status", L.status, kExtractOk);
    std::vector<uint8_t> side(L.side_len, 0), main(L.main_len, 0);
    std::vector<uint8_t> side_w(L.side_len, 0), main_w(L.main_len, 0);       // writes per byte
    std::vector<PlaceDesc> descs(size_t(L.n_long) + L.n_short, PlaceDesc{0, 0, 0xffffffffu, 0});
    std::vector<uint8_t> ref_room(L.side_len + 32, 0);                       // the emit writes references and the EOF into the sidecar itself
    for (size_t g = ng; g-- > 0;)
        extract_emit_gap(src.data(), t.span[g], g + 1 < ng ? t.span[g + 1].begin : 0, g + 1 == ng, L.base[g], strip, foot.size(), ref_room.data(), descs.data(), L.n_long);
    for (size_t i = 0; i < descs.size(); i++) {
        const PlaceDesc& d = descs[i];
        if (d.len == 0xffffffffu || d.len == 0 || d.len > kPlacePiece) fail("a descriptor slot left empty or of a bad length", long(i), long(d.len));
        if ((i < L.n_long) != (d.len > kExtractShortMax)) fail("a piece in the wrong list", long(i), long(d.len));
        const bool to_main = (d.pad & kExtractToMain) != 0, from_foot = (d.pad & kExtractFromFoot) != 0;
        std::vector<uint8_t>& dst = to_main ? main : side;
        std::vector<uint8_t>& w = to_main ? main_w : side_w;
        const std::vector<uint8_t>& from = from_foot ? foot : src;
        if (d.dst_off + d.len > dst.size() || d.src_off + d.len > from.size()) fail("a piece outside its buffers", long(i), long(d.dst_off));
        std::memcpy(dst.data() + d.dst_off, from.data() + d.src_off, d.len);
        for (uint32_t k = 0; k < d.len; k++) w[d.dst_off + k]++;
    }
    // what the lanes wrote themselves: the references and the sidecar's EOF chunk, wherever no piece went; the identifiers are the caller's
    for (size_t i = 10; i < L.side_len; i++)
        if (!side_w[i]) { side[i] = ref_room[i]; side_w[i]++; }
    for (size_t i = 0; i < 10; i++) { side[i] = src[i]; side_w[i]++; if (strip) { main[i] = src[i]; main_w[i]++; } }
    for (size_t i = 0; i < L.side_len; i++) if (side_w[i] != 1) fail("a sidecar byte not written exactly once", long(i), side_w[i]);
    for (size_t i = 0; i < L.main_len; i++) if (main_w[i] != 1) fail("a main byte not written exactly once", long(i), main_w[i]);
    for (size_t i = L.side_len; i < ref_room.size(); i++) if (ref_room[i]) fail("written behind the sidecar", long(i));
    *side_out = side; *main_out = main; *L_out = L;
}

static void check_real_random(uint64_t max_block) {
    const std::vector<Item> items = random_items(max_block, true, false);
    std::vector<uint8_t> src;
    for (const Item& it : items) {
        put_header(src, it.type, it.clen);
        for (uint64_t i = 0; i < it.clen; i++) src.push_back(uint8_t(rnd()));
    }
    std::memcpy(src.data() + 4, "MinLz", 5);
    std::vector<uint8_t> foot(1 + below(below(4) ? 90 : 70000));
    for (uint8_t& b : foot) b = uint8_t(rnd());
    for (int strip = 0; strip < 2; strip++) {
        const Serial s = serial(items, src.data(), max_block, strip != 0, foot, src.data());
        std::vector<uint8_t> side, main;
        ExtractLayout L;
        run_real(src, items, max_block, strip != 0, foot, &side, &main, &L);
        compare_layout(L, s, strip != 0);
        if (side != s.side) fail("the sidecar's bytes");
        if (strip && main != s.main) fail("the stripped main's bytes");
    }
}

static void classify_check() {
    for (int t = 0; t < 256; t++) {
        const ExtractClass want = (t == 0x44 || t == 0x45 || t == 0x46) ? kExSearch : (t == 0x40 || t == 0x99) ? kExIndex : t == 0x20 ? kExEof : t == 0xff ? kExIdent : t >= 0x40 ? kExOther : kExBad;
        same("classify", extract_classify(uint8_t(t)), want);
    }
    // refusals of the scan and the layout
    const uint8_t cut[6] = {0xfe, 0, 0, 0, 0xfe, 0}, past[4] = {0xfe, 1, 0, 0}, legacy[4] = {0x00, 0, 0, 0}, eof[5] = {0x20, 1, 0, 0, 0};
    same("a header cut short", extract_gap_scan(cut, 0, 6).bad, 1);
    same("a chunk past the gap", extract_gap_scan(past, 0, 4).bad, 1);
    same("an unskippable type", extract_gap_scan(legacy, 0, 4).bad, 1);
    same("an empty gap", extract_gap_scan(cut, 3, 3).bad, 0);
    Tables t;
    t.hdr = {10}; t.bytes = {20}; t.decoded = {5};
    std::vector<ExtractGap> g(2);
    same("no EOF chunk", layout_of(t, g, 1 << 16, true, 9).status, kExtractUnsupported);
    g[1] = extract_gap_scan(eof, 0, 5);
    same("one EOF chunk", layout_of(t, g, 1 << 16, true, 9).status, kExtractOk);
    g[1].eofs = 2;
    same("two EOF chunks", layout_of(t, g, 1 << 16, true, 9).status, kExtractUnsupported);
    g[1].eofs = 1; g[0].eofs = 1;
    same("an EOF chunk in front of a data chunk", layout_of(t, g, 1 << 16, true, 9).status, kExtractCorrupt);
    g[0].eofs = 0; t.decoded = {0};
    same("a data chunk of no bytes", layout_of(t, g, 1 << 16, false, 9).status, kExtractCorrupt);
    t.decoded = {(1 << 16) + 1};
    same("a data chunk beyond the block size", layout_of(t, g, 1 << 16, false, 9).status, kExtractCorrupt);
}

static std::string hex(const std::vector<uint8_t>& b) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (uint8_t v : b) { s.push_back(d[v >> 4]); s.push_back(d[v & 15]); }
    return s.empty() ? "-" : s;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto u32 = [&]() { uint32_t v = 0; if (std::fread(&v, 4, 1, f) != 1) { std::fprintf(stderr, "short case file\n"); std::exit(2); } return v; };
    uint32_t kind;
    while (std::fread(&kind, 4, 1, f) == 1) {
        if (kind == 1) {
            rng_state = u32() | 1;
            const uint32_t count = u32();
            classify_check();
            for (uint32_t i = 0; i < count; i++) check_real_random(uint64_t(1) << (10 + below(14)));
            std::printf("real ok %u\n", count);
        } else if (kind == 2) {
            rng_state = u32() | 1;
            for (int lg = 10; lg <= 23; lg += 13) designed(uint64_t(1) << lg);
            for (int i = 0; i < 40; i++) check_virtual(random_items(uint64_t(1) << (10 + below(14)), false, false), uint64_t(1) << 23, below(3000));
            // 16 MiB data chunks, 400 at the most: offsets up to 2^32 and a bit; the designed streams reach 2^35
            for (int i = 0; i < 6; i++) check_virtual(random_items(uint64_t(1) << 23, false, true), uint64_t(1) << 23, below(3000));
            std::printf("virtual ok\n");
        } else if (kind == 3) {
            const uint32_t strip = u32(), foot_n = u32();
            uint64_t n = u32();
            n |= uint64_t(u32()) << 32;
            std::vector<uint8_t> foot(foot_n), src(n);
            if ((foot_n && std::fread(foot.data(), 1, foot_n, f) != foot_n) || (n && std::fread(src.data(), 1, n, f) != n)) return 2;
            std::vector<Item> items;
            uint64_t max_block = 0;
            for (uint64_t p = 0; p + 4 <= n;) {
                uint8_t type;
                const uint64_t clen = walk_header(src.data(), p, &type);
                uint64_t dec = 0;
                if (type == 1) dec = clen - 4;
                else if (type == 2 || type == 3) walk_uvarint(src.data() + p + 8, size_t(clen - 4), &dec);
                else if (type == 0xff && !max_block) max_block = uint64_t(1) << ((src[p + 9] & 15) + 10);
                items.push_back(Item{type, clen, dec});
                p += 4 + clen;
            }
            std::vector<uint8_t> side, main;
            ExtractLayout L;
            run_real(src, items, max_block, strip != 0, foot, &side, &main, &L);
            std::printf("side %s main %s %llu %llu %llu %llu %llu %llu\n", hex(side).c_str(), hex(main).c_str(), (unsigned long long)L.blocks, (unsigned long long)L.info,
                        (unsigned long long)L.tables, (unsigned long long)L.tables46, (unsigned long long)L.passed, (unsigned long long)L.dropped);
        } else return 2;
    }
    std::fclose(f);
    return 0;
}
