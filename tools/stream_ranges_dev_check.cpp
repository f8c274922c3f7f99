// stream_ranges_dev_check.cpp — the device plan of mlz_dev_reader_read_device on the host (no GPU): runs the kernels' own rules
// (minlz_amd/csrc/mlz_stream_ranges_dev.h) as plain loops in the kernels' order — the per-range pass with its difference arrays and block
// prefixes, the scans, the per-chunk classification and compaction, the host's groups and places, the gather's piece search and intersection
// arithmetic — EXECUTES the outcome with memcpy, and compares the plan with what the host planner (plan_ranges, mlz_stream_ranges.h) gives for
// the same ranges with packed destinations.  tests/test_stream_ranges_device_host.py compares the rest with a brute-force model.
//
//   g++ -O2 -std=c++17 -o rdc tools/stream_ranges_dev_check.cpp && ./rdc cases.bin
// cases.bin, per case, little-endian u64s: n_chunks, n_ranges, dst_cap, flags (1 = plan only: no byte images; 2 = the chunks and bytes of the
// case before, none follow), then per chunk (decoded length, type), per range (off, len), and unless flags & 1 the decoded bytes of the stream.
// One line per case: `<rc> <touched chunks> <scratch bytes> <largest scratch extent> <groups> <long pieces> <crc32 of the destination image>
// <total> <differences>`; the image starts as dst_cap bytes of 0xa5.  differences: 0, or bits — 1 the return code, 2 the touched list, 4 a
// chunk's class, 8 a place, 16 the groups or the scratch bytes differ from plan_ranges'; 32 the starts are not the prefix sums; 64 a copy
// would have left its buffer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_ranges_dev.h"

using namespace mlz;

namespace {

constexpr uint32_t kShortMax = 1024, kPiece = 64 << 10;   // kRangeShortMax, kPlacePiece of the library

uint32_t crc32_ieee(const uint8_t* p, size_t n) {   // zlib.crc32
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
            tab[i] = c;
        }
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

bool get(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t head[4];
    std::vector<uint64_t> raw, off, len;
    std::vector<RdevChunk> ck;
    std::vector<ByteRange> rg;
    std::vector<uint8_t> data, dst, scratch;
    RangePlan plan;
    uint64_t size = 0;
    while (std::fread(head, 8, 4, f) == 4) {
        const uint64_t nck64 = head[0], n = head[1], dst_cap = head[2];
        const bool plan_only = (head[3] & 1) != 0, reuse = (head[3] & 2) != 0;
        if (!reuse) {
            raw.resize(size_t(nck64) * 2);
            if (!get(f, raw.data(), raw.size() * 8)) { std::fprintf(stderr, "short file\n"); return 2; }
            ck.resize(size_t(nck64));
            size = 0;
            for (size_t i = 0; i < nck64; i++) {
                ck[i] = RdevChunk{size, size, uint32_t(raw[2 * i]), uint32_t(raw[2 * i + 1])};   // (a stored chunk's body: the decoded bytes themselves)
                size += raw[2 * i];
            }
        }
        const uint32_t nck = uint32_t(ck.size());
        raw.resize(size_t(n) * 2);
        if (!get(f, raw.data(), raw.size() * 8)) { std::fprintf(stderr, "short file\n"); return 2; }
        off.resize(size_t(n)); len.resize(size_t(n));
        for (size_t i = 0; i < n; i++) { off[i] = raw[2 * i]; len[i] = raw[2 * i + 1]; }
        if (!reuse) data.clear();
        if (!plan_only && !reuse) {
            data.resize(size_t(size));
            if (!get(f, data.data(), data.size())) { std::fprintf(stderr, "short file\n"); return 2; }
        }
        unsigned diff = 0;

        // R1: the per-range pass
        const uint64_t avg = std::max<uint64_t>(1, nck ? size / nck : 1), nb = (n + kRdevBlock - 1) / kRdevBlock;
        const size_t nn = size_t(n), nbb = size_t(nb);
        std::vector<uint32_t> first(nn, 0), piece_local(nn, 0), cntd(size_t(nck) + 1, 0), whod(size_t(nck) + 1, 0), slot(nck, 0);
        std::vector<uint64_t> len_local(nn, 0), len_block(nbb, 0), piece_block(nbb, 0);
        RdevHeader hdr{};
        for (uint64_t b = 0; b < nb; b++) {
            uint64_t rl = 0, rp = 0;
            for (uint64_t i = b * kRdevBlock; i < n && i < (b + 1) * kRdevBlock; i++) {
                const RdevRange r = rdev_range_rule(ck.data(), nck, size, avg, off[i], len[i], kShortMax, kPiece);
                if (r.bad) hdr.err = 1;
                first[i] = r.j0;
                len_local[i] = rl; piece_local[i] = uint32_t(rp);
                rl = rdev_sat_add(rl, r.bad ? 0 : len[i]); rp = rdev_sat_add(rp, r.pieces);
                if (r.live) {
                    cntd[r.j0] += 1u; whod[r.j0] += uint32_t(i);
                    cntd[r.j1 + 1] += ~0u; whod[r.j1 + 1] += 0u - uint32_t(i);
                }
            }
            len_block[b] = rl; piece_block[b] = rp;
        }
        // R2: block sums -> block offsets; the chunks
        for (uint64_t b = 0, rl = 0, rp = 0; b <= nb; b++) {
            if (b == nb) { hdr.total = rl; hdr.pieces = rp; break; }
            const uint64_t l = len_block[b], p = piece_block[b];
            len_block[b] = rl; piece_block[b] = rp;
            rl = rdev_sat_add(rl, l); rp = rdev_sat_add(rp, p);
        }
        std::vector<RdevTouched> touched;
        {
            uint32_t c = 0, w = 0;
            RdevTouched t;
            for (uint32_t j = 0; j < nck; j++) {
                c += cntd[j]; w += whod[j];
                if (rdev_chunk_rule(ck[j], j, c, w, off.data(), len.data(), len_block.data(), len_local.data(), &t)) { slot[j] = uint32_t(touched.size()); touched.push_back(t); }
            }
            hdr.touched = uint32_t(touched.size());
        }
        const int rc = hdr.err ? -kRangeErrArg : (hdr.total > dst_cap || hdr.total == ~uint64_t(0)) ? -kRangeErrDstTooSmall : 0;

        // the host planner on the same ranges, packed
        rg.resize(size_t(n));
        {
            uint64_t s = 0;
            for (size_t i = 0; i < n; i++) { rg[i] = ByteRange{off[i], len[i], s}; s += len[i]; }
        }
        const int prc = plan_ranges(ck.data(), ck.size(), size, rg.data(), rg.size(), dst_cap, &plan);
        if (prc != rc) diff |= 1;
        if (rc < 0) { std::printf("%d 0 0 0 0 0 0 0 %u\n", rc, diff); continue; }
        for (size_t i = 0; i < n; i++) if (rdev_start(len_block.data(), len_local.data(), i) != rg[i].dst_off) diff |= 32;

        // host: groups and places
        std::vector<RdevPlace> places;
        std::vector<size_t> gend;
        std::vector<uint8_t> group_copies;
        uint64_t scratch_total = 0, scratch_max = 0, extent = 0;
        rdev_host_places(touched.data(), touched.size(), [&](uint32_t j) { return uint64_t(ck[j].n); }, &places, &gend, &group_copies, &scratch_total, &scratch_max);
        if (touched.size() != plan.touched.size()) diff |= 2;
        else
            for (size_t t = 0; t < touched.size(); t++) {
                const RangeTouched& p = plan.touched[t];
                if (touched[t].chunk != p.chunk) diff |= 2;
                if (touched[t].where != p.where) diff |= 4;
                else if ((p.where == kRangeDirect && touched[t].at != p.at) || (p.where == kRangeScratch && places[t].base != p.at)) diff |= 8;
            }
        if (gend.size() != plan.groups.size() || scratch_total != plan.scratch_total || scratch_max != plan.scratch_max) diff |= 16;
        else
            for (size_t g = 0; g < gend.size(); g++) if (gend[g] != plan.groups[g].t1) diff |= 16;

        uint32_t sum = 0;
        for (size_t t = 0; t < touched.size(); t++)
            if (touched[t].where == kRangeScratch) extent = std::max(extent, places[t].base + ck[touched[t].chunk].n);
        if (!plan_only) {
            dst.assign(size_t(dst_cap), 0xa5);
            scratch.assign(size_t(scratch_max), 0xee);
            uint64_t src, to, q;
            uint32_t cn;
            bool from_stream;
            auto copy = [&](const RdevChunk& c) {
                const std::vector<uint8_t>& from = from_stream ? data : scratch;
                if (src + cn > from.size() || to + cn > hdr.total || to + cn > dst.size() || cn > c.n) { diff |= 64; return; }
                std::memcpy(dst.data() + to, from.data() + src, cn);
            };
            for (size_t g = 0, t = 0; g < gend.size(); g++) {
                for (; t < gend[g]; t++) {   // the group's decode
                    const RdevChunk& c = ck[touched[t].chunk];
                    if (touched[t].where == kRangeDirect) {
                        if (touched[t].at + c.n > hdr.total || touched[t].at + c.n > dst.size()) { diff |= 64; continue; }
                        std::memcpy(dst.data() + touched[t].at, data.data() + c.out_off, c.n);
                    } else if (touched[t].where == kRangeScratch) {
                        if (places[t].base + c.n > scratch.size()) { diff |= 64; continue; }
                        std::memcpy(scratch.data() + places[t].base, data.data() + c.out_off, c.n);
                    }
                }
                if (group_copies[g]) {   // R4, as the kernel walks: the long pieces, then the short ranges
                    for (uint64_t p = 0; p < hdr.pieces; p++) {
                        const uint64_t i = rdev_piece_owner(piece_block.data(), piece_local.data(), n, nb, p, &q);
                        if (i >= n || len[i] <= kShortMax || q * kPiece >= len[i]) { diff |= 64; continue; }
                        const uint64_t o = off[i], end = o + len[i], start = rdev_start(len_block.data(), len_local.data(), i);
                        const uint64_t wb = o + q * kPiece, we = end - wb > kPiece ? wb + kPiece : end;
                        for (uint32_t j = q ? range_locate(ck.data(), nck, avg, wb) : first[i]; j < nck && ck[j].out_off < we; j++) {
                            if (!ck[j].n) continue;
                            if (rdev_intersect(ck[j], places[slot[j]], uint32_t(g), o, start, wb, we, &src, &to, &cn, &from_stream)) copy(ck[j]);
                        }
                    }
                    for (uint64_t i = 0; i < n; i++) {
                        if (!len[i] || len[i] > kShortMax) continue;
                        const uint64_t o = off[i], end = o + len[i], start = rdev_start(len_block.data(), len_local.data(), i);
                        for (uint32_t j = first[i]; j < nck && ck[j].out_off < end; j++) {
                            if (!ck[j].n) continue;
                            if (rdev_intersect(ck[j], places[slot[j]], uint32_t(g), o, start, o, end, &src, &to, &cn, &from_stream)) copy(ck[j]);
                        }
                    }
                }
                std::fill(scratch.begin(), scratch.end(), uint8_t(0xee));   // the next group reuses it
            }
            sum = crc32_ieee(dst.data(), dst.size());
        }
        std::printf("%d %zu %llu %llu %zu %llu %u %llu %u\n", rc, touched.size(), (unsigned long long)scratch_total, (unsigned long long)extent, gend.size(),
                    (unsigned long long)hdr.pieces, sum, (unsigned long long)hdr.total, diff);
    }
    std::fclose(f);
    return 0;
}
