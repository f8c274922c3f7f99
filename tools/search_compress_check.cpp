// search_compress_check.cpp — the write side of compressed block search tables (minlz_amd/csrc/mlz_search_compressed.h: code lengths,
// canonical codes, both forms of the table description, the sizes, the kind choice, the streams: cst_compress_host) as plain loops on the
// host, for tests/test_search_table_compress_host.py, which compares the lines with tests/search_compressed_model.py.  Stand-alone: built
// plain, and under AddressSanitizer and UBSan; every bitmap and every section lives in a heap block of exactly its size.  Every section is
// expanded again by the read side (cst_expand_host) and must give the bitmap back; a mismatch ends the program with status 4.
//   usage: search_compress_check <case file>;  a record: u32 kind | u32 len | len bytes
//   kind 1: the bytes are a bitmap.  A line: "<section bytes> <masked CRC32C of the section> <raw> <rle> <sparse> <huff> <direct> <fse>
//           <flattened> <no description>" (the counts over its sub-blocks), or "refused" for a size that is no power of two in 32 .. 2^20
//   kind 2: the bytes are u32 seed | u32 count: `count` pseudo-random bitmaps of 32 bytes to 64 KiB drawn from pseudo-random histograms (2 to
//           256 byte values; flat, geometric, Fibonacci-like and two-level counts; values in order or scattered).  A line: "searched <count>"
//           and the eight counts summed; the last one says whether any histogram left both description forms unusable.
//   kind 3: the bytes are u32 seed | u32 count: `count` pseudo-random weight vectors of 129 to 255 weights 0 .. 11 (more than 128 listed: the
//           direct form is out) go to cst_w_description directly, whatever histogram would give them, flat and skewed alike; each FSE
//           section that comes back is decoded again by the read side (cst_fse_weights).  A line: "weights <count> longest <the longest
//           FSE section, its length byte included> unusable <vectors for which it returned 0>", and the same three figures behind "wide"
//           for as many flat vectors of 250 to 255 weights 0 .. 12: weight 12 comes from no tree of this writer (its table log is at most
//           11), but the function takes it, and thirteen flat values are what makes a section of 128 bytes or more, so that the refusal
//           itself runs.  In front of them the kind choice without a description is checked on its own: cst_w_pick(sub, sparse, 0, bits) is raw or sparse by the sizes alone, whatever bits says.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_search_compressed.h"

using namespace mlz;

static uint64_t rng_state;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// bitmap[0, n) -> its section in a block of exactly its size (*out, the caller frees it); the section expanded again equals the bitmap,
// and one byte less of room is refused.  Returns the section's length; exits on a mismatch.
static uint32_t compress_checked(const uint8_t* bitmap, uint32_t n, CstWriteStats* st, uint8_t** out) {
    std::vector<uint8_t> wide(cst_w_bound(n));
    const int64_t len = cst_compress_host(bitmap, n, wide.data(), wide.size(), st);
    if (len < 2 || uint64_t(len) > cst_w_bound(n)) std::exit(4);
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(size_t(len)));
    if (cst_compress_host(bitmap, n, exact, size_t(len)) != len || std::memcmp(exact, wide.data(), size_t(len)) != 0) std::exit(4);
    if (cst_compress_host(bitmap, n, exact, size_t(len) - 1) != -1) std::exit(4);
    // a payload of type 1, M = 6, R = 0 around it: B = log2(n) + 3
    const uint32_t clen = 8 + uint32_t(len);
    uint8_t* body = static_cast<uint8_t*>(std::malloc(clen));
    const uint32_t crc = cst_crc_host(bitmap, n);
    body[0] = 1; body[1] = 6; body[2] = uint8_t(cst_highbit(n) + 3); body[3] = 0;
    for (int i = 0; i < 4; i++) body[4 + i] = uint8_t(crc >> (8 * i));
    std::memcpy(body + 8, exact, size_t(len));
    uint8_t* back = static_cast<uint8_t*>(std::malloc(n));
    CstPlan plan;
    if (cst_expand_host(body, clen, back, n, &plan) != int64_t(n) || std::memcmp(back, bitmap, n) != 0 || plan.crc != crc) std::exit(4);
    std::free(back);
    std::free(body);
    *out = exact;
    return uint32_t(len);
}

static void print_stats(const CstWriteStats& s) {
    std::printf(" %u %u %u %u %u %u %u %u\n", s.raw, s.rle, s.sparse, s.huff, s.direct, s.fse, s.flattened, s.no_description);
}

// One pseudo-random bitmap: a histogram's shape, then bytes drawn from it
static void draw(std::vector<uint8_t>* bm) {
    static const uint32_t sizes[] = {32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 8192, 16384, 65536};
    const uint32_t pick = rnd() % 64, n = sizes[pick < 60 ? pick % 10 : 10 + (pick & 1)];
    const uint32_t most = rnd() % 3 ? 24 : 255;   // (one draw a statement: their order is then the same in every build)
    const uint32_t values = 2 + rnd() % most;
    const uint32_t shape = rnd() % 4;
    uint8_t value[256];
    for (uint32_t i = 0; i < 256; i++) value[i] = uint8_t(i);
    if (rnd() & 1)
        for (uint32_t i = 255; i > 0; i--) { const uint32_t j = rnd() % (i + 1); const uint8_t t = value[i]; value[i] = value[j]; value[j] = t; }
    std::vector<uint64_t> cum(values);
    uint64_t total = 0, a = 1, b = 1;
    for (uint32_t i = 0; i < values; i++) {
        uint64_t w = 1;
        if (shape == 1) w = uint64_t(1) << (i < 40 ? i / (1 + values / 40) : 0);                 // geometric
        else if (shape == 2) { w = a; const uint64_t c = a + b; a = b; b = c < (uint64_t(1) << 40) ? c : b; }   // Fibonacci-like
        else if (shape == 3) w = i < 3 ? 1000 : 1 + rnd() % 8;                                        // a few heavy values, many light ones
        total += w;
        cum[i] = total;
    }
    bm->resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t top = uint64_t(rnd()) << 32;
        const uint64_t r = (top | rnd()) % total;
        uint32_t lo = 0, hi = values - 1;
        while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (cum[mid] > r) hi = mid; else lo = mid + 1; }
        (*bm)[i] = value[lo];
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    for (;;) {
        uint32_t head[2];
        if (std::fread(head, 4, 2, f) != 2) break;
        const uint32_t kind = head[0], len = head[1];
        uint8_t* data = static_cast<uint8_t*>(std::malloc(len ? len : 1));
        if (len && std::fread(data, 1, len, f) != len) return 3;
        if (kind == 1) {
            if (!cst_w_size_ok(len)) std::printf("refused\n");
            else {
                CstWriteStats st{};
                uint8_t* section = nullptr;
                const uint32_t slen = compress_checked(data, len, &st, &section);
                std::printf("%u %u", slen, cst_crc_host(section, slen));
                print_stats(st);
                std::free(section);
            }
        } else if (kind == 2 && len == 8) {
            uint32_t seed, count;
            std::memcpy(&seed, data, 4);
            std::memcpy(&count, data + 4, 4);
            rng_state = 0x9E3779B97F4A7C15ull ^ seed;
            CstWriteStats st{};
            std::vector<uint8_t> bm;
            for (uint32_t i = 0; i < count; i++) {
                draw(&bm);
                uint8_t* exact = static_cast<uint8_t*>(std::malloc(bm.size()));   // (the bitmap in a block of its size)
                std::memcpy(exact, bm.data(), bm.size());
                uint8_t* section = nullptr;
                compress_checked(exact, uint32_t(bm.size()), &st, &section);
                std::free(section);
                std::free(exact);
            }
            std::printf("searched %u", count);
            print_stats(st);
        } else if (kind == 3 && len == 8) {
            for (uint32_t sub = 32; sub <= 65536; sub <<= 1)
                for (uint32_t sparse = 0; sparse <= sub + 8; sparse += 1 + sub / 37)
                    for (uint32_t bits = 0; bits <= 8 * sub; bits += 1 + sub)
                        if (cst_w_pick(sub, sparse, 0, bits) != (sub <= sparse + 3 ? kCstRaw : kCstSparse)) return 4;
            uint32_t seed, count;
            std::memcpy(&seed, data, 4);
            std::memcpy(&count, data + 4, 4);
            rng_state = 0x9E3779B97F4A7C15ull ^ seed;
            CstFseScratch fs;
            for (uint32_t wide = 0; wide < 2; wide++) {
            uint32_t longest = 0, unusable = 0;
            for (uint32_t i = 0; i < count; i++) {
                const uint32_t n = wide ? 250 + rnd() % 6 : 129 + rnd() % 127;
                const uint32_t top = wide ? 12 : 2 + rnd() % 10;   // values 0 .. top
                const uint32_t skew = wide ? 0 : rnd() % 3;
                uint8_t* w = static_cast<uint8_t*>(std::malloc(n));
                for (uint32_t k = 0; k < n; k++) {
                    uint32_t v = rnd() % (top + 1);
                    if (skew == 1 && rnd() % 4) v = rnd() % 3;
                    if (skew == 2) { const uint32_t v2 = rnd() % (top + 1); v = v < v2 ? v : v2; }
                    w[k] = uint8_t(v);
                }
                uint8_t* desc = static_cast<uint8_t*>(std::malloc(1 + kCstFseOutCap));
                const uint32_t dlen = cst_w_description(w, n, desc, &fs);
                if (!dlen) unusable++;
                else {
                    if (desc[0] >= 128 || desc[0] + 1u != dlen || dlen > 128) return 4;
                    uint8_t back[256];
                    CstFseScratch rs;
                    if (cst_fse_weights(desc + 1, dlen - 1, back, &rs) != n || std::memcmp(back, w, n) != 0) return 4;
                    if (dlen > longest) longest = dlen;
                }
                std::free(desc);
                std::free(w);
            }
            std::printf("%s %u longest %u unusable %u%s", wide ? " wide" : "weights", count, longest, unusable, wide ? "\n" : "");
            }
        } else {
            return 3;
        }
        std::free(data);
    }
    std::fclose(f);
    return 0;
}
