// search_compressed_check.cpp — the rules of compressed block search tables (minlz_amd/csrc/mlz_search_compressed.h: the parse of a 0x46
// chunk, the weights and the decode table of a huff0 table description, one stream's decode loop, the sparse walk) as plain loops on the
// host, for tests/test_stream_search_compressed_host.py, which compares the lines with tests/search_compressed_model.py.  Stand-alone: built
// plain, and under AddressSanitizer and UBSan; every chunk and every bitmap lives in a heap block of exactly its size.
//   usage: search_compressed_check <case file>;  a record: u32 flags (1: the CRC is not compared) | u32 len | the chunk's payload
//   a line: "1 <R> <bytes> <masked CRC32C of the bitmap>" for a chunk that expands, "0" for one that is refused
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_search_compressed.h"

using namespace mlz;

// The decode tables of a chunk filled by 64 workers, as the kernel's lanes do it, against the fill by one
static bool fill_agrees(const uint8_t* body, uint32_t clen, const CstPlan& plan) {
    std::vector<uint16_t> one(kCstTableEntries), many(kCstTableEntries);
    uint8_t w[256];
    uint16_t start[256];
    CstFseScratch fs;
    for (uint32_t t = 0; t < plan.tc; t++) {
        const uint8_t* d = body + plan.tab_off[t];
        const uint32_t log = cst_weights(d, cst_desc_len(d, clen - plan.tab_off[t]), w, &fs);
        if (!log) continue;
        cst_table_starts(w, log, start);
        std::fill(one.begin(), one.end(), uint16_t(0xffff));
        std::fill(many.begin(), many.end(), uint16_t(0xffff));
        cst_table_fill(w, start, log, one.data(), 0, 1);
        for (uint32_t lane = 0; lane < 64; lane++) cst_table_fill(w, start, log, many.data(), lane, 64);
        if (one != many) return false;
        for (uint32_t i = 0; i < (1u << log); i++) if (one[i] == 0xffff) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    for (;;) {
        uint32_t head[2];
        if (std::fread(head, 4, 2, f) != 2) break;
        const uint32_t flags = head[0], len = head[1];
        uint8_t* body = static_cast<uint8_t*>(std::malloc(len ? len : 1));
        if (len && std::fread(body, 1, len, f) != len) return 3;
        CstPlan plan;
        int64_t n = cst_expand_host(body, len, nullptr, 0, &plan);   // (-1: the size is known and nothing was written)
        uint8_t* bitmap = nullptr;
        if (n == -1) {
            bitmap = static_cast<uint8_t*>(std::malloc(plan.n));
            n = cst_expand_host(body, len, bitmap, plan.n, &plan);
            if (n > 0 && !fill_agrees(body, len, plan)) return 4;
        }
        const uint32_t crc = n > 0 ? cst_crc_host(bitmap, size_t(n)) : 0;
        if (n > 0 && ((flags & 1) || crc == plan.crc)) std::printf("1 %u %lld %u\n", plan.R, static_cast<long long>(n), crc);
        else std::printf("0\n");
        std::free(bitmap);
        std::free(body);
    }
    std::fclose(f);
    return 0;
}
