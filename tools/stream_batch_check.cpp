// stream_batch_check.cpp — the batch calls over many streams in HBM, on the host (no GPU): the lane walk, its step cap and the verdict
// code of minlz_amd/csrc/mlz_stream_batch.h, the SAME functions walk_batch_kernel and the batch decode run, and the header step, record and
// running-state code of mlz_stream_walk.h.  tests/test_stream_batch_host.py compares what it prints with the host Reader's chunk walk of
// every stream alone.
//
//   g++ -O2 -std=c++17 -o sbc tools/stream_batch_check.cpp
//   ./sbc walk batch.bin       batch.bin: u64 n_streams, then (u64 src_off, u64 src_len) per stream, then u64 size and the ONE buffer
//                              in which the streams lie (back to back when the test says so), all little-endian.  One line per stream:
//                              `<result> <prefix_len> <table entries> <long>`, result as mlz_stream_decoded_len and prefix_len as
//                              mlz_stream_decoded_prefix_len of that stream alone.  A long stream (more than kBatchWalkSteps chunk
//                              headers) is walked once more without the cap, as the library hands it to its region walk.
//   ./sbc verdicts jobs.txt    jobs.txt: n_streams, then per stream `parsed n_jobs` and per job `compressed got n check_crc crc_got
//                              crc_want` (numbers in text).  One line per stream: its verdict.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_batch.h"

using namespace mlz;

namespace {

int walk_mode(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    uint64_t n = 0, size = 0;
    if (std::fread(&n, 8, 1, f) != 1) { std::fprintf(stderr, "short file\n"); return 2; }
    std::vector<uint64_t> spans(2 * n);
    if (n && std::fread(spans.data(), 16, n, f) != n) { std::fprintf(stderr, "short file\n"); return 2; }
    if (std::fread(&size, 8, 1, f) != 1) { std::fprintf(stderr, "short file\n"); return 2; }
    // the copy is exact: a read past the whole buffer is caught by a sanitizer build, a read past one stream changes a verdict
    std::vector<uint8_t> buf(size);
    if (size && std::fread(buf.data(), 1, size, f) != size) { std::fprintf(stderr, "short file\n"); return 2; }
    std::fclose(f);
    std::vector<WalkChunk> table;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = spans[2 * i], len = spans[2 * i + 1];
        if (off > size || len > size - off) { std::fprintf(stderr, "stream %llu leaves the buffer\n", (unsigned long long)i); return 2; }
        const uint8_t* src = buf.data() + off;
        bool is_long = false, again = false;
        uint32_t cnt = batch_walk_lane<false>(src, len, kBatchWalkSteps, nullptr, 0, &is_long);
        const uint32_t cap = is_long ? kWalkNoCap : kBatchWalkSteps;
        if (is_long) cnt = batch_walk_lane<false>(src, len, cap, nullptr, 0, &again);
        table.assign(cnt, WalkChunk{});
        const uint32_t put = batch_walk_lane<true>(src, len, cap, table.data(), cnt, &again);
        if (put != cnt || again) { std::fprintf(stderr, "stream %llu: the two passes disagree\n", (unsigned long long)i); return 3; }
        uint64_t prefix = 0;
        const int64_t r = walk_parse_table(table.data(), table.size(), uint64_t(8) << 20,
                                           [&](uint8_t, uint32_t, uint64_t, uint64_t, uint64_t nn, uint64_t out_off, uint64_t) { prefix = out_off + nn; });
        std::printf("%lld %llu %u %d\n", (long long)r, (unsigned long long)(r >= 0 ? uint64_t(r) : prefix), cnt, is_long ? 1 : 0);
    }
    return 0;
}

int verdict_mode(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::perror(path); return 2; }
    unsigned long long n = 0;
    if (std::fscanf(f, "%llu", &n) != 1) return 2;
    std::vector<int64_t> parsed(n), job_rc, out(n);
    std::vector<size_t> job_first(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        long long p = 0;
        unsigned long long nj = 0;
        if (std::fscanf(f, "%lld %llu", &p, &nj) != 2) return 2;
        parsed[i] = p;
        job_first[i] = job_rc.size();
        for (size_t j = 0; j < nj; j++) {
            int compressed = 0, check_crc = 0;
            long long got = 0;
            unsigned long long len = 0, crc_got = 0, crc_want = 0;
            if (std::fscanf(f, "%d %lld %llu %d %llu %llu", &compressed, &got, &len, &check_crc, &crc_got, &crc_want) != 6) return 2;
            job_rc.push_back(chunk_job_verdict(compressed != 0, got, len, check_crc != 0, uint32_t(crc_got), uint32_t(crc_want)));
        }
    }
    job_first[n] = job_rc.size();
    std::fclose(f);
    batch_stream_verdicts(parsed.data(), job_first.data(), job_rc.data(), n, out.data());
    for (size_t i = 0; i < n; i++) std::printf("%lld\n", (long long)out[i]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "walk")) return walk_mode(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "verdicts")) return verdict_mode(argv[2]);
    std::fprintf(stderr, "usage: %s walk batch.bin | verdicts jobs.txt\n", argv[0]);
    return 2;
}
