// stream_scratch_check.cpp — the staging rule of the scratch decode (minlz_amd/csrc/mlz_stream_scratch.h), run as plain loops for
// tests/test_stream_scratch_host.py:
//   g++ -O2 -std=c++17 -o ssc tools/stream_scratch_check.cpp && ./ssc cases.bin
// The case file is a sequence of little-endian records, one output line each:
//   kind 1  u32 jobs, groups; u64 stream bytes; per job u32 type, u64 n, body_off, at; per group u64 gend; the stream; the jobs' decoded
//           bytes, job after job
//           -> scratch_places over the list, then the decode as loops: per group a scratch of exactly scratch_max bytes, the group's
//           places by memcpy from the stream, the compressed chunks' bytes by memcpy to at[i], and every job's scratch[at[i], at[i] + n)
//           compared with its bytes.  place_end ascends, the places are the stored jobs' pieces, none reaches behind scratch_max or the
//           stream (status 3 otherwise):
//           "places <n> ends <place_end ...> max <scratch_max>"
//   kind 2  u32 chunks; per chunk u64 n -> chunks_with_bytes: "with bytes <k ...>"
//   kind 3  u32 chunks, groups; u64 size; per chunk u64 n, out_off; per group u64 gend (over the chunks with bytes)
//           -> whole_stream_list over chunks_with_bytes: "status <s>", and under status 0 " groups <first>+<bytes> ... at <at ...>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../minlz_amd/csrc/mlz_stream_scratch.h"

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    template <class T> T get() { T v; if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } std::memcpy(&v, b.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t* bytes(size_t n) { if (p + n > b.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); } const uint8_t* q = b.data() + p; p += n; return q; }
};

[[noreturn]] void fail(const char* what, uint64_t i) {
    std::fprintf(stderr, "%s (at %llu)\n", what, (unsigned long long)i);
    std::exit(3);
}

constexpr uint8_t kStored = 0x01;
struct Chunk { uint8_t type; uint64_t n, body_off; };

void staged(In& in) {
    const uint32_t nj = in.get<uint32_t>(), ng = in.get<uint32_t>();
    const uint64_t stream_len = in.get<uint64_t>();
    std::vector<Chunk> ck(nj);
    std::vector<uint64_t> at(nj);
    for (uint32_t i = 0; i < nj; i++) {
        ck[i].type = uint8_t(in.get<uint32_t>());
        ck[i].n = in.get<uint64_t>(); ck[i].body_off = in.get<uint64_t>(); at[i] = in.get<uint64_t>();
    }
    std::vector<size_t> gend(ng);
    for (uint32_t g = 0; g < ng; g++) gend[g] = size_t(in.get<uint64_t>());
    const uint8_t* stream = in.bytes(size_t(stream_len));
    std::vector<const uint8_t*> data(nj);
    for (uint32_t i = 0; i < nj; i++) data[i] = in.bytes(size_t(ck[i].n));

    const mlz::ScratchPlaces sp = mlz::scratch_places(nj, gend, [&](size_t i) -> const Chunk& { return ck[i]; }, at);
    const std::vector<mlz::PlaceDesc>& places = sp.places;
    const std::vector<size_t>& place_end = sp.place_end;
    const uint64_t scratch_max = sp.scratch_max;

    if (place_end.size() != ng) fail("place_end: not one entry per group", place_end.size());
    size_t pieces = 0;
    for (uint32_t i = 0; i < nj; i++) if (ck[i].type == kStored) pieces += size_t((ck[i].n + mlz::kPlacePiece - 1) / mlz::kPlacePiece);
    if (places.size() != pieces) fail("the places are not the stored jobs' pieces", places.size());
    for (uint32_t g = 0; g < ng; g++)
        if (place_end[g] < (g ? place_end[g - 1] : 0) || place_end[g] > places.size()) fail("place_end does not ascend", g);
    if (ng && place_end[ng - 1] != places.size()) fail("pieces behind the last group", ng);
    for (size_t q = 0; q < places.size(); q++) {
        const mlz::PlaceDesc& d = places[q];
        if (d.pad != 1 || d.len == 0 || d.len > mlz::kPlacePiece) fail("a piece's source or length", q);
        if (d.dst_off + d.len > scratch_max) fail("a piece reaches behind scratch_max", q);
        if (d.src_off + d.len > stream_len) fail("a piece reaches behind the stream", q);
    }
    for (size_t g = 0, j0 = 0; g < ng; j0 = gend[g++]) {
        uint8_t* scratch = static_cast<uint8_t*>(std::malloc(size_t(scratch_max) ? size_t(scratch_max) : 1));   // exactly: a sanitizer sees a byte too many
        std::memset(scratch, 0xEE, size_t(scratch_max));
        for (size_t q = g ? place_end[g - 1] : 0; q < place_end[g]; q++) std::memcpy(scratch + places[q].dst_off, stream + places[q].src_off, places[q].len);
        for (size_t i = j0; i < gend[g]; i++) {
            if (ck[i].type == kStored) continue;
            if (at[i] + ck[i].n > scratch_max) fail("a compressed chunk reaches behind scratch_max", i);
            std::memcpy(scratch + at[i], data[i], size_t(ck[i].n));
        }
        for (size_t i = j0; i < gend[g]; i++)
            if (std::memcmp(scratch + at[i], data[i], size_t(ck[i].n)) != 0) fail("a job's bytes are not in the scratch", i);
        std::free(scratch);
    }
    std::printf("places %zu ends", places.size());
    for (size_t e : place_end) std::printf(" %zu", e);
    std::printf(" max %llu\n", (unsigned long long)scratch_max);
}

void whole(In& in) {
    const uint32_t n = in.get<uint32_t>(), ng = in.get<uint32_t>();
    const uint64_t size = in.get<uint64_t>();
    std::vector<uint64_t> sizes(n), offs(n);
    for (uint32_t k = 0; k < n; k++) { sizes[k] = in.get<uint64_t>(); offs[k] = in.get<uint64_t>(); }
    std::vector<size_t> gend(ng);
    for (uint32_t g = 0; g < ng; g++) gend[g] = size_t(in.get<uint64_t>());
    const std::vector<size_t> dc = mlz::chunks_with_bytes(n, [&](size_t k) { return sizes[k]; });
    const mlz::WholeStreamList w = mlz::whole_stream_list(dc, gend, [&](size_t k) { return sizes[k]; }, [&](size_t k) { return offs[k]; }, size);
    std::printf("status %d", w.status);
    if (w.status == mlz::kWholeOk) {
        if (w.at.size() != dc.size() || w.first.size() != ng || w.bytes.size() != ng) fail("the list's arrays do not fit its jobs and groups", w.at.size());
        std::printf(" groups");
        for (uint32_t g = 0; g < ng; g++) std::printf(" %llu+%llu", (unsigned long long)w.first[g], (unsigned long long)w.bytes[g]);
        std::printf(" at");
        for (uint64_t a : w.at) std::printf(" %llu", (unsigned long long)a);
    }
    std::printf("\n");
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
        if (kind == 1) { staged(in); continue; }
        if (kind == 3) { whole(in); continue; }
        if (kind != 2) { std::fprintf(stderr, "unknown record %u\n", kind); return 2; }
        const uint32_t n = in.get<uint32_t>();
        std::vector<uint64_t> sizes(n);
        for (uint32_t k = 0; k < n; k++) sizes[k] = in.get<uint64_t>();
        std::printf("with bytes");
        for (size_t k : mlz::chunks_with_bytes(n, [&](size_t k) { return sizes[k]; })) std::printf(" %zu", k);
        std::printf("\n");
    }
    return 0;
}
