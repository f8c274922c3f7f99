// mlz_stream_scratch.h — how the chunks of a decode list reach the scratch of the device-resident Reader (ScratchDecode,
// mlz_stream_walk.hip.inc), shared with its host check (tools/stream_scratch_check.cpp).  Plain C++: compiles for the host alone.
//
// A caller decides the list (the jobs, in stream order), its groups (gend[g]: one past group g's last job; every group reuses the scratch
// from its start) and where every job's chunk lies in the scratch (at[i]).  The rest is the same for all callers: a compressed chunk (0x02 /
// 0x03) is decoded to scratch + at[i]; a stored chunk (0x01) is copied there from the stream in pieces of kPlacePiece bytes by one
// stream_place_kernel launch per group, and its CRC is taken over the stream's own bytes; a chunk that two groups hold (the sidecar build's
// overlap chunk) is two jobs and is copied for each.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace mlz {

// One piece of a copy that stream_place_kernel runs, a workgroup per piece; pad selects the source the offset counts in
struct PlaceDesc { uint64_t src_off, dst_off; uint32_t len, pad; };
constexpr uint32_t kPlacePiece = 64 << 10;
// The span of `len` bytes from src_off to dst_off, cut into pieces of 64 KiB: put(PlaceDesc) for each, in order
template <class Put> void place_pieces(uint64_t src_off, uint64_t dst_off, uint64_t len, uint32_t pad, Put put) {
    for (uint64_t o = 0; o < len; o += kPlacePiece) put(PlaceDesc{src_off + o, dst_off + o, uint32_t(std::min<uint64_t>(kPlacePiece, len - o)), pad});
}

// The data chunks with bytes of a chunk list, in stream order: n_of(k) = chunk k's decoded bytes
template <class N> std::vector<size_t> chunks_with_bytes(size_t n_chunks, N n_of) {
    std::vector<size_t> dc;
    for (size_t k = 0; k < n_chunks; k++) if (n_of(k)) dc.push_back(k);
    return dc;
}
// The whole-stream list (the record index build, the regex grep): every chunk with bytes is a job, and a group's chunks lie side by side from
// scratch[0] on.  dc: chunks_with_bytes; gend: the groups of that list; n_of(k), off_of(k): chunk k's decoded bytes and where they lie in the
// decoded stream; size: the stream's decoded bytes.  -> at[i]: job i's place in the scratch; first[g], bytes[g]: group g's first decoded
// position and its bytes; status: kWholeOk, or a chunk does not begin where the one in front of it in its group ends, or the groups are
// not [0, size) cut into non-empty pieces in order (no group and size == 0 are).  The arrays are complete under kWholeOk only.
enum { kWholeOk = 0, kWholeNotContiguous = 1, kWholeNotTiled = 2 };
struct WholeStreamList { std::vector<uint64_t> at, first, bytes; int status = kWholeOk; };
template <class N, class Off>
WholeStreamList whole_stream_list(const std::vector<size_t>& dc, const std::vector<size_t>& gend, N n_of, Off off_of, uint64_t size) {
    WholeStreamList w;
    w.at.resize(dc.size()); w.first.resize(gend.size()); w.bytes.resize(gend.size());
    uint64_t pos = 0;   // where the groups in front end: at most size
    for (size_t g = 0, i = 0; g < gend.size(); g++) {
        const size_t end = std::min(gend[g], dc.size());
        const uint64_t first = i < end ? uint64_t(off_of(dc[i])) : pos;
        uint64_t o = 0;
        for (; i < end; i++) {
            if (uint64_t(off_of(dc[i])) != first + o) { w.status = kWholeNotContiguous; return w; }
            w.at[i] = o;
            o += n_of(dc[i]);
        }
        w.first[g] = first; w.bytes[g] = o;
        if (o == 0 || first != pos || o > size - pos) { w.status = kWholeNotTiled; return w; }
        pos += o;
    }
    if (pos != size) w.status = kWholeNotTiled;
    return w;
}
// The copies of a staged list: the stored chunks' pieces (pad 1: the stream is stream_place_kernel's second source), group after group, in
// job order; group g's are places[place_end[g - 1], place_end[g]); the scratch holds scratch_max bytes, the largest at[i] + n of the list.
// chunk_of(i): job i's chunk, with the members type (0x01: stored), body_off and n.
struct ScratchPlaces { std::vector<PlaceDesc> places; std::vector<size_t> place_end; uint64_t scratch_max = 0; };
template <class ChunkOf> ScratchPlaces scratch_places(size_t n_jobs, const std::vector<size_t>& gend, ChunkOf chunk_of, const std::vector<uint64_t>& at) {
    ScratchPlaces sp;
    for (size_t g = 0, i = 0; g < gend.size(); g++) {
        for (; i < gend[g] && i < n_jobs; i++) {
            const auto& ck = chunk_of(i);
            if (ck.type == 0x01) place_pieces(ck.body_off, at[i], ck.n, 1, [&](const PlaceDesc& d) { sp.places.push_back(d); });
            sp.scratch_max = std::max<uint64_t>(sp.scratch_max, at[i] + ck.n);
        }
        sp.place_end.push_back(sp.places.size());
    }
    return sp;
}

}  // namespace mlz
