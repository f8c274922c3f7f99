// mlz_stream_sidecar_extract.h — the rules that mlz_dev_reader_extract_sidecar (mlz_stream_sidecar_extract.hip.inc) shares between its kernels,
// its host code and their host check (tools/sidecar_extract_check.cpp): what becomes of a chunk that is no data chunk (extract_classify), the
// pass over one gap between data chunks (extract_gap_scan), the pieces a copied span is cut into (extract_pieces, extract_put_pieces), the
// layout of the sidecar and of the stripped main stream (extract_layout) and what one gap's lane writes from it (extract_emit_gap).
// Plain C++: compiles for the host alone and for gfx950.
//
// The reference's ExtractSidecar (sidecar.go:546-771) for one stream.  The handle's chunk table holds the data chunks; everything else lies in
// the GAPS between them: gap g (0 <= g <= chunks) spans [end of data chunk g - 1 (0 for g = 0), header of data chunk g (the end of the stream
// for g = chunks)).  A gap's chunks go, in order:
//   0x44 0x45 0x46   search      -> the sidecar, verbatim
//   0x40 0x99        index       -> nowhere (the stripped main gets a fresh index)
//   0x20             EOF         -> the sidecar's `20 01 00 00 00`; the stripped main's foot (EOF with the decoded size, then the index)
//   0xff             identifier  -> nowhere (the caller writes the one identifier in front of both outputs)
//   other > 0x3f     other       -> the stripped main, verbatim (padding, user chunks, a 0x47 the source happens to hold)
//   other <= 0x3f                -> an error: no successful open leaves one in a gap
// and behind gap g's chunks the sidecar takes data chunk g's reference (0x47) and the stripped main takes data chunk g itself.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlz_stream_scratch.h"   // PlaceDesc, kPlacePiece
#include "mlz_stream_search.h"    // sidecar_put_ref, sidecar_ref_bytes; mlz_stream_walk.h: walk_header

namespace mlz {

enum ExtractClass : uint32_t { kExSearch = 0, kExIndex, kExEof, kExIdent, kExOther, kExBad };

MLZ_SEARCH_HD ExtractClass extract_classify(uint8_t type) {
    if (type == 0x44 || type == 0x45 || type == 0x46) return kExSearch;
    if (type == 0x40 || type == 0x99) return kExIndex;
    if (type == 0x20) return kExEof;
    if (type == 0xff) return kExIdent;
    return type > 0x3f ? kExOther : kExBad;   // (0x01 .. 0x03 lie in no gap)
}

// A copied span is cut into pieces of kPlacePiece bytes; a last piece of at most kExtractShortMax bytes is a SHORT piece (16 lanes copy
// it), every other piece a LONG one (a workgroup copies it).
constexpr uint32_t kExtractShortMax = 1024;
MLZ_SEARCH_HD void extract_pieces(uint64_t len, uint32_t* n_long, uint32_t* n_short) {
    const uint64_t rest = len % kPlacePiece;
    *n_long += uint32_t(len / kPlacePiece) + (rest > kExtractShortMax ? 1u : 0u);
    *n_short += rest && rest <= kExtractShortMax ? 1u : 0u;
}
// where: PlaceDesc.pad of an extract piece — bit 0: the destination is the stripped main (else the sidecar); bit 1: the source is the
// caller's foot bytes (else the stream)
constexpr uint32_t kExtractToMain = 1, kExtractFromFoot = 2;
MLZ_SEARCH_HD void extract_put_pieces(uint64_t src_off, uint64_t dst_off, uint64_t len, uint32_t where, PlaceDesc* descs, uint32_t* q_long, uint32_t* q_short) {
    for (uint64_t o = 0; o < len; o += kPlacePiece) {
        const uint32_t n = uint32_t(len - o < kPlacePiece ? len - o : kPlacePiece);
        descs[n <= kExtractShortMax ? (*q_short)++ : (*q_long)++] = PlaceDesc{src_off + o, dst_off + o, n, where};
    }
}

// What the gap pass finds in one gap: 64 bytes, the only bytes of a gap that visit the host
struct ExtractGap {
    uint64_t side_bytes, main_bytes;   // search chunks; other skippable chunks (headers included)
    uint64_t dropped_bytes;            // index chunks
    uint32_t info, tab45, tab46, eofs;
    uint32_t side_long, side_short, main_long, main_short;   // the pieces of side_bytes and of main_bytes, chunk by chunk
    uint32_t bad, pad;                 // 1: an unskippable type, a header cut short or a chunk that runs past the gap's end
};
static_assert(sizeof(ExtractGap) == 64, "a record shared with the kernels");

// One gap's span in the stream, and where its lane writes (the layout's result): 48 bytes go up per gap
struct ExtractSpan { uint64_t begin, end; };
struct ExtractBase { uint64_t side_off, main_off; uint32_t q_long, q_short, mma, pad; };
static_assert(sizeof(ExtractBase) == 32, "a record shared with the kernels");

// The chunks of the gap src[begin, end), header by header: visit(offset, type, bytes of the whole chunk, class) for each.  Returns false
// for a gap that is no row of whole chunks (fewer than 4 bytes left for a header, a chunk that runs past `end`) or that holds an
// unskippable type; the visit ends there.  Reads the 4-byte headers inside [begin, end) and nothing else.
template <class Visit> MLZ_SEARCH_HD bool extract_gap_walk(const uint8_t* src, uint64_t begin, uint64_t end, Visit visit) {
    for (uint64_t p = begin; p < end;) {
        if (end - p < 4) return false;
        uint8_t type;
        const uint64_t len = 4 + uint64_t(walk_header(src, p, &type));
        const ExtractClass cl = extract_classify(type);
        if (len > end - p || cl == kExBad) return false;
        visit(p, type, len, cl);
        p += len;
    }
    return true;
}

MLZ_SEARCH_HD ExtractGap extract_gap_scan(const uint8_t* src, uint64_t begin, uint64_t end) {
    ExtractGap g{};
    const bool ok = extract_gap_walk(src, begin, end, [&](uint64_t, uint8_t type, uint64_t len, ExtractClass cl) {
        if (cl == kExSearch) {
            g.side_bytes += len;
            extract_pieces(len, &g.side_long, &g.side_short);
            if (type == 0x44) g.info++; else if (type == 0x45) g.tab45++; else g.tab46++;
        } else if (cl == kExOther) {
            g.main_bytes += len;
            extract_pieces(len, &g.main_long, &g.main_short);
        } else if (cl == kExIndex) g.dropped_bytes += len;
        else if (cl == kExEof) g.eofs++;
    });
    g.bad = ok ? 0 : 1;
    return g;
}

// The layout.  n: data chunks; gap(g), g <= n: the gap pass's record; hdr_off(k), bytes(k), decoded(k): data chunk k's header offset, its
// bytes with the header and its decoded bytes; strip: mode b (a stripped main is written, and the references name ITS offsets);
// foot_bytes(main offsets known so far): the bytes of the stripped main's EOF chunk and index, asked for once, when the layout reaches
// the EOF chunk, which lies behind every data chunk.
//   main:     identifier (10) | per gap: its other chunks, then data chunk g | at the gap's EOF chunk: the foot
//   sidecar:  identifier (10) | per gap: its search chunks, then data chunk g's reference | at the gap's EOF chunk: 5 bytes
// A reference is 4 + uvarint(offset) + uvarint(max_block - decoded) bytes, and the offset it names is new_hdr[k] (strip) or hdr_off(k).
// -> base[g] for g <= n (q_long, q_short: where gap g's descriptors start in the long and in the short list; they hold, in this order, the
// gap's own pieces as its walk meets them — a foot's pieces at the EOF chunk — and data chunk g's), new_hdr[k], the totals.
// status: kExtractOk, or kExtractCorrupt (a bad gap, an EOF chunk in front of a data chunk, a data chunk of no bytes or of more than
// max_block), or kExtractUnsupported (not exactly one EOF chunk: the end of a further stream without an identifier).
enum { kExtractOk = 0, kExtractCorrupt = 1, kExtractUnsupported = 3 };
struct ExtractLayout {
    std::vector<ExtractBase> base;
    std::vector<uint64_t> new_hdr;
    uint64_t side_len = 0, main_len = 0, foot_at = 0, foot_n = 0;
    uint64_t blocks = 0, info = 0, tables = 0, tables46 = 0, passed = 0, dropped = 0;
    uint32_t n_long = 0, n_short = 0;
    int status = kExtractOk;
};
template <class Gap, class Hdr, class Bytes, class Decoded, class Foot>
ExtractLayout extract_layout(size_t n, uint64_t max_block, bool strip, Gap gap, Hdr hdr_off, Bytes bytes, Decoded decoded, Foot foot_bytes) {
    ExtractLayout L;
    L.base.resize(n + 1);
    L.new_hdr.resize(n);
    uint64_t side = 10, main = 10, eofs = 0;
    uint32_t ql = 0, qs = 0;
    for (size_t g = 0; g <= n; g++) {
        const ExtractGap& G = gap(g);
        if (G.bad || (G.eofs && g < n)) { L.status = kExtractCorrupt; return L; }
        eofs += G.eofs;
        ExtractBase& b = L.base[g];
        b = ExtractBase{side, main, ql, qs, 0, 0};
        side += G.side_bytes + 5 * uint64_t(G.eofs);
        ql += G.side_long; qs += G.side_short;
        L.info += G.info; L.tables += G.tab45 + G.tab46; L.tables46 += G.tab46;
        if (strip) {
            main += G.main_bytes;
            ql += G.main_long; qs += G.main_short;
            L.passed += G.main_bytes; L.dropped += G.dropped_bytes;
        }
        if (g == n) break;
        const uint64_t dec = decoded(g);
        if (dec == 0 || dec > max_block) { L.status = kExtractCorrupt; return L; }
        b.mma = uint32_t(max_block - dec);
        L.new_hdr[g] = strip ? main : hdr_off(g);
        side += sidecar_ref_bytes(L.new_hdr[g], b.mma);
        if (strip) {
            main += bytes(g);
            extract_pieces(bytes(g), &ql, &qs);
        }
    }
    if (eofs != 1) { L.status = kExtractUnsupported; return L; }
    if (strip) {
        // the foot lies where the last gap's EOF chunk is met: behind the other chunks in front of it.  Its length does not depend on
        // that place, so the total is known here; the place itself is the emit lane's (extract_emit_gap), which walks the gap.
        L.foot_n = foot_bytes(L);
        main += L.foot_n;
        extract_pieces(L.foot_n, &ql, &qs);
    }
    L.blocks = n;
    L.side_len = side; L.main_len = strip ? main : 0;
    L.n_long = ql; L.n_short = qs;
    return L;
}

// What gap g's lane writes: the descriptors of its chunks' pieces (short ones at descs[n_long + ...]), the sidecar's EOF chunk and the
// foot's pieces where it meets the EOF chunk, and — for g < n — data chunk g's reference and, with strip, its pieces.
// span: the gap; next_begin: where the gap behind it begins (data chunk g is src[span.end, next_begin)).
MLZ_SEARCH_HD void extract_emit_gap(const uint8_t* src, ExtractSpan span, uint64_t next_begin, bool last, ExtractBase b, bool strip, uint64_t foot_n,
                                    uint8_t* side, PlaceDesc* descs, uint32_t n_long) {
    uint64_t so = b.side_off, mo = b.main_off;
    uint32_t ql = b.q_long, qs = n_long + b.q_short;
    extract_gap_walk(src, span.begin, span.end, [&](uint64_t p, uint8_t, uint64_t len, ExtractClass cl) {
        if (cl == kExSearch) {
            extract_put_pieces(p, so, len, 0, descs, &ql, &qs);
            so += len;
        } else if (cl == kExOther && strip) {
            extract_put_pieces(p, mo, len, kExtractToMain, descs, &ql, &qs);
            mo += len;
        } else if (cl == kExEof) {
            side[so] = 0x20; side[so + 1] = 1; side[so + 2] = side[so + 3] = side[so + 4] = 0;
            so += 5;
            if (strip) {
                extract_put_pieces(0, mo, foot_n, kExtractToMain | kExtractFromFoot, descs, &ql, &qs);
                mo += foot_n;
            }
        }
    });
    if (last) return;
    sidecar_put_ref(side + so, strip ? mo : span.end, b.mma);
    if (strip) extract_put_pieces(span.end, mo, next_begin - span.end, kExtractToMain, descs, &ql, &qs);
}

}  // namespace mlz
