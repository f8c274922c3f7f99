// mlz_crc.hip.inc — masked CRC32C of whole blocks on the device (included by mlz_hip.hip).
//
// Replaces crc() of the reference (minlz.go:133-140: Castagnoli CRC, rotate by 15, add
// 0xa282ead8), which the stream Writer/Reader compute per block over the UNCOMPRESSED bytes
// (writer.go:887, reader.go:341-351).  CRCs are linear, so a block is cut into pieces; each piece's
// table CRC is multiplied by x^(8 * bytes_after_it) mod P (constants from tables, or square-and-multiply
// over a table of x^(2^k)), and the pieces are XOR-reduced:  crc(A || B) = crc(A) * x^(8|B|) xor crc(B).

namespace mlz {

constexpr uint32_t kCrcPoly = 0x82f63b78u;  // reflected Castagnoli polynomial

struct CrcPow { uint32_t x2n[32]; };  // x^(2^k) mod P, reflected (bit 31 = x^0)

__host__ __device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {   // a(x) * b(x) mod P, reflected; 0 for a == 0
    uint32_t p = 0;
    while (a) {                       // bit 31 of a is its x^0 term: terms of a from low degree up, b multiplied by x each step
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(n * 2^k) mod P
__host__ __device__ __forceinline__ uint32_t crc_x2n(const CrcPow& t, uint64_t n, uint32_t k) {
    uint32_t p = 1u << 31;
    while (n) {
        if (n & 1) p = crc_mulmod(t.x2n[k & 31], p);
        n >>= 1;
        k++;
    }
    return p;
}

// Round 4: the CRC as a tile pass.  (Rounds 1-3: one lane per 1 KiB piece, byte by byte through one LDS table, lane stride 1 KiB,
// a square-and-multiply power per lane, one atomic per wave: 0.105 ms per 100 MB.)  Now one 256-thread workgroup per 32 KiB tile:
// thread t takes bytes [128 t, 128 t + 128) of the tile with eight 16-byte loads (every 128-byte line of the tile is read by one
// lane: whole lines, no partial sectors), runs slice-by-4 over its 32 dwords (four INDEPENDENT table look-ups per dword instead of
// four dependent ones), multiplies by the constant x^(1024 (255 - t)) from a table, and the workgroup xors its 256 values into the
// tile's value; crc_block_kernel then folds a block's tiles with a second table of constants x^(2^18 j).  The affine parts
// (initial value, final complement) telescope over any partition into consecutive pieces (DESIGN.md §4 "CRC"), so tiles are
// pieces like any other.  Only a block's ragged last tile pays a computed power per lane.
struct CrcTabs { uint32_t k128[256]; uint32_t ktile[256]; };   // x^(1024 (255 - t)); x^(8 * 32768 * j)  (mod P, reflected)

__global__ __launch_bounds__(256) void crc_tile_kernel(const uint8_t* __restrict__ base, const BlockInfo* __restrict__ blocks,
                                                       const uint32_t* __restrict__ tile_block, const CrcTabs* __restrict__ tabs, CrcPow pw,
                                                       uint32_t* __restrict__ tile_crc) {
    __shared__ uint32_t T[4][256];
    __shared__ uint32_t red[4];
    const int tid = threadIdx.x;
    {
        uint32_t c = uint32_t(tid);
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        T[0][tid] = c;
    }
    __syncthreads();
    for (int j = 1; j < 4; j++) {   // T[j][i] = the CRC of byte i followed by j zero bytes
        const uint32_t p = T[j - 1][tid];
        T[j][tid] = (p >> 8) ^ T[0][p & 0xff];
        __syncthreads();
    }
    const uint32_t gt = blockIdx.x;
    const uint32_t bi = tile_block[gt];
    const BlockInfo b = blocks[bi];
    const uint64_t toff = uint64_t(gt - b.first_tile) << kTileLog;
    const uint32_t n = uint32_t(b.src_len - toff < kTile ? b.src_len - toff : kTile);
    const uint8_t* p = base + b.src_off + toff + 128 * uint32_t(tid);
    const uint32_t my0 = 128 * uint32_t(tid);
    uint32_t c = 0;
    if (my0 < n) {
        const uint32_t len = n - my0 < 128 ? n - my0 : 128;
        c = 0xffffffffu;
        if (len == 128) {
            uint4 x[8];
#pragma unroll
            for (int q = 0; q < 8; q++) __builtin_memcpy(&x[q], p + 16 * q, 16);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t w4[4] = {x[q].x, x[q].y, x[q].z, x[q].w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t v = c ^ w4[j];
                    c = T[3][v & 0xff] ^ T[2][(v >> 8) & 0xff] ^ T[1][(v >> 16) & 0xff] ^ T[0][v >> 24];
                }
            }
        } else {
            for (uint32_t i = 0; i < len; i++) c = T[0][(c ^ p[i]) & 0xff] ^ (c >> 8);
        }
        c = ~c;
        const uint32_t after = n - my0 - len;    // bytes of the tile behind my piece
        if (n == kTile) c = crc_mulmod(c, tabs->k128[tid]);   // (the product is symmetric; the loop runs over the bits of its first argument)
        else if (after) c = crc_mulmod(crc_x2n(pw, after, 3), c);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) tile_crc[gt] = red[0] ^ red[1] ^ red[2] ^ red[3];
}

// one wavefront per block: the block's tile values -> its masked CRC  ((c >> 15 | c << 17) + 0xa282ead8, minlz.go:139)
__global__ __launch_bounds__(64) void crc_block_kernel(const BlockInfo* __restrict__ blocks, const uint32_t* __restrict__ tile_crc,
                                                       const CrcTabs* __restrict__ tabs, CrcPow pw, uint32_t* __restrict__ out, int n_blocks) {
    const int bi = blockIdx.x, lane = threadIdx.x;
    if (bi >= n_blocks) return;
    const BlockInfo b = blocks[bi];
    uint32_t c = 0;
    if (b.n_tiles) {
        const uint32_t last = b.n_tiles - 1;
        // the whole tiles before the last one, a run of consecutive tiles per lane: Horner with the constant x^(8 * 32768) inside the run,
        // then the run's distance from the last tile (a table constant up to 255 tiles, a computed power beyond: buffers of over 8 MiB)
        uint32_t acc = 0;
        const uint32_t R = (last + 63) / 64;
        const uint32_t t0 = uint32_t(lane) * R, t1 = t0 + R < last ? t0 + R : last;
        if (t0 < last) {
            for (uint32_t t = t0; t < t1; t++) acc = crc_mulmod(acc, tabs->ktile[1]) ^ tile_crc[b.first_tile + t];
            const uint32_t j = last - t1;                      // whole tiles between my run and the last tile
            if (j) acc = j < 256 ? crc_mulmod(acc, tabs->ktile[j]) : crc_mulmod(crc_x2n(pw, uint64_t(j) << kTileLog, 3), acc);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
        const uint64_t rem = b.src_len - (uint64_t(last) << kTileLog);   // bytes of the last tile
        if (acc) acc = crc_mulmod(crc_x2n(pw, rem, 3), acc);
        c = acc ^ tile_crc[b.first_tile + last];
    }
    if (lane == 0) out[bi] = ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

}  // namespace mlz
