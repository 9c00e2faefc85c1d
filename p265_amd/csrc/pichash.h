// Device-side decoded picture hash (p265r_batch_hash_async): the decoded_picture_hash SEI values of D.3.19
// (MD5, CRC, checksum) of the output planes, computed where the planes are.  The arithmetic and the word
// addressing are pichash_math.h's (shared with the host, pichash_host.cpp).  No counterpart in the reference.
//
// A plane row is its rb = W * bps bytes (W the picture's OWN width, DevPic::wh), a multiple of 4; rows start
// 64-byte aligned (planes 256-byte aligned, strides a multiple of 64 samples), so a row is q = rb / 16 aligned
// 16-byte chunks plus 0..3 tail words.
//
// Checksum, CRC: one streaming pass, grid (row groups, 3 planes, pictures) like digest_kernel, 16-byte loads,
// a wave reduction by shuffles (add / XOR) and one 32-bit atomic per wave into a zeroed accumulator per plane;
// hash_final_kernel turns the accumulators into the SEI bytes.
// MD5: serial per plane, one chain per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "intra.h"
#include "pichash_math.h"

namespace p265r {

__device__ __constant__ const PichashXpow kHashXpow = pichash_make_xpow();
constexpr PichashXpow kHashXpowHost = pichash_make_xpow();      // compile-time constants below only

// x^(8 * 1024): a lane's step from one 64-chunk piece of a row to the next; x^(128 * 2^s): the lane joins
constexpr uint32_t kPiece = pichash_xpow(kHashXpowHost, 8u * 1024u);
constexpr uint32_t kJoin0 = pichash_xpow(kHashXpowHost, 128u), kJoin1 = pichash_xpow(kHashXpowHost, 256u),
                   kJoin2 = pichash_xpow(kHashXpowHost, 512u), kJoin3 = pichash_xpow(kHashXpowHost, 1024u),
                   kJoin4 = pichash_xpow(kHashXpowHost, 2048u), kJoin5 = pichash_xpow(kHashXpowHost, 4096u);

constexpr int kHashRows = 8;       // plane rows per workgroup (checksum, CRC)

struct HashPlane {
    const uint8_t* p;
    int rb, h;                      // row bytes, rows
    uint32_t stride;                // bytes
};

__device__ __forceinline__ HashPlane hash_plane(const DevPic& P, const Geo& g, int c) {
    const uint32_t wh = P.wh;
    const int sub = c ? 1 : 0, sh = g.pel16 ? 1 : 0;
    HashPlane hp;
    hp.p = P.out[c];
    hp.rb = ((int)(wh & 0xffffu) >> sub) << sh;
    hp.h = (int)(wh >> 16) >> sub;
    hp.stride = (uint32_t)g.stride[c] << sh;
    return hp;
}

// grid (ceil(max plane height / kHashRows), 3, pictures), 256 threads; acc[3 * pic + c] zero on entry
__global__ __launch_bounds__(256) void hash_checksum_kernel(const DevPic* __restrict__ pics, Geo g,
                                                            uint32_t* __restrict__ acc) {
    const int c = blockIdx.y, pic = blockIdx.z;
    const HashPlane hp = hash_plane(pics[pic], g, c);
    const int y0 = blockIdx.x * kHashRows;
    if (y0 >= hp.h) return;                              // (block-uniform)
    const int rows = min(kHashRows, hp.h - y0);
    const int bps = g.pel16 ? 2 : 1, spw = 4 / bps;
    const int wpr = hp.rb >> 2, cpr = (wpr + 3) >> 2;    // words, 16-byte chunks (the last one partial) per row
    uint32_t sum = 0;
    for (int e = threadIdx.x; e < rows * cpr; e += 256) {
        const int yy = e / cpr, ci = e - yy * cpr;
        const int y = y0 + yy;
        const uint8_t* q = hp.p + (size_t)y * hp.stride + 16 * ci;
        const int nw = min(4, wpr - 4 * ci);
        uint32_t w[4] = {0, 0, 0, 0};
        if (nw == 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(q);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            for (int i = 0; i < nw; ++i) w[i] = reinterpret_cast<const uint32_t*>(q)[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nw) sum += pichash_checksum_word(w[i], (uint32_t)((4 * ci + i) * spw), (uint32_t)y, bps);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += (uint32_t)__shfl_xor((int)sum, s, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc + 3 * pic + c, sum);
}

// CRC.  A wave takes a row: lane l of piece p (64 chunks, the pieces right-aligned at the end of the row's q
// whole chunks, so the lanes without a chunk are LEADING zeros) folds its 16 bytes into a zero register; over
// the pieces of a long row a lane carries its register forward by x^(8 * 1024); six shuffle steps with the
// fixed constants x^(128 * 2^s) join the 64 lanes (lane l's bytes end 16 (63 - l) bytes before the row's last
// whole chunk does); the tail words are shifted in; one position multiply x^(8 (L - e) + 16), e the row's end,
// places the row in the message.  The rows of a wave XOR; one atomicXor per wave.
__global__ __launch_bounds__(256) void hash_crc_kernel(const DevPic* __restrict__ pics, Geo g,
                                                       uint32_t* __restrict__ acc) {
    const int c = blockIdx.y, pic = blockIdx.z;
    const HashPlane hp = hash_plane(pics[pic], g, c);
    const int y0 = blockIdx.x * kHashRows;
    if (y0 >= hp.h) return;                              // (block-uniform)
    const int rows = min(kHashRows, hp.h - y0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wpr = hp.rb >> 2, q = wpr >> 2, tail = wpr & 3;
    const int np = (q + 63) >> 6;
    const uint32_t L = (uint32_t)hp.rb * (uint32_t)hp.h;
    uint32_t contrib = 0;
    for (int yy = wave; yy < rows; yy += 4) {            // (wave-uniform)
        const int y = y0 + yy;
        const uint8_t* row = hp.p + (size_t)y * hp.stride;
        uint32_t r = 0;
        for (int p = 0; p < np; ++p) {
            const int ci = q - 64 * (np - p) + lane;
            uint32_t v = 0;
            if (ci >= 0) {
                const uint4 d = *reinterpret_cast<const uint4*>(row + 16 * ci);
                v = pichash_crc_word(pichash_crc_word(pichash_crc_word(pichash_crc_word(0u, d.x), d.y), d.z), d.w);
            }
            r = pichash_mulmod16(r, kPiece) ^ v;
        }
        r = pichash_mulmod16(r, kJoin0) ^ (uint32_t)__shfl_down((int)r, 1, 64);
        r = pichash_mulmod16(r, kJoin1) ^ (uint32_t)__shfl_down((int)r, 2, 64);
        r = pichash_mulmod16(r, kJoin2) ^ (uint32_t)__shfl_down((int)r, 4, 64);
        r = pichash_mulmod16(r, kJoin3) ^ (uint32_t)__shfl_down((int)r, 8, 64);
        r = pichash_mulmod16(r, kJoin4) ^ (uint32_t)__shfl_down((int)r, 16, 64);
        r = pichash_mulmod16(r, kJoin5) ^ (uint32_t)__shfl_down((int)r, 32, 64);
        // (lane 0 holds the row's whole chunks; the other lanes go on with values nobody reads)
        for (int i = 0; i < tail; ++i) r = pichash_crc_word(r, reinterpret_cast<const uint32_t*>(row + 16 * q)[i]);
        const uint32_t e = (uint32_t)(y + 1) * (uint32_t)hp.rb;
        contrib ^= pichash_mulmod16(r, pichash_xpow(kHashXpow, 8u * (L - e) + 16u));
    }
    if (lane == 0) atomicXor(acc + 3 * pic + c, contrib);
}

// accumulators -> the SEI bytes: one thread per plane
__global__ __launch_bounds__(64) void hash_final_kernel(const DevPic* __restrict__ pics, Geo g, int crc, int n_planes,
                                                        const uint32_t* __restrict__ acc, uint4* __restrict__ out) {
    const int pl = blockIdx.x * 64 + threadIdx.x;
    if (pl >= n_planes || (g.mono && pl % 3)) return;   // (monochrome: planes 1 and 2 stay zero)
    uint32_t v = acc[pl];
    uint32_t word;
    if (crc) {
        const HashPlane hp = hash_plane(pics[pl / 3], g, pl % 3);
        v ^= pichash_crc_init_term(kHashXpow, (uint32_t)hp.rb * (uint32_t)hp.h);
        word = (v >> 8) | (v & 0xFFu) << 8;              // two bytes, big-endian
    } else {
        word = __builtin_bswap32(v);                     // four bytes, big-endian
    }
    out[pl] = make_uint4(word, 0u, 0u, 0u);
}

// MD5: one chain per LANE, grid ceil(3 * pictures / 64) one-wave workgroups; the luma planes take the first lanes,
// then Cb, then Cr, so the lanes of a wave run chains of equal length.  A lane walks its plane block by block
// (row pointer and word position carried along, no division): 64 bytes inside one row at a 16-byte boundary are
// four 16-byte loads, a block that crosses a row or the message's end goes word by word (past the end: the
// padding words).  The next block's loads are issued before the 64 steps of this one; the compiler still waits for
// them first (a full wait behind the divergent fetch), so a block's time includes its load latency.  (The first form, one chain per
// wave on LDS-staged blocks, ran every step on all 64 lanes for one result: EXPERIMENTS.md A.11.)
__device__ __forceinline__ void hash_md5_fetch(const HashPlane& hp, uint32_t wpr, uint32_t n_words, const uint8_t*& row,
                                               uint32_t& xw, uint32_t& k, uint32_t m[16]) {
    if (k < n_words && (xw & 3u) == 0u && xw + 16u <= wpr) {
        // (global, not flat, loads)
        typedef uint32_t hash_u4 __attribute__((ext_vector_type(4)));
        const __attribute__((address_space(1))) hash_u4* q = (const __attribute__((address_space(1))) hash_u4*)(row + 4u * xw);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const hash_u4 v = q[i];
            m[4 * i] = v.x; m[4 * i + 1] = v.y; m[4 * i + 2] = v.z; m[4 * i + 3] = v.w;
        }
        xw += 16u;
        k += 16u;
        if (xw == wpr) { xw = 0u; row += hp.stride; }
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (k < n_words) {
            m[i] = *(const __attribute__((address_space(1))) uint32_t*)(row + 4u * xw);
            if (++xw == wpr) { xw = 0u; row += hp.stride; }
        } else {
            m[i] = pichash_md5_pad_word(k, n_words);
        }
        ++k;
    }
}

__global__ __launch_bounds__(64) void hash_md5_kernel(const DevPic* __restrict__ pics, Geo g, int n_pics,
                                                      uint4* __restrict__ out) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= (g.mono ? 1 : 3) * n_pics) return;        // (monochrome: the luma chains alone)
    const int c = idx / n_pics, pic = idx - c * n_pics;
    const HashPlane hp = hash_plane(pics[pic], g, c);
    const uint32_t wpr = (uint32_t)hp.rb >> 2, n_words = wpr * (uint32_t)hp.h;
    const uint32_t nb = pichash_md5_blocks(n_words);
    uint32_t st[4], cur[16], nxt[16];
    pichash_md5_init(st);
    const uint8_t* row = hp.p;
    uint32_t xw = 0, k = 0;
    hash_md5_fetch(hp, wpr, n_words, row, xw, k, cur);
    for (uint32_t b = 0; b < nb; ++b) {
        if (b + 1u < nb) hash_md5_fetch(hp, wpr, n_words, row, xw, k, nxt);
        pichash_md5_block(st, cur);
#pragma unroll
        for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
    }
    out[3 * pic + c] = make_uint4(st[0], st[1], st[2], st[3]);
}

}  // namespace p265r
