// pichash_math.h -- the arithmetic of the decoded picture hash (H.265 D.3.19: MD5, CRC, checksum) in a form
// that splits over the plane, shared by the host (pichash_host.cpp, tools/hash_check.cpp) and the device
// (pichash.h).  Plain C++: no HIP types, no inline assembly; PICHASH_FN carries the qualifiers.
//
// pictureData of one plane = its W x H samples in raster order, one byte per sample at BitDepth 8 and two
// (little-endian) above: bps bytes per sample.  The hashes run over that byte string of L = W * H * bps bytes.
//
// Words.  Picture sizes are multiples of 8 luma samples, so a chroma plane is a multiple of 4 samples wide and
// high and every plane holds a multiple of 16 samples.  A row is W * bps bytes with W % 4 == 0: a multiple of
// 4 bytes, so the string is a sequence of L / 4 little-endian 32-bit words, wpr = W * bps / 4 per row, and no
// word straddles a row: word k sits in row k / wpr at word k % wpr.  In memory a row is exactly those W * bps
// bytes and consecutive rows are `stride` bytes apart (rows are in general not contiguous: the device planes
// have a stride of a multiple of 64 samples).  L is a multiple of 4 (even of 16), so MD5's 0x80 padding byte
// opens a word of its own, 0x00000080, and the padded message is whole words too.
//
// Checksum (D-23): sum mod 2^32 over the samples of ((s & 0xFF) ^ m) [+ ((s >> 8) ^ m) above 8 bits] with
// m = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8).  Position-keyed and order-free: partial sums add.
//
// CRC (D-22): CRC-16, polynomial P = x^16 + x^12 + x^5 + 1 (0x1021), register initialised to 0xFFFF, bits MSB
// first, 16 zero bits appended.  Over GF(2) the register after shifting in a bit b is (R * x + b) mod P, so
// with D(x) the message as a polynomial (first bit = highest power)
//     crc = (0xFFFF * x^(8L+16) + D(x) * x^16) mod P
// and for any cut of the message into byte segments [s, e)
//     D(x) * x^16 = XOR over segments of (D_seg(x) mod P) * x^(8 (L - e) + 16)      (mod P)
// where D_seg mod P is the ZERO-initialised register after the segment's bytes (pichash_crc_word).  The terms
// XOR in any order.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define PICHASH_FN __host__ __device__ constexpr
#else
#define PICHASH_FN constexpr
#endif

// ---- words -------------------------------------------------------------------------------------------------
// byte offset of message word k in a plane of wpr words per row and stride_bytes between rows
PICHASH_FN uint64_t pichash_word_offset(uint32_t k, uint32_t wpr, uint64_t stride_bytes) {
    const uint32_t y = k / wpr;
    return (uint64_t)y * stride_bytes + 4u * (uint64_t)(k - y * wpr);
}

// ---- checksum ----------------------------------------------------------------------------------------------
PICHASH_FN uint32_t pichash_mask(uint32_t x, uint32_t y) { return (x & 0xFFu) ^ (y & 0xFFu) ^ (x >> 8) ^ (y >> 8); }

// the checksum terms of one word: samples x0 .. x0 + 4 / bps - 1 of row y (x0 a multiple of 4 / bps).  The
// samples of a word share x >> 8 and all but the low bits of x & 0xFF, so their masks are m(x0, y) ^ i: the
// word is XORed with the per-byte masks at once and its four bytes are summed.
PICHASH_FN uint32_t pichash_checksum_word(uint32_t w, uint32_t x0, uint32_t y, int bps) {
    const uint32_t m = pichash_mask(x0, y) * 0x01010101u;
    const uint32_t v = w ^ m ^ (bps == 1 ? 0x03020100u : 0x01010000u);
    const uint32_t t = (v & 0x00FF00FFu) + ((v >> 8) & 0x00FF00FFu);
    return (t & 0xFFFFu) + (t >> 16);
}

// ---- CRC: GF(2)[x] mod P ----------------------------------------------------------------------------------
// a polynomial of degree < 32 reduced to degree < 16: x^16 = x^12 + x^5 + 1 (mod P), so the high half t folds
// down as t * 0x1021; the part of that product above bit 15 shrinks by 4 bits per round (16 -> 12 -> 8 -> 4 -> 0)
PICHASH_FN uint32_t pichash_crc_reduce32(uint32_t v) {
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = v >> 16;
        v = (v & 0xFFFFu) ^ t ^ (t << 5) ^ (t << 12);
    }
    return v;
}

// a * b mod P (a, b < 2^16)
PICHASH_FN uint32_t pichash_mulmod16(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 16; ++i) p ^= (a << i) & (0u - ((b >> i) & 1u));
    return pichash_crc_reduce32(p);
}

// the segment update: the register r (zero at the segment's start) after the four bytes of message word w
// (little-endian in memory, so the first byte is the low one) are shifted in, without appended zeros
PICHASH_FN uint32_t pichash_crc_word(uint32_t r, uint32_t w) {
    const uint32_t v = __builtin_bswap32(w);
    r = pichash_crc_reduce32((r << 16) ^ (v >> 16));
    return pichash_crc_reduce32((r << 16) ^ (v & 0xFFFFu));
}

// x^k mod P for any 32-bit k (8192 x 4320 x 2 bytes need 30 bits) from four tables of 256:
// t[i][d] = x^(d * 256^i) mod P, three multiplies per power.  The host builds it at compile time.
struct PichashXpow {
    uint16_t t[4][256];
};

PICHASH_FN PichashXpow pichash_make_xpow() {
    PichashXpow T{};
    uint32_t step = 2;                                   // x^(256^i)
    for (int i = 0; i < 4; ++i) {
        uint32_t v = 1;
        for (int d = 0; d < 256; ++d) {
            T.t[i][d] = (uint16_t)v;
            v = pichash_mulmod16(v, step);
        }
        step = v;                                        // x^(256 * 256^i)
    }
    return T;
}

PICHASH_FN uint32_t pichash_xpow(const PichashXpow& T, uint32_t k) {
    const uint32_t a = pichash_mulmod16(T.t[0][k & 255u], T.t[1][(k >> 8) & 255u]);
    const uint32_t b = pichash_mulmod16(T.t[2][(k >> 16) & 255u], T.t[3][k >> 24]);
    return pichash_mulmod16(a, b);
}

// the initial-value term of a message of L bytes: 0xFFFF * x^(8L+16) mod P
PICHASH_FN uint32_t pichash_crc_init_term(const PichashXpow& T, uint32_t L) {
    return pichash_mulmod16(0xFFFFu, pichash_xpow(T, 8u * L + 16u));
}

// ---- MD5 (RFC 1321) ----------------------------------------------------------------------------------------
PICHASH_FN uint32_t pichash_rol(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define PICHASH_MD5_STEP(f, a, b, c, d, m, k, s) a = b + pichash_rol(a + (f) + (k) + (m), s)
// (the select form: one bit-field-insert instruction where the target has one)
#define PICHASH_F(b, c, d) (((b) & (c)) | (~(b) & (d)))
#define PICHASH_G(b, c, d) (((d) & (b)) | (~(d) & (c)))
#define PICHASH_H(b, c, d) ((b) ^ (c) ^ (d))
#define PICHASH_I(b, c, d) ((c) ^ ((b) | ~(d)))

// the block function on 16 little-endian words
PICHASH_FN void pichash_md5_block(uint32_t st[4], const uint32_t m[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    PICHASH_MD5_STEP(PICHASH_F(b, c, d), a, b, c, d, m[0], 0xd76aa478u, 7);
    PICHASH_MD5_STEP(PICHASH_F(a, b, c), d, a, b, c, m[1], 0xe8c7b756u, 12);
    PICHASH_MD5_STEP(PICHASH_F(d, a, b), c, d, a, b, m[2], 0x242070dbu, 17);
    PICHASH_MD5_STEP(PICHASH_F(c, d, a), b, c, d, a, m[3], 0xc1bdceeeu, 22);
    PICHASH_MD5_STEP(PICHASH_F(b, c, d), a, b, c, d, m[4], 0xf57c0fafu, 7);
    PICHASH_MD5_STEP(PICHASH_F(a, b, c), d, a, b, c, m[5], 0x4787c62au, 12);
    PICHASH_MD5_STEP(PICHASH_F(d, a, b), c, d, a, b, m[6], 0xa8304613u, 17);
    PICHASH_MD5_STEP(PICHASH_F(c, d, a), b, c, d, a, m[7], 0xfd469501u, 22);
    PICHASH_MD5_STEP(PICHASH_F(b, c, d), a, b, c, d, m[8], 0x698098d8u, 7);
    PICHASH_MD5_STEP(PICHASH_F(a, b, c), d, a, b, c, m[9], 0x8b44f7afu, 12);
    PICHASH_MD5_STEP(PICHASH_F(d, a, b), c, d, a, b, m[10], 0xffff5bb1u, 17);
    PICHASH_MD5_STEP(PICHASH_F(c, d, a), b, c, d, a, m[11], 0x895cd7beu, 22);
    PICHASH_MD5_STEP(PICHASH_F(b, c, d), a, b, c, d, m[12], 0x6b901122u, 7);
    PICHASH_MD5_STEP(PICHASH_F(a, b, c), d, a, b, c, m[13], 0xfd987193u, 12);
    PICHASH_MD5_STEP(PICHASH_F(d, a, b), c, d, a, b, m[14], 0xa679438eu, 17);
    PICHASH_MD5_STEP(PICHASH_F(c, d, a), b, c, d, a, m[15], 0x49b40821u, 22);

    PICHASH_MD5_STEP(PICHASH_G(b, c, d), a, b, c, d, m[1], 0xf61e2562u, 5);
    PICHASH_MD5_STEP(PICHASH_G(a, b, c), d, a, b, c, m[6], 0xc040b340u, 9);
    PICHASH_MD5_STEP(PICHASH_G(d, a, b), c, d, a, b, m[11], 0x265e5a51u, 14);
    PICHASH_MD5_STEP(PICHASH_G(c, d, a), b, c, d, a, m[0], 0xe9b6c7aau, 20);
    PICHASH_MD5_STEP(PICHASH_G(b, c, d), a, b, c, d, m[5], 0xd62f105du, 5);
    PICHASH_MD5_STEP(PICHASH_G(a, b, c), d, a, b, c, m[10], 0x02441453u, 9);
    PICHASH_MD5_STEP(PICHASH_G(d, a, b), c, d, a, b, m[15], 0xd8a1e681u, 14);
    PICHASH_MD5_STEP(PICHASH_G(c, d, a), b, c, d, a, m[4], 0xe7d3fbc8u, 20);
    PICHASH_MD5_STEP(PICHASH_G(b, c, d), a, b, c, d, m[9], 0x21e1cde6u, 5);
    PICHASH_MD5_STEP(PICHASH_G(a, b, c), d, a, b, c, m[14], 0xc33707d6u, 9);
    PICHASH_MD5_STEP(PICHASH_G(d, a, b), c, d, a, b, m[3], 0xf4d50d87u, 14);
    PICHASH_MD5_STEP(PICHASH_G(c, d, a), b, c, d, a, m[8], 0x455a14edu, 20);
    PICHASH_MD5_STEP(PICHASH_G(b, c, d), a, b, c, d, m[13], 0xa9e3e905u, 5);
    PICHASH_MD5_STEP(PICHASH_G(a, b, c), d, a, b, c, m[2], 0xfcefa3f8u, 9);
    PICHASH_MD5_STEP(PICHASH_G(d, a, b), c, d, a, b, m[7], 0x676f02d9u, 14);
    PICHASH_MD5_STEP(PICHASH_G(c, d, a), b, c, d, a, m[12], 0x8d2a4c8au, 20);

    PICHASH_MD5_STEP(PICHASH_H(b, c, d), a, b, c, d, m[5], 0xfffa3942u, 4);
    PICHASH_MD5_STEP(PICHASH_H(a, b, c), d, a, b, c, m[8], 0x8771f681u, 11);
    PICHASH_MD5_STEP(PICHASH_H(d, a, b), c, d, a, b, m[11], 0x6d9d6122u, 16);
    PICHASH_MD5_STEP(PICHASH_H(c, d, a), b, c, d, a, m[14], 0xfde5380cu, 23);
    PICHASH_MD5_STEP(PICHASH_H(b, c, d), a, b, c, d, m[1], 0xa4beea44u, 4);
    PICHASH_MD5_STEP(PICHASH_H(a, b, c), d, a, b, c, m[4], 0x4bdecfa9u, 11);
    PICHASH_MD5_STEP(PICHASH_H(d, a, b), c, d, a, b, m[7], 0xf6bb4b60u, 16);
    PICHASH_MD5_STEP(PICHASH_H(c, d, a), b, c, d, a, m[10], 0xbebfbc70u, 23);
    PICHASH_MD5_STEP(PICHASH_H(b, c, d), a, b, c, d, m[13], 0x289b7ec6u, 4);
    PICHASH_MD5_STEP(PICHASH_H(a, b, c), d, a, b, c, m[0], 0xeaa127fau, 11);
    PICHASH_MD5_STEP(PICHASH_H(d, a, b), c, d, a, b, m[3], 0xd4ef3085u, 16);
    PICHASH_MD5_STEP(PICHASH_H(c, d, a), b, c, d, a, m[6], 0x04881d05u, 23);
    PICHASH_MD5_STEP(PICHASH_H(b, c, d), a, b, c, d, m[9], 0xd9d4d039u, 4);
    PICHASH_MD5_STEP(PICHASH_H(a, b, c), d, a, b, c, m[12], 0xe6db99e5u, 11);
    PICHASH_MD5_STEP(PICHASH_H(d, a, b), c, d, a, b, m[15], 0x1fa27cf8u, 16);
    PICHASH_MD5_STEP(PICHASH_H(c, d, a), b, c, d, a, m[2], 0xc4ac5665u, 23);

    PICHASH_MD5_STEP(PICHASH_I(b, c, d), a, b, c, d, m[0], 0xf4292244u, 6);
    PICHASH_MD5_STEP(PICHASH_I(a, b, c), d, a, b, c, m[7], 0x432aff97u, 10);
    PICHASH_MD5_STEP(PICHASH_I(d, a, b), c, d, a, b, m[14], 0xab9423a7u, 15);
    PICHASH_MD5_STEP(PICHASH_I(c, d, a), b, c, d, a, m[5], 0xfc93a039u, 21);
    PICHASH_MD5_STEP(PICHASH_I(b, c, d), a, b, c, d, m[12], 0x655b59c3u, 6);
    PICHASH_MD5_STEP(PICHASH_I(a, b, c), d, a, b, c, m[3], 0x8f0ccc92u, 10);
    PICHASH_MD5_STEP(PICHASH_I(d, a, b), c, d, a, b, m[10], 0xffeff47du, 15);
    PICHASH_MD5_STEP(PICHASH_I(c, d, a), b, c, d, a, m[1], 0x85845dd1u, 21);
    PICHASH_MD5_STEP(PICHASH_I(b, c, d), a, b, c, d, m[8], 0x6fa87e4fu, 6);
    PICHASH_MD5_STEP(PICHASH_I(a, b, c), d, a, b, c, m[15], 0xfe2ce6e0u, 10);
    PICHASH_MD5_STEP(PICHASH_I(d, a, b), c, d, a, b, m[6], 0xa3014314u, 15);
    PICHASH_MD5_STEP(PICHASH_I(c, d, a), b, c, d, a, m[13], 0x4e0811a1u, 21);
    PICHASH_MD5_STEP(PICHASH_I(b, c, d), a, b, c, d, m[4], 0xf7537e82u, 6);
    PICHASH_MD5_STEP(PICHASH_I(a, b, c), d, a, b, c, m[11], 0xbd3af235u, 10);
    PICHASH_MD5_STEP(PICHASH_I(d, a, b), c, d, a, b, m[2], 0x2ad7d2bbu, 15);
    PICHASH_MD5_STEP(PICHASH_I(c, d, a), b, c, d, a, m[9], 0xeb86d391u, 21);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

PICHASH_FN void pichash_md5_init(uint32_t st[4]) {
    st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u;
}

// blocks of the padded message of n_words message words: the 0x80 word, zero words up to word 14 of the last
// block, then the two words of the bit length (32 * n_words, low word first)
PICHASH_FN uint32_t pichash_md5_blocks(uint32_t n_words) { return (n_words + 3u + 15u) / 16u; }

// word k >= n_words of the padded message
PICHASH_FN uint32_t pichash_md5_pad_word(uint32_t k, uint32_t n_words) {
    const uint32_t last = 16u * pichash_md5_blocks(n_words);
    if (k == n_words) return 0x80u;
    if (k == last - 2u) return n_words << 5;
    if (k == last - 1u) return n_words >> 27;
    return 0u;
}
