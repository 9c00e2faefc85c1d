// pichash_host.cpp -- p265r_plane_hash_host: the decoded picture hash of a host plane through the split forms
// of pichash_math.h, the same functions the device kernels (pichash.h) run.  Plain C++ (no HIP): it is also
// compiled into tools/hash_check.cpp under the host sanitizers.
#include <cstring>

#include "../../include/p265r.h"
#include "pichash_math.h"

namespace {

constexpr PichashXpow kXpow = pichash_make_xpow();

struct Plane {
    const unsigned char* p;
    uint32_t wpr;            // words per row
    uint64_t stride;         // bytes
    uint32_t word(uint32_t k) const {
        const unsigned char* q = p + pichash_word_offset(k, wpr, stride);
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
};

}  // namespace

extern "C" int p265r_plane_hash_host(const void* plane, int width, int height, uint64_t stride_bytes,
                                     int bytes_per_sample, int hash_type, uint32_t seg_words, uint8_t out[16]) {
    if (!plane || !out || width <= 0 || height <= 0 || width % 4 || height % 4) return P265R_EINVAL;
    if (bytes_per_sample != 1 && bytes_per_sample != 2) return P265R_EINVAL;
    if (stride_bytes < (uint64_t)width * (uint64_t)bytes_per_sample) return P265R_EINVAL;
    if (hash_type != P265R_HASH_MD5 && hash_type != P265R_HASH_CRC && hash_type != P265R_HASH_CHECKSUM) return P265R_EINVAL;
    if ((uint64_t)width * (uint64_t)height * (uint64_t)bytes_per_sample >= (1ull << 29)) return P265R_EINVAL;   // 8 L + 16 in 32 bits
    const int bps = bytes_per_sample;
    const Plane P{static_cast<const unsigned char*>(plane), (uint32_t)(width * bps) / 4u, stride_bytes};
    const uint32_t n_words = P.wpr * (uint32_t)height;
    const uint32_t seg = seg_words ? seg_words : n_words;
    const uint32_t n_seg = (n_words + seg - 1) / seg;
    std::memset(out, 0, 16);
    if (hash_type == P265R_HASH_MD5) {
        // the chain is serial: the segmentation changes nothing but the addressing (word by word)
        uint32_t st[4], m[16];
        pichash_md5_init(st);
        const uint32_t nb = pichash_md5_blocks(n_words);
        for (uint32_t b = 0; b < nb; ++b) {
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t k = 16 * b + i;
                m[i] = k < n_words ? P.word(k) : pichash_md5_pad_word(k, n_words);
            }
            pichash_md5_block(st, m);
        }
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(st[i] >> (8 * k));
        return P265R_OK;
    }
    const uint32_t spw = 4u / (uint32_t)bps;                  // samples per word
    uint32_t acc = 0;
    for (uint32_t s = n_seg; s-- > 0;) {                       // last segment first: the terms combine in any order
        const uint32_t k0 = s * seg, k1 = k0 + seg < n_words ? k0 + seg : n_words;
        if (hash_type == P265R_HASH_CHECKSUM) {
            uint32_t sum = 0;
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t y = k / P.wpr;
                sum += pichash_checksum_word(P.word(k), (k - y * P.wpr) * spw, y, bps);
            }
            acc += sum;
        } else {
            uint32_t r = 0;
            for (uint32_t k = k0; k < k1; ++k) r = pichash_crc_word(r, P.word(k));
            acc ^= pichash_mulmod16(r, pichash_xpow(kXpow, 8u * (4u * (n_words - k1)) + 16u));
        }
    }
    if (hash_type == P265R_HASH_CHECKSUM) {
        out[0] = (uint8_t)(acc >> 24); out[1] = (uint8_t)(acc >> 16); out[2] = (uint8_t)(acc >> 8); out[3] = (uint8_t)acc;
    } else {
        acc ^= pichash_crc_init_term(kXpow, 4u * n_words);
        out[0] = (uint8_t)(acc >> 8); out[1] = (uint8_t)acc;
    }
    return P265R_OK;
}
