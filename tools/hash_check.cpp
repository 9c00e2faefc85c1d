// hash_check.cpp -- `make hash-check`: the picture hash arithmetic (pichash_math.h through p265r_plane_hash_host,
// pichash_host.cpp) as a stand-alone CPU program under ASan + UBSan: RFC 1321's test vectors, the CRC and the
// checksum against restatements of D.3.19 written here (bit-serial, per sample), exact-size buffers with
// padded strides, every rejection code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../include/p265r.h"
#include "../p265_amd/csrc/pichash_math.h"

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static std::string hex(const uint8_t* p, int n) {
    std::string s;
    char b[3];
    for (int i = 0; i < n; ++i) { std::snprintf(b, sizeof b, "%02x", p[i]); s += b; }
    return s;
}

// MD5 of a byte string: byte-wise padding written here, the block function of pichash_math.h
static std::string md5_bytes(const std::string& msg) {
    std::vector<uint8_t> m(msg.begin(), msg.end());
    const uint64_t bits = 8ull * msg.size();
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 0; i < 8; ++i) m.push_back((uint8_t)(bits >> (8 * i)));
    uint32_t st[4];
    pichash_md5_init(st);
    for (size_t b = 0; b < m.size(); b += 64) {
        uint32_t w[16];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)m[b + 4 * i] | (uint32_t)m[b + 4 * i + 1] << 8 | (uint32_t)m[b + 4 * i + 2] << 16 |
                   (uint32_t)m[b + 4 * i + 3] << 24;
        pichash_md5_block(st, w);
    }
    uint8_t out[16];
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(st[i] >> (8 * k));
    return hex(out, 16);
}

// (D-22), bit by bit: the register starts at 0xFFFF, the data bits go in MSB first, then 16 zero bits
static uint32_t crc_bit_serial(const std::vector<uint8_t>& data) {
    uint32_t crc = 0xFFFF;
    auto shift = [&](uint32_t bit) {
        const uint32_t msb = (crc >> 15) & 1u;
        crc = (((crc << 1) | bit) & 0xFFFFu) ^ (msb * 0x1021u);
    };
    for (uint8_t b : data)
        for (int k = 7; k >= 0; --k) shift((b >> k) & 1u);
    for (int k = 0; k < 16; ++k) shift(0);
    return crc;
}

// a plane of exactly (h - 1) * stride + w * bps bytes: a read past a row's end in the last row leaves the buffer
struct Plane {
    int w, h, bps;
    size_t stride;
    uint8_t* p;
    Plane(int w_, int h_, int bps_, size_t pad) : w(w_), h(h_), bps(bps_), stride((size_t)w_ * bps_ + pad) {
        p = static_cast<uint8_t*>(std::malloc((size_t)(h - 1) * stride + (size_t)w * bps));
        std::memset(p, 0xEE, (size_t)(h - 1) * stride + (size_t)w * bps);
    }
    ~Plane() { std::free(p); }
    Plane(const Plane&) = delete;
    void set(int x, int y, uint32_t v) {
        uint8_t* q = p + (size_t)y * stride + (size_t)x * bps;
        q[0] = (uint8_t)v;
        if (bps == 2) q[1] = (uint8_t)(v >> 8);
    }
    uint32_t get(int x, int y) const {
        const uint8_t* q = p + (size_t)y * stride + (size_t)x * bps;
        return bps == 2 ? (uint32_t)q[0] | (uint32_t)q[1] << 8 : q[0];
    }
    std::vector<uint8_t> picture_data() const {
        std::vector<uint8_t> d;
        for (int y = 0; y < h; ++y)
            for (int i = 0; i < w * bps; ++i) d.push_back(p[(size_t)y * stride + i]);
        return d;
    }
};

static void check_plane(const Plane& P) {
    const std::vector<uint8_t> data = P.picture_data();
    // the restatements
    const uint32_t crc = crc_bit_serial(data);
    uint32_t sum = 0;
    for (int y = 0; y < P.h; ++y)
        for (int x = 0; x < P.w; ++x) {
            const uint32_t m = (uint32_t)((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)), s = P.get(x, y);
            sum += (s & 0xFF) ^ m;
            if (P.bps == 2) sum += (s >> 8) ^ m;
        }
    const std::string md5 = md5_bytes(std::string(data.begin(), data.end()));
    for (uint32_t seg : {0u, 1u, 3u, 16u, 64u, 1000u}) {
        uint8_t out[16];
        CHECK(p265r_plane_hash_host(P.p, P.w, P.h, P.stride, P.bps, P265R_HASH_CRC, seg, out) == P265R_OK);
        CHECK(out[0] == (crc >> 8) && out[1] == (crc & 0xFF));
        for (int i = 2; i < 16; ++i) CHECK(out[i] == 0);
        CHECK(p265r_plane_hash_host(P.p, P.w, P.h, P.stride, P.bps, P265R_HASH_CHECKSUM, seg, out) == P265R_OK);
        CHECK(out[0] == (uint8_t)(sum >> 24) && out[1] == (uint8_t)(sum >> 16) && out[2] == (uint8_t)(sum >> 8) && out[3] == (uint8_t)sum);
        for (int i = 4; i < 16; ++i) CHECK(out[i] == 0);
        CHECK(p265r_plane_hash_host(P.p, P.w, P.h, P.stride, P.bps, P265R_HASH_MD5, seg, out) == P265R_OK);
        CHECK(hex(out, 16) == md5);
    }
}

int main() {
    // RFC 1321, appendix A.5
    const char* digits = "12345678901234567890123456789012345678901234567890123456789012345678901234567890";
    CHECK(md5_bytes("") == "d41d8cd98f00b204e9800998ecf8427e");
    CHECK(md5_bytes("a") == "0cc175b9c0f1b6a831c399e269772661");
    CHECK(md5_bytes("abc") == "900150983cd24fb0d6963f7d28e17f72");
    CHECK(md5_bytes("message digest") == "f96b697d7cb7938d525a2f31aaf161d0");
    CHECK(md5_bytes("abcdefghijklmnopqrstuvwxyz") == "c3fcd3d76192e4007dfb496cca67e13b");
    CHECK(md5_bytes("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789") == "d174ab98d277d9f5a5611c2c9f419d9f");
    CHECK(md5_bytes(digits) == "57edf4a22be3c955ac49da2e2107b67a");
    {   // the 80-byte vector is a 20 x 4 plane: the word padding of the ABI function
        uint8_t out[16];
        CHECK(p265r_plane_hash_host(digits, 20, 4, 20, 1, P265R_HASH_MD5, 0, out) == P265R_OK);
        CHECK(hex(out, 16) == "57edf4a22be3c955ac49da2e2107b67a");
        CHECK(p265r_plane_hash_host(digits, 4, 4, 8, 2, P265R_HASH_MD5, 7, out) == P265R_OK);        // 32 of its bytes
        CHECK(hex(out, 16) == md5_bytes(std::string(digits, 32)));
    }
    // GF(2) helpers: x^k by the tables against repeated multiplication by x
    {
        constexpr PichashXpow T = pichash_make_xpow();
        uint32_t v = 1;
        for (uint32_t k = 0; k < 70000; ++k) {
            if (k < 600 || k % 257 == 0 || k > 69000) CHECK(pichash_xpow(T, k) == v);
            v = pichash_mulmod16(v, 2);
        }
        CHECK(pichash_mulmod16(pichash_xpow(T, 0x12345678u), pichash_xpow(T, 0x0FEDCBA9u)) == pichash_xpow(T, 0x22222221u));
    }
    // planes: random, zero, one maximal sample at either end; tight and padded strides
    std::srand(5);
    const int sizes[][2] = {{4, 4}, {8, 8}, {8, 4}, {12, 4}, {36, 20}, {68, 36}, {260, 260}, {520, 264}};
    for (const auto& s : sizes)
        for (int bps : {1, 2})
            for (size_t pad : {(size_t)0, (size_t)44}) {
                const uint32_t mx = bps == 2 ? 0xFFFFu : 0xFFu;
                Plane P(s[0], s[1], bps, pad);
                for (int y = 0; y < P.h; ++y)
                    for (int x = 0; x < P.w; ++x) P.set(x, y, (uint32_t)std::rand() & (bps == 2 ? 0xFFFu : 0xFFu));
                check_plane(P);
                if (s[0] > 68 && pad) continue;
                for (int where = 0; where < 3; ++where) {
                    for (int y = 0; y < P.h; ++y)
                        for (int x = 0; x < P.w; ++x) P.set(x, y, 0);
                    if (where == 1) P.set(0, 0, mx);
                    if (where == 2) P.set(P.w - 1, P.h - 1, mx);
                    check_plane(P);
                }
            }
    // rejections
    {
        uint8_t buf[16 * 32] = {0}, out[16];
        auto call = [&](const void* p, int w, int h, uint64_t st, int bps, int t, uint8_t* o) {
            return p265r_plane_hash_host(p, w, h, st, bps, t, 0, o);
        };
        CHECK(call(buf, 16, 16, 32, 1, 0, out) == P265R_OK);
        CHECK(call(buf, 16, 16, 32, 2, 2, out) == P265R_OK);
        CHECK(call(nullptr, 16, 16, 32, 1, 0, out) == P265R_EINVAL);
        CHECK(call(buf, 16, 16, 32, 1, 0, nullptr) == P265R_EINVAL);
        for (int v : {0, -4, 14, 18, 6}) {
            CHECK(call(buf, v, 16, 32, 1, 0, out) == P265R_EINVAL);
            CHECK(call(buf, 16, v, 32, 1, 0, out) == P265R_EINVAL);
        }
        for (int bps : {0, 3, 4, -1}) CHECK(call(buf, 16, 16, 32, bps, 0, out) == P265R_EINVAL);
        CHECK(call(buf, 16, 16, 15, 1, 0, out) == P265R_EINVAL);
        CHECK(call(buf, 16, 16, 31, 2, 0, out) == P265R_EINVAL);
        for (int t : {-1, 3, 100}) CHECK(call(buf, 16, 16, 32, 1, t, out) == P265R_EINVAL);
        CHECK(call(buf, 32768, 16384, 32768, 1, 0, out) == P265R_EINVAL);       // 2^29 bytes: 8 L + 16 leaves 32 bits
    }
    if (g_fail) {
        std::printf("hash-check: %d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("hash-check ok\n");
    return 0;
}
