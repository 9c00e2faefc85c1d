// resize_check.cpp -- stand-alone host check of the scaled device-side output's host code (make resize-check:
// g++ -fsanitize=address,undefined).  resize_plane_host (the arithmetic of resize_math.h, which the kernels share)
// against a brute-force restatement with 64-bit arithmetic and plain division over random and extreme planes; the
// reciprocal division against floor division; malformed descriptors.  Exits 0 when everything agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../p265_amd/csrc/resize_host.h"

using namespace p265r;

static int g_fail = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// ---- brute force, from the words of include/p265r.h ----------------------------------------------------------
static int64_t brute_h(int i, int cg, int vertical) { return cg ? 4 * (int64_t)i + (vertical ? 2 : 1) : 2 * (int64_t)i + 1; }
static int64_t brute_u(int n, int m, int64_t h) { return (h * (((int64_t)n << 16) / m)) >> 1; }
static int64_t fl_shift(int64_t v, int s) { return v >= 0 ? v >> s : -((-v + (1ll << s) - 1) >> s); }   // floor(v / 2^s)

static void brute(const std::vector<uint16_t>& src, int stride, int nw, int nh, int cp, int cg, uint32_t f, int mw, int mh,
                  std::vector<int32_t>& out) {
    const int ow = cg ? mw / 2 : mw, oh = cg ? mh / 2 : mh;
    const int pw = cp ? nw / 2 : nw, ph = cp ? nh / 2 : nh;
    out.assign((size_t)ow * oh, 0);
    auto at = [&](int64_t y, int64_t x) { return (int64_t)src[(size_t)y * stride + (size_t)x]; };
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            const int64_t ux = brute_u(nw, mw, brute_h(x, cg, 0)), uy = brute_u(nh, mh, brute_h(y, cg, 1));
            int64_t v;
            if (f == P265R_RS_NEAREST) {
                int64_t ix = ux >> 16, iy = uy >> 16;
                if (cp) { ix >>= 1; iy >>= 1; }
                v = at(iy < ph - 1 ? iy : ph - 1, ix < pw - 1 ? ix : pw - 1);
            } else if (f == P265R_RS_BILINEAR) {
                int64_t px = cp ? fl_shift(ux - 32768, 1) : ux - 32768, py = cp ? fl_shift(uy - 65536, 1) : uy - 32768;
                const int64_t tx = ((int64_t)pw - 1) << 16, ty = ((int64_t)ph - 1) << 16;
                px = px < 0 ? 0 : (px > tx ? tx : px);
                py = py < 0 ? 0 : (py > ty ? ty : py);
                const int64_t x0 = px >> 16, y0 = py >> 16, x1 = x0 + 1 < pw ? x0 + 1 : pw - 1, y1 = y0 + 1 < ph ? y0 + 1 : ph - 1;
                const int64_t fx = (px >> 8) & 255, fy = (py >> 8) & 255;
                v = (((256 - fx) * at(y0, x0) + fx * at(y0, x1)) * (256 - fy) + ((256 - fx) * at(y1, x0) + fx * at(y1, x1)) * fy +
                     32768) >> 16;
            } else {
                // every sample of the plane against the output's interval
                const int64_t Nx = cg ? nw / 2 : nw, Ny = cg ? nh / 2 : nh;
                const int64_t Mx = cg ? mw / 2 : (cp ? 2 * mw : mw), My = cg ? mh / 2 : (cp ? 2 * mh : mh);
                unsigned __int128 sum = 0;
                int64_t wsum_x = 0;
                for (int ky = 0; ky < ph; ++ky) {
                    const int64_t lo = std::max<int64_t>(ky * My, y * Ny), hi = std::min<int64_t>((ky + 1) * My, (y + 1) * Ny);
                    if (hi <= lo) continue;
                    for (int kx = 0; kx < pw; ++kx) {
                        const int64_t l2 = std::max<int64_t>(kx * Mx, x * Nx), h2 = std::min<int64_t>((kx + 1) * Mx, (x + 1) * Nx);
                        if (h2 <= l2) continue;
                        sum += (unsigned __int128)((hi - lo) * (h2 - l2)) * (uint64_t)at(ky, kx);
                        if (ky == (int)(y * Ny / My)) wsum_x += h2 - l2;
                    }
                }
                CHECK(wsum_x == Nx);
                v = (int64_t)((sum + (uint64_t)((Nx * Ny) >> 1)) / (uint64_t)(Nx * Ny));
            }
            out[(size_t)y * ow + x] = (int32_t)v;
        }
}

static void compare(int nw, int nh, int mw, int mh, int mode, int top) {
    // mode: 0 random, 1 all zero, 2 all max, 3 checkerboard, 4 2 x 2 checkerboard
    const int stride = nw + 5;
    std::vector<uint16_t> src((size_t)stride * nh);
    for (int y = 0; y < nh; ++y)
        for (int x = 0; x < stride; ++x) {
            uint16_t v;
            switch (mode) {
                case 1: v = 0; break;
                case 2: v = (uint16_t)top; break;
                case 3: v = (x + y) & 1 ? (uint16_t)top : 0; break;
                case 4: v = ((x >> 1) + (y >> 1)) & 1 ? (uint16_t)top : 0; break;
                default: v = (uint16_t)(rnd() % (uint32_t)(top + 1)); break;
            }
            src[(size_t)y * stride + x] = v;
        }
    for (uint32_t f = 0; f <= P265R_RS_AREA; ++f) {
        if (f == P265R_RS_AREA && (mw > nw || mh > nh)) continue;
        for (int kind = 0; kind < 3; ++kind) {          // luma on luma grid, chroma on luma grid, chroma on chroma grid
            const int cp = kind > 0, cg = kind == 2;
            if (cp && ((nw | nh) & 1)) continue;
            if (cg && ((mw | mh) & 1)) continue;
            const int ow = cg ? mw / 2 : mw, oh = cg ? mh / 2 : mh;
            std::vector<int32_t> got((size_t)ow * oh, -1), want;
            const int rc = resize_plane_host(src.data(), (uint64_t)stride, nw, nh, cp, cg, f, mw, mh, got.data());
            CHECK(rc == P265R_OK);
            brute(src, stride, nw, nh, cp, cg, f, mw, mh, want);
            const bool same = got == want;
            if (!same) std::printf("  %dx%d -> %dx%d filter %u kind %d mode %d\n", nw, nh, mw, mh, f, kind, mode);
            CHECK(same);
            for (int32_t v : got) CHECK(v >= 0 && v <= top);
        }
    }
}

static void check_division() {
    // exhaustive in the numerator for small divisors; around every quotient boundary for the rest of the range
    const uint32_t small[][2] = {{1, 1}, {1, 2}, {1, 3}, {2, 2}, {3, 5}, {7, 9}, {16, 16}, {17, 31}, {40, 25}};
    for (const auto& p : small) {
        const RsDiv d = rs_div_make(p[0], p[1]);
        const uint64_t dd = (uint64_t)p[0] * p[1];
        for (uint64_t sum = 0; sum <= 4095 * dd; ++sum)
            if (rs_div(d, sum) != (sum + (dd >> 1)) / dd) { CHECK(!"division (small)"); break; }
    }
    const uint32_t big[][2] = {{8192, 8192}, {8191, 8192}, {8191, 8191}, {8192, 4097}, {1920, 1080}, {1916, 1078}, {6143, 8189},
                               {4096, 4096}, {5793, 5793}, {8192, 1}, {1, 8191}, {4099, 8179}};
    for (const auto& p : big) {
        const RsDiv d = rs_div_make(p[0], p[1]);
        const uint64_t dd = (uint64_t)p[0] * p[1];
        bool ok = true;
        for (uint64_t q = 0; q <= 4096 && ok; ++q)
            for (int e = -2; e <= 2 && ok; ++e) {
                const int64_t x = (int64_t)(q * dd) + e;                 // x = sum + (d >> 1) crosses q d here
                if (x < (int64_t)(dd >> 1) || (uint64_t)x - (dd >> 1) > 4095 * dd) continue;
                const uint64_t sum = (uint64_t)x - (dd >> 1);
                ok = rs_div(d, sum) == (sum + (dd >> 1)) / dd;
            }
        for (int k = 0; k < 200000 && ok; ++k) {
            const uint64_t sum = (((uint64_t)rnd() << 32) | rnd()) % (4095 * dd + 1);
            ok = rs_div(d, sum) == (sum + (dd >> 1)) / dd;
        }
        CHECK(ok);
    }
}

static void check_f16() {
    // every fp16 value and the midpoints between neighbours round as specified (nearest, ties to even)
    const float cases[][2] = {{0.0f, 0}, {1.0f, 0x3c00}, {65504.0f, 0x7bff}, {65519.99f, 0x7bff}, {65520.0f, 0x7c00},
                              {5.9604645e-8f, 0x0001}, {2.9802322e-8f, 0x0000}, {2.9802326e-8f, 0x0001}, {-2.0f, 0xc000},
                              {1.00048828125f, 0x3c00}, {1.00146484375f, 0x3c02}, {6.1035156e-5f, 0x0400}, {6.0975552e-5f, 0x03ff}};
    for (const auto& c : cases) {
        const uint16_t got = resize_f16_bits(c[0]);
        if (got != (uint16_t)c[1]) std::printf("  f16(%.9g) = %04x, want %04x\n", c[0], got, (unsigned)c[1]);
        CHECK(got == (uint16_t)c[1]);
    }
}

static void check_malformed() {
    p265r_params prm{};
    prm.version = P265R_ABI_VERSION; prm.pic_width = 72; prm.pic_height = 40; prm.chroma_format_idc = 1;
    prm.bit_depth_luma = prm.bit_depth_chroma = 8; prm.ctb_log2_size = 4; prm.min_tb_log2_size = 2; prm.max_tb_log2_size = 4;
    p265r_export_desc d{};
    d.format = P265R_FMT_RGB_PLANAR; d.sample = P265R_SMP_F32;
    p265r_resize_desc rs{};
    rs.out_width = 31; rs.out_height = 17; rs.filter = P265R_RS_BILINEAR;
    CHECK(p265r_resize_layout(&prm, &d, &rs, 1) == P265R_OK);
    CHECK(d.pitch[0] == 31 * 4 && d.plane_off[2] == 2 * 31 * 4 * 17 && d.frame_bytes == 3 * 31 * 4 * 17);
    CHECK(p265r_resize_layout(&prm, &d, &rs, 256) == P265R_OK);
    CHECK(d.pitch[1] == 256 && d.plane_off[1] == 256 * 17 && d.frame_bytes == 3 * 256 * 17);
    CHECK(p265r_resize_layout(nullptr, &d, &rs, 1) == P265R_EINVAL);
    CHECK(p265r_resize_layout(&prm, nullptr, &rs, 1) == P265R_EINVAL);
    CHECK(p265r_resize_layout(&prm, &d, nullptr, 1) == P265R_EINVAL);
    CHECK(p265r_resize_layout(&prm, &d, &rs, 3) == P265R_EINVAL);           // no multiple of the element
    auto bad = [&](p265r_export_desc dd, p265r_resize_desc r) { return p265r_resize_layout(&prm, &dd, &r, 1); };
    p265r_resize_desc r = rs;
    r.filter = 3; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.flags = 2; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.out_width = 0; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.out_height = 0; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.out_width = 16385; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.out_height = 0xffffffffu; CHECK(bad(d, r) == P265R_EINVAL);
    r = rs; r.out_width = r.out_height = 16384; CHECK(bad(d, r) == P265R_OK);
    r = rs; r.flags = P265R_RS_NORM; r.scale[0] = r.scale[1] = r.scale[2] = 1.0f; CHECK(bad(d, r) == P265R_OK);
    r.scale[1] = std::numeric_limits<float>::infinity(); CHECK(bad(d, r) == P265R_EINVAL);
    r.scale[1] = 1.0f; r.bias[2] = std::nanf(""); CHECK(bad(d, r) == P265R_EINVAL);
    r.bias[2] = 0.0f;
    p265r_export_desc dd = d;
    dd.sample = P265R_SMP_U8; CHECK(bad(dd, r) == P265R_EINVAL);            // NORM on an integer sample
    dd.sample = P265R_SMP_NATIVE; CHECK(bad(dd, r) == P265R_EINVAL);
    dd = d; dd.upsample = 77; CHECK(bad(dd, rs) == P265R_OK);               // ignored
    dd = d; dd.format = P265R_FMT_PLANAR; dd.sample = P265R_SMP_NATIVE;
    CHECK(bad(dd, rs) == P265R_EINVAL);                                     // odd size, half-size chroma
    r = rs; r.out_width = 32; CHECK(bad(dd, r) == P265R_EINVAL);
    r.out_height = 18; CHECK(bad(dd, r) == P265R_OK);
    dd.format = P265R_FMT_SEMIPLANAR; CHECK(bad(dd, rs) == P265R_EINVAL);
    dd.crop_left = 1; CHECK(bad(dd, r) == P265R_EINVAL);
    // a monochrome source: planar and RGB take odd sizes, semi-planar does not
    prm.chroma_format_idc = 0;
    dd = d; dd.format = P265R_FMT_PLANAR; dd.sample = P265R_SMP_NATIVE;
    CHECK(bad(dd, rs) == P265R_OK);
    CHECK(bad(d, rs) == P265R_OK);
    dd.format = P265R_FMT_SEMIPLANAR; CHECK(bad(dd, rs) == P265R_EINVAL);
    prm.chroma_format_idc = 1;
    // windows
    r = rs; r.filter = P265R_RS_AREA;
    CHECK(resize_check_window(r, 72, 40) == P265R_OK);
    CHECK(resize_check_window(r, 30, 40) == P265R_EINVAL && resize_check_window(r, 72, 16) == P265R_EINVAL);
    CHECK(resize_check_window(r, 31, 17) == P265R_OK && resize_check_window(r, 8193, 40) == P265R_EINVAL);
    CHECK(resize_check_window(rs, 0, 40) == P265R_EINVAL && resize_check_window(rs, 2, 2) == P265R_OK);
    CHECK(resize_check_window(rs, 32768, 40) == P265R_EINVAL && resize_check_window(rs, 32767, 40) == P265R_OK);
    // positions
    int32_t i0, i1, fr;
    CHECK(p265r_resize_position(P265R_RS_BILINEAR, 8, 8, 1, 0, 0, &i0, &i1, &fr) == P265R_OK && i0 == 0 && i1 == 1 && fr == 0);
    CHECK(p265r_resize_position(P265R_RS_AREA, 8, 8, 1, 0, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 0, 8, 1, 0, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 8, 0, 1, 0, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 8, 8, 17, 0, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 8, 8, -1, 0, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 7, 8, 1, 1, 0, &i0, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 8, 8, 1, 0, 0, nullptr, &i1, &fr) == P265R_EINVAL);
    CHECK(p265r_resize_position(P265R_RS_NEAREST, 32767, 16384, 32768, 0, 1, &i0, &i1, &fr) == P265R_OK && i0 == 32766);
    // the reference's own refusals
    uint16_t s4[4] = {1, 2, 3, 4};
    int32_t o4[16];
    CHECK(resize_plane_host(nullptr, 2, 2, 2, 0, 0, 0, 2, 2, o4) == P265R_EINVAL);
    CHECK(resize_plane_host(s4, 1, 2, 2, 0, 0, 0, 2, 2, o4) == P265R_EINVAL);          // stride below the row
    CHECK(resize_plane_host(s4, 2, 2, 2, 0, 1, 0, 2, 2, o4) == P265R_EINVAL);          // a luma plane on the chroma grid
    CHECK(resize_plane_host(s4, 2, 2, 2, 0, 0, P265R_RS_AREA, 3, 2, o4) == P265R_EINVAL);
    CHECK(resize_plane_host(s4, 2, 2, 2, 0, 0, 3, 2, 2, o4) == P265R_EINVAL);
    CHECK(resize_plane_host(s4, 2, 2, 2, 0, 0, P265R_RS_AREA, 1, 1, o4) == P265R_OK && o4[0] == 3);   // (1+2+3+4+2) >> 2
    float nb[2] = {0.5f, 1.0f}, f32[4];
    uint16_t f16[4];
    CHECK(p265r_resize_plane_host(s4, 2, 2, 2, 0, 0, 0, 2, 2, o4, nb, f32, f16) == P265R_OK && f32[3] == 3.0f && f16[3] == 0x4200);
    CHECK(p265r_resize_plane_host(s4, 2, 2, 2, 0, 0, 0, 2, 2, o4, nullptr, f32, nullptr) == P265R_EINVAL);
}

int main() {
    const int tops[] = {255, 1023, 4095};
    const int shapes[][4] = {{2, 2, 1, 1}, {2, 2, 2, 2}, {2, 2, 4, 4}, {8, 6, 4, 3}, {8, 6, 3, 5}, {24, 10, 7, 4}, {24, 10, 24, 10},
                             {24, 10, 23, 9}, {24, 10, 25, 11}, {24, 10, 48, 20}, {72, 40, 34, 18}, {72, 40, 31, 17}, {72, 40, 100, 56},
                             {72, 40, 36, 20}, {66, 26, 2, 2}, {66, 26, 1, 1}, {130, 8, 2, 2}, {7, 5, 3, 2}, {9, 9, 9, 9}, {40, 8, 16, 8}};
    for (const auto& s : shapes)
        for (int mode = 0; mode < 5; ++mode) compare(s[0], s[1], s[2], s[3], mode, tops[(s[0] + mode) % 3]);
    compare(1032, 8, 16, 8, 0, 4095);
    compare(1032, 8, 520, 8, 3, 255);
    compare(8192, 2, 1, 1, 2, 4095);        // the largest box of one axis, all max
    compare(2, 8192, 1, 1, 2, 4095);
    check_division();
    check_f16();
    check_malformed();
    if (g_fail) {
        std::printf("resize_check: %d FAILED\n", g_fail);
        return 1;
    }
    std::printf("resize_check: ok\n");
    return 0;
}
