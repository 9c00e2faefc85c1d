// grid_check.cpp -- host sanitizer check of the grid export's host code (p265_amd/csrc/grid_host.cpp): every refusal
// of p265r_grid_layout, the window and the orientation's reversal flags, and the layout arithmetic at the size
// extremes (256 x 256 tiles, 16384-wide canvases, offsets in 64 bits).  Stand-alone: `make grid-check` builds it with
// -fsanitize=address,undefined and runs it; no device, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../p265_amd/csrc/grid_host.h"

using namespace p265r;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static p265r_params params(int w, int h, int bd, int mono) {
    p265r_params p;
    std::memset(&p, 0, sizeof(p));
    p.version = P265R_ABI_VERSION;
    p.pic_width = (uint16_t)w; p.pic_height = (uint16_t)h;
    p.chroma_format_idc = mono ? 0 : 1;
    p.bit_depth_luma = p.bit_depth_chroma = (uint8_t)bd;
    p.ctb_log2_size = 4; p.min_tb_log2_size = 2; p.max_tb_log2_size = 4;
    return p;
}

static p265r_grid_desc grid(uint32_t r, uint32_t c, uint32_t w, uint32_t h, uint32_t o) {
    p265r_grid_desc g;
    std::memset(&g, 0, sizeof(g));
    g.rows = r; g.cols = c; g.out_width = w; g.out_height = h; g.orientation = o;
    return g;
}

static p265r_export_desc desc(uint32_t fmt, uint32_t smp, int l = 0, int r = 0, int t = 0, int b = 0) {
    p265r_export_desc d;
    std::memset(&d, 0, sizeof(d));
    d.format = fmt; d.sample = smp;
    d.crop_left = (uint16_t)l; d.crop_right = (uint16_t)r; d.crop_top = (uint16_t)t; d.crop_bottom = (uint16_t)b;
    return d;
}

static int layout(const p265r_params& p, p265r_grid_desc g, p265r_export_desc d, uint32_t align = 1, p265r_export_desc* out = nullptr) {
    const int rc = p265r_grid_layout(&p, 0, 0, &g, &d, align);
    if (out) *out = d;
    return rc;
}

int main() {
    const p265r_params p8 = params(40, 24, 8, 0), m8 = params(40, 24, 8, 1), p10 = params(40, 24, 10, 0);
    const auto Y = desc(P265R_FMT_PLANAR, P265R_SMP_NATIVE);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), Y) == P265R_OK);
    // rows / cols / orientation / reserved
    CHECK(layout(p8, grid(0, 3, 100, 42, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 0, 100, 42, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(257, 1, 40, 24 * 257 - 2, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(1, 257, 40 * 257 - 2, 24, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 8), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0xffffffffu), Y) == P265R_EINVAL);
    for (int k = 0; k < 3; ++k) {
        p265r_grid_desc g = grid(2, 3, 100, 42, 0);
        g.reserved[k] = 1;
        CHECK(layout(p8, g, Y) == P265R_EINVAL);
    }
    // the HEIF rule
    CHECK(layout(p8, grid(2, 3, 80, 42, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 82, 42, 0), Y) == P265R_OK);
    CHECK(layout(p8, grid(2, 3, 120, 48, 0), Y) == P265R_OK);
    CHECK(layout(p8, grid(2, 3, 122, 48, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 24, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 50, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 0xffffffffu, 42, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 0, 0, 0), Y) == P265R_EINVAL);
    // windows: empty, odd sizes, odd origins
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_PLANAR, P265R_SMP_NATIVE, 50, 50)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_PLANAR, P265R_SMP_NATIVE, 0, 0, 42, 0)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_PLANAR, P265R_SMP_NATIVE, 65535, 65535)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 101, 42, 0), Y) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 43, 0), desc(P265R_FMT_SEMIPLANAR, P265R_SMP_NATIVE)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 101, 43, 0), desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8)) == P265R_OK);
    CHECK(layout(m8, grid(2, 3, 101, 43, 0), Y) == P265R_OK);
    CHECK(layout(m8, grid(2, 3, 101, 43, 0), desc(P265R_FMT_SEMIPLANAR, P265R_SMP_NATIVE)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8, 1, 1)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8, 0, 0, 1, 1)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8, 0, 3, 0, 1)) == P265R_OK);
    CHECK(layout(m8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8, 1, 0, 1, 0)) == P265R_OK);
    // what the plain export refuses
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(4, 0)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_PLANAR, P265R_SMP_F16)) == P265R_EINVAL);
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), desc(P265R_FMT_SEMIPLANAR, P265R_SMP_MSB16)) == P265R_EINVAL);
    CHECK(layout(p10, grid(2, 3, 100, 42, 0), desc(P265R_FMT_SEMIPLANAR, P265R_SMP_MSB16)) == P265R_OK);
    CHECK(layout(p10, grid(2, 3, 102, 42, 0), Y, 5) == P265R_EINVAL);          // pitch 205: no multiple of 2
    CHECK(layout(p8, grid(2, 3, 100, 42, 0), Y, (1u << 20) + 1) == P265R_EINVAL);
    {
        p265r_params bad = p8;
        bad.version = 1;
        CHECK(layout(bad, grid(2, 3, 100, 42, 0), Y) == P265R_EINVAL);
        p265r_params split = p10;
        split.split_bit_depth = 1; split.bit_depth_chroma = 8;
        CHECK(layout(split, grid(2, 3, 100, 42, 0), Y) == P265R_EUNSUPPORTED);
        p265r_grid_desc g = grid(2, 3, 100, 42, 0);
        p265r_export_desc d = Y;
        CHECK(p265r_grid_layout(nullptr, 0, 0, &g, &d, 1) == P265R_EINVAL);
        CHECK(p265r_grid_layout(&p8, 0, 0, nullptr, &d, 1) == P265R_EINVAL);
        CHECK(p265r_grid_layout(&p8, 0, 0, &g, nullptr, 1) == P265R_EINVAL);
        CHECK(p265r_grid_layout(&p8, 41, 24, &g, &d, 1) == P265R_EINVAL);       // an odd tile
        CHECK(p265r_grid_layout(&p8, 70000, 24, &g, &d, 1) == P265R_EINVAL);
        CHECK(p265r_grid_layout(&p8, -8, 24, &g, &d, 1) == P265R_EINVAL);
    }
    // the orientation as reversals + transpose, the oriented size, for all eight
    static const int want[8][3] = {{0, 0, 0}, {1, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 1, 1}, {0, 1, 0}, {0, 0, 1}};
    for (uint32_t o = 0; o < 8; ++o) {
        GridShape s;
        CHECK(grid_check(desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8, 2, 3, 4, 1), grid(2, 3, 101, 43, o), 8, false, 40, 24, &s) == P265R_OK);
        CHECK(s.W == 96 && s.H == 38 && s.wl == 2 && s.wt == 4 && s.cw == 120 && s.ch == 48);
        CHECK(s.fx == want[o][0] && s.fy == want[o][1] && s.transpose == want[o][2]);
        CHECK(s.dw == (o & 1 ? 38 : 96) && s.dh == (o & 1 ? 96 : 38));
    }
    // size extremes: 256 x 256 tiles; a 16384-wide canvas; a canvas above 65535; offsets beyond 32 bits
    p265r_export_desc d;
    const p265r_params t8 = params(8, 8, 8, 0), t256 = params(256, 256, 10, 0), t512 = params(512, 512, 8, 0);
    CHECK(layout(t8, grid(256, 256, 2048, 2048, 3), desc(P265R_FMT_RGB_PLANAR, P265R_SMP_F32), 1, &d) == P265R_OK);
    CHECK(d.frame_bytes == 3ull * 4 * 2048 * 2048 && d.pitch[0] == 4ull * 2048);
    CHECK(layout(t256, grid(64, 64, 16384, 16384, 1), desc(P265R_FMT_RGB_PLANAR, P265R_SMP_F32), 1u << 20, &d) == P265R_OK);
    CHECK(d.pitch[0] == (1ull << 20) && d.plane_off[2] == 2ull * 16384 * (1ull << 20) && d.frame_bytes == 3ull * 16384 * (1ull << 20));
    CHECK(d.frame_bytes > 0xffffffffull);
    CHECK(layout(t256, grid(64, 64, 16383, 16129, 5), desc(P265R_FMT_RGB_PACKED, P265R_SMP_F32), 1, &d) == P265R_OK);
    CHECK(d.pitch[0] == 12ull * 16129 && d.frame_bytes == 12ull * 16129 * 16383);
    CHECK(layout(t512, grid(2, 127, 65000, 600, 0), Y) == P265R_OK);
    CHECK(layout(t512, grid(2, 128, 65500, 600, 0), Y) == P265R_EINVAL);         // canvas 65536 wide
    CHECK(layout(t512, grid(256, 256, 100000, 100000, 0), Y) == P265R_EINVAL);
    // a layout the caller bent: overlap, short pitch, short slot
    {
        GridShape s;
        p265r_export_desc c = Y;
        CHECK(grid_check(c, grid(2, 3, 100, 42, 1), 8, false, 40, 24, &s) == P265R_OK);
        grid_fill_layout(&c, s.e, s.dw, s.dh, 1);
        uint64_t sb = 0;
        CHECK(grid_check_layout(c, s.e, s.dw, s.dh, &sb) == P265R_OK && sb == 42ull * 100 * 3 / 2 && c.pitch[0] == 42);
        p265r_export_desc b = c; b.pitch[0] = 41;
        CHECK(grid_check_layout(b, s.e, s.dw, s.dh, nullptr) == P265R_EINVAL);
        b = c; b.plane_off[1] -= 1;
        CHECK(grid_check_layout(b, s.e, s.dw, s.dh, nullptr) == P265R_EINVAL);
        b = c; b.frame_bytes -= 1;
        CHECK(grid_check_layout(b, s.e, s.dw, s.dh, nullptr) == P265R_EINVAL);
        b = c; b.pitch[2] = 1ull << 46;
        CHECK(grid_check_layout(b, s.e, s.dw, s.dh, nullptr) == P265R_EINVAL);
    }
    if (fails) { std::printf("grid_check: %d failure(s)\n", fails); return 1; }
    std::printf("grid_check ok\n");
    return 0;
}
