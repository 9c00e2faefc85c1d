// grid_resize_check.cpp -- host sanitizer check of the scaled grid export's host code
// (p265_amd/csrc/grid_resize_host.cpp): every refusal of p265r_grid_resize_plan, the per-frame constants (window,
// pre-turn size, reversal flags, staging index, first tile) for all eight orientations and a ragged list, and the
// tile-width reciprocal against the division at every step.  Stand-alone: `make grid-resize-check` builds it with
// -fsanitize=address,undefined and runs it; no device, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../p265_amd/csrc/grid_resize_host.h"

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

static p265r_grid_frame frame(uint32_t r, uint32_t c, uint32_t w, uint32_t h, uint32_t o = 0, uint32_t cl = 0, uint32_t cr = 0,
                              uint32_t ct = 0, uint32_t cb = 0) {
    p265r_grid_frame f;
    std::memset(&f, 0, sizeof(f));
    f.rows = r; f.cols = c; f.out_width = w; f.out_height = h; f.orientation = o;
    f.crop_left = cl; f.crop_right = cr; f.crop_top = ct; f.crop_bottom = cb;
    return f;
}

static p265r_export_desc desc(uint32_t fmt, uint32_t smp) {
    p265r_export_desc d;
    std::memset(&d, 0, sizeof(d));
    d.format = fmt; d.sample = smp;
    return d;
}

static p265r_resize_desc resize(uint32_t w, uint32_t h, uint32_t filter, uint32_t flags = 0) {
    p265r_resize_desc r;
    std::memset(&r, 0, sizeof(r));
    r.out_width = w; r.out_height = h; r.filter = filter; r.flags = flags;
    for (int c = 0; c < 3; ++c) r.scale[c] = 1.0f;
    return r;
}

static int plan(const p265r_params& p, p265r_export_desc d, p265r_resize_desc rs, const std::vector<p265r_grid_frame>& f,
                std::vector<int32_t>* out = nullptr, int tw = 0, int th = 0) {
    std::vector<int32_t> o(12 * (f.empty() ? 1 : f.size()), -77);
    const int rc = p265r_grid_resize_plan(&p, tw, th, &d, &rs, f.data(), (int)f.size(), o.data());
    if (out) *out = o;
    return rc;
}

int main() {
    static_assert(sizeof(p265r_grid_frame) == 48, "twelve words");
    static_assert(sizeof(GridRsFrame) == 48, "six 64-bit words");
    const p265r_params p8 = params(40, 24, 8, 0), m8 = params(40, 24, 8, 1), p10 = params(40, 24, 10, 0);
    const auto Y = desc(P265R_FMT_PLANAR, P265R_SMP_NATIVE), RGB = desc(P265R_FMT_RGB_PACKED, P265R_SMP_U8);
    const auto NV = desc(P265R_FMT_SEMIPLANAR, P265R_SMP_NATIVE);
    const auto bil = resize(50, 38, P265R_RS_BILINEAR), area = resize(50, 38, P265R_RS_AREA);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42)}) == P265R_OK);
    // what the grid export refuses, per frame: rows / cols / orientation / reserved, the HEIF rule, windows
    CHECK(plan(p8, Y, bil, {frame(0, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 0, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(257, 1, 40, 24 * 257 - 2)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(1, 257, 40 * 257 - 2, 24)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 8)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 0xffffffffu)}) == P265R_EINVAL);
    for (int k = 0; k < 3; ++k) {
        p265r_grid_frame f = frame(2, 3, 100, 42);
        f.reserved[k] = 1;
        CHECK(plan(p8, Y, bil, {f}) == P265R_EINVAL);
        CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42), f}) == P265R_EINVAL);          // the second frame of two
    }
    CHECK(plan(p8, Y, bil, {frame(2, 3, 80, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 82, 42)}) == P265R_OK);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 122, 48)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 24)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 50)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 0xffffffffu, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 0, 50, 50)}) == P265R_EINVAL);      // an empty window
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 0, 0, 0, 42, 0)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 0, 65536, 0)}) == P265R_EINVAL);    // a crop beyond 16 bits
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 0, 0, 0x80000000u)}) == P265R_EINVAL);
    CHECK(plan(p8, RGB, bil, {frame(2, 3, 100, 42, 0, 1, 1)}) == P265R_EINVAL);      // an odd origin, 4:2:0
    CHECK(plan(p8, RGB, bil, {frame(2, 3, 100, 42, 0, 0, 0, 1, 1)}) == P265R_EINVAL);
    // an odd window on a 4:2:0 source: every format; a monochrome source: semi-planar only
    CHECK(plan(p8, Y, bil, {frame(2, 3, 101, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, NV, bil, {frame(2, 3, 100, 43)}) == P265R_EINVAL);
    CHECK(plan(p8, RGB, bil, {frame(2, 3, 101, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, RGB, bil, {frame(2, 3, 100, 42, 0, 0, 1)}) == P265R_EINVAL);
    CHECK(plan(m8, Y, resize(51, 37, P265R_RS_AREA), {frame(2, 3, 101, 43, 2, 1, 0, 1, 0)}) == P265R_OK);
    CHECK(plan(m8, RGB, resize(51, 37, P265R_RS_AREA), {frame(2, 3, 101, 43)}) == P265R_OK);
    CHECK(plan(m8, NV, bil, {frame(2, 3, 101, 43)}) == P265R_EINVAL);
    // desc: its crop must be 0; what the plain export refuses
    for (int k = 0; k < 4; ++k) {
        p265r_export_desc d = Y;
        (k == 0 ? d.crop_left : k == 1 ? d.crop_right : k == 2 ? d.crop_top : d.crop_bottom) = 2;
        CHECK(plan(p8, d, bil, {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    }
    CHECK(plan(p8, desc(4, 0), bil, {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, desc(P265R_FMT_PLANAR, P265R_SMP_F16), bil, {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, desc(P265R_FMT_SEMIPLANAR, P265R_SMP_MSB16), bil, {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p10, desc(P265R_FMT_SEMIPLANAR, P265R_SMP_MSB16), bil, {frame(2, 3, 100, 42)}) == P265R_OK);
    // what the scaled export refuses: filter, flags, sizes, NORM, the window against the filter -- at the pre-turn size
    CHECK(plan(p8, Y, resize(50, 38, 3), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, resize(50, 38, P265R_RS_BILINEAR, 2), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, resize(0, 38, P265R_RS_BILINEAR), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, resize(50, 16386, P265R_RS_BILINEAR), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, Y, resize(51, 38, P265R_RS_BILINEAR), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, RGB, resize(51, 37, P265R_RS_BILINEAR), {frame(2, 3, 100, 42)}) == P265R_OK);
    CHECK(plan(p8, RGB, resize(50, 38, P265R_RS_BILINEAR, P265R_RS_NORM), {frame(2, 3, 100, 42)}) == P265R_EINVAL);
    CHECK(plan(p8, desc(P265R_FMT_RGB_PLANAR, P265R_SMP_F16), resize(50, 38, P265R_RS_AREA, P265R_RS_NORM), {frame(2, 3, 100, 42)}) == P265R_OK);
    CHECK(plan(p8, Y, area, {frame(2, 3, 100, 42)}) == P265R_OK);                    // 50 x 38 out of 100 x 42
    CHECK(plan(p8, Y, area, {frame(2, 3, 100, 42, 1)}) == P265R_EINVAL);             // turned: 38 x 50 out of 100 x 42
    CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42, 1)}) == P265R_OK);
    CHECK(plan(p8, Y, area, {frame(2, 3, 100, 42, 0, 0, 52)}) == P265R_EINVAL);      // 48 wide
    CHECK(plan(p8, Y, area, {frame(2, 3, 100, 42), frame(1, 1, 40, 24)}) == P265R_EINVAL);
    {
        const p265r_params t512 = params(512, 512, 8, 0);
        // windows above 8192 (area) and above 32767 (every filter)
        CHECK(plan(t512, Y, resize(64, 64, P265R_RS_AREA), {frame(16, 16, 8192, 8192)}) == P265R_OK);
        CHECK(plan(t512, Y, resize(64, 64, P265R_RS_AREA), {frame(16, 17, 8194, 8192)}) == P265R_EINVAL);
        CHECK(plan(t512, Y, resize(64, 64, P265R_RS_BILINEAR), {frame(16, 64, 32766, 8192)}) == P265R_OK);
        CHECK(plan(t512, Y, resize(64, 64, P265R_RS_BILINEAR), {frame(16, 64, 32768, 8192)}) == P265R_EINVAL);
        // tiles above 65535 in all
        const p265r_params t8 = params(8, 8, 8, 0);
        std::vector<p265r_grid_frame> many(2, frame(256, 128, 1024, 2048));
        CHECK(plan(t8, Y, resize(64, 64, P265R_RS_NEAREST), {many[0]}) == P265R_OK);
        CHECK(plan(t8, Y, resize(64, 64, P265R_RS_NEAREST), many) == P265R_EINVAL);
    }
    // arguments
    {
        p265r_params bad = p8;
        bad.version = 1;
        CHECK(plan(bad, Y, bil, {frame(2, 3, 100, 42)}) == P265R_EINVAL);
        p265r_params split = p10;
        split.split_bit_depth = 1; split.bit_depth_chroma = 8;
        CHECK(plan(split, Y, bil, {frame(2, 3, 100, 42)}) == P265R_EUNSUPPORTED);
        CHECK(plan(p8, Y, bil, {}) == P265R_EINVAL);
        CHECK(plan(p8, Y, bil, {frame(2, 3, 100, 42)}, nullptr, 41, 24) == P265R_EINVAL);   // an odd tile
        p265r_grid_frame f = frame(2, 3, 100, 42);
        p265r_export_desc d = Y;
        p265r_resize_desc r = bil;
        int32_t o[12];
        CHECK(p265r_grid_resize_plan(nullptr, 0, 0, &d, &r, &f, 1, o) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, nullptr, &r, &f, 1, o) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, &d, nullptr, &f, 1, o) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, &d, &r, nullptr, 1, o) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, &d, &r, &f, 1, nullptr) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, &d, &r, &f, 0, o) == P265R_EINVAL);
        CHECK(p265r_grid_resize_plan(&p8, 0, 0, &d, &r, &f, 65536, o) == P265R_EINVAL);
    }
    // the constants: rot90(R, k) then the mirror as reversals of R followed (k odd) by a plain transpose
    static const int want[8][3] = {{0, 0, 0}, {1, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 1, 1}, {0, 1, 0}, {0, 0, 1}};
    {
        std::vector<p265r_grid_frame> f;
        for (uint32_t o = 0; o < 8; ++o) f.push_back(frame(2, 3, 101 - (o & 1), 43 - (o & 1), o, 2, 3 - (o & 1), 4, 1 - (o & 1)));
        std::vector<int32_t> out;
        CHECK(plan(p8, RGB, resize(50, 38, P265R_RS_BILINEAR), f, &out) == P265R_OK);
        int stage = 0;
        for (int o = 0; o < 8; ++o) {
            const int32_t* v = out.data() + 12 * o;
            CHECK(v[0] == 6 * o && v[1] == 3 && v[2] == 2 && v[3] == 4 && v[4] == 96 && v[5] == 38);
            CHECK(v[6] == (o & 1 ? 38 : 50) && v[7] == (o & 1 ? 50 : 38));
            CHECK(v[8] == want[o][0] && v[9] == want[o][1] && v[10] == want[o][2]);
            CHECK(v[11] == (o & 1 ? stage : -1));
            stage += o & 1;
        }
    }
    {
        // a ragged list: first tiles are the running sum of rows * cols
        std::vector<int32_t> out;
        CHECK(plan(p8, RGB, resize(20, 12, P265R_RS_AREA), {frame(1, 1, 36, 20, 0, 2, 4, 0, 2), frame(2, 3, 100, 42, 1),
                                                            frame(3, 2, 80, 70, 6, 4, 2, 6, 4), frame(1, 1, 40, 24, 5)}, &out) == P265R_OK);
        CHECK(out[0] == 0 && out[12] == 1 && out[24] == 7 && out[36] == 13);
        CHECK(out[1] == 1 && out[13] == 3 && out[25] == 2);
        CHECK(out[4] == 30 && out[5] == 18 && out[24 + 2] == 4 && out[24 + 3] == 6 && out[24 + 4] == 74 && out[24 + 5] == 60);
        CHECK(out[11] == -1 && out[23] == 0 && out[35] == -1 && out[47] == 1);
    }
    // the reciprocal: equal to the division on both sides of every step, for every divisor
    for (uint32_t d = 1; d < 65536; ++d) {
        const uint32_t rcp = grid_rs_rcp(d);
        for (uint32_t k = 0; k * d < 65536; ++k) {
            const uint32_t x = k * d;
            if (grid_rs_div(x, d, rcp) != k) { CHECK(!"reciprocal at a step"); break; }
            if (x && grid_rs_div(x - 1, d, rcp) != k - 1) { CHECK(!"reciprocal below a step"); break; }
        }
        if (grid_rs_div(65535, d, rcp) != 65535 / d) CHECK(!"reciprocal at 65535");
    }
    if (fails) { std::printf("grid_resize_check: %d failure(s)\n", fails); return 1; }
    std::printf("grid_resize_check ok\n");
    return 0;
}
