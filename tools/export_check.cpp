// export_check.cpp -- `make export-check`: the host-only part of the device-side output (export_host.cpp:
// descriptor validation, layout, slot checks, RGB coefficients) as a stand-alone CPU program under ASan + UBSan.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../p265_amd/csrc/export_host.h"

using namespace p265r;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static p265r_params params_of(int w, int h, int bd) {
    p265r_params p;
    std::memset(&p, 0, sizeof(p));
    p.version = P265R_ABI_VERSION;
    p.pic_width = (uint16_t)w; p.pic_height = (uint16_t)h;
    p.chroma_format_idc = 1;
    p.bit_depth_luma = p.bit_depth_chroma = (uint8_t)bd;
    return p;
}

int main() {
    int layouts = 0;
    for (int bd : {8, 10, 12})
        for (uint32_t fmt = 0; fmt <= P265R_FMT_RGB_PACKED; ++fmt)
            for (uint32_t smp = 0; smp <= P265R_SMP_F32; ++smp)
                for (uint32_t align : {0u, 1u, 2u, 16u, 256u, 4096u}) {
                    const p265r_params p = params_of(72, 40, bd);
                    p265r_export_desc d;
                    std::memset(&d, 0, sizeof(d));
                    d.format = fmt; d.sample = smp;
                    d.crop_left = 2; d.crop_right = 4; d.crop_top = 2; d.crop_bottom = 6;
                    const bool rgb = fmt >= P265R_FMT_RGB_PLANAR;
                    const bool legal = rgb ? smp != P265R_SMP_MSB16
                                           : (smp == P265R_SMP_NATIVE || (smp == P265R_SMP_MSB16 && bd > 8));
                    const int rc = p265r_export_layout(&p, 0, 0, &d, align);
                    CHECK((rc == P265R_OK) == legal);
                    if (rc) continue;
                    ++layouts;
                    ExportShape s;
                    CHECK(export_check_desc(d, bd, &s) == P265R_OK);
                    uint64_t slot = 0;
                    CHECK(export_check_layout(d, s, 72, 40, &slot) == P265R_OK && slot <= d.frame_bytes);
                    CHECK(export_check_layout(d, s, 64, 32, &slot) == P265R_OK);          // a smaller picture of a ragged batch fits
                    CHECK(align > 2 || export_check_layout(d, s, 80, 40, &slot) == P265R_EINVAL);   // a wider one does not (tight pitch)
                    CHECK(export_check_layout(d, s, 6, 40, &slot) == P265R_EINVAL);       // the crop leaves nothing
                    for (int k = 0; k < s.n_planes; ++k) {
                        p265r_export_desc b = d;
                        b.pitch[k] -= (uint64_t)s.es;
                        CHECK(align > 1 || export_check_layout(b, s, 72, 40, nullptr) == P265R_EINVAL);
                        b = d;
                        b.pitch[k] += 1;
                        CHECK(s.es == 1 || export_check_layout(b, s, 72, 40, nullptr) == P265R_EINVAL);
                        if (k) {
                            b = d;
                            b.plane_off[k] = d.plane_off[k - 1];
                            CHECK(export_check_layout(b, s, 72, 40, nullptr) == P265R_EINVAL);
                        }
                    }
                    p265r_export_desc b = d;
                    b.frame_bytes = slot - (uint64_t)s.es;
                    CHECK(export_check_layout(b, s, 72, 40, nullptr) == P265R_EINVAL);
                    b = d;
                    b.pitch[0] = ~0ull;
                    CHECK(export_check_layout(b, s, 72, 40, nullptr) == P265R_EINVAL);
                    int32_t co[8];
                    CHECK((p265r_export_coefficients(&d, bd, co) == P265R_OK) == rgb);
                }
    CHECK(layouts == 3 * 6 * (1 + 1 + 4 + 4) + 2 * 6 * 2);
    // BT.601 limited range at 8 bits: 1.164 / 1.596 / 0.392 / 0.813 / 2.017 at 14 fractional bits
    p265r_export_desc d;
    std::memset(&d, 0, sizeof(d));
    d.format = P265R_FMT_RGB_PACKED; d.sample = P265R_SMP_U8; d.matrix = P265R_MAT_BT601;
    int32_t co[8];
    CHECK(p265r_export_coefficients(&d, 8, co) == P265R_OK);
    const int32_t want[8] = {19077, 26149, 6419, 13320, 33050, 16, 128, 8};
    CHECK(std::memcmp(co, want, sizeof(want)) == 0);
    d.full_range = 1;
    CHECK(p265r_export_coefficients(&d, 12, co) == P265R_OK && co[5] == 0 && co[6] == 2048 && co[7] == 8);
    for (int bd : {7, 13, -1, 1 << 30}) CHECK(p265r_export_coefficients(&d, bd, co) == P265R_EINVAL);
    d.matrix = 3;
    CHECK(p265r_export_coefficients(&d, 8, co) == P265R_EINVAL);
    CHECK(p265r_export_coefficients(nullptr, 8, co) == P265R_EINVAL);
    const p265r_params p = params_of(72, 40, 8);
    CHECK(p265r_export_layout(&p, 0, 0, nullptr, 1) == P265R_EINVAL);
    CHECK(p265r_export_layout(nullptr, 0, 0, &d, 1) == P265R_EINVAL);
    std::printf("export_check: %d layouts, %d failures\n", layouts, g_fail);
    return g_fail ? 1 : 0;
}
