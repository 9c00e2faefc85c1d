// export_host.cpp -- see export_host.h.
#include "export_host.h"

#include <algorithm>
#include <cmath>

namespace p265r {

int export_check_desc(const p265r_export_desc& d, int bit_depth, ExportShape* s, bool mono) {
    if (bit_depth < 8 || bit_depth > 12) return P265R_EINVAL;
    if (d.format > P265R_FMT_RGB_PACKED || d.sample > P265R_SMP_F32) return P265R_EINVAL;
    const bool rgb = d.format >= P265R_FMT_RGB_PLANAR;
    if (rgb) {
        if (d.matrix > P265R_MAT_BT2020 || d.full_range > 1 || d.upsample > P265R_UP_BILINEAR) return P265R_EINVAL;
        if (d.sample == P265R_SMP_MSB16) return P265R_EINVAL;
    } else {
        if (d.sample != P265R_SMP_NATIVE && d.sample != P265R_SMP_MSB16) return P265R_EINVAL;
        if (d.sample == P265R_SMP_MSB16 && bit_depth == 8) return P265R_EINVAL;
    }
    // crops in whole chroma samples: 4:2:0 sources, and the 2 x 2-subsampled CbCr plane semi-planar always has
    // (monochrome: SubWidthC = SubHeightC = 1, any crop, for the formats without one)
    if (!(mono && d.format != P265R_FMT_SEMIPLANAR) && ((d.crop_left | d.crop_right | d.crop_top | d.crop_bottom) & 1))
        return P265R_EINVAL;
    switch (d.sample) {
        case P265R_SMP_NATIVE: s->es = bit_depth > 8 ? 2 : 1; break;
        case P265R_SMP_U8: s->es = 1; break;
        case P265R_SMP_F32: s->es = 4; break;
        default: s->es = 2; break;                       // MSB16, F16
    }
    s->rgb = rgb ? 1 : 0;
    s->mono = mono ? 1 : 0;
    s->n_planes = d.format == P265R_FMT_SEMIPLANAR ? 2 : (d.format == P265R_FMT_RGB_PACKED ? 1 : 3);
    if (mono && d.format == P265R_FMT_PLANAR) s->n_planes = 1;
    return P265R_OK;
}

int export_planes(const p265r_export_desc& d, const ExportShape& s, int pw, int ph, ExportPlane pl[3]) {
    const int w = pw - d.crop_left - d.crop_right, h = ph - d.crop_top - d.crop_bottom;
    if (pw <= 0 || ph <= 0 || (pw & 1) || (ph & 1) || w <= 0 || h <= 0) return P265R_EINVAL;
    const uint64_t luma = (uint64_t)w * s.es;
    if (s.mono && d.format == P265R_FMT_PLANAR) {            // the luma plane alone
        pl[0] = {luma, h};
        pl[1] = pl[2] = {0, 0};
        return P265R_OK;
    }
    switch (d.format) {
        case P265R_FMT_PLANAR: pl[0] = {luma, h}; pl[1] = pl[2] = {luma / 2, h / 2}; break;
        case P265R_FMT_SEMIPLANAR: pl[0] = {luma, h}; pl[1] = {luma, h / 2}; pl[2] = {0, 0}; break;
        case P265R_FMT_RGB_PLANAR: pl[0] = pl[1] = pl[2] = {luma, h}; break;
        default: pl[0] = {3 * luma, h}; pl[1] = pl[2] = {0, 0}; break;
    }
    return P265R_OK;
}

int export_check_layout(const p265r_export_desc& d, const ExportShape& s, int pw, int ph, uint64_t* slot_bytes) {
    ExportPlane pl[3];
    if (const int rc = export_planes(d, s, pw, ph, pl)) return rc;
    const uint64_t lim = 1ull << 46;                     // keeps every product below 2^63
    uint64_t lo[3], hi[3], end = 0;
    for (int k = 0; k < s.n_planes; ++k) {
        if (d.pitch[k] < pl[k].row_bytes || d.pitch[k] % s.es || d.plane_off[k] % s.es) return P265R_EINVAL;
        if (d.pitch[k] >= lim || d.plane_off[k] >= lim) return P265R_EINVAL;
        lo[k] = d.plane_off[k];
        hi[k] = lo[k] + d.pitch[k] * (uint64_t)(pl[k].rows - 1) + pl[k].row_bytes;
        end = std::max(end, hi[k]);
        for (int j = 0; j < k; ++j)
            if (lo[k] < hi[j] && lo[j] < hi[k]) return P265R_EINVAL;
    }
    if (d.frame_bytes < end || d.frame_bytes % s.es || d.frame_bytes >= lim) return P265R_EINVAL;
    if (slot_bytes) *slot_bytes = end;
    return P265R_OK;
}

int export_coefficients(const p265r_export_desc& d, int bit_depth, int32_t out[8]) {
    ExportShape s;
    if (const int rc = export_check_desc(d, bit_depth, &s)) return rc;
    if (!s.rgb) return P265R_EINVAL;
    static const double kKr[3] = {0.299, 0.2126, 0.2627}, kKb[3] = {0.114, 0.0722, 0.0593};
    const int B = bit_depth, D = d.sample == P265R_SMP_U8 ? 8 : B;
    const double kr = kKr[d.matrix], kb = kKb[d.matrix], kg = 1 - kr - kb;
    const double top = (double)((1 << D) - 1);
    const double my = d.full_range ? top / ((1 << B) - 1) : top / (219 * (1 << (B - 8)));
    const double mc = d.full_range ? top / ((1 << B) - 1) : top / (224 * (1 << (B - 8)));
    const double one = 16384.0;
    out[0] = (int32_t)std::nearbyint(my * one);
    out[1] = (int32_t)std::nearbyint(2 * (1 - kr) * mc * one);
    out[2] = (int32_t)std::nearbyint(2 * kb * (1 - kb) / kg * mc * one);
    out[3] = (int32_t)std::nearbyint(2 * kr * (1 - kr) / kg * mc * one);
    out[4] = (int32_t)std::nearbyint(2 * (1 - kb) * mc * one);
    out[5] = d.full_range ? 0 : 16 << (B - 8);
    out[6] = 1 << (B - 1);
    out[7] = D;
    return P265R_OK;
}

}  // namespace p265r

using namespace p265r;

extern "C" {

int p265r_export_layout(const p265r_params* params, int pic_width, int pic_height, p265r_export_desc* desc,
                        uint32_t pitch_align) {
    if (!params || !desc || params->version != P265R_ABI_VERSION) return P265R_EINVAL;
    const bool mono = params->chroma_format_idc == 0;        // (bit_depth_chroma means nothing then)
    if (!mono && params->bit_depth_chroma != params->bit_depth_luma) return P265R_EINVAL;
    const int pw = pic_width ? pic_width : params->pic_width, ph = pic_height ? pic_height : params->pic_height;
    if (pw <= 0 || ph <= 0 || pw > 0xffff || ph > 0xffff || pitch_align > (1u << 20)) return P265R_EINVAL;
    ExportShape s;
    if (const int rc = export_check_desc(*desc, params->bit_depth_luma, &s, mono)) return rc;
    ExportPlane pl[3];
    if (const int rc = export_planes(*desc, s, pw, ph, pl)) return rc;
    const uint64_t a = pitch_align > 1 ? pitch_align : 1;
    auto up = [a](uint64_t v) { return (v + a - 1) / a * a; };
    uint64_t off = 0;
    for (int k = 0; k < 3; ++k) {
        desc->plane_off[k] = k < s.n_planes ? off : 0;
        desc->pitch[k] = k < s.n_planes ? up(pl[k].row_bytes) : 0;
        if (k < s.n_planes) off = up(off + desc->pitch[k] * (uint64_t)pl[k].rows);
    }
    desc->frame_bytes = off;
    return export_check_layout(*desc, s, pw, ph, nullptr);      // (an alignment that is no multiple of the element)
}

int p265r_export_coefficients(const p265r_export_desc* desc, int bit_depth, int32_t out[8]) {
    if (!desc || !out) return P265R_EINVAL;
    return export_coefficients(*desc, bit_depth, out);
}

}  // extern "C"
