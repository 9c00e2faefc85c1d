// resize_host.cpp -- see resize_host.h.
#include "resize_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace p265r {

int resize_check_desc(const p265r_export_desc& d, const p265r_resize_desc& rs, int bit_depth, bool mono, ExportShape* s) {
    p265r_export_desc dc = d;
    dc.upsample = P265R_UP_NEAREST;                      // ignored: the filter decides how chroma is sampled
    if (const int rc = export_check_desc(dc, bit_depth, s, mono)) return rc;
    if (rs.filter > P265R_RS_AREA || (rs.flags & ~P265R_RS_NORM)) return P265R_EINVAL;
    if (rs.out_width < 1 || rs.out_width > (uint32_t)kRsMaxOut || rs.out_height < 1 || rs.out_height > (uint32_t)kRsMaxOut)
        return P265R_EINVAL;
    // half-size chroma in the destination: planar / semi-planar of a 4:2:0 source, semi-planar of a monochrome one
    const bool half = d.format == P265R_FMT_SEMIPLANAR || (d.format == P265R_FMT_PLANAR && !mono);
    if (half && ((rs.out_width | rs.out_height) & 1)) return P265R_EINVAL;
    if (rs.flags & P265R_RS_NORM) {
        if (d.sample != P265R_SMP_F16 && d.sample != P265R_SMP_F32) return P265R_EINVAL;
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(rs.scale[c]) || !std::isfinite(rs.bias[c])) return P265R_EINVAL;
    }
    return P265R_OK;
}

void resize_planes(const p265r_export_desc& d, const ExportShape& s, const p265r_resize_desc& rs, ExportPlane pl[3]) {
    const int w = (int)rs.out_width, h = (int)rs.out_height;
    const uint64_t luma = (uint64_t)w * s.es;
    pl[0] = {luma, h};
    pl[1] = pl[2] = {0, 0};
    if (s.mono && d.format == P265R_FMT_PLANAR) return;      // the luma plane alone
    switch (d.format) {
        case P265R_FMT_PLANAR: pl[1] = pl[2] = {luma / 2, h / 2}; break;
        case P265R_FMT_SEMIPLANAR: pl[1] = {luma, h / 2}; break;
        case P265R_FMT_RGB_PLANAR: pl[1] = pl[2] = {luma, h}; break;
        default: pl[0] = {3 * luma, h}; break;
    }
}

int resize_check_layout(const p265r_export_desc& d, const ExportShape& s, const p265r_resize_desc& rs, uint64_t* slot_bytes) {
    ExportPlane pl[3];
    resize_planes(d, s, rs, pl);
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

int resize_check_window(const p265r_resize_desc& rs, int w, int h) {
    if (w <= 0 || h <= 0 || w > kRsMaxWindow || h > kRsMaxWindow) return P265R_EINVAL;
    if (rs.filter == P265R_RS_AREA) {
        if (w > kRsMaxArea || h > kRsMaxArea) return P265R_EINVAL;
        if (rs.out_width > (uint32_t)w || rs.out_height > (uint32_t)h) return P265R_EINVAL;
    }
    return P265R_OK;
}

void resize_norm(const p265r_resize_desc& rs, int bit_depth, float scale[3], float bias[3]) {
    for (int c = 0; c < 3; ++c) {
        const bool on = (rs.flags & P265R_RS_NORM) != 0;
        scale[c] = on ? rs.scale[c] : (float)(1.0 / (double)((1 << bit_depth) - 1));
        bias[c] = on ? rs.bias[c] : 0.0f;
    }
}

uint16_t resize_f16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0));
    if (mag >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);             // rounds to 65520 or above: infinity
    if (mag < 0x33000001u) return (uint16_t)sign;                          // at most 2^-25: rounds to zero
    const int e = (int)(mag >> 23) - 127;
    uint32_t man = (mag & 0x7fffffu) | 0x800000u;
    int shift = 13;                                                        // normal: 23 -> 10 mantissa bits
    uint32_t base;
    if (e < -14) { shift += -14 - e; base = 0; }                           // subnormal
    else base = (uint32_t)(e + 15) << 10;
    const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    uint32_t r = (e < -14 ? q : (q & 0x3ffu)) + base;
    if (rem > halfway || (rem == halfway && (q & 1))) ++r;                 // (a carry moves into the exponent)
    return (uint16_t)(sign | r);
}

int resize_plane_host(const uint16_t* src, uint64_t stride, int nw, int nh, int chroma_plane, int chroma_grid,
                      uint32_t filter, int mw, int mh, int32_t* dst) {
    if (!src || !dst || filter > P265R_RS_AREA) return P265R_EINVAL;
    if (nw < 1 || nh < 1 || mw < 1 || mh < 1 || mw > kRsMaxOut || mh > kRsMaxOut) return P265R_EINVAL;
    if (chroma_grid && !chroma_plane) return P265R_EINVAL;
    if (chroma_plane && ((nw | nh) & 1)) return P265R_EINVAL;
    if (chroma_grid && ((mw | mh) & 1)) return P265R_EINVAL;
    p265r_resize_desc rs{};
    rs.out_width = (uint32_t)mw; rs.out_height = (uint32_t)mh; rs.filter = filter;
    if (const int rc = resize_check_window(rs, nw, nh)) return rc;
    const int ow = chroma_grid ? mw / 2 : mw, oh = chroma_grid ? mh / 2 : mh;
    const int pw = chroma_plane ? nw / 2 : nw;
    if (stride < (uint64_t)pw) return P265R_EINVAL;
    const RsAxis ax = rs_axis(nw, mw), ay = rs_axis(nh, mh);
    auto hx = [&](int i) { return (uint32_t)(chroma_grid ? 4 * i + 1 : 2 * i + 1); };
    auto hy = [&](int i) { return (uint32_t)(chroma_grid ? 4 * i + 2 : 2 * i + 1); };
    auto at = [&](int y, int x) { return (int)src[(uint64_t)y * stride + (uint64_t)x]; };
    if (filter == P265R_RS_NEAREST) {
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x)
                dst[(size_t)y * ow + x] = at(rs_nearest(ay, hy(y), chroma_plane), rs_nearest(ax, hx(x), chroma_plane));
    } else if (filter == P265R_RS_BILINEAR) {
        for (int y = 0; y < oh; ++y) {
            const RsTap ty = rs_bilinear(ay, hy(y), chroma_plane, 1);
            for (int x = 0; x < ow; ++x) {
                const RsTap tx = rs_bilinear(ax, hx(x), chroma_plane, 0);
                dst[(size_t)y * ow + x] = rs_blend(at(ty.i0, tx.i0), at(ty.i0, tx.i1), at(ty.i1, tx.i0), at(ty.i1, tx.i1), tx.f, ty.f);
            }
        }
    } else {
        const RsBox bx = rs_box(nw, mw, chroma_plane, chroma_grid), by = rs_box(nh, mh, chroma_plane, chroma_grid);
        const RsDiv dv = rs_div_make(bx.N, by.N);
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x) {
                uint64_t sum = 0;
                for (uint32_t ky = rs_box_first(by, (uint32_t)y); ky * by.M < ((uint32_t)y + 1) * by.N; ++ky) {
                    uint64_t row = 0;
                    for (uint32_t kx = rs_box_first(bx, (uint32_t)x); kx * bx.M < ((uint32_t)x + 1) * bx.N; ++kx)
                        row += (uint64_t)rs_box_weight(bx, (uint32_t)x, kx) * (uint64_t)at((int)ky, (int)kx);
                    sum += row * rs_box_weight(by, (uint32_t)y, ky);
                }
                dst[(size_t)y * ow + x] = (int32_t)rs_div(dv, sum);
            }
    }
    return P265R_OK;
}

}  // namespace p265r

using namespace p265r;

extern "C" {

int p265r_resize_layout(const p265r_params* params, p265r_export_desc* desc, const p265r_resize_desc* rs, uint32_t pitch_align) {
    if (!params || !desc || !rs || params->version != P265R_ABI_VERSION) return P265R_EINVAL;
    const bool mono = params->chroma_format_idc == 0;
    if (!mono && params->bit_depth_chroma != params->bit_depth_luma) return P265R_EINVAL;
    if (pitch_align > (1u << 20)) return P265R_EINVAL;
    ExportShape s;
    if (const int rc = resize_check_desc(*desc, *rs, params->bit_depth_luma, mono, &s)) return rc;
    ExportPlane pl[3];
    resize_planes(*desc, s, *rs, pl);
    const uint64_t a = pitch_align > 1 ? pitch_align : 1;
    auto up = [a](uint64_t v) { return (v + a - 1) / a * a; };
    uint64_t off = 0;
    for (int k = 0; k < 3; ++k) {
        desc->plane_off[k] = k < s.n_planes ? off : 0;
        desc->pitch[k] = k < s.n_planes ? up(pl[k].row_bytes) : 0;
        if (k < s.n_planes) off = up(off + desc->pitch[k] * (uint64_t)pl[k].rows);
    }
    desc->frame_bytes = off;
    return resize_check_layout(*desc, s, *rs, nullptr);      // (an alignment that is no multiple of the element)
}

int p265r_resize_position(uint32_t filter, int n, int m, int h, int chroma, int vertical, int32_t* i0, int32_t* i1,
                          int32_t* frac) {
    if (!i0 || !i1 || !frac || filter > P265R_RS_BILINEAR) return P265R_EINVAL;
    if (n < 1 || n > kRsMaxWindow || m < 1 || m > kRsMaxOut || h < 0 || h > 2 * m) return P265R_EINVAL;
    if (chroma && (n & 1)) return P265R_EINVAL;
    const RsAxis a = rs_axis(n, m);
    if (filter == P265R_RS_NEAREST) {
        *i0 = *i1 = rs_nearest(a, (uint32_t)h, chroma != 0);
        *frac = 0;
    } else {
        const RsTap t = rs_bilinear(a, (uint32_t)h, chroma != 0, vertical != 0);
        *i0 = t.i0; *i1 = t.i1; *frac = t.f;
    }
    return P265R_OK;
}

int p265r_resize_plane_host(const uint16_t* src, uint64_t stride, int nw, int nh, int chroma_plane, int chroma_grid,
                            uint32_t filter, int mw, int mh, int32_t* dst, const float* norm, float* f32_out,
                            uint16_t* f16_out) {
    if (const int rc = resize_plane_host(src, stride, nw, nh, chroma_plane, chroma_grid, filter, mw, mh, dst)) return rc;
    if (!norm) return (f32_out || f16_out) ? P265R_EINVAL : P265R_OK;
    if (!std::isfinite(norm[0]) || !std::isfinite(norm[1])) return P265R_EINVAL;
    const size_t count = (size_t)(chroma_grid ? mw / 2 : mw) * (size_t)(chroma_grid ? mh / 2 : mh);
    for (size_t i = 0; i < count; ++i) {
        const float f = rs_norm(dst[i], norm[0], norm[1]);
        if (f32_out) f32_out[i] = f;
        if (f16_out) f16_out[i] = resize_f16_bits(f);
    }
    return P265R_OK;
}

}  // extern "C"
