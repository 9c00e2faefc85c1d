// grid_host.cpp -- see grid_host.h.
#include "grid_host.h"

#include <algorithm>

namespace p265r {

int grid_check(const p265r_export_desc& d, const p265r_grid_desc& gd, int bit_depth, bool mono, int tile_w, int tile_h,
               GridShape* s) {
    if (gd.rows < 1 || gd.rows > 256 || gd.cols < 1 || gd.cols > 256 || gd.orientation > 7) return P265R_EINVAL;
    if (gd.reserved[0] | gd.reserved[1] | gd.reserved[2]) return P265R_EINVAL;
    if (tile_w <= 0 || tile_h <= 0 || tile_w > 0xffff || tile_h > 0xffff || (tile_w & 1) || (tile_h & 1)) return P265R_EINVAL;
    // enums and sample type; the crop parity has rules of its own here (crop_right / crop_bottom may be odd)
    p265r_export_desc dz = d;
    dz.crop_left = dz.crop_right = dz.crop_top = dz.crop_bottom = 0;
    if (const int rc = export_check_desc(dz, bit_depth, &s->e, mono)) return rc;
    const int64_t cw = (int64_t)gd.cols * tile_w, ch = (int64_t)gd.rows * tile_h;        // (below 2^24)
    if (cw > 0xffff || ch > 0xffff) return P265R_EINVAL;
    // the HEIF rule: the output ends inside the last tile column / row
    if ((int64_t)gd.out_width <= cw - tile_w || (int64_t)gd.out_width > cw) return P265R_EINVAL;
    if ((int64_t)gd.out_height <= ch - tile_h || (int64_t)gd.out_height > ch) return P265R_EINVAL;
    const int64_t W = (int64_t)gd.out_width - d.crop_left - d.crop_right;
    const int64_t H = (int64_t)gd.out_height - d.crop_top - d.crop_bottom;
    if (W <= 0 || H <= 0) return P265R_EINVAL;
    // a 4:2:0 source: the window starts on a chroma sample; formats with a half-size plane: whole chroma samples
    const bool half_plane = d.format == P265R_FMT_SEMIPLANAR || (!mono && d.format == P265R_FMT_PLANAR);
    if ((!mono || half_plane) && ((d.crop_left | d.crop_top) & 1)) return P265R_EINVAL;
    if (half_plane && ((W | H) & 1)) return P265R_EINVAL;
    s->tw = tile_w; s->th = tile_h;
    s->cw = (int)cw; s->ch = (int)ch;
    s->wl = d.crop_left; s->wt = d.crop_top;
    s->W = (int)W; s->H = (int)H;
    s->k = (int)(gd.orientation & 3); s->m = (int)(gd.orientation >> 2);
    s->transpose = s->k & 1;
    s->dw = s->transpose ? s->H : s->W;
    s->dh = s->transpose ? s->W : s->H;
    // rot90(F, k) then the mirror, as reversals of F followed (k odd) by a plain transpose:
    //   k = 0: (m, 0)   k = 2: (!m, 1)   k = 1: (1, m), transposed   k = 3: (0, !m), transposed
    switch (s->k) {
        case 0: s->fx = s->m; s->fy = 0; break;
        case 1: s->fx = 1; s->fy = s->m; break;
        case 2: s->fx = !s->m; s->fy = 1; break;
        default: s->fx = 0; s->fy = !s->m; break;
    }
    return P265R_OK;
}

void grid_planes(const p265r_export_desc& d, const ExportShape& s, int w, int h, ExportPlane pl[3]) {
    const uint64_t luma = (uint64_t)w * s.es;
    pl[0] = {luma, h};
    pl[1] = pl[2] = {0, 0};
    if (s.mono && d.format == P265R_FMT_PLANAR) return;     // the luma plane alone
    switch (d.format) {
        case P265R_FMT_PLANAR: pl[1] = pl[2] = {(uint64_t)(w / 2) * s.es, h / 2}; break;
        case P265R_FMT_SEMIPLANAR: pl[1] = {(uint64_t)(w / 2) * 2 * s.es, h / 2}; break;
        case P265R_FMT_RGB_PLANAR: pl[1] = pl[2] = {luma, h}; break;
        default: pl[0] = {3 * luma, h}; break;
    }
}

int grid_check_layout(const p265r_export_desc& d, const ExportShape& s, int w, int h, uint64_t* slot_bytes) {
    ExportPlane pl[3];
    grid_planes(d, s, w, h, pl);
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

void grid_fill_layout(p265r_export_desc* d, const ExportShape& s, int w, int h, uint64_t pitch_align) {
    ExportPlane pl[3];
    grid_planes(*d, s, w, h, pl);
    const uint64_t a = pitch_align > 1 ? pitch_align : 1;
    auto up = [a](uint64_t v) { return (v + a - 1) / a * a; };
    uint64_t off = 0;
    for (int k = 0; k < 3; ++k) {
        d->plane_off[k] = k < s.n_planes ? off : 0;
        d->pitch[k] = k < s.n_planes ? up(pl[k].row_bytes) : 0;
        if (k < s.n_planes) off = up(off + d->pitch[k] * (uint64_t)pl[k].rows);
    }
    d->frame_bytes = off;
}

}  // namespace p265r

using namespace p265r;

extern "C" {

int p265r_grid_layout(const p265r_params* params, int tile_width, int tile_height, const p265r_grid_desc* grid,
                      p265r_export_desc* desc, uint32_t pitch_align) {
    if (!params || !desc || !grid || params->version != P265R_ABI_VERSION) return P265R_EINVAL;
    const bool mono = params->chroma_format_idc == 0;        // (bit_depth_chroma means nothing then)
    if (!mono && params->bit_depth_chroma != params->bit_depth_luma) return P265R_EUNSUPPORTED;
    const int tw = tile_width ? tile_width : params->pic_width, th = tile_height ? tile_height : params->pic_height;
    if (pitch_align > (1u << 20)) return P265R_EINVAL;
    GridShape s;
    if (const int rc = grid_check(*desc, *grid, params->bit_depth_luma, mono, tw, th, &s)) return rc;
    grid_fill_layout(desc, s.e, s.dw, s.dh, pitch_align);
    return grid_check_layout(*desc, s.e, s.dw, s.dh, nullptr);  // (an alignment that is no multiple of the element)
}

}  // extern "C"
