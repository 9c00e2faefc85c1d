// grid_resize_host.cpp -- see grid_resize_host.h.
#include "grid_resize_host.h"

#include <algorithm>

namespace p265r {

int grid_resize_plan(const p265r_export_desc& d, const p265r_resize_desc& rs, const p265r_grid_frame* frames, int n,
                     int bit_depth, bool mono, int tile_w, int tile_h, GridRsPlan* plan) {
    if (!frames || n <= 0 || n > 65535) return P265R_EINVAL;
    if (d.crop_left | d.crop_right | d.crop_top | d.crop_bottom) return P265R_EINVAL;    // the crop is per frame
    if (const int rc = resize_check_desc(d, rs, bit_depth, mono, &plan->e)) return rc;
    plan->tw = tile_w; plan->th = tile_h;
    plan->ow = (int)rs.out_width; plan->oh = (int)rs.out_height;
    plan->n_tiles = plan->n_stage = 0;
    plan->max_pw = plan->max_ph = 0;
    plan->frames.assign((size_t)n, GridRsFrame{});
    plan->stage.assign((size_t)n, -1);
    p265r_export_desc dg = d;
    dg.upsample = P265R_UP_NEAREST;                      // ignored: the filter decides how chroma is sampled
    for (int f = 0; f < n; ++f) {
        const p265r_grid_frame& fr = frames[f];
        if ((fr.crop_left | fr.crop_right | fr.crop_top | fr.crop_bottom) > 0xffffu) return P265R_EINVAL;
        p265r_grid_desc gd{};
        gd.rows = fr.rows; gd.cols = fr.cols;
        gd.out_width = fr.out_width; gd.out_height = fr.out_height;
        gd.orientation = fr.orientation;
        for (int k = 0; k < 3; ++k) gd.reserved[k] = fr.reserved[k];
        dg.crop_left = (uint16_t)fr.crop_left; dg.crop_right = (uint16_t)fr.crop_right;
        dg.crop_top = (uint16_t)fr.crop_top; dg.crop_bottom = (uint16_t)fr.crop_bottom;
        GridShape gs;
        if (const int rc = grid_check(dg, gd, bit_depth, mono, tile_w, tile_h, &gs)) return rc;
        // a chroma plane's window is W / 2 x H / 2: whole chroma samples, whatever the format
        if (!mono && ((gs.W | gs.H) & 1)) return P265R_EINVAL;
        p265r_resize_desc rf = rs;                        // the filter sees the pre-turn size
        rf.out_width = gs.transpose ? rs.out_height : rs.out_width;
        rf.out_height = gs.transpose ? rs.out_width : rs.out_height;
        if (const int rc = resize_check_window(rf, gs.W, gs.H)) return rc;
        GridRsFrame& o = plan->frames[(size_t)f];
        o.tile0 = plan->n_tiles;
        o.rows = (int32_t)fr.rows; o.cols = (int32_t)fr.cols;
        o.wl = gs.wl; o.wt = gs.wt; o.W = gs.W; o.H = gs.H;
        o.pw = (int32_t)rf.out_width; o.ph = (int32_t)rf.out_height;
        o.flags = (gs.fx ? kGridRsFx : 0) | (gs.fy ? kGridRsFy : 0) | (gs.transpose ? kGridRsTr : 0);
        if (gs.transpose) plan->stage[(size_t)f] = plan->n_stage++;
        plan->max_pw = std::max(plan->max_pw, (int)o.pw);
        plan->max_ph = std::max(plan->max_ph, (int)o.ph);
        plan->n_tiles += (int)(fr.rows * fr.cols);        // (at most 65536 a frame)
        if (plan->n_tiles > 65535) return P265R_EINVAL;
    }
    return P265R_OK;
}

}  // namespace p265r

using namespace p265r;

extern "C" {

int p265r_grid_resize_plan(const p265r_params* params, int tile_width, int tile_height, const p265r_export_desc* desc,
                           const p265r_resize_desc* rs, const p265r_grid_frame* frames, int n_frames, int32_t* out) {
    if (!params || !desc || !rs || !frames || !out || params->version != P265R_ABI_VERSION) return P265R_EINVAL;
    const bool mono = params->chroma_format_idc == 0;        // (bit_depth_chroma means nothing then)
    if (!mono && params->bit_depth_chroma != params->bit_depth_luma) return P265R_EUNSUPPORTED;
    const int tw = tile_width ? tile_width : params->pic_width, th = tile_height ? tile_height : params->pic_height;
    GridRsPlan plan;
    if (const int rc = grid_resize_plan(*desc, *rs, frames, n_frames, params->bit_depth_luma, mono, tw, th, &plan)) return rc;
    for (int f = 0; f < n_frames; ++f) {
        const GridRsFrame& o = plan.frames[(size_t)f];
        const int32_t v[12] = {o.tile0, o.cols, o.wl, o.wt, o.W, o.H, o.pw, o.ph, (o.flags & kGridRsFx) ? 1 : 0,
                               (o.flags & kGridRsFy) ? 1 : 0, (o.flags & kGridRsTr) ? 1 : 0, plan.stage[(size_t)f]};
        std::copy(v, v + 12, out + (size_t)f * 12);
    }
    return P265R_OK;
}

}  // extern "C"
