// grid_host.h -- the host-only part of the grid export (p265r_batch_export_grid): validation of a p265r_grid_desc
// against a tile size and an export desc, the window, the oriented frame's planes and layout.  No HIP: p265r.hip
// calls it before anything is launched, and a CPU build can check it on its own (tools/grid_check.cpp).
#pragma once
#include <stdint.h>
#include "../../include/p265r.h"
#include "export_host.h"

namespace p265r {

struct GridShape {
    ExportShape e;
    int tw, th;         // tile (picture) size, luma
    int cw, ch;         // canvas size, luma: cols * tw, rows * th
    int wl, wt;         // window origin on the canvas
    int W, H;           // window size = the size of F
    int dw, dh;         // size of the oriented frame: H x W when the turn count is odd
    int k, m;           // orientation: quarter turns anticlockwise, then the left-right mirror
    int fx, fy;         // F is written reversed along x / y (before the transpose, when there is one)
    int transpose;      // k odd
};

// everything of desc + grid that needs no batch (P265R_EINVAL); mono: the source pictures are 4:0:0
int grid_check(const p265r_export_desc& d, const p265r_grid_desc& gd, int bit_depth, bool mono, int tile_w, int tile_h,
               GridShape* s);
// the planes of a w x h frame (no crop) in d's format
void grid_planes(const p265r_export_desc& d, const ExportShape& s, int w, int h, ExportPlane pl[3]);
// plane_off / pitch / frame_bytes against a w x h frame, as export_check_layout
int grid_check_layout(const p265r_export_desc& d, const ExportShape& s, int w, int h, uint64_t* slot_bytes);
// fill plane_off / pitch / frame_bytes with the tight (pitch_align) layout of a w x h frame
void grid_fill_layout(p265r_export_desc* d, const ExportShape& s, int w, int h, uint64_t pitch_align);

}  // namespace p265r
