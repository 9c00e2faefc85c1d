// grid_resize_host.h -- the host-only part of the scaled grid export (p265r_batch_export_grid_resized): validation
// of every p265r_grid_frame against a tile size, an export desc and a resize desc, and the per-frame constants the
// kernels of grid_resize.h read from their device table.  No HIP: p265r.hip calls it before anything is launched,
// and a CPU build can check it on its own (tools/grid_resize_check.cpp).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/p265r.h"
#include "export_host.h"
#include "grid_host.h"
#include "resize_host.h"
#include "resize_math.h"

namespace p265r {

// One frame of the device table (48 bytes).  R = the resized window before the quarter turn: ph rows of pw.
struct GridRsFrame {
    uint64_t dst;            // where R's frame begins: its slot, or (transpose) its frame of the staging area
    int32_t tile0;           // the frame's first tile in the table of plane addresses
    int32_t rows, cols;      // tiles
    int32_t wl, wt, W, H;    // the window on the canvas
    int32_t pw, ph;          // the size of R: (ow, oh), or (oh, ow) under a quarter turn
    int32_t flags;           // kGridRsFx | kGridRsFy: R is written reversed along x / y; kGridRsTr: transposed after
};
constexpr int32_t kGridRsFx = 1, kGridRsFy = 2, kGridRsTr = 4;

// x / d for x < 65536 and 1 <= d < 65536 by one multiply: rcp = ceil(2^32 / d) = (2^32 + e) / d with 0 <= e < d, so
// x rcp / 2^32 = x / d + x e / (d 2^32), and x e / (d 2^32) < x / 2^32 < 2^-16 < 1 / d.  The fractional part of x / d
// is at most 1 - 1 / d: the floor is that of x / d.  (d = 1: rcp would be 2^32; the quotient is x.)
// tools/grid_resize_check.cpp compares both sides at every x = k d - 1, k d below 65536 for every d: two
// non-decreasing step functions that agree on both sides of every step of one of them, and at 65535, are equal.
RESIZE_FN uint32_t grid_rs_rcp(uint32_t d) { return d > 1 ? 0xffffffffu / d + 1 : 0; }
RESIZE_FN uint32_t grid_rs_div(uint32_t x, uint32_t d, uint32_t rcp) {
    return d > 1 ? (uint32_t)(((uint64_t)x * rcp) >> 32) : x;
}

struct GridRsPlan {
    ExportShape e;
    int tw, th;                       // tile size, luma
    int ow, oh;                       // slot size
    int n_tiles, n_stage;             // tiles listed; frames with a quarter turn
    int max_pw, max_ph;               // the largest R
    std::vector<GridRsFrame> frames;  // dst = 0: the caller knows the addresses
    std::vector<int32_t> stage;       // per frame: its index in the staging area, -1 without a quarter turn
};

// Everything of desc + rs + frames[0..n) that needs no batch.  mono: the source pictures are 4:0:0.
int grid_resize_plan(const p265r_export_desc& d, const p265r_resize_desc& rs, const p265r_grid_frame* frames, int n,
                     int bit_depth, bool mono, int tile_w, int tile_h, GridRsPlan* plan);

}  // namespace p265r
