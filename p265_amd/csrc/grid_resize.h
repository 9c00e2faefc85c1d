// grid_resize.h -- scaled grid export (p265r_batch_export_grid_resized): every frame a grid of tiles of its own
// shape, cut to its own window, filtered into a slot of one fixed size ow x oh and turned / mirrored.  The
// arithmetic is the one include/p265r.h states: resize.h's filters (resize_math.h) applied to the WINDOW of a canvas,
// then grid.h's orientation; tests/grid_resize_ref.py restates it.  No counterpart in the reference.  export.h,
// resize.h and grid.h are used, not changed.
//
// Pass 1 cuts the work as resize.h does: a workgroup is 4 waves, a wave per row of R (the resized window before
// the quarter turn: ph rows of pw), a lane per 16-byte group of the destination row, groups anchored at the row's
// first 16-byte boundary and written with export_store.  What differs is the source: a row of the canvas, found
// through the device table of the tiles' plane addresses as in grid.h.  A frame's constants (GridRsFrame: tiles,
// window, R's size, flips, where R is written) are read once per workgroup through readfirstlane: scalar.  Frames
// of different shapes share a launch, so a workgroup that has nothing to do in ITS frame returns -- always
// block-uniformly and before the first barrier.
//
// NEAREST / BILINEAR gather their taps: the row's vertical taps and their tile row are wave-uniform, the tile column
// of a horizontal tap is found per lane with one division by the tile width (the second tap of a pair is the same
// sample or the next: a compare, not a division).  The division is a multiply by the tile width's reciprocal
// (grid_rs_div: exact below 65536, grid_resize_host.h says why); the generic x / tw is a sequence of some thirty
// instructions per tap.
// AREA has the structure of rs_area_group: 256 lanes x 8 columns per chunk, vertical sums in registers, 4 x 2048
// column sums through 32 KB of LDS, the horizontal reduction and rs_div.  The walk over source rows crosses tile
// rows (the tile row stays uniform); a lane's 8 columns inside one tile take the wide load, a load that straddles a
// seam or the window's end reads element by element.
// Orientation: the flips are index reversals as in grid.h (the mirrored span of R, reversed in registers; rows by
// their index).  A frame with a quarter turn writes R into its frame of the batch's staging area, and pass 2
// (grid_resize_transpose_kernel: grid.h's tile routine) transposes it into the slot; frames without one are written
// straight to their slot, and their transpose blocks return at once.
#pragma once
#include "export.h"
#include "resize_math.h"
#include "grid.h"
#include "resize.h"
#include "grid_resize_host.h"

namespace p265r {

struct GridRsArgs {
    ResizeArgs r;                        // the slot's layout (e.plane_off / e.pitch), coef, shift, ow, oh, grey, scale, bias
    uint64_t st_off[3], st_pitch[3];     // the layout of a frame of the staging area (quarter turns: oh x ow)
    const GridRsFrame* frames;           // device: one entry per frame
    const uint64_t* tab;                 // device: plane addresses [tile][3]
    int tw, th;                          // tile size (luma)
    uint32_t rcp_w[2], rcp_h[2];         // grid_rs_rcp of the tile width / height in a luma, a chroma plane
};

// a frame's table entry, scalar
__device__ __forceinline__ GridRsFrame grid_rs_frame(const GridRsFrame* __restrict__ frames, int f) {
    const GridRsFrame* p = frames + f;
    GridRsFrame o;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p->dst);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p->dst >> 32));
    o.dst = (uint64_t)hi << 32 | lo;
    o.tile0 = __builtin_amdgcn_readfirstlane(p->tile0);
    o.rows = __builtin_amdgcn_readfirstlane(p->rows);
    o.cols = __builtin_amdgcn_readfirstlane(p->cols);
    o.wl = __builtin_amdgcn_readfirstlane(p->wl);
    o.wt = __builtin_amdgcn_readfirstlane(p->wt);
    o.W = __builtin_amdgcn_readfirstlane(p->W);
    o.H = __builtin_amdgcn_readfirstlane(p->H);
    o.pw = __builtin_amdgcn_readfirstlane(p->pw);
    o.ph = __builtin_amdgcn_readfirstlane(p->ph);
    o.flags = __builtin_amdgcn_readfirstlane(p->flags);
    return o;
}

// plane k of a frame's window: its tiles, the window's origin and size in the plane's own samples
struct GridRsPlane {
    const uint64_t* t;       // the table entry of tile (0, 0), plane k
    int cols;                // tiles per tile row
    int x0, y0, w, h;        // the window
    int tw, th;              // tile size in this plane
    uint32_t rw, rh;         // their reciprocals
    size_t stride;
};
__device__ __forceinline__ GridRsPlane grid_rs_plane(const GridRsArgs& a, const Geo& g, const GridRsFrame& f, int k) {
    const int sub = k ? 1 : 0;
    GridRsPlane p;
    p.t = a.tab + (size_t)f.tile0 * 3 + k;
    p.cols = f.cols;
    p.x0 = f.wl >> sub; p.y0 = f.wt >> sub;
    p.w = f.W >> sub; p.h = f.H >> sub;
    p.tw = a.tw >> sub; p.th = a.th >> sub;
    p.rw = a.rcp_w[sub]; p.rh = a.rcp_h[sub];
    p.stride = (size_t)g.stride[k];
    return p;
}

// row y of the window (0 <= y < h): the table entries of its tile row, the row's sample offset  (wave-uniform)
__device__ __forceinline__ GridRow grid_rs_row(const GridRsPlane& p, int y) {
    const int Y = p.y0 + y;
    const int ty = (int)grid_rs_div((uint32_t)Y, (uint32_t)p.th, p.rh);
    GridRow r;
    r.t = p.t + ((size_t)ty * (size_t)p.cols) * 3;
    r.off = (size_t)(Y - ty * p.th) * p.stride;
    return r;
}

// column x of the window (0 <= x < w): its tile column and the column inside the tile
struct GridRsCol {
    int t, o;
};
__device__ __forceinline__ GridRsCol grid_rs_col(const GridRsPlane& p, int x) {
    const int X = p.x0 + x;
    GridRsCol c;
    c.t = (int)grid_rs_div((uint32_t)X, (uint32_t)p.tw, p.rw);
    c.o = X - c.t * p.tw;
    return c;
}
template <typename S>
__device__ __forceinline__ S grid_rs_at(const GridRow& r, const GridRsCol& c) {
    return reinterpret_cast<const S*>(r.t[3 * c.t])[r.off + (size_t)c.o];
}

// samples [c0, c0 + N) of a window row, c0 >= 0: the wide load when they lie inside the window and one tile, else
// elements with their index clamped to the window
template <typename S, int N>
__device__ __forceinline__ void grid_rs_load(const GridRsPlane& p, const GridRow& r, int c0, S* v) {
    const GridRsCol c = grid_rs_col(p, c0);
    if (c0 + N <= p.w && c.o + N <= p.tw) {
        export_load<S, N>(reinterpret_cast<const S*>(r.t[3 * c.t]) + r.off + (size_t)c.o, v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = grid_rs_at<S>(r, grid_rs_col(p, min(c0 + i, p.w - 1)));
    }
}

// G gathered outputs of one row of R: output columns x0 .. x0 + G - 1 (clamped to the row: the caller stores only
// the ones inside), cg = the output is on the chroma grid
template <typename S, int FILTER, int G>
__device__ __forceinline__ void grid_rs_gather_group(const GridRsPlane& p, const RsAxis& ax, const RsAxis& ay, int chroma,
                                                     bool cg, int row, int x0, int cols, int* out) {
    const RsRow rr = rs_row<FILTER>(ay, (uint32_t)(cg ? 4 * row + 2 : 2 * row + 1), chroma);
    const GridRow r0 = grid_rs_row(p, rr.y0);                                      // (wave-uniform)
    const GridRow r1 = FILTER == (int)kRsBilinear ? grid_rs_row(p, rr.y1) : r0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int x = min(max(x0 + i, 0), cols - 1);
        const uint32_t hx = (uint32_t)(cg ? 4 * x + 1 : 2 * x + 1);
        if (FILTER == (int)kRsNearest) {
            out[i] = (int)grid_rs_at<S>(r0, grid_rs_col(p, rs_nearest(ax, hx, chroma)));
        } else {
            const RsTap t = rs_bilinear(ax, hx, chroma, 0);
            const GridRsCol c0 = grid_rs_col(p, t.i0);
            GridRsCol c1 = c0;                                                     // i1 = i0 or i0 + 1
            if (t.i1 != t.i0 && ++c1.o == p.tw) { ++c1.t; c1.o = 0; }
            out[i] = rs_blend((int)grid_rs_at<S>(r0, c0), (int)grid_rs_at<S>(r0, c1), (int)grid_rs_at<S>(r1, c0),
                              (int)grid_rs_at<S>(r1, c1), t.f, rr.fy);
        }
    }
}

// AREA: rs_area_group with the window of a canvas as its source.  Every thread of the workgroup calls it (block
// barriers).  rows x cols: the plane's outputs; [xlo, xhi): the output columns of the whole workgroup (uniform, not
// empty); outputs outside the plane come back as 0.
template <typename S, int G>
__device__ __forceinline__ void grid_rs_area_group(const GridRsPlane& p, const RsBox& bx, const RsBox& by, int r0, int rows,
                                                   int cols, int xlo, int xhi, int x0, uint32_t* __restrict__ lds, int* out) {
    const int t = (int)threadIdx.x, wave = t >> 6;
    const int pw = p.w, ph = p.h;
    const RsDiv dv = rs_div_make(bx.N, by.N);
    const int c_lo = (int)rs_box_first(bx, (uint32_t)xlo);
    const int c_hi = min(pw, (int)(((uint32_t)xhi * bx.N + bx.M - 1) / bx.M));
    const bool mine = r0 + wave < rows;
    uint64_t sum[G];
#pragma unroll
    for (int i = 0; i < G; ++i) sum[i] = 0;
    for (int cb = c_lo; cb < c_hi; cb += kRsChunk) {                               // (uniform)
        // ---- vertical: this lane's kRsV columns, one set of sums per output row of the band
        const int c0 = cb + t * kRsV;
        const bool active = c0 < c_hi;
        uint32_t acc[kExportRows][kRsV];
        S cur[kRsV];
        uint32_t k = rs_box_first(by, (uint32_t)r0);                               // source row (uniform)
        if (active) grid_rs_load<S, kRsV>(p, grid_rs_row(p, (int)k), c0, cur);
#pragma unroll
        for (int j = 0; j < kExportRows; ++j) {
#pragma unroll
            for (int v = 0; v < kRsV; ++v) acc[j][v] = 0;
            if (r0 + j < rows) {
                const uint32_t o_end = (uint32_t)(r0 + j + 1) * by.N;
                for (;;) {
                    const uint32_t w = rs_box_weight(by, (uint32_t)(r0 + j), k);
                    if (active) {
#pragma unroll
                        for (int v = 0; v < kRsV; ++v) acc[j][v] += w * (uint32_t)cur[v];
                    }
                    const uint32_t s_end = (k + 1) * by.M;
                    if (s_end <= o_end) {                                          // the sample ends here: next source row
                        ++k;
                        if (active && (int)k < ph) grid_rs_load<S, kRsV>(p, grid_rs_row(p, (int)k), c0, cur);
                    }
                    if (s_end >= o_end) break;                                     // the output ends here
                }
            }
        }
        if (active) {
#pragma unroll
            for (int j = 0; j < kExportRows; ++j)
#pragma unroll
                for (int v = 0; v < kRsV; ++v) lds[j * kRsChunk + t * kRsV + v] = acc[j][v];
        }
        __syncthreads();
        // ---- horizontal: the columns of this chunk under each of this lane's outputs
        if (mine) {
            const uint32_t* col = lds + wave * kRsChunk;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int x = x0 + i;
                if (x >= 0 && x < cols) {
                    const int ka = max((int)rs_box_first(bx, (uint32_t)x), cb);
                    const int kb = min(min(cb + kRsChunk, c_hi), (int)(((uint32_t)(x + 1) * bx.N + bx.M - 1) / bx.M));
                    for (int kk = ka; kk < kb; ++kk)
                        sum[i] += (uint64_t)rs_box_weight(bx, (uint32_t)x, (uint32_t)kk) * (uint64_t)col[kk - cb];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < G; ++i) out[i] = (int)rs_div(dv, sum[i]);
}

// The G outputs a destination group at x0 holds, of plane k of R, through the instance's filter: R's columns
// x0 .. x0 + G - 1, or -- reversed along x -- the mirrored span, reversed in registers.  [xlo, xhi): the destination
// columns of the whole workgroup.  AREA: every thread of the workgroup calls it.
template <typename S, int FILTER, int G>
__device__ __forceinline__ void grid_rs_group(const GridRsArgs& a, const Geo& g, const GridRsFrame& f, int k, bool cg, int r0,
                                              int x0, int xlo, int xhi, uint32_t* lds, int* out) {
    const GridRsPlane p = grid_rs_plane(a, g, f, k);
    const int chroma = k ? 1 : 0;
    const int rows = cg ? f.ph >> 1 : f.ph, cols = cg ? f.pw >> 1 : f.pw;
    const bool fx = (f.flags & kGridRsFx) != 0;
    const int xs = fx ? cols - x0 - G : x0;                                        // the span of R
    if constexpr (FILTER == (int)kRsArea) {
        const RsBox bx = rs_box(f.W, f.pw, chroma, cg), by = rs_box(f.H, f.ph, chroma, cg);
        grid_rs_area_group<S, G>(p, bx, by, r0, rows, cols, fx ? cols - xhi : xlo, fx ? cols - xlo : xhi, xs, lds, out);
    } else {
        const int row = min(r0 + (int)(threadIdx.x >> 6), rows - 1);
        grid_rs_gather_group<S, FILTER, G>(p, rs_axis(f.W, f.pw), rs_axis(f.H, f.ph), chroma, cg, row, xs, cols, out);
    }
    if (fx) grid_reverse<int, G, 1>(out);
}

// YUV formats.  grid (ceil(groups of the widest luma row of R / 64), row blocks of the tallest R, frames), 256
// threads; the row blocks of a frame are resize_yuv_kernel's, counted with ITS ph.
template <typename S, int FILTER>
__global__ __launch_bounds__(256) void grid_resize_yuv_kernel(Geo g, GridRsArgs a, int semi) {
    __shared__ uint32_t lds[FILTER == (int)kRsArea ? kRsLds : 1];
    constexpr int E = 16 / (int)sizeof(S);
    const GridRsFrame f = grid_rs_frame(a.frames, (int)blockIdx.z);
    const int nbl = (f.ph + kExportRows - 1) / kExportRows, nbc = ((f.ph >> 1) + kExportRows - 1) / kExportRows;
    int by = blockIdx.y, k = 0;
    if (by >= nbl) {                                                               // (all of it block-uniform)
        by -= nbl;
        if (nbc == 0 || (g.mono && !semi)) return;
        k = semi ? 1 : 1 + by / nbc;
        by -= (k - 1) * nbc;
        if (k > 2 || by >= nbc) return;
    }
    const bool tr = (f.flags & kGridRsTr) != 0;
    const uint64_t plane_off = tr ? a.st_off[k] : a.r.e.plane_off[k];
    const uint64_t pitch = tr ? a.st_pitch[k] : a.r.e.pitch[k];
    const int r0 = by * kExportRows, r = r0 + (int)(threadIdx.x >> 6);             // (wave-uniform) rows of R
    const int rows = k ? f.ph >> 1 : f.ph;
    const bool pairs = semi && k == 1;                                              // CbCr pairs: E / 2 per group
    const int EU = pairs ? E / 2 : E;
    const int units = pairs || k ? f.pw >> 1 : f.pw;                                // outputs of a row (pairs count once)
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)f.dst) + plane_off;
    const int h = pairs ? export_head<2 * (int)sizeof(S)>((uint64_t)(uintptr_t)base)
                        : export_head<(int)sizeof(S)>((uint64_t)(uintptr_t)base);
    const bool vec = h >= 0 && pitch % 16 == 0;
    const int shiftu = vec && h > 0 ? h - EU : 0;
    const int xb = shiftu + (int)blockIdx.x * kExportLanes * EU;                    // the workgroup's first output
    if (xb >= units) return;                                                        // (uniform)
    const int xlo = max(xb, 0), xhi = min(xb + kExportLanes * EU, units);
    const int u0 = xb + (int)(threadIdx.x & 63) * EU;
    const int lo = max(0, -u0), hi = min(EU, units - u0);
    const bool live = r < rows && u0 < units;
    const int rd = (f.flags & kGridRsFy) ? rows - 1 - r : r;                        // the row R's row r is written to
    S v[E];
    if (pairs) {
        constexpr int P = E / 2;
        int cb[P], cr[P];
        if (g.mono) {
#pragma unroll
            for (int i = 0; i < P; ++i) cb[i] = cr[i] = a.r.grey;
        } else {
            if (FILTER != (int)kRsArea && !live) return;
            grid_rs_group<S, FILTER, P>(a, g, f, 1, true, r0, u0, xlo, xhi, lds, cb);
            grid_rs_group<S, FILTER, P>(a, g, f, 2, true, r0, u0, xlo, xhi, lds, cr);
#pragma unroll
            for (int i = 0; i < P; ++i) { cb[i] <<= a.r.e.shift; cr[i] <<= a.r.e.shift; }
        }
        if (!live) return;
#pragma unroll
        for (int i = 0; i < P; ++i) { v[2 * i] = (S)cb[i]; v[2 * i + 1] = (S)cr[i]; }
        export_store<S, E>(reinterpret_cast<S*>(base + (uint64_t)rd * pitch) + 2 * u0, v, 2 * lo, 2 * hi, vec);
    } else {
        if (FILTER != (int)kRsArea && !live) return;
        int o[E];
        grid_rs_group<S, FILTER, E>(a, g, f, k, k != 0, r0, u0, xlo, xhi, lds, o);
        if (!live) return;
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (S)(o[i] << a.r.e.shift);
        export_store<S, E>(reinterpret_cast<S*>(base + (uint64_t)rd * pitch) + u0, v, lo, hi, vec);
    }
}

// RGB formats.  grid (ceil(groups of the widest row of R / 64), ceil(rows of the tallest R / 4), frames), 256
// threads: one row of R per wave, Y, Cb and Cr filtered to the luma grid, then export.h's conversion as
// resize_rgb_kernel applies it.  A monochrome source: Cb = Cr = 1 << (B - 1).
template <typename S, typename D, bool PACKED, int FILTER>
__global__ __launch_bounds__(256) void grid_resize_rgb_kernel(Geo g, GridRsArgs a) {
    __shared__ uint32_t lds[FILTER == (int)kRsArea ? kRsLds : 1];
    constexpr int G = sizeof(D) == 1 ? 16 : 8;
    constexpr int UB = (PACKED ? 3 : 1) * (int)sizeof(D);
    constexpr int NP = PACKED ? 1 : 3;
    const GridRsFrame f = grid_rs_frame(a.frames, (int)blockIdx.z);
    const int r0 = blockIdx.y * kExportRows, r = r0 + (int)(threadIdx.x >> 6);      // (wave-uniform) rows of R
    if (r0 >= f.ph) return;                                                         // (block-uniform)
    const bool tr = (f.flags & kGridRsTr) != 0;
    uint8_t* base[NP];
    uint64_t pitch[NP];
    bool vec[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        base[k] = reinterpret_cast<uint8_t*>((uintptr_t)f.dst) + (tr ? a.st_off[k] : a.r.e.plane_off[k]);
        pitch[k] = tr ? a.st_pitch[k] : a.r.e.pitch[k];
    }
    int h = export_head<UB>((uint64_t)(uintptr_t)base[0]);
    if (h < 0 || pitch[0] % 16 != 0) h = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        vec[k] = pitch[k] % 16 == 0 && (((uint64_t)(uintptr_t)base[k] + (uint64_t)(h * UB)) & 15) == 0;
    const int xb = (h > 0 ? h - G : 0) + (int)blockIdx.x * kExportLanes * G;
    if (xb >= f.pw) return;                                                         // (uniform)
    const int xlo = max(xb, 0), xhi = min(xb + kExportLanes * G, f.pw);
    const int x0 = xb + (int)(threadIdx.x & 63) * G;
    const int lo = max(0, -x0), hi = min(G, f.pw - x0);
    const bool live = r < f.ph && x0 < f.pw;
    if (FILTER != (int)kRsArea && !live) return;
    int yv[G], cb[G], cr[G];
    const int half = a.r.e.coef[6];
    grid_rs_group<S, FILTER, G>(a, g, f, 0, false, r0, x0, xlo, xhi, lds, yv);
    if (g.mono) {
#pragma unroll
        for (int i = 0; i < G; ++i) cb[i] = cr[i] = half;
    } else {
        grid_rs_group<S, FILTER, G>(a, g, f, 1, false, r0, x0, xlo, xhi, lds, cb);
        grid_rs_group<S, FILTER, G>(a, g, f, 2, false, r0, x0, xlo, xhi, lds, cr);
    }
    if (!live) return;
    const int rd = (f.flags & kGridRsFy) ? f.ph - 1 - r : r;
    const int cy = a.r.e.coef[0], crr = a.r.e.coef[1], cgb = a.r.e.coef[2], cgr = a.r.e.coef[3], cbb = a.r.e.coef[4];
    const int yoff = a.r.e.coef[5], top = (1 << a.r.e.coef[7]) - 1;
    D o[3 * G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int u = cb[i] - half, w = cr[i] - half;
        const int yy = cy * (yv[i] - yoff) + 8192;
        const int R = min(max((yy + crr * w) >> 14, 0), top);
        const int Gn = min(max((yy - cgb * u - cgr * w) >> 14, 0), top);
        const int B = min(max((yy + cbb * u) >> 14, 0), top);
        o[PACKED ? 3 * i : i] = rs_out<D>(R, a.r.scale[0], a.r.bias[0]);
        o[PACKED ? 3 * i + 1 : G + i] = rs_out<D>(Gn, a.r.scale[1], a.r.bias[1]);
        o[PACKED ? 3 * i + 2 : 2 * G + i] = rs_out<D>(B, a.r.scale[2], a.r.bias[2]);
    }
    if (PACKED) {
        export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)rd * pitch[0]) + 3 * x0, o, 3 * lo, 3 * hi, vec[0]);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)rd * pitch[k]) + x0, o + k * G, lo, hi, vec[k]);
    }
}

// Pass 2: grid_transpose_kernel over the frames of a ragged call.  a.src / a.src_frame are not used: a frame's staged
// R begins at its table entry's dst.  A frame without a quarter turn has nothing staged: its blocks return at once.
// grid (ceil(w[0] / 64), planes * tiles_y, frames), 256 threads.
template <typename U, int C0, int C1>
__global__ __launch_bounds__(256) void grid_resize_transpose_kernel(GridTransposeArgs a, const GridRsFrame* __restrict__ frames) {
    constexpr int CM = C0 > C1 ? C0 : C1;
    __shared__ uint32_t lds[kGridTile * (kGridTile * CM * (int)sizeof(U) / 4 + 1)];
    const GridRsFrame* fp = frames + blockIdx.z;
    if (!(__builtin_amdgcn_readfirstlane(fp->flags) & kGridRsTr)) return;           // (block-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)fp->dst);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(fp->dst >> 32));
    const int k = (int)blockIdx.y / a.tiles_y;                                      // (block-uniform)
    const int x0 = (int)blockIdx.x * kGridTile, y0 = ((int)blockIdx.y - k * a.tiles_y) * kGridTile;
    if (x0 >= a.w[k] || y0 >= a.h[k]) return;
    const U* src = reinterpret_cast<const U*>((uintptr_t)((uint64_t)hi << 32 | lo) + a.src_off[k]);
    U* dst = reinterpret_cast<U*>(a.dst + (uint64_t)blockIdx.z * a.dst_frame + a.dst_off[k]);
    const size_t sp = (size_t)(a.src_pitch[k] / sizeof(U)), dp = (size_t)(a.dst_pitch[k] / sizeof(U));
    if (k == 0) grid_transpose_tile<U, C0>(src, sp, dst, dp, a.w[k], a.h[k], x0, y0, reinterpret_cast<U*>(lds));
    else grid_transpose_tile<U, C1>(src, sp, dst, dp, a.w[k], a.h[k], x0, y0, reinterpret_cast<U*>(lds));
}

}  // namespace p265r
