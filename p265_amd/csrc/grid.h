// grid.h -- grid export (p265r_batch_export_grid): rows x cols decoded pictures of a batch assembled into ONE frame,
// cut to a window, converted as export.h converts a picture, and turned / mirrored.  The arithmetic is the one
// include/p265r.h states; tests/grid_ref.py restates it in numpy.  No counterpart in the reference.
//
// Pass 1 (grid_yuv_kernel / grid_rgb_kernel) cuts the work as export.h does -- a wave per destination row unit, a lane
// per 16-byte group anchored at the destination row's first 16-byte boundary -- and reuses its loads, stores and RGB
// arithmetic.  What differs is the source: a row of the CANVAS, found through a device table of the tiles' plane
// addresses (DevPic::out[] of the listed pictures; the tile row is wave-uniform, the tile column per lane).  A group
// that lies inside one tile takes the wide load; one that straddles a tile seam or the canvas edge reads element by
// element, every index clamped to the canvas and resolved to its tile.
// The half turn and the mirror are index reversals: a destination group reads the mirrored source span and reverses
// its elements in registers (a CbCr pair or an RGB triple as one element), rows are reversed by their index, so the
// stores stay 16-byte and contiguous per wave.  The flips are arguments, not template parameters.
// Quarter turns: pass 1 writes the (reversed) frame F into a staging area with 16-byte pitches, pass 2
// (grid_transpose_kernel) transposes every plane through LDS in 64 x 64-element tiles: a wave reads consecutive units
// of a staging row and writes consecutive units of a destination row; nothing gathers a unit per source row.  A tile
// row in LDS is padded by one dword, which makes its stride an odd number of dwords: the 64 lanes that read one
// tile column touch 64 different banks (64 banks of 4 bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "export.h"

namespace p265r {

struct GridArgs {
    ExportArgs e;            // dst / frame_bytes / plane_off / pitch: the destination of pass 1; crop_l / crop_t: the
                             // window's origin on the canvas (crop_r / crop_b and pic_index are not used)
    const uint64_t* tab;     // device: plane addresses [frame][tile][3]
    int rows, cols, tw, th;  // tiles per frame, tile size (luma)
    int W, H;                // the window
    int fx, fy;              // write F reversed along x / y
    int grey;                // monochrome semi-planar: the CbCr value
};

struct GridRow {             // one row of a canvas plane: the table entries of its tile row, the row's sample offset
    const uint64_t* t;
    size_t off;
};

__device__ __forceinline__ GridRow grid_row(const GridArgs& a, const Geo& g, int frame, int k, int y) {
    const int th = k ? a.th >> 1 : a.th;
    const int ty = y / th;                                                      // (wave-uniform)
    GridRow r;
    r.t = a.tab + ((size_t)(frame * a.rows + ty) * (size_t)a.cols) * 3 + k;
    r.off = (size_t)(y - ty * th) * (size_t)g.stride[k];
    return r;
}

// sample x of a canvas plane row (tiles tw wide), x inside the canvas
template <typename S>
__device__ __forceinline__ S grid_at(const GridRow& r, int x, int tw) {
    const int t = x / tw;
    return reinterpret_cast<const S*>(r.t[3 * t])[r.off + (size_t)(x - t * tw)];
}

// samples [x0, x0 + N) of a canvas plane row of width cw: the wide load for a whole group inside one tile, else
// elements with their index clamped to the canvas
template <typename S, int N>
__device__ __forceinline__ void grid_load(const GridRow& r, int x0, int tw, int cw, bool whole, S* v) {
    const int t = x0 / tw;
    if (whole && x0 >= 0 && x0 + N <= cw && (x0 + N - 1) / tw == t) {
        export_load<S, N>(reinterpret_cast<const S*>(r.t[3 * t]) + r.off + (size_t)(x0 - t * tw), v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = grid_at<S>(r, min(max(x0 + i, 0), cw - 1), tw);
    }
}

// reverse the N elements of C units each
template <typename T, int N, int C>
__device__ __forceinline__ void grid_reverse(T* v) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const T x = v[C * i + c];
            v[C * i + c] = v[C * (N - 1 - i) + c];
            v[C * (N - 1 - i) + c] = x;
        }
    }
}

// YUV formats.  grid (ceil(groups of the widest row / 64), ceil(row units / 4), frames), 256 threads; row units of a
// frame: H luma rows, then H/2 Cb and H/2 Cr rows (planar; monochrome: none) or H/2 CbCr rows (semi-planar).
template <typename S, bool SEMI>
__global__ __launch_bounds__(256) void grid_yuv_kernel(Geo g, GridArgs a) {
    const int frame = blockIdx.z;
    const int W = a.W, H = a.H;
    int r = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);                 // (wave-uniform)
    if (r >= (SEMI ? H + H / 2 : (g.mono ? H : 2 * H))) return;
    int k = 0;
    if (r >= H) {
        r -= H; k = 1;
        if (!SEMI && r >= H / 2) { r -= H / 2; k = 2; }
    }
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    uint8_t* base = a.e.dst + (uint64_t)frame * a.e.frame_bytes + a.e.plane_off[k];
    uint8_t* drow = base + (uint64_t)r * a.e.pitch[k];
    const int sub = k ? 1 : 0;
    const int rs = a.fy ? (H >> sub) - 1 - r : r;                               // source row of the window plane
    if (SEMI && k == 1) {
        constexpr int E = 8 / (int)sizeof(S);                                   // CbCr pairs per group
        const int units = W >> 1;
        const int h = export_head<2 * (int)sizeof(S)>((uint64_t)(uintptr_t)base);
        const bool vec = h >= 0 && a.e.pitch[1] % 16 == 0;
        const int u0 = (vec && h > 0 ? h - E : 0) + gi * E;
        if (u0 >= units) return;
        const int lo = max(0, -u0), hi = min(E, units - u0);
        S cb[E], cr[E], v[2 * E];
        if (g.mono) {
#pragma unroll
            for (int i = 0; i < 2 * E; ++i) v[i] = (S)a.grey;
        } else {
            const int xs = (a.e.crop_l >> 1) + (a.fx ? units - u0 - E : u0);    // on the canvas chroma plane
            const int y = (a.e.crop_t >> 1) + rs;
            const GridRow rb = grid_row(a, g, frame, 1, y), rr = grid_row(a, g, frame, 2, y);
            grid_load<S, E>(rb, xs, a.tw >> 1, (a.cols * a.tw) >> 1, lo == 0 && hi == E, cb);
            grid_load<S, E>(rr, xs, a.tw >> 1, (a.cols * a.tw) >> 1, lo == 0 && hi == E, cr);
            if (a.fx) { grid_reverse<S, E, 1>(cb); grid_reverse<S, E, 1>(cr); }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                v[2 * i] = (S)(cb[i] << a.e.shift);
                v[2 * i + 1] = (S)(cr[i] << a.e.shift);
            }
        }
        export_store<S, 2 * E>(reinterpret_cast<S*>(drow) + 2 * u0, v, 2 * lo, 2 * hi, vec);
    } else {
        constexpr int E = 16 / (int)sizeof(S);
        const int units = W >> sub;
        const int h = export_head<(int)sizeof(S)>((uint64_t)(uintptr_t)base);
        const bool vec = h >= 0 && a.e.pitch[k] % 16 == 0;
        const int u0 = (vec && h > 0 ? h - E : 0) + gi * E;
        if (u0 >= units) return;
        const int lo = max(0, -u0), hi = min(E, units - u0);
        const int xs = (a.e.crop_l >> sub) + (a.fx ? units - u0 - E : u0);      // on the canvas plane
        const GridRow rw = grid_row(a, g, frame, k, (a.e.crop_t >> sub) + rs);
        S v[E];
        grid_load<S, E>(rw, xs, a.tw >> sub, (a.cols * a.tw) >> sub, lo == 0 && hi == E, v);
        if (a.fx) grid_reverse<S, E, 1>(v);
        if (sizeof(S) == 2) {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (S)(v[i] << a.e.shift);
        }
        export_store<S, E>(reinterpret_cast<S*>(drow) + u0, v, lo, hi, vec);
    }
}

// RGB formats.  grid (ceil(groups of the widest row / 64), ceil(row pairs / 4), frames), 256 threads.  Row pair p: canvas
// luma rows t + 2 p, t + 2 p + 1 (NEAREST; ceil(H / 2) pairs) or t + 2 p - 1, t + 2 p (BILINEAR: chroma rows clamped to
// the canvas; H / 2 + 1 pairs), as export_rgb_kernel.  A monochrome source runs the NEAREST instance with Cb = Cr =
// 1 << (B - 1) and reads no chroma: R = G = B.
template <typename S, typename D, bool PACKED, bool BIL>
__global__ __launch_bounds__(256) void grid_rgb_kernel(Geo g, GridArgs a) {
    constexpr int G = sizeof(D) == 1 ? 16 : 8;
    constexpr int NC = G / 2 + 1;
    constexpr int UB = (PACKED ? 3 : 1) * (int)sizeof(D);
    constexpr int NP = PACKED ? 1 : 3;
    const int frame = blockIdx.z;
    const int W = a.W, H = a.H;
    const int p = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);           // (wave-uniform)
    if (p >= (BIL ? H / 2 + 1 : (H + 1) / 2)) return;
    const int ya = a.e.crop_t + 2 * p - (BIL ? 1 : 0), yb = ya + 1;
    const bool ok_a = ya >= a.e.crop_t, ok_b = yb < a.e.crop_t + H;
    const int lw = a.cols * a.tw;                                               // canvas luma width
    const int cw = lw >> 1, ch = (a.rows * a.th) >> 1;
    const int j = ya >> 1;                                                      // (-1 >> 1 = -1: clamped below)
    const int j0 = min(max(j, 0), ch - 1), j1 = min(max(j + 1, 0), ch - 1);
    uint8_t* base[NP];
    bool vec[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) base[k] = a.e.dst + (uint64_t)frame * a.e.frame_bytes + a.e.plane_off[k];
    int h = export_head<UB>((uint64_t)(uintptr_t)base[0]);
    if (h < 0 || a.e.pitch[0] % 16 != 0) h = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        vec[k] = a.e.pitch[k] % 16 == 0 && (((uint64_t)(uintptr_t)base[k] + (uint64_t)(h * UB)) & 15) == 0;
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    const int x0 = (h > 0 ? h - G : 0) + gi * G;                                // in the destination row
    if (x0 >= W) return;
    const int lo = max(0, -x0), hi = min(G, W - x0);
    const bool whole = lo == 0 && hi == G;
    const int X0 = a.e.crop_l + (a.fx ? W - x0 - G : x0);                       // the source span on the canvas
    const int ib = X0 >> 1;                                                     // (arithmetic: floor for a negative X0)
    S la[G], lb[G], cb0[NC], cb1[NC], cr0[NC], cr1[NC];
    grid_load<S, G>(grid_row(a, g, frame, 0, ok_a ? ya : yb), X0, a.tw, lw, whole, la);
    grid_load<S, G>(grid_row(a, g, frame, 0, ok_b ? yb : ya), X0, a.tw, lw, whole, lb);
    if (g.mono) {
#pragma unroll
        for (int k = 0; k < NC; ++k) cb0[k] = cr0[k] = cb1[k] = cr1[k] = (S)a.e.coef[6];
    } else {
        auto chroma = [&](int c, int row, S* v) {
            const GridRow rw = grid_row(a, g, frame, c, row);
            grid_load<S, G / 2>(rw, ib, a.tw >> 1, cw, whole, v);
#pragma unroll
            for (int k = G / 2; k < NC; ++k) v[k] = grid_at<S>(rw, min(max(ib + k, 0), cw - 1), a.tw >> 1);
        };
        chroma(1, j0, cb0);
        chroma(2, j0, cr0);
        if (BIL) {
            chroma(1, j1, cb1);
            chroma(2, j1, cr1);
        }
    }
    D oa[3 * G], ob[3 * G];
    if (X0 & 1) {
        export_rgb_row<S, D, PACKED, BIL, G, 1>(la, cb0, cb1, cr0, cr1, 3, 1, a.e, oa);
        export_rgb_row<S, D, PACKED, BIL, G, 1>(lb, cb0, cb1, cr0, cr1, 1, 3, a.e, ob);
    } else {
        export_rgb_row<S, D, PACKED, BIL, G, 0>(la, cb0, cb1, cr0, cr1, 3, 1, a.e, oa);
        export_rgb_row<S, D, PACKED, BIL, G, 0>(lb, cb0, cb1, cr0, cr1, 1, 3, a.e, ob);
    }
    if (a.fx) {
        if (PACKED) {
            grid_reverse<D, G, 3>(oa);
            grid_reverse<D, G, 3>(ob);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { grid_reverse<D, G, 1>(oa + k * G); grid_reverse<D, G, 1>(ob + k * G); }
        }
    }
    int ra = ya - a.e.crop_t, rb = yb - a.e.crop_t;                             // window rows
    if (a.fy) { ra = H - 1 - ra; rb = H - 1 - rb; }
    if (PACKED) {
        if (ok_a) export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)ra * a.e.pitch[0]) + 3 * x0, oa, 3 * lo, 3 * hi, vec[0]);
        if (ok_b) export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)rb * a.e.pitch[0]) + 3 * x0, ob, 3 * lo, 3 * hi, vec[0]);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (ok_a) export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)ra * a.e.pitch[k]) + x0, oa + k * G, lo, hi, vec[k]);
            if (ok_b) export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)rb * a.e.pitch[k]) + x0, ob + k * G, lo, hi, vec[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------
// Pass 2 of a quarter turn: dst plane = transpose of the staged plane, element (C units of U) by element.
// ---------------------------------------------------------------------------------------
constexpr int kGridTile = 64;    // elements per tile side

struct GridTransposeArgs {
    const uint8_t* src;          // staging, frame 0
    uint8_t* dst;
    uint64_t src_frame, dst_frame;
    uint64_t src_off[3], dst_off[3], src_pitch[3], dst_pitch[3];   // bytes
    int w[3], h[3];              // the staged planes' sizes in elements
    int tiles_y;                 // ceil(h[0] / 64): blockIdx.y = plane * tiles_y + tile row
};

template <typename U, int C>
__device__ __forceinline__ void grid_transpose_tile(const U* __restrict__ src, size_t sp, U* __restrict__ dst, size_t dp,
                                                    int w, int h, int x0, int y0, U* tile) {
    constexpr int T = kGridTile, RU = T * C;                                    // units per tile row
    constexpr int RS = (RU * (int)sizeof(U) + 4) / (int)sizeof(U);              // + one dword: an odd dword stride
    for (int idx = (int)threadIdx.x; idx < T * RU; idx += 256) {
        const int ry = idx / RU, cu = idx - ry * RU;
        if (y0 + ry < h && x0 * C + cu < w * C) tile[ry * RS + cu] = src[(size_t)(y0 + ry) * sp + (size_t)(x0 * C + cu)];
    }
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < T * RU; idx += 256) {
        const int oy = idx / RU, ocu = idx - oy * RU;                           // destination row / unit inside the tile
        const int ox = ocu / C, c = ocu - ox * C;
        if (x0 + oy < w && y0 + ox < h) dst[(size_t)(x0 + oy) * dp + (size_t)((y0 + ox) * C + c)] = tile[ox * RS + oy * C + c];
    }
}

// grid (ceil(w[0] / 64), planes * tiles_y, frames), 256 threads.  Plane 0 has C0 units per element, the others C1.
template <typename U, int C0, int C1>
__global__ __launch_bounds__(256) void grid_transpose_kernel(GridTransposeArgs a) {
    constexpr int CM = C0 > C1 ? C0 : C1;
    __shared__ uint32_t lds[kGridTile * (kGridTile * CM * (int)sizeof(U) / 4 + 1)];
    const int k = (int)blockIdx.y / a.tiles_y;                                  // (block-uniform)
    const int x0 = (int)blockIdx.x * kGridTile, y0 = ((int)blockIdx.y - k * a.tiles_y) * kGridTile;
    if (x0 >= a.w[k] || y0 >= a.h[k]) return;
    const U* src = reinterpret_cast<const U*>(a.src + (uint64_t)blockIdx.z * a.src_frame + a.src_off[k]);
    U* dst = reinterpret_cast<U*>(a.dst + (uint64_t)blockIdx.z * a.dst_frame + a.dst_off[k]);
    const size_t sp = (size_t)(a.src_pitch[k] / sizeof(U)), dp = (size_t)(a.dst_pitch[k] / sizeof(U));
    if (k == 0) grid_transpose_tile<U, C0>(src, sp, dst, dp, a.w[k], a.h[k], x0, y0, reinterpret_cast<U*>(lds));
    else grid_transpose_tile<U, C1>(src, sp, dst, dp, a.w[k], a.h[k], x0, y0, reinterpret_cast<U*>(lds));
}

}  // namespace p265r
