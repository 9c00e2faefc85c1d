// resize.h -- scaled device-side output (p265r_batch_export_resized): the crop window of every listed picture,
// whatever its size, filtered into a frame slot of one fixed size out_width x out_height and written in the formats
// of export.h.  The arithmetic is the one include/p265r.h states and resize_math.h implements for host and device;
// tests/resize_ref.py restates it in numpy.  No counterpart in the reference.  export.h is used, not changed.
//
// The work is cut as in export.h: a workgroup is 4 waves, one wave per destination row, 64 lanes side by side
// along the row, a lane owns one GROUP of the row (16 destination bytes for YUV, 16 / 8 pixels for RGB), groups
// anchored at the row's first 16-byte boundary and written with export_store.  A workgroup's 4 rows belong to one
// destination plane (the row blocks of the planes follow one another in grid y).  Sizes, steps and boxes of a slot
// come from DevPic::wh through one readfirstlane (export_pic): scalar per slot.
//
// NEAREST / BILINEAR gather their taps: a lane reads the 1 / 4 source samples of each of its outputs, the row's
// vertical taps are wave-uniform.  A large shrink reads only the taps it needs.
//
// AREA reads every source sample under a workgroup's 4 output rows once, with 8-sample loads of consecutive lanes
// (export_load_row: 8 bytes per lane at 8 bits, 16 above): the source columns under the workgroup's output columns
// are walked in chunks of 256 lanes x 8 columns; a lane sums its 8 columns vertically in registers, one set of
// sums per output row (the walk keeps the source row two output rows share in registers), the 4 x 2048 column sums
// go to LDS (32 KB: four workgroups fit a CU's 160 KB), and every lane reduces the columns under its own outputs
// from there with the horizontal weights into 64-bit sums.  A source row shared by two WORKGROUPS' bands is read by
// both.  The division is rs_div (a reciprocal multiply, exact on the whole range: resize_math.h).
#pragma once
#include "export.h"
#include "resize_math.h"

namespace p265r {

struct ResizeArgs {
    ExportArgs e;                // dst, pic_index, layout, crop, coef, shift (fscale is not used)
    int ow, oh;                  // the frame: luma output size
    int grey;                    // semi-planar of a monochrome source: every CbCr element
    float scale[3], bias[3];     // float outputs: fl32(fl32(v * scale) + bias)
};

constexpr int kRsV = 8;                          // AREA: source columns per lane and chunk
constexpr int kRsChunk = 256 * kRsV;             // columns per chunk
constexpr int kRsLds = kExportRows * kRsChunk;   // column sums (uint32_t)

// the vertical taps of one output row (wave-uniform)
struct RsRow {
    int y0, y1, fy;
};
template <int FILTER>
__device__ __forceinline__ RsRow rs_row(const RsAxis& ay, uint32_t hy, int chroma) {
    RsRow r;
    if (FILTER == (int)kRsNearest) {
        r.y0 = r.y1 = rs_nearest(ay, hy, chroma);
        r.fy = 0;
    } else {
        const RsTap t = rs_bilinear(ay, hy, chroma, 1);
        r.y0 = t.i0; r.y1 = t.i1; r.fy = t.f;
    }
    return r;
}
// one gathered output: win = the plane's window origin
template <typename S, int FILTER>
__device__ __forceinline__ int rs_gather(const S* __restrict__ win, size_t stride, const RsAxis& ax, uint32_t hx, int chroma,
                                         const RsRow& r) {
    if (FILTER == (int)kRsNearest) {
        return (int)win[(size_t)r.y0 * stride + (size_t)rs_nearest(ax, hx, chroma)];
    } else {
        const RsTap t = rs_bilinear(ax, hx, chroma, 0);
        const S* r0 = win + (size_t)r.y0 * stride;
        const S* r1 = win + (size_t)r.y1 * stride;
        return rs_blend((int)r0[t.i0], (int)r0[t.i1], (int)r1[t.i0], (int)r1[t.i1], t.f, r.fy);
    }
}

// G gathered outputs of one row: output columns x0 .. x0 + G - 1 (clamped to the row: the caller stores only the
// ones inside), CG = the output is on the chroma grid
template <typename S, int FILTER, int G>
__device__ __forceinline__ void rs_gather_group(const S* __restrict__ win, size_t stride, const RsAxis& ax, const RsAxis& ay,
                                                int chroma, bool cg, int row, int x0, int cols, int* out) {
    const RsRow r = rs_row<FILTER>(ay, (uint32_t)(cg ? 4 * row + 2 : 2 * row + 1), chroma);
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int x = min(max(x0 + i, 0), cols - 1);
        out[i] = rs_gather<S, FILTER>(win, stride, ax, (uint32_t)(cg ? 4 * x + 1 : 2 * x + 1), chroma, r);
    }
}

// AREA: the G outputs x0 .. x0 + G - 1 of output row r0 + wave of one plane, for every lane of the workgroup at
// once (all 256 threads call it: it has block barriers).  win, stride, pw x ph: the plane's window; bx, by: its
// boxes; rows x cols: the plane's outputs; [xlo, xhi): the output columns of the whole workgroup (uniform, not
// empty).  Outputs outside the plane come back as 0.
template <typename S, int G>
__device__ __forceinline__ void rs_area_group(const S* __restrict__ win, size_t stride, int pw, int ph, const RsBox& bx,
                                              const RsBox& by, int r0, int rows, int cols, int xlo, int xhi, int x0,
                                              uint32_t* __restrict__ lds, int* out) {
    const int t = (int)threadIdx.x, wave = t >> 6;
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
        const bool whole = c0 + kRsV <= pw;
        uint32_t acc[kExportRows][kRsV];
        S cur[kRsV];
        uint32_t k = rs_box_first(by, (uint32_t)r0);                               // source row (uniform)
        if (active) export_load_row<S, kRsV>(win + (size_t)k * stride, c0, pw, whole, cur);
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
                        if (active && (int)k < ph) export_load_row<S, kRsV>(win + (size_t)k * stride, c0, pw, whole, cur);
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

// G outputs of one plane row through the instance's filter.  AREA: every thread of the workgroup calls it.
template <typename S, int FILTER, int G>
__device__ __forceinline__ void rs_group(const S* __restrict__ win, size_t stride, int W, int H, const ResizeArgs& a,
                                         int chroma, bool cg, int r0, int x0, int xlo, int xhi, uint32_t* lds, int* out) {
    const int rows = cg ? a.oh >> 1 : a.oh, cols = cg ? a.ow >> 1 : a.ow;
    if constexpr (FILTER == (int)kRsArea) {
        const RsBox bx = rs_box(W, a.ow, chroma, cg), by = rs_box(H, a.oh, chroma, cg);
        rs_area_group<S, G>(win, stride, chroma ? W >> 1 : W, chroma ? H >> 1 : H, bx, by, r0, rows, cols, xlo, xhi, x0, lds, out);
    } else {
        const int row = min(r0 + (int)(threadIdx.x >> 6), rows - 1);
        rs_gather_group<S, FILTER, G>(win, stride, rs_axis(W, a.ow), rs_axis(H, a.oh), chroma, cg, row, x0, cols, out);
    }
}

// the window origin of plane k of a slot's picture
template <typename S>
__device__ __forceinline__ const S* rs_window(const ExportPic& e, const Geo& g, const ExportArgs& a, int k) {
    const int sub = k ? 1 : 0;
    return reinterpret_cast<const S*>(e.P->out[k]) + (size_t)(a.crop_t >> sub) * g.stride[k] + (a.crop_l >> sub);
}

// YUV formats.  grid (ceil(groups of the luma row / 64), row blocks, slots), 256 threads; row blocks of a frame:
// ceil(oh / 4) of luma rows, then -- unless the source is monochrome and the format planar -- ceil(oh / 2 / 4) of
// Cb rows and as many of Cr rows (planar) or of CbCr rows (semi-planar; a monochrome source: grey).
template <typename S, int FILTER>
__global__ __launch_bounds__(256) void resize_yuv_kernel(const DevPic* __restrict__ pics, Geo g, ResizeArgs a, int semi) {
    __shared__ uint32_t lds[FILTER == (int)kRsArea ? kRsLds : 1];
    constexpr int E = 16 / (int)sizeof(S);
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a.e, slot);
    const int nbl = (a.oh + kExportRows - 1) / kExportRows, nbc = ((a.oh >> 1) + kExportRows - 1) / kExportRows;
    int by = blockIdx.y, k = 0;
    if (by >= nbl) {
        by -= nbl;
        k = semi ? 1 : 1 + by / nbc;
        by -= (k - 1) * nbc;
    }
    const int r0 = by * kExportRows, r = r0 + (int)(threadIdx.x >> 6);             // (wave-uniform)
    const int rows = k ? a.oh >> 1 : a.oh;
    const bool pairs = semi && k == 1;                                              // CbCr pairs: E / 2 per group
    const int EU = pairs ? E / 2 : E;
    const int units = pairs || k ? a.ow >> 1 : a.ow;                                // outputs of a row (pairs count once)
    uint8_t* base = a.e.dst + (uint64_t)slot * a.e.frame_bytes + a.e.plane_off[k];
    const int h = pairs ? export_head<2 * (int)sizeof(S)>((uint64_t)(uintptr_t)base)
                        : export_head<(int)sizeof(S)>((uint64_t)(uintptr_t)base);
    const bool vec = h >= 0 && a.e.pitch[k] % 16 == 0;
    const int shiftu = vec && h > 0 ? h - EU : 0;
    const int xb = shiftu + (int)blockIdx.x * kExportLanes * EU;                    // the workgroup's first output
    if (xb >= units) return;                                                        // (uniform)
    const int xlo = max(xb, 0), xhi = min(xb + kExportLanes * EU, units);
    const int u0 = xb + (int)(threadIdx.x & 63) * EU;
    const int lo = max(0, -u0), hi = min(EU, units - u0);
    const bool live = r < rows && u0 < units;
    S v[E];
    if (pairs) {
        constexpr int P = E / 2;
        int cb[P], cr[P];
        if (g.mono) {
#pragma unroll
            for (int i = 0; i < P; ++i) cb[i] = cr[i] = a.grey;
        } else {
            if (FILTER != (int)kRsArea && !live) return;
            rs_group<S, FILTER, P>(rs_window<S>(e, g, a.e, 1), g.stride[1], e.W, e.H, a, 1, true, r0, u0, xlo, xhi, lds, cb);
            rs_group<S, FILTER, P>(rs_window<S>(e, g, a.e, 2), g.stride[1], e.W, e.H, a, 1, true, r0, u0, xlo, xhi, lds, cr);
#pragma unroll
            for (int i = 0; i < P; ++i) { cb[i] <<= a.e.shift; cr[i] <<= a.e.shift; }
        }
        if (!live) return;
#pragma unroll
        for (int i = 0; i < P; ++i) { v[2 * i] = (S)cb[i]; v[2 * i + 1] = (S)cr[i]; }
        export_store<S, E>(reinterpret_cast<S*>(base + (uint64_t)r * a.e.pitch[1]) + 2 * u0, v, 2 * lo, 2 * hi, vec);
    } else {
        if (FILTER != (int)kRsArea && !live) return;
        int o[E];
        rs_group<S, FILTER, E>(rs_window<S>(e, g, a.e, k), g.stride[k], e.W, e.H, a, k ? 1 : 0, k != 0, r0, u0, xlo, xhi, lds, o);
        if (!live) return;
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (S)(o[i] << a.e.shift);
        export_store<S, E>(reinterpret_cast<S*>(base + (uint64_t)r * a.e.pitch[k]) + u0, v, lo, hi, vec);
    }
}

template <typename D>
__device__ __forceinline__ D rs_out(int v, float scale, float bias) {
    if constexpr (sizeof(D) == 4) return rs_norm(v, scale, bias);
    else if constexpr (std::is_same<D, _Float16>::value) return (_Float16)rs_norm(v, scale, bias);
    else return (D)v;
}

// RGB formats.  grid (ceil(groups of a row / 64), ceil(oh / 4), slots), 256 threads: one output row per wave, Y,
// Cb and Cr filtered to the luma grid, then export.h's conversion.  A monochrome source: Cb = Cr = 1 << (B - 1).
template <typename S, typename D, bool PACKED, int FILTER>
__global__ __launch_bounds__(256) void resize_rgb_kernel(const DevPic* __restrict__ pics, Geo g, ResizeArgs a) {
    __shared__ uint32_t lds[FILTER == (int)kRsArea ? kRsLds : 1];
    constexpr int G = sizeof(D) == 1 ? 16 : 8;
    constexpr int UB = (PACKED ? 3 : 1) * (int)sizeof(D);
    constexpr int NP = PACKED ? 1 : 3;
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a.e, slot);
    const int r0 = blockIdx.y * kExportRows, r = r0 + (int)(threadIdx.x >> 6);      // (wave-uniform)
    uint8_t* base[NP];
    bool vec[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) base[k] = a.e.dst + (uint64_t)slot * a.e.frame_bytes + a.e.plane_off[k];
    int h = export_head<UB>((uint64_t)(uintptr_t)base[0]);
    if (h < 0 || a.e.pitch[0] % 16 != 0) h = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        vec[k] = a.e.pitch[k] % 16 == 0 && (((uint64_t)(uintptr_t)base[k] + (uint64_t)(h * UB)) & 15) == 0;
    const int xb = (h > 0 ? h - G : 0) + (int)blockIdx.x * kExportLanes * G;
    if (xb >= a.ow) return;                                                         // (uniform)
    const int xlo = max(xb, 0), xhi = min(xb + kExportLanes * G, a.ow);
    const int x0 = xb + (int)(threadIdx.x & 63) * G;
    const int lo = max(0, -x0), hi = min(G, a.ow - x0);
    const bool live = r < a.oh && x0 < a.ow;
    if (FILTER != (int)kRsArea && !live) return;
    int yv[G], cb[G], cr[G];
    const int half = a.e.coef[6];
    rs_group<S, FILTER, G>(rs_window<S>(e, g, a.e, 0), g.stride[0], e.W, e.H, a, 0, false, r0, x0, xlo, xhi, lds, yv);
    if (g.mono) {
#pragma unroll
        for (int i = 0; i < G; ++i) cb[i] = cr[i] = half;
    } else {
        rs_group<S, FILTER, G>(rs_window<S>(e, g, a.e, 1), g.stride[1], e.W, e.H, a, 1, false, r0, x0, xlo, xhi, lds, cb);
        rs_group<S, FILTER, G>(rs_window<S>(e, g, a.e, 2), g.stride[1], e.W, e.H, a, 1, false, r0, x0, xlo, xhi, lds, cr);
    }
    if (!live) return;
    const int cy = a.e.coef[0], crr = a.e.coef[1], cgb = a.e.coef[2], cgr = a.e.coef[3], cbb = a.e.coef[4];
    const int yoff = a.e.coef[5], top = (1 << a.e.coef[7]) - 1;
    D o[3 * G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int u = cb[i] - half, w = cr[i] - half;
        const int yy = cy * (yv[i] - yoff) + 8192;
        const int R = min(max((yy + crr * w) >> 14, 0), top);
        const int Gn = min(max((yy - cgb * u - cgr * w) >> 14, 0), top);
        const int B = min(max((yy + cbb * u) >> 14, 0), top);
        o[PACKED ? 3 * i : i] = rs_out<D>(R, a.scale[0], a.bias[0]);
        o[PACKED ? 3 * i + 1 : G + i] = rs_out<D>(Gn, a.scale[1], a.bias[1]);
        o[PACKED ? 3 * i + 2 : 2 * G + i] = rs_out<D>(B, a.scale[2], a.bias[2]);
    }
    if (PACKED) {
        export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)r * a.e.pitch[0]) + 3 * x0, o, 3 * lo, 3 * hi, vec[0]);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)r * a.e.pitch[k]) + x0, o + k * G, lo, hi, vec[k]);
    }
}

}  // namespace p265r
