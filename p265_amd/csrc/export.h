// export.h -- device-side output (p265r_batch_export): the decoded planes of a batch (DevPic::out[]),
// cropped to the conformance window and written into caller-owned device memory as planar / semi-planar
// YUV or planar / packed RGB.  The arithmetic is the one include/p265r.h states; tests/export_ref.py
// restates it in numpy.  No counterpart in the reference.
//
// Streaming kernels, no LDS, nothing shared between workgroups.  A workgroup is 4 waves, one wave per
// row unit (YUV: one destination plane row; RGB: the two luma rows that share a chroma row pair, so
// chroma is read once), 64 lanes side by side along the row.  A lane owns one GROUP of a row:
//   YUV   16 destination bytes (16 / 8 samples; semi-planar chroma 8 / 4 CbCr pairs)
//   RGB   16 pixels for uint8 output, 8 for uint16 / fp16 / fp32 (16 .. 96 bytes per row)
// The groups of a row are anchored at the row's first 16-byte boundary: group 0 is the element-wise
// head before it, the last group the element-wise tail, every group between is written with 16-byte
// stores.  That needs the plane's pitch to be a multiple of 16 (every row then has the same head) and,
// for the second and third RGB plane, the same phase as the first (a lane's pixels are the same in all
// three); a plane that fails either is written element by element -- still one lane per group, so the
// stores of a wave stay contiguous.  The source is read with the widest load its address allows (16, 8,
// 4, 2 or 1 bytes: the crop origin and the head shift it off alignment); partial groups read element by
// element with clamped indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "intra.h"

namespace p265r {

struct ExportArgs {
    uint8_t* dst;                // frame slot 0
    const int32_t* pic_index;    // device: slot -> picture of the batch; nullptr = identity
    uint64_t frame_bytes, plane_off[3], pitch[3];
    int crop_l, crop_r, crop_t, crop_b;
    int coef[8];                 // p265r_export_coefficients (RGB)
    float fscale;                // float(1 / (2^B - 1)) (F16 / F32)
    int shift;                   // 16 - B for MSB16, else 0 (YUV)
};

constexpr int kExportRows = 4;   // row units (waves) per workgroup
constexpr int kExportLanes = 64; // groups per workgroup along a row

// N samples from p with the widest loads p's alignment allows
template <typename T, int N>
__device__ __forceinline__ void export_load(const T* __restrict__ p, T* v) {
    constexpr int BYTES = N * (int)sizeof(T), WORDS = BYTES / 4;
    static_assert(BYTES % 4 == 0, "a group is whole dwords");
    uint32_t w[WORDS];
    const uint32_t a = (uint32_t)(uintptr_t)p;
    if (BYTES % 16 == 0 && a % 16 == 0) {
#pragma unroll
        for (int k = 0; k < WORDS / 4; ++k) {
            const uint4 q = reinterpret_cast<const uint4*>(p)[k];
            w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
        }
    } else if (BYTES % 8 == 0 && a % 8 == 0) {
#pragma unroll
        for (int k = 0; k < WORDS / 2; ++k) {
            const uint2 q = reinterpret_cast<const uint2*>(p)[k];
            w[2 * k] = q.x; w[2 * k + 1] = q.y;
        }
    } else if (a % 4 == 0) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
    } else if (a % 2 == 0) {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int k = 0; k < WORDS; ++k) w[k] = (uint32_t)h[2 * k] | (uint32_t)h[2 * k + 1] << 16;
    } else {
        const uint8_t* c = reinterpret_cast<const uint8_t*>(p);
#pragma unroll
        for (int k = 0; k < WORDS; ++k)
            w[k] = (uint32_t)c[4 * k] | (uint32_t)c[4 * k + 1] << 8 | (uint32_t)c[4 * k + 2] << 16 | (uint32_t)c[4 * k + 3] << 24;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        constexpr int PER = 4 / (int)sizeof(T);
        v[i] = (T)(w[i / PER] >> (8 * (int)sizeof(T) * (i % PER)));
    }
}

// samples [x0, x0 + N) of a row of `width`: the wide load for a whole group, else index-clamped elements
template <typename T, int N>
__device__ __forceinline__ void export_load_row(const T* __restrict__ row, int x0, int width, bool whole, T* v) {
    if (whole) {
        export_load<T, N>(row + x0, v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = row[min(max(x0 + i, 0), width - 1)];
    }
}

// elements [lo, hi) of the N at p: 16-byte stores when the group is whole and its plane allows them
template <typename D, int N>
__device__ __forceinline__ void export_store(D* __restrict__ p, const D* v, int lo, int hi, bool vec) {
    constexpr int BYTES = N * (int)sizeof(D);
    static_assert(BYTES % 16 == 0, "a group is whole 16-byte vectors");
    if (vec && lo == 0 && hi == N) {
        uint32_t w[BYTES / 4];
        __builtin_memcpy(w, v, BYTES);
#pragma unroll
        for (int k = 0; k < BYTES / 16; ++k)
            reinterpret_cast<uint4*>(p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i >= lo && i < hi) p[i] = v[i];
    }
}

// units of UB bytes before the first 16-byte boundary at or after address a; -1: no unit starts on one
template <int UB>
__device__ __forceinline__ int export_head(uint64_t a) {
    for (int h = 0; h < 16; ++h)
        if (((a + (uint64_t)(h * UB)) & 15) == 0) return h;
    return -1;
}

// slot -> picture of the batch, its decoded and its cropped size
struct ExportPic {
    const DevPic* P;
    int pw, ph, W, H;
};
__device__ __forceinline__ ExportPic export_pic(const DevPic* __restrict__ pics, const ExportArgs& a, int slot) {
    const int pic = a.pic_index ? a.pic_index[slot] : slot;
    ExportPic e;
    e.P = pics + pic;
    const uint32_t wh = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.P->wh);
    e.pw = (int)(wh & 0xffffu);
    e.ph = (int)(wh >> 16);
    e.W = e.pw - a.crop_l - a.crop_r;
    e.H = e.ph - a.crop_t - a.crop_b;
    return e;
}

// YUV formats.  grid (ceil(groups of the widest row / 64), ceil(row units / 4), slots), 256 threads; row units of
// a picture: H luma rows, then H/2 Cb rows and H/2 Cr rows (planar) or H/2 CbCr rows (semi-planar).
template <typename S, bool SEMI>
__global__ __launch_bounds__(256) void export_yuv_kernel(const DevPic* __restrict__ pics, Geo g, ExportArgs a) {
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a, slot);
    int r = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);                 // (wave-uniform)
    if (r >= (SEMI ? e.H + e.H / 2 : 2 * e.H)) return;
    int k = 0;
    if (r >= e.H) {
        r -= e.H; k = 1;
        if (!SEMI && r >= e.H / 2) { r -= e.H / 2; k = 2; }
    }
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    uint8_t* base = a.dst + (uint64_t)slot * a.frame_bytes + a.plane_off[k];
    uint8_t* drow = base + (uint64_t)r * a.pitch[k];
    if (SEMI && k == 1) {
        constexpr int E = 8 / (int)sizeof(S);                                   // CbCr pairs per group
        const int units = e.W >> 1;
        const int h = export_head<2 * (int)sizeof(S)>((uint64_t)(uintptr_t)base);
        const bool vec = h >= 0 && a.pitch[1] % 16 == 0;
        const int u0 = (vec && h > 0 ? h - E : 0) + gi * E;
        if (u0 >= units) return;
        const int lo = max(0, -u0), hi = min(E, units - u0);
        const size_t so = (size_t)((a.crop_t >> 1) + r) * g.stride[1] + (a.crop_l >> 1);
        S cb[E], cr[E], v[2 * E];
        export_load_row<S, E>(reinterpret_cast<const S*>(e.P->out[1]) + so, u0, units, lo == 0 && hi == E, cb);
        export_load_row<S, E>(reinterpret_cast<const S*>(e.P->out[2]) + so, u0, units, lo == 0 && hi == E, cr);
#pragma unroll
        for (int i = 0; i < E; ++i) {
            v[2 * i] = (S)(cb[i] << a.shift);
            v[2 * i + 1] = (S)(cr[i] << a.shift);
        }
        export_store<S, 2 * E>(reinterpret_cast<S*>(drow) + 2 * u0, v, 2 * lo, 2 * hi, vec);
    } else {
        constexpr int E = 16 / (int)sizeof(S);
        const int sub = k ? 1 : 0;
        const int units = e.W >> sub;
        const int h = export_head<(int)sizeof(S)>((uint64_t)(uintptr_t)base);
        const bool vec = h >= 0 && a.pitch[k] % 16 == 0;
        const int u0 = (vec && h > 0 ? h - E : 0) + gi * E;
        if (u0 >= units) return;
        const int lo = max(0, -u0), hi = min(E, units - u0);
        const size_t so = (size_t)((a.crop_t >> sub) + r) * g.stride[k] + (a.crop_l >> sub);
        S v[E];
        export_load_row<S, E>(reinterpret_cast<const S*>(e.P->out[k]) + so, u0, units, lo == 0 && hi == E, v);
        if (sizeof(S) == 2) {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (S)(v[i] << a.shift);
        }
        export_store<S, E>(reinterpret_cast<S*>(drow) + u0, v, lo, hi, vec);
    }
}

template <typename D>
__device__ __forceinline__ D export_sample(int v, float fscale) {
    if constexpr (sizeof(D) == 4) return (float)v * fscale;
    else if constexpr (std::is_same<D, _Float16>::value) {
        // F16 is the F32 value rounded again: keep the product in an fp32 register of its own, or the compiler
        // folds multiply and conversion into v_fma_mixlo_f16, which rounds the exact product once
        float f = (float)v * fscale;
        asm volatile("" : "+v"(f));
        return (_Float16)f;
    }
    else return (D)v;
}

// One output row of a lane's G pixels.  PAR = parity of the group's first luma x in the decoded picture; c0 / c1:
// the two chroma rows (NEAREST: c0 only) from column x0 >> 1 on; w0 / w1: their vertical weights (3, 1 / 1, 3).
template <typename S, typename D, bool PACKED, bool BIL, int G, int PAR>
__device__ __forceinline__ void export_rgb_row(const S* y, const S* cb0, const S* cb1, const S* cr0, const S* cr1,
                                               int w0, int w1, const ExportArgs& a, D* o) {
    constexpr int NC = G / 2 + 1;
    int ub[NC], vr[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        ub[k] = BIL ? w0 * (int)cb0[k] + w1 * (int)cb1[k] : (int)cb0[k];
        vr[k] = BIL ? w0 * (int)cr0[k] + w1 * (int)cr1[k] : (int)cr0[k];
    }
    const int cy = a.coef[0], crr = a.coef[1], cgb = a.coef[2], cgr = a.coef[3], cbb = a.coef[4];
    const int yoff = a.coef[5], half = a.coef[6], top = (1 << a.coef[7]) - 1;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int ci = (PAR + i) >> 1;
        const bool odd = ((PAR + i) & 1) != 0;
        int cb, cr;
        if (!BIL) { cb = ub[ci]; cr = vr[ci]; }
        else if (odd) { cb = (ub[ci] + ub[ci + 1] + 4) >> 3; cr = (vr[ci] + vr[ci + 1] + 4) >> 3; }
        else { cb = (ub[ci] + 2) >> 2; cr = (vr[ci] + 2) >> 2; }
        cb -= half; cr -= half;
        const int yy = cy * ((int)y[i] - yoff) + 8192;
        const int R = min(max((yy + crr * cr) >> 14, 0), top);
        const int Gn = min(max((yy - cgb * cb - cgr * cr) >> 14, 0), top);
        const int B = min(max((yy + cbb * cb) >> 14, 0), top);
        o[PACKED ? 3 * i : i] = export_sample<D>(R, a.fscale);
        o[PACKED ? 3 * i + 1 : G + i] = export_sample<D>(Gn, a.fscale);
        o[PACKED ? 3 * i + 2 : 2 * G + i] = export_sample<D>(B, a.fscale);
    }
}

// RGB formats.  grid (ceil(groups of the widest row / 64), ceil(row pairs / 4), slots), 256 threads.  Row pair p of a
// picture: decoded luma rows t + 2 p, t + 2 p + 1 (NEAREST: chroma row (t >> 1) + p) or t + 2 p - 1, t + 2 p
// (BILINEAR: chroma rows (t >> 1) + p - 1 and + p, clamped to the decoded picture; H / 2 + 1 pairs, the first and
// last with one row inside the window).
template <typename S, typename D, bool PACKED, bool BIL>
__global__ __launch_bounds__(256) void export_rgb_kernel(const DevPic* __restrict__ pics, Geo g, ExportArgs a) {
    constexpr int G = sizeof(D) == 1 ? 16 : 8;
    constexpr int NC = G / 2 + 1;
    constexpr int UB = (PACKED ? 3 : 1) * (int)sizeof(D);
    constexpr int NP = PACKED ? 1 : 3;
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a, slot);
    const int p = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);           // (wave-uniform)
    if (p >= e.H / 2 + (BIL ? 1 : 0)) return;
    const int ya = a.crop_t + 2 * p - (BIL ? 1 : 0), yb = ya + 1;
    const bool ok_a = ya >= a.crop_t, ok_b = yb < a.crop_t + e.H;
    const int cw = e.pw >> 1, ch = e.ph >> 1;
    const int j = ya >> 1;                                                      // (-1 >> 1 = -1: clamped below)
    const int j0 = min(max(j, 0), ch - 1), j1 = min(max(j + 1, 0), ch - 1);
    // the planes' bases in this slot, the head of plane 0 and which planes take 16-byte stores
    uint8_t* base[NP];
    bool vec[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) base[k] = a.dst + (uint64_t)slot * a.frame_bytes + a.plane_off[k];
    int h = export_head<UB>((uint64_t)(uintptr_t)base[0]);
    if (h < 0 || a.pitch[0] % 16 != 0) h = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        vec[k] = a.pitch[k] % 16 == 0 && (((uint64_t)(uintptr_t)base[k] + (uint64_t)(h * UB)) & 15) == 0;
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    const int x0 = (h > 0 ? h - G : 0) + gi * G;                                // in the window
    if (x0 >= e.W) return;
    const int lo = max(0, -x0), hi = min(G, e.W - x0);
    const bool whole = lo == 0 && hi == G;
    const int X0 = a.crop_l + x0;                                               // in the decoded picture
    const int ib = X0 >> 1;
    const S* Y = reinterpret_cast<const S*>(e.P->out[0]);
    const S* Cb = reinterpret_cast<const S*>(e.P->out[1]);
    const S* Cr = reinterpret_cast<const S*>(e.P->out[2]);
    S la[G], lb[G], cb0[NC], cb1[NC], cr0[NC], cr1[NC];
    export_load_row<S, G>(Y + (size_t)(ok_a ? ya : yb) * g.stride[0], X0, e.pw, whole, la);
    export_load_row<S, G>(Y + (size_t)(ok_b ? yb : ya) * g.stride[0], X0, e.pw, whole, lb);
    auto chroma = [&](const S* plane, int row, S* c) {
        const S* src = plane + (size_t)row * g.stride[1];
        const bool wide = whole && ib >= 0 && ib + G / 2 <= cw;
        export_load_row<S, G / 2>(src, ib, cw, wide, c);
#pragma unroll
        for (int k = G / 2; k < NC; ++k) c[k] = src[min(max(ib + k, 0), cw - 1)];
    };
    chroma(Cb, j0, cb0);
    chroma(Cr, j0, cr0);
    if (BIL) {
        chroma(Cb, j1, cb1);
        chroma(Cr, j1, cr1);
    }
    D oa[3 * G], ob[3 * G];
    if (X0 & 1) {
        export_rgb_row<S, D, PACKED, BIL, G, 1>(la, cb0, cb1, cr0, cr1, 3, 1, a, oa);
        export_rgb_row<S, D, PACKED, BIL, G, 1>(lb, cb0, cb1, cr0, cr1, 1, 3, a, ob);
    } else {
        export_rgb_row<S, D, PACKED, BIL, G, 0>(la, cb0, cb1, cr0, cr1, 3, 1, a, oa);
        export_rgb_row<S, D, PACKED, BIL, G, 0>(lb, cb0, cb1, cr0, cr1, 1, 3, a, ob);
    }
    const int ra = ya - a.crop_t, rb = yb - a.crop_t;                           // window rows
    if (PACKED) {
        if (ok_a) export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)ra * a.pitch[0]) + 3 * x0, oa, 3 * lo, 3 * hi, vec[0]);
        if (ok_b) export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)rb * a.pitch[0]) + 3 * x0, ob, 3 * lo, 3 * hi, vec[0]);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (ok_a) export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)ra * a.pitch[k]) + x0, oa + k * G, lo, hi, vec[k]);
            if (ok_b) export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)rb * a.pitch[k]) + x0, ob + k * G, lo, hi, vec[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------
// Monochrome sources (Geo::mono, 4:0:0): the same groups, heads and stores; no chroma plane exists or is read.
// ---------------------------------------------------------------------------------------
// YUV.  Row units of a picture: H luma rows (planar: one plane, that is all), then -- semi-planar -- H / 2 CbCr rows
// of W elements, every one `grey` = (1 << (B - 1)) << shift: grey NV12 / P010 for consumers that take nothing else.
template <typename S, bool SEMI>
__global__ __launch_bounds__(256) void export_mono_yuv_kernel(const DevPic* __restrict__ pics, Geo g, ExportArgs a, int grey) {
    constexpr int E = 16 / (int)sizeof(S);
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a, slot);
    int r = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);                 // (wave-uniform)
    if (r >= (SEMI ? e.H + e.H / 2 : e.H)) return;
    const int k = r >= e.H ? 1 : 0;
    if (k) r -= e.H;
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    uint8_t* base = a.dst + (uint64_t)slot * a.frame_bytes + a.plane_off[k];
    uint8_t* drow = base + (uint64_t)r * a.pitch[k];
    const int units = e.W;                                                      // luma samples / W / 2 CbCr pairs
    const int h = export_head<(int)sizeof(S)>((uint64_t)(uintptr_t)base);
    const bool vec = h >= 0 && a.pitch[k] % 16 == 0;
    const int u0 = (vec && h > 0 ? h - E : 0) + gi * E;
    if (u0 >= units) return;
    const int lo = max(0, -u0), hi = min(E, units - u0);
    S v[E];
    if (k) {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (S)grey;
    } else {
        const size_t so = (size_t)(a.crop_t + r) * g.stride[0] + a.crop_l;
        export_load_row<S, E>(reinterpret_cast<const S*>(e.P->out[0]) + so, u0, units, lo == 0 && hi == E, v);
        if (sizeof(S) == 2) {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (S)(v[i] << a.shift);
        }
    }
    export_store<S, E>(reinterpret_cast<S*>(drow) + u0, v, lo, hi, vec);
}

// RGB: R = G = B = Clip((cy (Y - yoff) + 8192) >> 14), the formula of export_rgb_row at Cb = Cr = 1 << (B - 1).
// grid (ceil(groups of the widest row / 64), ceil(rows / 4), slots): one window row per wave.
template <typename S, typename D, bool PACKED>
__global__ __launch_bounds__(256) void export_mono_rgb_kernel(const DevPic* __restrict__ pics, Geo g, ExportArgs a) {
    constexpr int G = sizeof(D) == 1 ? 16 : 8;
    constexpr int UB = (PACKED ? 3 : 1) * (int)sizeof(D);
    constexpr int NP = PACKED ? 1 : 3;
    const int slot = blockIdx.z;
    const ExportPic e = export_pic(pics, a, slot);
    const int r = blockIdx.y * kExportRows + (int)(threadIdx.x >> 6);           // (wave-uniform)
    if (r >= e.H) return;
    uint8_t* base[NP];
    bool vec[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) base[k] = a.dst + (uint64_t)slot * a.frame_bytes + a.plane_off[k];
    int h = export_head<UB>((uint64_t)(uintptr_t)base[0]);
    if (h < 0 || a.pitch[0] % 16 != 0) h = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        vec[k] = a.pitch[k] % 16 == 0 && (((uint64_t)(uintptr_t)base[k] + (uint64_t)(h * UB)) & 15) == 0;
    const int gi = blockIdx.x * kExportLanes + (int)(threadIdx.x & 63);
    const int x0 = (h > 0 ? h - G : 0) + gi * G;                                // in the window
    if (x0 >= e.W) return;
    const int lo = max(0, -x0), hi = min(G, e.W - x0);
    const S* Y = reinterpret_cast<const S*>(e.P->out[0]) + (size_t)(a.crop_t + r) * g.stride[0] + a.crop_l;
    S la[G];
    export_load_row<S, G>(Y, x0, e.W, lo == 0 && hi == G, la);
    const int cy = a.coef[0], yoff = a.coef[5], top = (1 << a.coef[7]) - 1;
    D o[3 * G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const D d = export_sample<D>(min(max((cy * ((int)la[i] - yoff) + 8192) >> 14, 0), top), a.fscale);
        o[PACKED ? 3 * i : i] = d;
        o[PACKED ? 3 * i + 1 : G + i] = d;
        o[PACKED ? 3 * i + 2 : 2 * G + i] = d;
    }
    if (PACKED) {
        export_store<D, 3 * G>(reinterpret_cast<D*>(base[0] + (uint64_t)r * a.pitch[0]) + 3 * x0, o, 3 * lo, 3 * hi, vec[0]);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            export_store<D, G>(reinterpret_cast<D*>(base[k] + (uint64_t)r * a.pitch[k]) + x0, o + k * G, lo, hi, vec[k]);
    }
}

}  // namespace p265r
