// resize_math.h -- the arithmetic of the scaled device-side output (p265r_batch_export_resized), shared by the
// host (resize_host.cpp, tools/resize_check.cpp) and the device (resize.h): the position rule of the gathered
// filters, the area weights and the division.  Plain C++: no HIP types, no inline assembly; RESIZE_FN carries the
// qualifiers.  include/p265r.h states the same arithmetic in words; tests/resize_ref.py restates it.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define RESIZE_FN __host__ __device__ inline
#else
#define RESIZE_FN inline
#endif

constexpr uint32_t kRsNearest = 0, kRsBilinear = 1, kRsArea = 2;
constexpr int kRsMaxOut = 16384;      // largest output length
constexpr int kRsMaxWindow = 32767;   // largest window of the gathered filters: (n << 16) and h * step fit 32 bits
constexpr int kRsMaxArea = 8192;      // largest window of the area filter: sum < 2^38, Nx Ny <= 2^26

// One axis of one slot: n, m = luma window and output length
struct RsAxis {
    uint32_t n, m, step;              // step = floor((n << 16) / m)
};
RESIZE_FN RsAxis rs_axis(int n, int m) {
    RsAxis a;
    a.n = (uint32_t)n; a.m = (uint32_t)m;
    a.step = ((uint32_t)n << 16) / (uint32_t)m;
    return a;
}
// U(h): the source position x 2^16 in luma samples from the window's edge
RESIZE_FN uint32_t rs_u(const RsAxis& a, uint32_t h) { return (h * a.step) >> 1; }

// NEAREST: the index in a luma (chroma = 0) or chroma plane
RESIZE_FN int rs_nearest(const RsAxis& a, uint32_t h, int chroma) {
    const uint32_t i = rs_u(a, h) >> 16;
    const uint32_t np = chroma ? a.n >> 1 : a.n;
    const uint32_t k = chroma ? i >> 1 : i;
    return (int)(k < np - 1 ? k : np - 1);
}

// BILINEAR: taps i0, i1 and the 8-bit fraction
struct RsTap {
    int i0, i1, f;
};
RESIZE_FN RsTap rs_bilinear(const RsAxis& a, uint32_t h, int chroma, int vertical) {
    const int32_t u = (int32_t)rs_u(a, h);
    const int32_t np = (int32_t)(chroma ? a.n >> 1 : a.n);
    int32_t pos = !chroma ? u - 32768 : ((u - (vertical ? 65536 : 32768)) >> 1);
    const int32_t top = (np - 1) << 16;
    pos = pos < 0 ? 0 : (pos > top ? top : pos);
    RsTap t;
    t.i0 = pos >> 16;
    t.i1 = t.i0 + 1 < np ? t.i0 + 1 : np - 1;
    t.f = (pos >> 8) & 255;
    return t;
}
RESIZE_FN int rs_blend(int a, int b, int c, int d, int fx, int fy) {
    return (((256 - fx) * a + fx * b) * (256 - fy) + ((256 - fx) * c + fx * d) * fy + 32768) >> 16;
}

// AREA, one axis: output i covers [i N, (i + 1) N), plane sample k covers [k M, (k + 1) M), in units of 1 / m of a
// luma sample.  luma plane on the luma grid: N = n, M = m; chroma plane on the luma grid: N = n, M = 2 m; chroma
// plane on the chroma grid: N = n / 2, M = m / 2.  (samples of the plane) x M = (outputs) x N.
struct RsBox {
    uint32_t N, M;
};
RESIZE_FN RsBox rs_box(int n, int m, int chroma_plane, int chroma_grid) {
    RsBox b;
    if (chroma_grid) { b.N = (uint32_t)n >> 1; b.M = (uint32_t)m >> 1; }
    else { b.N = (uint32_t)n; b.M = chroma_plane ? 2u * (uint32_t)m : (uint32_t)m; }
    return b;
}
// first sample under output i
RESIZE_FN uint32_t rs_box_first(const RsBox& b, uint32_t i) { return i * b.N / b.M; }
// overlap of sample k with output i (0 when they do not meet)
RESIZE_FN uint32_t rs_box_weight(const RsBox& b, uint32_t i, uint32_t k) {
    const uint32_t lo0 = i * b.N, hi0 = lo0 + b.N, lo1 = k * b.M, hi1 = lo1 + b.M;
    const uint32_t lo = lo0 > lo1 ? lo0 : lo1, hi = hi0 < hi1 ? hi0 : hi1;
    return hi > lo ? hi - lo : 0;
}

// The division of the area filter by a reciprocal.  d = Nx Ny in 1 .. 2^26; x = sum + (d >> 1) < 2^12 d (the
// samples are at most 4095).  rcp = ceil(2^64 / d) = 2^64 / d + e, 0 <= e < 1 (d = 1: 0, and the quotient is x).
// mulhi(x, rcp) = floor(x / d + x e / 2^64); x e / 2^64 < 2^12 d / 2^64 <= 1 / d as d^2 <= 2^52, and the
// fractional part of x / d is at most 1 - 1 / d: the floor is that of x / d.  (At d = 2^26 e = 0.)
struct RsDiv {
    uint64_t rcp, d;
};
RESIZE_FN RsDiv rs_div_make(uint32_t nx, uint32_t ny) {
    RsDiv r;
    r.d = (uint64_t)nx * ny;
    r.rcp = r.d > 1 ? ~0ull / r.d + 1 : 0;      // (2^64 - 1) / d + 1 = ceil(2^64 / d): also when d divides 2^64
    return r;
}
RESIZE_FN uint64_t rs_mulhi(uint64_t a, uint64_t b) {
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
}
RESIZE_FN uint32_t rs_div(const RsDiv& r, uint64_t sum) {
    const uint64_t x = sum + (r.d >> 1);
    return (uint32_t)(r.d > 1 ? rs_mulhi(x, r.rcp) : x);
}

// float outputs: two separately rounded fp32 operations, never one fma
RESIZE_FN float rs_norm(int v, float scale, float bias) {
#if defined(__clang__)
    // the plain operators under this pragma carry no contract flag, on host and device; __fmul_rn / __fadd_rn are
    // header functions compiled under the translation unit's own mode (fast for HIP), which may fuse after inlining
#pragma clang fp contract(off)
    const float p = (float)v * scale;
    return p + bias;
#else
    volatile float p = (float)v * scale;        // (volatile: no fusing whatever -ffp-contract says)
    return p + bias;
#endif
}
