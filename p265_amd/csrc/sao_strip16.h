// SAO-only in-loop filter pass (H.265 8.7.3), CTB 32 / 64 without deblocking: a streaming strip
// kernel with 16 samples per lane.  (CTB 16 keeps sao_rows.h, whose 4-sample lanes never straddle
// an 8-sample chroma CTB; batches with deblocking the fused window kernel of loopfilter.h.)  The
// reference parses the SAO syntax (decoder/sao.py:15-136) and never filters.
//
// The strip walk of sao.h with 16 samples per lane, 992-sample strips.  Every row is ONE coalesced 1-KB load per wave instruction (the per-CTB layout of a row group would
// touch 16 half cache lines per instruction, which measured texture-addresser bound); the wave walks
// down its CTB row K rows at a time, the next K rows loaded before the current ones are filtered.
// A lane's 16 samples lie in one CTB (16 | CTB width), so its SaoTypeIdx, class and offsets are
// per-lane constants; the neighbours a, b of edge offset are selected per lane (v_cndmask on the
// class) and byte-aligned with one v_alignbyte each, the dwords beside the lane's column come from
// lanes l -/+ 1 (DPP wave shifts).  4 samples per dword in two packed 16-bit halves: sgn by clamped
// packed subtraction, the SaoOffsetVal table looked up with one v_perm_b32 per half, saturation by
// packed min.  (Measured against a class-uniform one-wave-per-CTB layout -- 16 lanes per row group,
// every load touching 16 half cache lines: texture-addresser bound, 1.09 vs 0.85 ms per 512 1080p
// pictures.)
// HBM traffic per sample: one read (+ 2 halo rows per CTB height) and one write.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/p265r.h"
#include "intra.h"
#include "loopfilter.h"
#include "sao.h"

namespace p265r {

__device__ __forceinline__ uint32_t pk_sub_i16(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_sub_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
// clamp each signed 16-bit half to [-1, 1]
__device__ __forceinline__ uint32_t pk_sgn_i16(uint32_t d) {
    uint32_t r;
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(d), "v"(0xffffffffu));
    asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(r), "v"(0x00010001u));
    return r;
}

// 16-bit ok mask (bit i: sample i of the lane's 16 may change) -> 4 dword byte masks
__device__ __forceinline__ void expand_mask(uint32_t m16, uint32_t* d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t b = ((m16 >> (4 * j)) & 0xfu) * 0x00204081u & 0x01010101u;   // bit k -> byte k (24-bit mul)
        d[j] = bytes_ff(b);
    }
}

constexpr int kSao16Wpe = 6;               // the kernel's waves-per-SIMD attribute
// rows per load batch: 2 (80 VGPRs, 6 waves per SIMD) rather than 4 (100 VGPRs): 0.74 -> 0.77 ms
// alone, but two SAO waves per SIMD fit beside the W = 8 row kernel of another lane: pipelined
// 46.9-47.1 -> 47.0-48.0 M CTU/s (3 interleaved reps, round 3)
constexpr int kSao16Chunk = 2;

// grid: 4 waves per block, one wave per (picture, CTB row, component, 992-sample strip), XCD-aware
// order (sao.h strip_pos)
template <int L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kSao16Wpe))) void sao_strip16_kernel(
        const DevPic* __restrict__ pics, Geo gb, BatchView v, int n_pics) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) uint8_t gu8;
    const StripPos p = strip_pos<16>(pics, gb, n_pics, L);
    if (p.outside) return;                                        // whole wave (no barriers below)
    const Geo& g = p.g;
    const int pic = p.pic, c = p.c, sub = p.sub, H = p.H, st = p.st;
    const int Xc = p.Xc, yb = p.yb, ye = p.ye;
    const bool act = p.act;
    // CTU records: slots of the context size; a ragged batch's smaller picture uses its own raster
    const p265r_ctu* crec = v.ctus0 + (size_t)pic * gb.wc * gb.hc;
    const uint64_t pofs = (uint64_t)pic * v.pic_bytes + v.plane_off[c];
    const gu8* src = (const gu8*)(v.rec0 + pofs);
    gu8* dst = (gu8*)(v.out0 + pofs);
    auto row_ld = [&](int y) {
        return *(const __attribute__((address_space(1))) u4v*)(src + __umul24((uint32_t)min(max(y, 0), H - 1), (uint32_t)st) + Xc);
    };
    // ---- first: the rows of the first chunk (position only) ----------------------------------
    constexpr int K = kSao16Chunk;
    u4v rowv[K + 2], nxt[K];
#pragma unroll
    for (int k = 0; k < K + 2; ++k) rowv[k] = row_ld(yb - 1 + k);

    // ---- this lane's CTB: SAO parameters, 8.7.3.2 permissions of its 3x3 neighbourhood ----------
    const SaoCtb ctb = sao_lane_ctb(crec, g, p.cy, p.bx, c);
    const uint8_t* nf = pics[pic].nofilter;
    const int typ = ctb.typ, cls = ctb.cls;
    const SaoTable tab = sao_table(typ, ctb.o);
    const uint32_t badd = sao_band_add(cls);
    const int ecls = typ == 2 ? (cls & 3) : 0;
    const bool c0 = ecls == 0, c3 = ecls == 3;
    // a = alignbyte(a_hi, a_lo, sha), b = alignbyte(b_hi, b_lo, shb) with the sources per class:
    //   class 0: a = (cur j, cur j-1, 3)  b = (cur j+1, cur j, 1);  class 1: a = up j, b = dn j (shift 0)
    //   class 2: a = (up j, up j-1, 3)    b = (dn j+1, dn j, 1);    class 3: a = (up j+1, up j, 1)  b = (dn j, dn j-1, 3)
    const uint32_t sha = ecls == 1 ? 0u : (c3 ? 1u : 3u), shb = ecls == 1 ? 0u : (c3 ? 3u : 1u);
    // the same as sources of one shifted row view: a = alignbyte(V[j + ea], V[j + ea - 1], sha) of
    // V = the a-row (class 0: this row, else the row above), b likewise with eb, the b-row
    const bool ea = ecls == 1 || c3, eb = !c3;

    // ---- byte masks: which of the lane's 16 samples may change, per row kind (sao.h sao_eo_masks) ----
    const int ylast = ye - 1;
    const EoMasks em = sao_eo_masks<16>(p, ctb);
    uint32_t m_top[4], m_mid[4], m_bot[4];
    expand_mask(em.top, m_top);
    expand_mask(em.mid, m_mid);
    expand_mask(em.bot, m_bot);
    const bool meo = typ == 2;

    // this kernel's own forms (measured): the table looked up per 16-bit half, the selector's high bytes
    // 0x0c (-> 0); sgn by clamped signed packed subtraction
    auto apply16 = [&](uint32_t v16, uint32_t sel16) {
        const uint32_t pos = __builtin_amdgcn_perm(tab.tp_hi, tab.tp_lo, sel16);
        const uint32_t neg = __builtin_amdgcn_perm(tab.tn_hi, tab.tn_lo, sel16);
        return pk_min_u16(pk_subsat_u16(pk_add_u16(v16, pos), neg), 0x00ff00ffu);
    };
    auto edge16 = [&](uint32_t v16, uint32_t a16, uint32_t b16) {
        return pk_add_u16(pk_add_u16(pk_sgn_i16(pk_sub_i16(v16, a16)), pk_sgn_i16(pk_sub_i16(v16, b16))), 0x0c020c02u);
    };

    // waves without a band-offset lane skip the band arithmetic (wave-uniform choice)
    auto filter_rows = [&](auto has_bo) {
        constexpr bool HB = decltype(has_bo)::value;
        for (int y0 = yb; y0 < ye; y0 += K) {
            if (y0 + K < ye) {
#pragma unroll
                for (int k = 0; k < K; ++k) nxt[k] = row_ld(y0 + K + k + 1);
            }
            // dwords beside the column, per loaded row
            uint32_t lft[K + 2], rgt[K + 2];
#pragma unroll
            for (int k = 0; k < K + 2; ++k) { lft[k] = left_of(rowv[k].w); rgt[k] = right_of(rowv[k].x); }
            auto dw = [&](int k, int j) -> uint32_t {                // dword j (-1 .. 4) of loaded row k
                return j < 0 ? lft[k] : (j > 3 ? rgt[k] : (j == 0 ? rowv[k].x : (j == 1 ? rowv[k].y : (j == 2 ? rowv[k].z : rowv[k].w))));
            };
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int y = y0 + r;
                const int k = r + 1;
                uint32_t nfm[4] = {0u, 0u, 0u, 0u};
                if (nf) {
                    const int ny = (int)__umul24((uint32_t)((min(y, H - 1) << sub) >> 3), (uint32_t)g.nf_w);
#pragma unroll
                    for (int j = 0; j < 4; ++j) nfm[j] = nf[ny + min(((Xc + 4 * j) << sub) >> 3, g.nf_w - 1)] ? 0xffffffffu : 0u;
                }
                // plane heights are multiples of 4 samples (host-checked), so a chunk's first row is
                // the only one that can be the CTB row's first, its last the only one that can be the last
                const uint32_t* m = r == 0 ? (y == yb ? m_top : m_mid) : (r == K - 1 ? (y == ylast ? m_bot : m_mid) : m_mid);
                // neighbours per lane class: a from row U (this row for class 0, the row above
                // otherwise), b from row D (this row / the row below), each horizontally shifted
                // by the class's dx: one select per dword of U / D and of their shifted views,
                // shared by the row's four dwords
                uint32_t U[6], D[6], Ua[5], Db[5];
#pragma unroll
                for (int j = -1; j <= 4; ++j) {
                    U[j + 1] = c0 ? dw(k, j) : dw(k - 1, j);
                    D[j + 1] = c0 ? dw(k, j) : dw(k + 1, j);
                }
#pragma unroll
                for (int j = -1; j <= 3; ++j) {
                    Ua[j + 1] = ea ? U[j + 2] : U[j + 1];
                    Db[j + 1] = eb ? D[j + 2] : D[j + 1];
                }
                uint32_t out[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t cur = dw(k, j);
                    const uint32_t a = __builtin_amdgcn_alignbyte(Ua[j + 1], Ua[j], sha);
                    const uint32_t b = __builtin_amdgcn_alignbyte(Db[j + 1], Db[j], shb);
                    const uint32_t v_lo = split_lo(cur), v_hi = split_hi(cur);
                    uint32_t sel_lo = edge16(v_lo, split_lo(a), split_lo(b));
                    uint32_t sel_hi = edge16(v_hi, split_hi(a), split_hi(b));
                    if constexpr (HB) {
                        const uint32_t sel = sao_band_sel(cur, badd);
                        sel_lo = meo ? sel_lo : __builtin_amdgcn_perm(0x0c0c0c0cu, sel, 0x04020400u);
                        sel_hi = meo ? sel_hi : __builtin_amdgcn_perm(0x0c0c0c0cu, sel, 0x04030401u);
                    }
                    const uint32_t res = join(apply16(v_lo, sel_lo), apply16(v_hi, sel_hi));
                    const uint32_t mk = m[j] & ~nfm[j];
                    out[j] = (res & mk) | (cur & ~mk);
                }
                if (act && y < ye) {
                    __attribute__((address_space(1))) u4v* q = (__attribute__((address_space(1))) u4v*)(dst + __umul24((uint32_t)y, (uint32_t)st) + Xc);
                    *q = u4v{out[0], out[1], out[2], out[3]};
                }
            }
            rowv[0] = rowv[K];
            rowv[1] = rowv[K + 1];
#pragma unroll
            for (int k = 0; k < K; ++k) rowv[k + 2] = nxt[k];
        }
    };
    if (__ballot(act && typ == 1)) filter_rows(std::integral_constant<bool, true>{});
    else filter_rows(std::integral_constant<bool, false>{});
}

}  // namespace p265r
