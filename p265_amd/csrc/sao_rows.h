// SAO-only in-loop filter pass (H.265 8.7.3) for batches without deblocking: a streaming
// kernel, no LDS.  (Batches with deblocking keep the fused deblocking + SAO window kernel of
// loopfilter.h.)  The reference parses the SAO syntax (decoder/sao.py:15-136) and never filters.
//
// The strip walk of sao.h with 4 samples (one dword) per lane, 248-sample strips.  The wave walks
// down the CTB row 8 output rows at a time: the 10 rows a chunk needs are loaded one chunk ahead
// (one dword per lane and row, a 256-byte coalesced load per row, all in flight together), the
// dword is filtered with the SWAR arithmetic of sao.h and stored to the output plane.  HBM traffic
// per sample: one read (+ 2 halo rows per CTB height, + 2 / 62 halo columns) and one write.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/p265r.h"
#include "intra.h"
#include "loopfilter.h"
#include "sao.h"

namespace p265r {

constexpr int kSaoRowsChunk = 8;   // output rows per load batch

// grid: 4 waves per block, one wave per (picture, CTB row, component, 248-sample strip), XCD-aware
// order (sao.h strip_pos)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void sao_rows_kernel(const DevPic* __restrict__ pics, Geo gb, int n_pics) {
    typedef __attribute__((address_space(1))) uint8_t gu8;
    typedef __attribute__((address_space(1))) uint32_t gu32;
    const StripPos p = strip_pos<4>(pics, gb, n_pics, gb.ctb_log2);
    if (p.outside) return;                                        // whole wave (no barriers below)
    const Geo& g = p.g;
    const DevPic* P = pics + p.pic;
    const int sub = p.sub, cs = p.cs, W = p.W, H = p.H, st = p.st;
    const int X = p.X, Xc = p.Xc, yb = p.yb, ye = p.ye, xb = p.xb;
    const bool act = p.act;
    const gu8* src = (const gu8*)P->rec[p.c];
    gu8* dst = (gu8*)P->out[p.c];

    // ---- this lane's CTB: SAO parameters and 8.7.3.2 permissions of its 3x3 neighbourhood ----
    const SaoCtb ctb = sao_lane_ctb(P->ctus, g, p.cy, p.bx, p.c);
    auto rok = [&](int rr, int cc) { return ctb.ok(rr, cc); };
    const int typ = ctb.typ, cls = ctb.cls;
    const SaoTable tab = sao_table(typ, ctb.o);
    const uint32_t badd = sao_band_add(cls);
    const int cl = Xc == xb ? 0 : 1, cr = Xc + 4 == xb + cs ? 2 : 1;
    const bool has_l = Xc > 0, right_in = Xc + 4 < W;
    const gu8* nf = (const gu8*)P->nofilter;
    // Everything per lane below is a bit mask, not a branch: the lanes of a wave span several
    // CTBs of different type / class (the compiler otherwise branches with EXEC juggling per row).
    auto msk = [](bool b) { return b ? 0xffffffffu : 0u; };
    const uint32_t mc0 = msk(cls == 0), mc1 = msk(cls == 1), mc2 = msk(cls == 2), mc3 = msk(cls == 3);
    const uint32_t meo = msk(typ == 2);
    // which samples may change (8.7.3.2: EO neighbours inside the picture and in a CTB this one
    // may use; SaoTypeIdx != 0), per kind of row: rup / rdn = CTB row of the up / down neighbour
    auto okm_of = [&](bool vert, int rup, int rdn) -> uint32_t {
        if (typ == 0) return 0u;
        if (typ == 1) return 0xffffffffu;
        const bool v_ok = vert && rok(rup, 1) && rok(rdn, 1);
        bool mid, first, last;
        if (cls == 0) { mid = true; first = has_l && rok(1, cl); last = right_in && rok(1, cr); }
        else if (cls == 1) { mid = first = last = v_ok; }
        else if (cls == 2) {
            mid = v_ok;
            first = vert && has_l && rok(rup, cl) && rok(rdn, 1);
            last = vert && right_in && rok(rup, 1) && rok(rdn, cr);
        } else {
            mid = v_ok;
            first = vert && has_l && rok(rup, 1) && rok(rdn, cl);
            last = vert && right_in && rok(rup, cr) && rok(rdn, 1);
        }
        return (mid ? 0x00ffff00u : 0u) | (first ? 0xffu : 0u) | (last ? 0xff000000u : 0u);
    };
    const uint32_t ok_top = okm_of(true, 0, 1), ok_mid = okm_of(true, 1, 1), ok_bot = okm_of(true, 1, 2);
    const uint32_t ok_nv = okm_of(false, 1, 1);                   // picture's first / last row

    auto row_ld = [&](int y) { return *(const gu32*)(src + (size_t)min(max(y, 0), H - 1) * st + Xc); };
    constexpr int K = kSaoRowsChunk;
    // rows y0 - 1 .. y0 + K of the current chunk; the next chunk's K new rows are loaded before
    // the current chunk is filtered.  A chunk is one basic block (rows past the CTB row are
    // computed and not stored), so the scheduler interleaves its independent rows.
    // waves without a band-offset CTB (about half of them: ~82 % of CTBs are edge-offset) skip the
    // band arithmetic; the choice is wave-uniform
    auto filter_rows = [&](auto has_bo) {
        constexpr bool HB = decltype(has_bo)::value;
        uint32_t rowv[K + 2], nxt[K];
        rowv[0] = row_ld(yb - 1);
        rowv[1] = row_ld(yb);
#pragma unroll
        for (int k = 2; k < K + 2; ++k) rowv[k] = row_ld(yb + k - 1);
        for (int y0 = yb; y0 < ye; y0 += K) {
            if (y0 + K < ye) {
#pragma unroll
                for (int k = 0; k < K; ++k) nxt[k] = row_ld(y0 + K + k + 1);
            }
            uint32_t nfm[K];                                          // PCM / bypass samples: unchanged
#pragma unroll
            for (int k = 0; k < K; ++k) nfm[k] = 0u;
            if (nf) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    nfm[k] = nf[(size_t)((min(y0 + k, H - 1) << sub) >> 3) * g.nf_w + ((Xc << sub) >> 3)] ? 0xffffffffu : 0u;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int y = y0 + k;
                const uint32_t cur = rowv[k + 1], up = rowv[k], dn = rowv[k + 2];
                const uint32_t lc = left_of(cur), rc = right_of(cur);
                const uint32_t lu = left_of(up), ru_ = right_of(up);
                const uint32_t ld = left_of(dn), rd_ = right_of(dn);
                // edge offset: neighbours a, b of the 4 samples (byte-aligned) per SaoEoClass
                const uint32_t a = (__builtin_amdgcn_alignbyte(cur, lc, 3) & mc0) | (up & mc1) |
                                   (__builtin_amdgcn_alignbyte(up, lu, 3) & mc2) | (__builtin_amdgcn_alignbyte(ru_, up, 1) & mc3);
                const uint32_t b = (__builtin_amdgcn_alignbyte(rc, cur, 1) & mc0) | (dn & mc1) |
                                   (__builtin_amdgcn_alignbyte(rd_, dn, 1) & mc2) | (__builtin_amdgcn_alignbyte(dn, ld, 3) & mc3);
                const uint32_t sel_eo = sao_edge_sel(cur, a, b);
                uint32_t sel = sel_eo;
                if constexpr (HB) sel = (sel_eo & meo) | (sao_band_sel(cur, badd) & ~meo);
                // row kind (wave-uniform): picture's first / last row, CTB's first / last row, other
                const uint32_t okm = ((y == 0 || y + 1 == H) ? ok_nv : (y == yb ? ok_top : (y == yb + cs - 1 ? ok_bot : ok_mid))) & ~nfm[k];
                const uint32_t res = (sao_apply(tab, cur, sel) & okm) | (cur & ~okm);
                if (act && y < ye) *(gu32*)(dst + (size_t)y * st + X) = res;
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
