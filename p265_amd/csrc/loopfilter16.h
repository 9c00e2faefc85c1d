// In-loop filters of the 16-bit sample path (BitDepth 9..12; Geo::pel16): deblocking (8.7.2)
// + SAO (8.7.3) fused in one pass, as loopfilter.h does for 8-bit samples, with the bit-depth rules:
//   beta = beta' * (1 << (BitDepthY - 8)), tC = tC' * (1 << (BitDepth - 8))   (8.7.2.5.3, 8.7.2.5.5)
//   QpY = Qp'Y - QpBdOffsetY on both sides of an edge (the deblocking map carries Qp'Y, loopfilter.h)
//   bandShift = BitDepth - 5, SaoOffsetVal as recorded (<< (BitDepth - Min(BitDepth, 10)) by the
//   front-end), clipping to (1 << BitDepth) - 1                              (8.7.3.2, 7.4.9.3.2)
// The reference has neither filter (decoder/sao.py:15-136 parses the syntax, sao.py:174-178 derives
// cMax from the bit depth); oracle/recon_oracle.py restates both for every bit depth.
//
// One workgroup per (CTB, picture), XCD-aware order; the CTB plus a 4-sample halo is staged in LDS as
// uint16 samples (luma (S+8)^2, chroma (S/2+8)^2 each), deblocked there (the window is closed under
// deblocking, loopfilter.h), and SAO of the CTB runs from it, one sample per thread and step.  Plain
// per-sample arithmetic: this path is for correctness and coverage of Main 10, not the headline.
// The filters (dbk_luma_seg<true>, dbk_chroma_line<true>), the window prologue, the map fill and the
// edge-task decode are the ones of loopfilter.h; the LDS layout, sample access and SAO stage are this file's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/p265r.h"
#include "intra.h"
#include "loopfilter.h"
#include "sao.h"

namespace p265r {

// grid (8 * ceil(CTUs * pictures / 8)), 256 threads; planes of uint16_t samples, Geo::stride samples
template <int CTBL, bool DBK>
__global__ __launch_bounds__(256) void loopfilter16_kernel(const DevPic* __restrict__ pics, Geo g, int sao_on, int n_pics) {
    constexpr int S = 1 << CTBL, SC = S / 2;
    constexpr int RL = S + 8, RC = SC + 8;                   // window rows / columns (halo 4)
    constexpr int NB = S / 8 + 2;                             // 8x8 luma blocks per window row (map)
    constexpr int NLE = S / 8 + 1, NCE = SC / 8 + 1;          // edges per direction
    constexpr int WL = RL / 4, WC = RC / 4;                   // 4-line segments per edge
    constexpr int T = 256;
    __shared__ uint16_t s_l[RL * RL];
    __shared__ uint16_t s_c[2][RC * RC];
    __shared__ uint16_t s_map[NB * NB];
    __shared__ uint8_t s_nf[NB * NB];
    __shared__ LfCtu s_ctu[9];
    __shared__ uint32_t s_allow;

    const LfWindow w = lf_window<CTBL>(pics, g, n_pics);     // (g: this picture's from here on)
    if (w.outside) return;                                   // whole workgroup: before any barrier
    const DevPic* P = pics + w.pic;
    const int x0 = w.x0, y0 = w.y0, xc0 = x0 >> 1, yc0 = y0 >> 1;
    const int tid = threadIdx.x;
    const p265r_ctu me = P->ctus[w.rs];
    const int qp_off = 6 * (g.bd[0] - 8);                    // QpBdOffsetY: the map holds Qp'Y

    lf_fill_maps<uint16_t, NB, DBK, T>(P, w, g, me, s_map, s_nf, s_ctu, &s_allow);
    {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(P->rec[0]);
        for (int i = tid; i < RL * RL; i += T) {
            const int r = i / RL, q = i - r * RL;
            const int gy = y0 - 4 + r, gx = x0 - 4 + q;
            s_l[i] = (gy >= 0 && gy < g.h && gx >= 0 && gx < g.w) ? src[(size_t)gy * g.stride[0] + gx] : 0;
        }
        for (int i = tid; i < 2 * RC * RC; i += T) {
            const int c = i >= RC * RC, k = i - c * RC * RC;
            const int r = k / RC, q = k - r * RC;
            const int gy = yc0 - 4 + r, gx = xc0 - 4 + q;
            const uint16_t* cs = reinterpret_cast<const uint16_t*>(P->rec[1 + c]);
            s_c[c][k] = (gy >= 0 && gy < g.ch && gx >= 0 && gx < g.cw) ? cs[(size_t)gy * g.stride[1] + gx] : 0;
        }
    }
    __syncthreads();

    if constexpr (DBK) {
        constexpr int N_DBK = NLE * WL + 2 * NCE * WC;
        for (int dir = 0; dir < 2; ++dir) {                  // 0: vertical edges, 1: horizontal edges
            for (int t = tid; t < N_DBK; t += T) {
                if (t < NLE * WL) {
                    const int i = t / WL, j = t % WL;
                    const DbkEdge ed = dbk_edge_task<CTBL, uint16_t, NB>(w, g, s_map, s_ctu, dir, 0, i, j);
                    if (!ed.on) continue;
                    const int bq = ed.bq, bp = ed.bp, mq = ed.mq, offs = ed.offs;
                    // window sample of P_a / Q_a on line k
                    auto at = [&](int a, int k, bool q) -> uint16_t& {
                        const int e = 8 * i + (q ? 4 + a : 3 - a), l = 4 * j + k;
                        return dir ? s_l[e * RL + l] : s_l[l * RL + e];
                    };
                    int Pm[4][4], Qm[4][4];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int k = 0; k < 4; ++k) { Pm[a][k] = at(a, k, false); Qm[a][k] = at(a, k, true); }
                    dbk_luma_seg<true>(Pm, Qm, (s_map[bp] & DBK16_QP) - qp_off, (mq & DBK16_QP) - qp_off, nib4(offs & 15),
                                       nib4(offs >> 4), s_nf[bp] != 0, s_nf[bq] != 0, g.bd[0]);
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int k = 0; k < 4; ++k) { at(a, k, false) = (uint16_t)Pm[a][k]; at(a, k, true) = (uint16_t)Qm[a][k]; }
                } else {
                    const int u = t - NLE * WL;
                    const int c = u / (NCE * WC), v = u % (NCE * WC);
                    const int i = v / WC, j = v % WC;
                    const DbkEdge e = dbk_edge_task<CTBL, uint16_t, NB>(w, g, s_map, s_ctu, dir, 1, i, j);
                    if (!e.on) continue;
                    const int bq = e.bq, bp = e.bp;
                    const int tc = dbk_chroma_tc<true>((s_map[bp] & DBK16_QP) - qp_off, (e.mq & DBK16_QP) - qp_off,
                                                       c ? g.cqp[1] : g.cqp[0], nib4(e.offs >> 4), g.bd[1]);
                    const bool nop = s_nf[bp] != 0, noq = s_nf[bq] != 0;
                    uint16_t* win = s_c[c];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int l = 4 * j + k, eo = 8 * i;
                        uint16_t& rp0 = dir ? win[(eo + 3) * RC + l] : win[l * RC + eo + 3];
                        uint16_t& rq0 = dir ? win[(eo + 4) * RC + l] : win[l * RC + eo + 4];
                        const int p1 = dir ? win[(eo + 2) * RC + l] : win[l * RC + eo + 2];
                        const int q1 = dir ? win[(eo + 5) * RC + l] : win[l * RC + eo + 5];
                        int p0 = rp0, q0 = rq0;
                        dbk_chroma_line<true>(p0, p1, q0, q1, tc, nop, noq, g.bd[1]);
                        if (!nop) rp0 = (uint16_t)p0;
                        if (!noq) rq0 = (uint16_t)q0;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- SAO of the CTB from the (deblocked) window, one sample per thread and step ----
    const uint32_t allow = s_allow;
    constexpr int NL = S * S, NC = SC * SC;
    for (int u = tid; u < NL + 2 * NC; u += T) {
        const int c = u < NL ? 0 : 1 + (u - NL) / NC;
        const int t = u < NL ? u : (u - NL) % NC;
        const int sub = c ? 1 : 0;
        const int cs = S >> sub;
        const int row = t >> (CTBL - sub), col = t & (cs - 1);
        const int W = c ? g.cw : g.w, H = c ? g.ch : g.h;
        const int xb = c ? xc0 : x0, yb = c ? yc0 : y0;
        const int X = xb + col, Y = yb + row;
        if (X >= W || Y >= H) continue;
        const uint16_t* win = c ? s_c[c - 1] : s_l;
        const int ws = c ? RC : RL;
        auto smp = [&](int dx, int dy) { return (int)win[(row + 4 + dy) * ws + col + 4 + dx]; };
        const int v = smp(0, 0);
        int r = v;
        const int typ = sao_on ? me.sao_type[c] : 0;
        const int lx = X << sub, ly = Y << sub;
        const bool nf = s_nf[((ly >> 3) - (y0 >> 3) + 1) * NB + (lx >> 3) - (x0 >> 3) + 1] != 0;
        if (typ != 0 && !nf) {
            const int bd = g.bd[c], maxv = (1 << bd) - 1;
            const int cls = me.sao_class[c];
            if (typ == 1) {
                const int k = ((v >> (bd - 5)) - cls) & 31;              // band slot relative to the position
                if (k < 4) r = min(max(v + (int)me.sao_offset[c][k], 0), maxv);
            } else {
                const int ax = cls == 0 ? -1 : (cls == 1 ? 0 : (cls == 2 ? -1 : 1));
                const int ay = cls == 0 ? 0 : -1;
                const int bx = -ax, by = -ay;
                bool ok = X + ax >= 0 && X + ax < W && Y + ay >= 0 && Y + ay < H &&
                          X + bx >= 0 && X + bx < W && Y + by >= 0 && Y + by < H;
                auto reg = [&](int dx, int dy) {
                    const int cx = col + dx < 0 ? 0 : (col + dx >= cs ? 2 : 1);
                    const int cy = row + dy < 0 ? 0 : (row + dy >= cs ? 2 : 1);
                    return ((allow >> (cy * 3 + cx)) & 1u) != 0;
                };
                ok = ok && reg(ax, ay) && reg(bx, by);
                if (ok) {
                    const int a = smp(ax, ay), b = smp(bx, by);
                    int e = 2 + (v > a) - (v < a) + (v > b) - (v < b);
                    e = e == 2 ? 0 : (e < 2 ? e + 1 : e);                 // edgeIdx 0..4
                    if (e) r = min(max(v + (int)me.sao_offset[c][e - 1], 0), maxv);
                }
            }
        }
        reinterpret_cast<uint16_t*>(P->out[c])[(size_t)Y * g.stride[c] + X] = (uint16_t)r;
    }
}

}  // namespace p265r
