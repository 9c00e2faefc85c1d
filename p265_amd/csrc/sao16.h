// SAO only (8.7.3) for 16-bit samples (BitDepth 9..12), batches without deblocking: a
// streaming strip kernel: the strip walk of sao.h with 8 samples (16 B) per lane, 496-sample strips.  The
// wave walks down its CTB row with the rows above, at and below the current one in registers, so every
// sample is read once (+ 2 halo rows per CTB height) and written once, each row one coalesced load and
// store per wave instruction.  A lane's 8 samples lie in one CTB (8 divides every CTB width down to CTB 16
// chroma), so its SaoTypeIdx, class, offsets and 8.7.3.2 neighbourhood permissions are per-lane constants
// (sao.h sao_lane_ctb).  Per sample: band (bandShift = BitDepth - 5) or
// edge class and its SaoOffsetVal, two samples per packed 16-bit instruction; PCM / bypass samples
// (nofilter) untouched.  Main 10, 512 x 1080p: 2.05 ms per-sample form -> 1.44 ms packed (6.4 GB).
//
// The reference only parses the SAO syntax (decoder/sao.py:15-136, SaoOffsetVal sao.py:174-178); the
// filter rests on the spec restatement (oracle/recon_oracle.py sao_picture), as loopfilter16.h does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/p265r.h"
#include "intra.h"
#include "loopfilter.h"
#include "sao.h"

namespace p265r {

__device__ __forceinline__ int off_e(uint32_t o, int e) { return (int)(int8_t)(o >> (8 * e)); }   // SaoOffsetVal[e + 1]

// grid: 4 waves per block, one wave per (picture, CTB row, component, 496-sample strip), XCD-aware
// order (sao.h strip_pos)
__global__ __launch_bounds__(256) void sao16_strip_kernel(const DevPic* __restrict__ pics, Geo gb, BatchView v, int n_pics) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) uint16_t gu16;
    const StripPos p = strip_pos<8>(pics, gb, n_pics, gb.ctb_log2);
    if (p.outside) return;                                        // whole wave (no barriers below)
    const Geo& g = p.g;
    const int pic = p.pic, c = p.c, sub = p.sub, H = p.H, st = p.st;   // (st in samples)
    const int Xc = p.Xc, yb = p.yb, ye = p.ye;
    const bool act = p.act;
    // CTU records: slots of the context size; a ragged batch's smaller picture uses its own raster
    const p265r_ctu* crec = v.ctus0 + (size_t)pic * gb.wc * gb.hc;
    const int bd = c ? g.bd[1] : g.bd[0], maxv = (1 << bd) - 1;
    const uint64_t pofs = (uint64_t)pic * v.pic_bytes + v.plane_off[c];
    const gu16* src = (const gu16*)(v.rec0 + pofs);
    gu16* dst = (gu16*)(v.out0 + pofs);
    auto row_ld = [&](int y) {
        return *(const __attribute__((address_space(1))) u4v*)(src + (size_t)min(max(y, 0), H - 1) * st + Xc);
    };
    u4v up = row_ld(yb - 1), cur = row_ld(yb), dn = row_ld(yb + 1);

    // ---- this lane's CTB: SAO parameters, 8.7.3.2 permissions of its 3x3 neighbourhood ----------
    const SaoCtb ctb = sao_lane_ctb(crec, g, p.cy, p.bx, c);
    const uint8_t* nf = pics[pic].nofilter;
    const int typ = ctb.typ, cls = ctb.cls;
    const uint32_t o = ctb.o;
    const int ecls = typ == 2 ? (cls & 3) : 0;

    // ---- which of the lane's 8 samples may change, per row kind (first / inner / last row of the
    // CTB row): sao.h sao_eo_masks
    const int ylast = ye - 1;
    const EoMasks em = sao_eo_masks<8>(p, ctb);
    const uint32_t m_top = em.top, m_mid = em.mid, m_bot = em.bot;

    // Packed form: two samples per dword and VOP3P instruction.  Every row is kept with its copies shifted by
    // one sample (mi: sample i - 1, pl: sample i + 1; the lane's outer neighbours by DPP), built once when the
    // row is loaded; the lane's edge class picks its neighbour rows a / b once per row.  Per dword: the two
    // signs by clamped packed differences, and one byte-permute lookup of a per-lane table of the offsets
    // biased by 128 (band: slots 0..3, 4 = none; edge: s + 2 = 0..4 -> SaoOffsetVal[1, 2, -, 3, 4]); samples
    // outside the row's mask keep their value.
    typedef short s2v __attribute__((ext_vector_type(2)));
    auto as_s2 = [](uint32_t x) { return __builtin_bit_cast(s2v, x); };
    auto as_u = [](s2v x) { return __builtin_bit_cast(uint32_t, x); };
    auto pmax = [&](uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_s2(a), as_s2(b))); };
    auto pmin = [&](uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_s2(a), as_s2(b))); };
    auto psub = [&](uint32_t a, uint32_t b) { return as_u(as_s2(a) - as_s2(b)); };
    auto padd = [&](uint32_t a, uint32_t b) { return as_u(as_s2(a) + as_s2(b)); };
    struct Row { u4v v, mi, pl; };
    auto shifted = [&](const u4v& r) {
        const uint32_t lw = left_of(r.w), rx = right_of(r.x);
        const uint32_t t1 = __builtin_amdgcn_alignbit(r.y, r.x, 16), t2 = __builtin_amdgcn_alignbit(r.z, r.y, 16),
                       t3 = __builtin_amdgcn_alignbit(r.w, r.z, 16);
        return Row{r, u4v{__builtin_amdgcn_alignbit(r.x, lw, 16), t1, t2, t3}, u4v{t1, t2, t3, __builtin_amdgcn_alignbit(rx, r.w, 16)}};
    };
    // the lane's offset table: bytes 0..4 of (thi:tlo), each SaoOffsetVal + 128; byte 5 (= 0) fills the high bytes
    auto ob = [&](int e) { return (uint32_t)(off_e(o, e) + 128) & 0xffu; };
    uint32_t tlo, thi;
    if (typ == 1) { tlo = ob(0) | ob(1) << 8 | ob(2) << 16 | ob(3) << 24; thi = 128u; }
    else { tlo = ob(0) | ob(1) << 8 | 128u << 16 | ob(2) << 24; thi = ob(3); }
    const int bsh = bd - 5;                                       // bandShift
    const uint32_t bshv = (uint32_t)bsh * 0x00010001u, clsv = (uint32_t)cls * 0x00010001u;
    const uint32_t maxvv = (uint32_t)maxv * 0x00010001u;
    Row rup = shifted(up), rcur = shifted(cur), rdn = shifted(dn);
    for (int y = yb; y < ye; ++y) {
        const u4v nxt = row_ld(y + 2);                            // (in flight while this row is filtered)
        uint32_t nfm = 0;                                         // bit i: sample i untouched (PCM / bypass)
        if (nf) {
            const uint8_t* nr = nf + (size_t)((y << sub) >> 3) * g.nf_w;
            const int b0 = (Xc << sub) >> 3;
            if (nr[b0]) nfm |= sub ? 0x0fu : 0xffu;
            if (sub && b0 + 1 < g.nf_w && nr[b0 + 1]) nfm |= 0xf0u;
        }
        const uint32_t m = (y == yb ? m_top : (y == ylast ? m_bot : m_mid)) & ~nfm;
        const u4v av = ecls == 0 ? rcur.mi : (ecls == 1 ? rup.v : (ecls == 2 ? rup.mi : rup.pl));
        const u4v bv = ecls == 0 ? rcur.pl : (ecls == 1 ? rdn.v : (ecls == 2 ? rdn.pl : rdn.mi));
        uint32_t outw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t cv = rcur.v[j];
            uint32_t sel;
            if (typ == 1) {                                       // band slot min(k, 4), k = (v >> bandShift) - position
                const uint32_t k = as_u(as_s2(psub(as_u(__builtin_bit_cast(s2v, cv) >> as_s2(bshv)), clsv))) & 0x001f001fu;
                sel = pmin(k, 0x00040004u);
            } else {                                              // s + 2, s = sign(v - a) + sign(v - b)
                const uint32_t sa = pmax(pmin(psub(cv, av[j]), 0x00010001u), 0xffffffffu);
                const uint32_t sb = pmax(pmin(psub(cv, bv[j]), 0x00010001u), 0xffffffffu);
                sel = padd(padd(sa, sb), 0x00020002u);
            }
            const uint32_t ofs = psub(__builtin_amdgcn_perm(thi, tlo, sel | 0x05000500u), 0x00800080u);
            const uint32_t rv = pmin(pmax(padd(cv, ofs), 0u), maxvv);
            const uint32_t mk = ((m >> (2 * j)) & 1u ? 0x0000ffffu : 0u) | ((m >> (2 * j + 1)) & 1u ? 0xffff0000u : 0u);
            outw[j] = (rv & mk) | (cv & ~mk);
        }
        if (act)
            *(__attribute__((address_space(1))) u4v*)(dst + (size_t)y * st + Xc) = u4v{outw[0], outw[1], outw[2], outw[3]};
        rup = rcur;
        rcur = rdn;
        rdn = shifted(nxt);
    }
}

}  // namespace p265r
