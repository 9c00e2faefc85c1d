// SAO (H.265 8.7.3) pieces shared by the in-loop filter kernels: the window kernels (loopfilter.h,
// loopfilter16.h) and the streaming strip kernels (sao_rows.h, sao_strip16.h, sao16.h).
//
// The reference only parses the SAO syntax (decoder/sao.py:15-136) and never filters
// a sample.  8.7.3.2: a sample's edge-offset neighbour in another CTB is usable only if
// that CTB is inside the picture, in the same tile (unless loop_filter_across_tiles),
// and - across slices - the slice containing the later of the two samples allows it.
// That rule is stated twice: sao_allow() on p265r_ctu records (one neighbour per thread, window
// kernels) and sao_lane_ctb() on the records' raw dwords (all nine per lane, strip kernels).
//
// The strip kernels share one walk: one wave = one CTB row of one component over a strip of 62 lanes
// x N samples (N = 4, 8 or 16; lane l holds the N samples at x = 62 N s + N (l - 1), lanes 0 and 63
// only supply the neighbours of lanes 1 and 62 by DPP wave shifts).  strip_pos() places the wave and
// the lane, sao_lane_ctb() gives the lane's SAO parameters and 3x3 permissions, sao_eo_masks() the
// samples of the lane an edge offset may change; the byte-sample kernels (4 samples per dword) share
// the SWAR arithmetic below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/p265r.h"
#include "intra.h"

namespace p265r {

__device__ __forceinline__ bool ts_before(const p265r_ctu& a, int ra, const p265r_ctu& b, int rb) {
    // CtbAddrRsToTs[a] < CtbAddrRsToTs[b]; tiles are numbered in tile-scan order
    return a.tile_id < b.tile_id || (a.tile_id == b.tile_id && ra < rb);
}

__device__ __forceinline__ int sgn(int v) { return (v > 0) - (v < 0); }

// may samples of CTB rs use samples of the neighbouring CTB (dx, dy)?  (8.7.3.2)
__device__ __forceinline__ bool sao_allow(const p265r_ctu* ctus, const p265r_ctu& me, int rs, int rx, int ry,
                                          int dx, int dy, const Geo& g) {
    const int nx = rx + dx, ny = ry + dy;
    if (nx < 0 || ny < 0 || nx >= g.wc || ny >= g.hc) return false;
    if (!dx && !dy) return true;
    const int ro = ny * g.wc + nx;
    const p265r_ctu o = ctus[ro];
    bool ok = true;
    if (o.slice_addr != me.slice_addr) {
        // the flag of the slice containing the LATER of the two samples
        ok = ts_before(o, ro, me, rs) ? (me.flags & P265R_CTU_LF_ACROSS_SLICES) != 0
                                      : (o.flags & P265R_CTU_LF_ACROSS_SLICES) != 0;
    }
    if (!g.lf_tiles && o.tile_id != me.tile_id) ok = false;
    return ok;
}

// XCD-aware block order: hardware block b runs on XCD b % 8 (observed round-robin,
// MI355X_MICROARCH.md); logical unit = (b % 8) * per + b / 8, so each XCD walks one contiguous
// range of units and the halo rows / columns neighbouring units share are read from its own L2.
__device__ __forceinline__ int xcd_unit(int b, int n_units) {
    const int per = (n_units + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

// ---------------------------------------------------------------------------------------
// Strip kernels: position of the wave and the lane
// ---------------------------------------------------------------------------------------
// samples per strip with n samples per lane (62 output lanes)
constexpr int strip_samples(int n) { return 62 * n; }

// waves per picture: hc CTB rows x (luma strips + 2 x chroma strips) of `strip` samples
__host__ __device__ __forceinline__ int strip_units(const Geo& g, int strip) {
    return g.hc * ((g.w + strip - 1) / strip + 2 * ((g.cw + strip - 1) / strip));
}

struct StripPos {
    Geo g;                      // the picture's geometry (its own size in a ragged batch)
    bool outside;               // the whole wave has no work (past the grid, or outside a ragged picture)
    // wave-uniform (SGPRs): picture, CTB row, component, strip; the component's CTB size, plane size, stride
    int pic, cy, c, sx;
    int sub, Ls, cs, W, H, st;
    int yb, ye;                 // the CTB row's sample rows [yb, ye)
    // per lane: its N samples start at X (act: inside the plane, lanes 1..62); Xc = X clamped so that
    // every lane reads a valid column; bx = the lane's CTB column, starting at sample xb
    int X, Xc, bx, xb;
    bool act;
};

// grid: 4 waves per block, one wave per (picture, CTB row, component, strip of 62 N samples), blocks
// dealt XCD-aware.  ctb_log2: g.ctb_log2, or the same as a compile-time constant.
// Straight-line on purpose: a wave past the grid decodes the last unit and leaves at the caller's
// `if (p.outside) return;`.  Early returns in here would merge with the full path in front of that
// branch, which pins every field in a register from there on (the caller's code cannot sink them to
// their uses) and costs the strip kernels VGPRs.
template <int N>
__device__ __forceinline__ StripPos strip_pos(const DevPic* __restrict__ pics, const Geo& gb, int n_pics, int ctb_log2) {
    constexpr int strip = strip_samples(N);
    StripPos p;
    const int lane = threadIdx.x & 63;
    const int per_pic = strip_units(gb, strip);
    const int total = per_pic * n_pics;
    const int nblk = (total + 3) >> 2;
    const int bunit = xcd_unit(blockIdx.x, nblk);                 // block -> 4 consecutive units
    // wave-uniform (readfirstlane): everything derived from the unit lives in SGPRs
    const int wunit = __builtin_amdgcn_readfirstlane(bunit * 4 + (int)(threadIdx.x >> 6));
    p.outside = bunit >= nblk || wunit >= total;
    const int unit = min(wunit, total - 1);
    p.pic = unit / per_pic;
    int u = unit - p.pic * per_pic;
    const int nsl = (gb.w + strip - 1) / strip, nsc = (gb.cw + strip - 1) / strip;
    // unit order inside a picture: CTB row major, then luma strips, Cb strips, Cr strips
    p.cy = u / (nsl + 2 * nsc);
    u -= p.cy * (nsl + 2 * nsc);
    if (u < nsl) { p.c = 0; p.sx = u; }
    else { p.c = 1 + (u - nsl) / nsc; p.sx = (u - nsl) % nsc; }
    const int c = p.c;
    p.g = gb;
    if (gb.ragged) {                              // this picture's size and CTU raster
        p.g = pic_geo(gb, (uint32_t)__builtin_amdgcn_readfirstlane((int)pics[p.pic].wh));
        p.outside = p.outside || p.cy >= p.g.hc || p.sx * strip >= (c ? p.g.cw : p.g.w);
    }
    const Geo& g = p.g;
    p.sub = c ? 1 : 0;
    p.Ls = ctb_log2 - p.sub;
    p.cs = 1 << p.Ls;
    p.W = c ? g.cw : g.w;
    p.H = c ? g.ch : g.h;
    p.st = c ? g.stride[1] : g.stride[0];
    p.X = p.sx * strip + N * (lane - 1);
    p.act = lane >= 1 && lane <= 62 && p.X < p.W;
    p.Xc = min(max(p.X, 0), (p.W - 1) & ~(N - 1));                // every lane reads a valid column
    p.yb = p.cy << p.Ls;
    p.ye = min(p.yb + p.cs, p.H);
    p.bx = p.Xc >> p.Ls;
    p.xb = p.bx << p.Ls;
    return p;
}

// ---------------------------------------------------------------------------------------
// Strip kernels: the lane's CTB
// ---------------------------------------------------------------------------------------
struct SaoCtb {
    uint32_t allow;             // bit 3 (dy + 1) + dx + 1: the CTB may use its neighbour (dx, dy)  (8.7.3.2)
    int typ, cls;               // SaoTypeIdx; sao_band_position (type 1) or SaoEoClass (type 2)
    uint32_t o;                 // SaoOffsetVal[1..4], signed bytes
    __device__ __forceinline__ bool ok(int ay, int ax) const { return ((allow >> (ay * 3 + ax)) & 1u) != 0; }
};

// SAO parameters of component c of CTB (bx, cy) and the 8.7.3.2 permissions of its 3x3 neighbourhood,
// as sao_allow() above, on the raw dwords of the 32-byte p265r_ctu records (include/p265r.h):
//   dword 1: tb_count | tile_id << 16        dword 2: slice_addr
//   dword 3: flags | sao_type[0..2] << 8     dword 4: sao_class[0..2] | deblock_offsets << 24
//   dword 5 + c: sao_offset[c][0..3]
// The nine records' first 16 B are loaded together (neighbours outside the picture clamped to it).
__device__ __forceinline__ SaoCtb sao_lane_ctb(const p265r_ctu* ctus, const Geo& g, int cy, int bx, int c) {
    static_assert(sizeof(p265r_ctu) == 32, "record dwords below");
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u4v gu4v;
    const uint32_t* crec = reinterpret_cast<const uint32_t*>(ctus);
    const int rs = cy * g.wc + bx;
    u4v nb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int nx = min(max(bx + k % 3 - 1, 0), g.wc - 1), ny = min(max(cy + k / 3 - 1, 0), g.hc - 1);
        nb[k] = *(gu4v*)(crec + (size_t)(ny * g.wc + nx) * 8);
    }
    const u4v mt = *(gu4v*)(crec + (size_t)rs * 8 + 4);
    SaoCtb r;
    r.allow = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int dx = k % 3 - 1, dy = k / 3 - 1;
        const int nx = bx + dx, ny = cy + dy;
        bool ok = nx >= 0 && ny >= 0 && nx < g.wc && ny < g.hc;
        const uint32_t ti = nb[4].y >> 16, to = nb[k].y >> 16;
        if (ok && nb[k].z != nb[4].z) {                          // other slice: the later sample's slice flag
            const bool o_first = to < ti || (to == ti && k < 4);   // (k < 4: before this CTB in raster order)
            ok = ((o_first ? nb[4].w : nb[k].w) & P265R_CTU_LF_ACROSS_SLICES) != 0;
        }
        if (!g.lf_tiles && to != ti) ok = false;
        if (ok) r.allow |= 1u << k;
    }
    r.typ = (int)((nb[4].w >> (8 * (c + 1))) & 0xffu);
    r.cls = (int)((mt.x >> (8 * c)) & 0xffu);
    r.o = c == 0 ? mt.y : (c == 1 ? mt.z : mt.w);
    return r;
}

// ---------------------------------------------------------------------------------------
// Strip kernels with N = 8 / 16 samples per lane: which samples an edge offset may change
// ---------------------------------------------------------------------------------------
// Neighbour (dx, dy) of sample i of row y is usable iff inside the picture and its CTB allowed; only
// sample 0 / N - 1 can leave the lane's CTB column (N divides the CTB width), only the CTB row's first /
// last row its rows; samples at x >= W are stored into the row padding and never read: don't care.
// ay: row of the 3x3 neighbourhood the neighbour's sample row lies in, -1 outside the picture.
// One set of masks per row kind: the CTB row's first, inner and last row.
struct EoMasks { uint32_t top, mid, bot; };    // bit i: sample i of the lane's N may change

template <int N>
__device__ __forceinline__ EoMasks sao_eo_masks(const StripPos& p, const SaoCtb& k) {
    constexpr uint32_t all = (1u << N) - 1u;
    const int typ = k.typ, Xc = p.Xc, yb = p.yb, ylast = p.ye - 1, H = p.H;
    const int ecls = typ == 2 ? (k.cls & 3) : 0;
    // edge neighbours: a at (dxa, dya), b at (-dxa, -dya) (Table 8-13 hPos / vPos)
    const int dxa = ecls == 1 ? 0 : (ecls == 3 ? 1 : -1);
    const int dya = ecls == 0 ? 0 : -1;
    const int n_in = p.W - Xc;
    const bool ctb_first = Xc == p.xb, ctb_last = Xc + N == p.xb + p.cs;
    auto col_bits = [&](int dx, int ay) -> uint32_t {
        if (ay < 0) return 0u;
        if (dx == 0) return k.ok(ay, 1) ? all : 0u;
        if (dx < 0) return (k.ok(ay, 1) ? all - 1u : 0u) | ((Xc > 0 && k.ok(ay, ctb_first ? 0 : 1)) ? 1u : 0u);
        const uint32_t inner = n_in >= N ? all >> 1 : ((1u << max(n_in - 1, 0)) - 1u);
        return (k.ok(ay, 1) ? inner : 0u) | ((n_in > N && k.ok(ay, ctb_last ? 2 : 1)) ? 1u << (N - 1) : 0u);
    };
    auto row_a = [&](int y, int dy) -> int {
        if (dy == 0) return 1;
        if (dy < 0) return y == yb ? 0 : 1;
        return y == ylast ? (y == H - 1 ? -1 : 2) : 1;
    };
    auto mask = [&](int y) -> uint32_t {
        if (typ == 0) return 0u;
        if (typ == 1) return all;
        return col_bits(dxa, row_a(y, dya)) & col_bits(-dxa, row_a(y, -dya));
    };
    return EoMasks{mask(yb), mask(yb + 1), mask(ylast)};
}

// ---------------------------------------------------------------------------------------
// Byte samples, 4 per dword (SWAR): per sample a table index (edgeIdx or band slot) is built in a
// byte, the offsets are looked up 4 at a time with v_perm_b32 from 8-byte tables, and v + offset is
// clipped in two packed 16-bit halves
// ---------------------------------------------------------------------------------------
// packed unsigned 16-bit ops (two samples per dword); inline asm keeps them packed (the
// compiler otherwise splits clamped / min forms into per-element compares)
__device__ __forceinline__ uint32_t pk_add_u16(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_add_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_sub_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ uint32_t pk_subsat_u16(uint32_t a, uint32_t b) {       // max(a - b, 0)
    uint32_t r; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}

// byte-wise 0 / 1 -> 0x00 / 0xff (0x80 - 1 per byte never borrows; LLVM turns x * 255 and
// (x << 8) - x into a quarter-rate v_mul_lo_u32)
__device__ __forceinline__ uint32_t bytes_ff(uint32_t b01) { return (0x80808080u - b01) ^ 0x80808080u; }

__device__ __forceinline__ uint32_t split_lo(uint32_t v) { return __builtin_amdgcn_perm(0u, v, 0x0c020c00u); }   // bytes 0, 2
__device__ __forceinline__ uint32_t split_hi(uint32_t v) { return __builtin_amdgcn_perm(0u, v, 0x0c030c01u); }   // bytes 1, 3
__device__ __forceinline__ uint32_t join(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x06020400u); }

// the dword of lane l - 1 / l + 1 (DPP wave shifts; lanes 0 / 63 of a strip are not output)
__device__ __forceinline__ uint32_t left_of(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t right_of(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false); }

// 8-entry byte tables (lo: entries 0..3, hi: 4..7) of max(off, 0) and max(-off, 0).  Edge offset: raw
// e = 2 + sgn(v - a) + sgn(v - b) -> edgeIdx 1, 2, 0, 3, 4; band offset: slot 1..4 = the four bands from
// sao_band_position, slot 0 = no offset
struct SaoTable { uint32_t tp_lo, tp_hi, tn_lo, tn_hi; };

__device__ __forceinline__ SaoTable sao_table(int typ, uint32_t o) {   // o: SaoOffsetVal[1..4], signed bytes
    const uint32_t t_lo = typ == 2 ? __builtin_amdgcn_perm(0u, o, 0x020c0100u) : (o << 8);
    const uint32_t t_hi = o >> 24;
    const uint32_t n_lo = (t_lo >> 7) & 0x01010101u, n_hi = (t_hi >> 7) & 0x01010101u;
    return SaoTable{t_lo & ~bytes_ff(n_lo), t_hi & ~bytes_ff(n_hi),
                    (~t_lo & bytes_ff(n_lo)) + n_lo, (~t_hi & bytes_ff(n_hi)) + n_hi};
}

// v + table[sel] clipped to [0, 255], 4 samples
__device__ __forceinline__ uint32_t sao_apply(const SaoTable& t, uint32_t v, uint32_t sel) {
    const uint32_t pos = __builtin_amdgcn_perm(t.tp_hi, t.tp_lo, sel);
    const uint32_t neg = __builtin_amdgcn_perm(t.tn_hi, t.tn_lo, sel);
    const uint32_t m255 = 0x00ff00ffu;
    const uint32_t rl = pk_min_u16(pk_subsat_u16(pk_add_u16(split_lo(v), split_lo(pos)), split_lo(neg)), m255);
    const uint32_t rh = pk_min_u16(pk_subsat_u16(pk_add_u16(split_hi(v), split_hi(pos)), split_hi(neg)), m255);
    return join(rl, rh);
}

// 2 + sgn(v - a) + sgn(v - b) in unsigned 16-bit lanes: [v > a] = min(sat(v - a), 1)
__device__ __forceinline__ uint32_t swar_gt(uint32_t v, uint32_t a) { return pk_min_u16(pk_subsat_u16(v, a), 0x00010001u); }
__device__ __forceinline__ uint32_t swar_edge(uint32_t v, uint32_t a, uint32_t b) {
    return pk_sub_u16(pk_add_u16(pk_add_u16(swar_gt(v, a), swar_gt(v, b)), 0x00020002u), pk_add_u16(swar_gt(a, v), swar_gt(b, v)));
}
// the edge-offset table index of 4 samples v with neighbours a, b (byte-aligned)
__device__ __forceinline__ uint32_t sao_edge_sel(uint32_t v, uint32_t a, uint32_t b) {
    return join(swar_edge(split_lo(v), split_lo(a), split_lo(b)), swar_edge(split_hi(v), split_hi(a), split_hi(b)));
}

// band offset: (32 - sao_band_position) in every byte, and the table slot of 4 samples: 1..4 for the
// four bands from the position, else 0
__device__ __forceinline__ uint32_t sao_band_add(int cls) {
    const uint32_t bsh = (uint32_t)((32 - cls) & 31);
    return __umul24(bsh, 0x010101u) | bsh << 24;
}
__device__ __forceinline__ uint32_t sao_band_sel(uint32_t v, uint32_t badd) {
    const uint32_t kk = (((v >> 3) & 0x1f1f1f1fu) + badd) & 0x1f1f1f1fu;
    const uint32_t big = (((kk & 0x1c1c1c1cu) + 0x7f7f7f7fu) & 0x80808080u) >> 7;
    return (kk + 0x01010101u) & ~bytes_ff(big);
}

}  // namespace p265r
