// upload_host.cpp -- host side of the batch upload: validation, layout, chunking and packing (upload_host.h).
// Plain C++ without HIP, so that it also builds stand-alone under the host sanitizers (make upload-check,
// tools/upload_check.cpp).
#include "upload_host.h"

#include <cstdint>
#include <cstring>

#include "sparse_host.h"

namespace p265r {

std::array<int, 2> pic_size(const p265r_params& p, const p265r_picture& pic) {
    return {pic.pic_width ? (int)pic.pic_width : (int)p.pic_width, pic.pic_height ? (int)pic.pic_height : (int)p.pic_height};
}

namespace {

// p265r_tb.qp (qP incl. QpBdOffset of the TB's component) is 0 .. 51 + 6 * (BitDepth - 8) (8.6.1).  PCM TBs
// too: a luma TB's qp goes into the deblocking map entry beside the edge bits (dbk_map_kernel: one byte at 8
// bits, where 64 and above would set them), and a coded TB's qp / 6 sets Dequant's shift (residual.h).
inline bool qp_ok(const p265r_params& p, const p265r_tb& t) {
    return t.qp <= 51 + 6 * ((t.c_idx ? p.bit_depth_chroma : p.bit_depth_luma) - 8);
}

// The fields of a TB record that the packing and the residual kernels read (class, size, job): validate_picture
// checks them for the TBs the CTUs list, the counting pass for every coded TB of the array.  Else P265R_EINVAL.
inline bool tb_fields_ok(const p265r_params& p, const p265r_tb& t) {
    return t.log2_size >= 2 && t.log2_size <= 5 && t.c_idx <= 2 && qp_ok(p, t);
}
// ... and that its dense N x N levels lie inside the picture's coefficients (a sparse TB's coef_off indexes
// entries: sparse_validate_tb).  Else P265R_ERANGE.
inline bool tb_coef_ok(const p265r_tb& t, uint64_t n_coef, bool sparse) {
    if (!(t.flags & (P265R_TB_CBF | P265R_TB_PCM)) || (sparse && tb_is_sparse(t))) return true;
    return (uint64_t)t.coef_off + ((uint64_t)1 << (2 * t.log2_size)) <= n_coef;
}

}  // namespace

int validate_picture(const p265r_params& p, const Geo& geo, const p265r_picture& pic, bool sparse) {
    const auto sz = pic_size(p, pic);
    const int pw = sz[0], ph = sz[1];
    if (pw > p.pic_width || ph > p.pic_height || pw % 8 || ph % 8 || pw <= 0 || ph <= 0) return P265R_EINVAL;
    if (pic.reserved) return P265R_EINVAL;
    Geo g = geo;
    g.wc = (pw + (1 << g.ctb_log2) - 1) >> g.ctb_log2;
    g.hc = (ph + (1 << g.ctb_log2) - 1) >> g.ctb_log2;
    const int n_ctus = g.wc * g.hc;
    if (!pic.ctus || (!pic.tbs && pic.n_tbs) || (!pic.coef && pic.n_coef)) return P265R_EINVAL;
    if (pic.flags & ~P265R_PIC_RECON_INPUT) return P265R_EINVAL;
    // (monochrome: the reconstruction is the luma plane alone; recon[1..2] are never read)
    if ((pic.flags & P265R_PIC_RECON_INPUT) && (!pic.recon[0] || (!geo.mono && (!pic.recon[1] || !pic.recon[2])))) return P265R_EINVAL;
    const int ctb = 1 << p.ctb_log2_size;
    const int max_tbs = 3 * (ctb / 4) * (ctb / 4) / 2;                  // all-4x4 luma + 4x4 chroma per 8x8
    for (int rs = 0; rs < n_ctus; ++rs) {
        const p265r_ctu& c = pic.ctus[rs];
        if ((uint64_t)c.tb_begin + c.tb_count > pic.n_tbs) return P265R_ERANGE;
        if (c.tb_count > max_tbs) return P265R_EINVAL;                  // more TBs than 4x4 units
        for (int k = 0; k < 2; ++k) {
            const int v = ((c.deblock_offsets >> (4 * k)) & 15) ^ 8;   // biased: -6..6 -> 2..14
            if (v < 2 || v > 14) return P265R_EINVAL;
        }
        for (int k = 0; k < 3; ++k) {
            if (c.sao_type[k] > 2) return P265R_EINVAL;
            if (c.sao_type[k] == 2 && c.sao_class[k] > 3) return P265R_EINVAL;
            if (c.sao_type[k] == 1 && c.sao_class[k] > 31) return P265R_EINVAL;
        }
        // Cb and Cr share SaoTypeIdx and SaoEoClass (7.4.9.3.2; sao.py:57-59, 75-77)
        if (c.sao_type[1] != c.sao_type[2] || (c.sao_type[1] == 2 && c.sao_class[1] != c.sao_class[2])) return P265R_EINVAL;
        // monochrome (ChromaArrayType 0): no chroma SAO, no chroma TB (the kernels have no plane to put them in)
        if (geo.mono && (c.sao_type[1] | c.sao_type[2])) return P265R_EINVAL;
        const int cx0 = (rs % g.wc) * ctb, cy0 = (rs / g.wc) * ctb;
        int n_luma = 0, n_chroma = 0;
        for (uint32_t i = c.tb_begin; i < c.tb_begin + c.tb_count; ++i) {
            const p265r_tb& t = pic.tbs[i];
            if (t.c_idx == 0 && ++n_luma > (ctb / 4) * (ctb / 4)) return P265R_EINVAL;   // intra_prep.h kMaxCtuLuma
            if (t.c_idx && ++n_chroma > 2 * (ctb / 8) * (ctb / 8)) return P265R_EINVAL;  // kMaxCtuChroma
            if (!tb_fields_ok(p, t) || t.pred_mode > 34) return P265R_EINVAL;
            if (geo.mono && t.c_idx) return P265R_EINVAL;
            if (t.c_idx && t.log2_size > 4) return P265R_EINVAL;        // 4:2:0 chroma TBs are 4..16
            const int sub = t.c_idx ? 1 : 0;
            const int n = 1 << t.log2_size;
            const int xl = t.x << sub, yl = t.y << sub, nl = n << sub;
            if (xl + nl > pw || yl + nl > ph) return P265R_ERANGE;
            if (xl < cx0 || yl < cy0 || xl + nl > cx0 + ctb || yl + nl > cy0 + ctb) return P265R_ERANGE;
            if ((t.x & 3) || (t.y & 3) || (t.x & (n - 1)) || (t.y & (n - 1))) return P265R_EINVAL;
            if (!tb_coef_ok(t, pic.n_coef, sparse)) return P265R_ERANGE;
            if (t.flags & ~0x0fu) return P265R_EINVAL;
        }
    }
    return P265R_OK;
}

int plan_upload(const p265r_params& p, const Geo& g, int n_ctus, int xg, bool split, int num_cus, const p265r_picture* pics,
                const p265r_sparse_coef* sp, int n_pics, UploadPlan* plan) {
    if (!pics || n_pics <= 0 || !plan) return P265R_EINVAL;
    if (n_pics > 65535) return P265R_ERANGE;                     // pictures index a grid dimension
    for (int i = 0; i < n_pics; ++i)
        if ((pics[i].flags ^ pics[0].flags) & P265R_PIC_RECON_INPUT) return P265R_EINVAL;
    UploadPlan& u = *plan;
    u = UploadPlan{};
    u.n_pics = n_pics;
    u.nc = n_ctus;
    u.sparse = sp != nullptr;
    u.recon_input = (pics[0].flags & P265R_PIC_RECON_INPUT) != 0;
    u.psize.resize(n_pics);
    u.pnc.resize(n_pics);
    u.pnf.resize(n_pics);
    for (int i = 0; i < n_pics; ++i) {
        u.psize[i] = pic_size(p, pics[i]);
        const int wc = (u.psize[i][0] + (1 << g.ctb_log2) - 1) >> g.ctb_log2, hc = (u.psize[i][1] + (1 << g.ctb_log2) - 1) >> g.ctb_log2;
        u.pnc[i] = wc * hc;
        u.pnf[i] = (size_t)((u.psize[i][0] + 7) / 8) * ((u.psize[i][1] + 7) / 8);
        u.ragged |= u.psize[i][0] != g.w || u.psize[i][1] != g.h;
    }
    // ---- pool sizing per class (per picture, so pictures can be packed in parallel) ----
    std::vector<std::array<size_t, N_POOLS>> cnt_pool(n_pics);
    std::vector<std::array<int, RC_NUM>> cnt_job(n_pics);
    std::vector<int> crc(n_pics, 0);
    std::vector<std::array<size_t, RC_NUM>> cnt_nz(sp ? n_pics : 0);    // sparse: entries per class
    parallel_for(n_pics, [&](int i) {
        // every record of every picture is checked (pictures are independent), then its coded TBs are counted
        // per class with thread-local counters, stored once (neighbouring pictures' counters share cache
        // lines).  Every TB of the array is packed, so the fields the packing reads are checked here for all
        // of them (validate_picture checks the TBs the CTUs reference, by position); one pass per picture
        // right after its validation, while its TB array is still in the cache
        const p265r_picture& pic = pics[i];
        if ((crc[i] = validate_picture(p, g, pic, sp != nullptr)) != 0) return;
        // (sparse: every entry of every TB is checked here, on the host, in the same pass -- the expand
        // kernel trusts pos)
        if (sp && !sp[i].nz && sp[i].n_nz) { crc[i] = P265R_EINVAL; return; }
        std::array<size_t, N_POOLS> cp{};
        std::array<int, RC_NUM> cj{};
        std::array<size_t, RC_NUM> cn{};
        for (uint32_t t = 0; t < pic.n_tbs; ++t) {
            const p265r_tb& tb = pic.tbs[t];
            if (sp) {                                  // (a local code: crc's elements share cache lines)
                const int rc = sparse_validate_tb(tb, sp[i].nz, sp[i].n_nz, pic.n_coef);
                if (rc) { crc[i] = rc; return; }
            }
            if (!(tb.flags & (P265R_TB_CBF | P265R_TB_PCM))) continue;
            if (!tb_fields_ok(p, tb) || (g.mono && tb.c_idx)) { crc[i] = P265R_EINVAL; return; }
            if (!tb_coef_ok(tb, pic.n_coef, sp != nullptr)) { crc[i] = P265R_ERANGE; return; }
            const int cls = tb_class(tb);
            cp[cls] += (size_t)1 << (2 * tb.log2_size);
            if (cls < RC_NUM) {
                ++cj[cls];
                if (sp) cn[cls] += tb_sparse_count(tb);
            }
        }
        cnt_pool[i] = cp;
        cnt_job[i] = cj;
        if (sp) cnt_nz[i] = cn;
    });
    for (int i = 0; i < n_pics; ++i)
        if (crc[i]) return crc[i];
    // per-picture start offsets (row n_pics: the totals)
    u.pool_at.resize(n_pics + 1);
    u.job_at.resize(n_pics + 1);
    u.tb_at.resize(n_pics + 1);
    u.nf_at.resize(n_pics + 1);
    for (int i = 0; i < n_pics; ++i) {
        u.n_tbs_total += pics[i].n_tbs;
        for (int c = 0; c < N_POOLS; ++c) u.pool_sz[c] += cnt_pool[i][c];
        for (int c = 0; c < RC_NUM; ++c) u.n_jobs[c] += cnt_job[i][c];
    }
    for (int c = 0; c < N_POOLS; ++c) { u.pool_base[c] = u.pool_total; u.pool_total += u.pool_sz[c]; }
    // the row kernel addresses every residual as a signed 32-bit int16 offset relative to the
    // residual pool: raw samples down to -(pool_total + 128) (coefficient pool + its pad), the
    // zero block and the fast jobs' over-read up to pool_total + 512 + 64
    if (u.pool_total + 2048 > (size_t)INT32_MAX) return P265R_ERANGE;
    {
        size_t pf[N_POOLS];
        std::copy(u.pool_base, u.pool_base + N_POOLS, pf);
        int jf[RC_NUM] = {};
        size_t tf = 0, nf = 0;
        for (int i = 0; i <= n_pics; ++i) {
            for (int c = 0; c < N_POOLS; ++c) { u.pool_at[i][c] = pf[c]; if (i < n_pics) pf[c] += cnt_pool[i][c]; }
            for (int c = 0; c < RC_NUM; ++c) { u.job_at[i][c] = jf[c]; if (i < n_pics) jf[c] += cnt_job[i][c]; }
            u.tb_at[i] = tf;
            u.nf_at[i] = nf;
            if (i < n_pics) { tf += pics[i].n_tbs; nf += pics[i].nofilter ? 1 : 0; }
        }
        u.n_nf = nf;
    }
    // ---- device layout -----------------------------------------------------------
    u.sao = p.sample_adaptive_offset != 0;
    for (int i = 0; i < n_pics && !u.dbk; ++i)
        for (int rs = 0; rs < u.pnc[i]; ++rs)
            if (pics[i].ctus[rs].flags & P265R_CTU_DEBLOCK) { u.dbk = true; break; }
    u.lf = u.sao || u.dbk;                       // separate output planes
    u.pel_bytes = g.pel16 ? 2 : 1;               // bytes per sample
    const size_t pb = u.pel_bytes, nc = (size_t)n_ctus;
    const size_t plane_bytes[3] = {(size_t)g.stride[0] * g.h * pb, (size_t)g.stride[1] * g.ch * pb, (size_t)g.stride[2] * g.ch * pb};
    // (monochrome: plane_bytes[1..2] = 0 -- a picture is its luma plane; plane_off[1..2] are unused)
    u.mono = g.mono != 0;
    u.plane_off[0] = 0;
    u.plane_off[1] = align_up(plane_bytes[0], 256);
    u.plane_off[2] = u.plane_off[1] + align_up(plane_bytes[1], 256);
    u.pic_plane_bytes = align_up(plane_bytes[0], 256) + 2 * align_up(plane_bytes[1], 256);
    size_t off = 0;
    u.o_pics = off; off = align_up(off + sizeof(DevPic) * n_pics, 256);
    // error word (+ the row kernel's per-CU workgroup slots, kRowCuSlots x 16 B, intra_rows.h)
    // cross-group row kernel (a batch whose chains fit xg workgroups each on the CUs): its progress words
    // follow the CU slots (cleared together per run), its lines get their own range
    u.xg_ok = !g.mono && xg > 0 && split && 2 * (long long)n_pics * xg <= num_cus;   // (not offered to monochrome)
    // (+ one row ticket per chain)
    const size_t xg_prog_bytes = u.xg_ok ? sizeof(int) * 2 * ((size_t)g.hc + 1) * n_pics : 0;
    u.o_err = off; off = align_up(off + 256 + kRowCuSlots * 16 + xg_prog_bytes, 256);
    u.o_xgl = off;
    if (u.xg_ok) off = align_up(off + 2 * (size_t)g.hc * ((size_t)(g.wc + 2) << g.ctb_log2) * n_pics, 256);
    u.o_ctus = off; off = align_up(off + sizeof(p265r_ctu) * nc * n_pics, 256);
    u.o_tbs = off; off = align_up(off + sizeof(p265r_tb) * u.n_tbs_total, 256);
    // both pools padded by 64 B: the intra kernel reads fixed-shape 32-B runs
    // (the row kernel reads every residual relative to the residual pool: raw TBs at negative
    // offsets into the coefficient pool, uncoded halves from a zero block after the residuals;
    // fast jobs read one sample per lane, lanes past the TB up to 126 B beyond it)
    u.o_pool = off; off = align_up(off + sizeof(int16_t) * u.pool_total + 256, 256);
    u.o_res = off; off = align_up(off + sizeof(int16_t) * u.pool_total + 1024, 256);
    for (int c = 0; c < RC_NUM; ++c) { u.o_jobs[c] = off; off = align_up(off + sizeof(ResJob) * u.n_jobs[c], 256); }
    // intra jobs (same index space as the TB records) + per-CTU job counts
    u.o_ijobs = off; off = align_up(off + sizeof(IntraJob) * u.n_tbs_total, 256);
    u.o_jcount = off; off = align_up(off + 4 * sizeof(uint32_t) * nc * n_pics, 256);
    u.o_nf = off;
    u.nf_bytes = (size_t)g.nf_w * ((g.h + 7) / 8);
    off = align_up(off + u.nf_bytes * u.n_nf, 256);
    u.map_bytes = u.nf_bytes << g.pel16;                           // uint16 entries above 8 bits (loopfilter.h)
    u.o_map = off; if (u.dbk) off = align_up(off + u.map_bytes * n_pics, 256);
    u.o_rec = off; off += u.pic_plane_bytes * n_pics;
    u.o_out = off; if (u.lf) off += u.pic_plane_bytes * n_pics;
    u.total = align_up(off, 256);

    // ---- host staging and chunks ---------------------------------------------------
    u.s_jobs = sp ? align_up(u.o_pool + sizeof(int16_t) * u.pool_sz[RC_RAW], 256) : u.o_res;
    u.s_nf = u.s_jobs + (u.o_ijobs - u.o_jobs[0]);
    u.n_chunks = std::max(1, std::min(n_pics / 8, 16));
    size_t n_jobs_total = 0;
    for (int i = 0; sp && i < n_pics; ++i)
        for (int c = 0; c < RC_NUM; ++c) u.nz_total += cnt_nz[i][c];
    for (int c = 0; c < RC_NUM; ++c) n_jobs_total += (size_t)u.n_jobs[c];
    if (u.nz_total > (size_t)UINT32_MAX) return P265R_ERANGE;       // begin words are 32-bit entry indices
    const size_t beg_words = sp ? n_jobs_total + (size_t)u.n_chunks * RC_NUM : 0;
    u.s_ent = align_up(u.s_nf + u.nf_bytes * u.n_nf, 256);
    u.s_beg = u.s_ent + align_up(sizeof(uint32_t) * u.nz_total, 256);
    u.sp_need = sp ? align_up(sizeof(uint32_t) * u.nz_total, 256) + align_up(sizeof(uint32_t) * beg_words, 256) : 0;
    u.stage_need = sp ? u.s_ent + u.sp_need : u.s_nf + u.nf_bytes * u.n_nf;
    if (sp) {
        u.ent_at.resize(n_pics);
        u.beg_at.resize(n_pics);
        size_t ef = 0, bf = 0;
        for (int k = 0; k < u.n_chunks; ++k)
            for (int c = 0; c < RC_NUM; ++c) {
                u.ent_kc.push_back(ef);
                u.beg_kc.push_back(bf);
                for (int i = u.chunk_lo(k); i < u.chunk_lo(k + 1); ++i) {
                    u.ent_at[i][c] = ef; ef += cnt_nz[i][c];
                    u.beg_at[i][c] = bf; bf += (size_t)cnt_job[i][c];
                }
                ++bf;                                            // the class range's closing word
            }
        u.ent_kc.push_back(ef);
        u.beg_kc.push_back(bf);
    }
    // recon input in a wide context: the planes of an 8-bit component go up as uint16_t, widened into the staging
    // buffer behind everything else
    if (u.recon_input && g.pel16 && (g.bd[0] <= 8 || (!g.mono && g.bd[1] <= 8))) {
        u.s_wide = align_up(u.stage_need, 256);
        u.wide_at.assign(n_pics, {SIZE_MAX, SIZE_MAX, SIZE_MAX});
        size_t wf = u.s_wide;
        for (int i = 0; i < n_pics; ++i)
            for (int c = 0; c < (g.mono ? 1 : 3); ++c) {
                if (g.bd[c] > 8) continue;
                u.wide_at[i][c] = wf;
                wf = align_up(wf + sizeof(uint16_t) * (size_t)(u.psize[i][0] >> (c ? 1 : 0)) * (size_t)(u.psize[i][1] >> (c ? 1 : 0)), 256);
            }
        u.stage_need = wf;
    }
    return P265R_OK;
}

CopyList UploadPlan::chunk_copies(int k) const {
    const int p0 = chunk_lo(k), p1 = chunk_lo(k + 1);
    CopyList l;
    const size_t ctu_bytes = sizeof(p265r_ctu) * (size_t)nc;
    l.add(false, o_ctus + ctu_bytes * p0, o_ctus + ctu_bytes * p0, ctu_bytes * (p1 - p0));
    l.add(false, o_tbs + sizeof(p265r_tb) * tb_at[p0], o_tbs + sizeof(p265r_tb) * tb_at[p0], sizeof(p265r_tb) * (tb_at[p1] - tb_at[p0]));
    for (int c = sparse ? (int)RC_RAW : 0; c < N_POOLS; ++c) {
        const size_t q0 = pool_at[p0][c], q1 = pool_at[p1][c];
        l.add(false, o_pool + sizeof(int16_t) * q0, o_pool + sizeof(int16_t) * (sparse ? q0 - pool_base[RC_RAW] : q0), sizeof(int16_t) * (q1 - q0));
    }
    for (int c = 0; c < RC_NUM; ++c) {
        const size_t j0 = (size_t)job_at[p0][c], j1 = (size_t)job_at[p1][c];
        l.add(false, o_jobs[c] + sizeof(ResJob) * j0, s_jobs + (o_jobs[c] - o_jobs[0]) + sizeof(ResJob) * j0, sizeof(ResJob) * (j1 - j0));
    }
    l.add(false, o_nf + nf_bytes * nf_at[p0], s_nf + nf_bytes * nf_at[p0], nf_bytes * (nf_at[p1] - nf_at[p0]));
    if (sparse) {
        const size_t e0 = ent_kc[k * RC_NUM], e1 = ent_kc[(k + 1) * RC_NUM], b0 = beg_kc[k * RC_NUM], b1 = beg_kc[(k + 1) * RC_NUM];
        l.add(true, sizeof(uint32_t) * e0, s_ent + sizeof(uint32_t) * e0, sizeof(uint32_t) * (e1 - e0));
        l.add(true, (s_beg - s_ent) + sizeof(uint32_t) * b0, s_beg + sizeof(uint32_t) * b0, sizeof(uint32_t) * (b1 - b0));
    }
    return l;
}

std::array<ZeroRange, 3> UploadPlan::gap_zeros() const {
    const size_t ctus_end = o_ctus + sizeof(p265r_ctu) * (size_t)nc * n_pics;
    const size_t tbs_end = o_tbs + sizeof(p265r_tb) * n_tbs_total;
    const size_t pool_end = o_pool + sizeof(int16_t) * pool_total;
    return {ZeroRange{ctus_end, o_tbs - ctus_end}, ZeroRange{tbs_end, o_pool - tbs_end}, ZeroRange{pool_end, o_res - pool_end}};
}

void pack_picture(const UploadPlan& u, int i, const p265r_picture* pics, const p265r_sparse_coef* sp, unsigned char* stage,
                  unsigned char* dbase, DevPic* out) {
    const p265r_picture& pic = pics[i];
    const size_t nc = (size_t)u.nc;
    p265r_ctu* ctu_dst = reinterpret_cast<p265r_ctu*>(stage + u.o_ctus) + (size_t)i * nc;
    std::memcpy(ctu_dst, pic.ctus, sizeof(p265r_ctu) * u.pnc[i]);
    if ((size_t)u.pnc[i] < nc) std::memset(ctu_dst + u.pnc[i], 0, sizeof(p265r_ctu) * (nc - u.pnc[i]));
    p265r_tb* tb_dst = reinterpret_cast<p265r_tb*>(stage + u.o_tbs) + u.tb_at[i];
    int16_t* h_pool = reinterpret_cast<int16_t*>(stage + u.o_pool);
    const size_t pool_first = sp ? u.pool_base[RC_RAW] : 0;           // sparse: the raw slab alone is staged
    uint32_t* h_ent = sp ? reinterpret_cast<uint32_t*>(stage + u.s_ent) : nullptr;
    uint32_t* h_beg = sp ? reinterpret_cast<uint32_t*>(stage + u.s_beg) : nullptr;
    ResJob* h_jobs[RC_NUM];
    size_t pool_fill[N_POOLS];
    int job_fill[RC_NUM];
    size_t ent_fill[RC_NUM] = {}, beg_fill[RC_NUM] = {};
    for (int c = 0; c < N_POOLS; ++c) pool_fill[c] = u.pool_at[i][c];
    for (int c = 0; c < RC_NUM; ++c) {
        h_jobs[c] = reinterpret_cast<ResJob*>(stage + u.s_jobs + (u.o_jobs[c] - u.o_jobs[0]));
        job_fill[c] = u.job_at[i][c];
        if (sp) { ent_fill[c] = u.ent_at[i][c]; beg_fill[c] = u.beg_at[i][c]; }
    }
    for (uint32_t t = 0; t < pic.n_tbs; ++t) {
        p265r_tb tb = pic.tbs[t];
        if (sp) std::memset(tb.reserved, 0, sizeof(tb.reserved));     // (the entry count: not part of the image)
        if (tb.flags & (P265R_TB_CBF | P265R_TB_PCM)) {
            const int cls = tb_class(tb);
            const size_t nn = (size_t)1 << (2 * tb.log2_size);
            if (sp && cls < RC_NUM) {              // sparse TB: its entries + the index of the first
                const uint32_t cnt = tb_sparse_count(pic.tbs[t]);
                h_beg[beg_fill[cls]++] = (uint32_t)ent_fill[cls];
                if (cnt) std::memcpy(h_ent + ent_fill[cls], sp[i].nz + tb.coef_off, sizeof(uint32_t) * cnt);
                ent_fill[cls] += cnt;
            } else {
                int16_t* dst = h_pool + (pool_fill[cls] - pool_first);
                const int16_t* src = pic.coef + tb.coef_off;
                switch (tb.log2_size) {            // fixed sizes: inlined vector moves, no memcpy call per TB
                    case 2: std::memcpy(dst, src, 16 * sizeof(int16_t)); break;
                    case 3: std::memcpy(dst, src, 64 * sizeof(int16_t)); break;
                    case 4: std::memcpy(dst, src, 256 * sizeof(int16_t)); break;
                    default: std::memcpy(dst, src, 1024 * sizeof(int16_t)); break;
                }
            }
            tb.coef_off = (uint32_t)pool_fill[cls];
            if (cls < RC_NUM) h_jobs[cls][job_fill[cls]++] = ResJob{tb.coef_off, tb.qp, tb.flags, tb.log2_size, tb.c_idx};
            pool_fill[cls] += nn;
        }
        tb_dst[t] = tb;
    }
    DevPic& dp = *out;
    dp.ctus = reinterpret_cast<const p265r_ctu*>(dbase + u.o_ctus) + (size_t)i * nc;
    dp.tbs = reinterpret_cast<const p265r_tb*>(dbase + u.o_tbs) + u.tb_at[i];
    dp.jobs = reinterpret_cast<IntraJob*>(dbase + u.o_ijobs) + u.tb_at[i];
    dp.jcount = reinterpret_cast<uint32_t*>(dbase + u.o_jcount) + 4 * (size_t)i * nc;
    dp.dbk_map = u.dbk ? dbase + u.o_map + u.map_bytes * i : nullptr;
    dp.pool_rel = -(int32_t)((u.o_res - u.o_pool) / sizeof(int16_t));
    dp.zero_off = (uint32_t)u.pool_total;
    dp.wh = (uint32_t)u.psize[i][0] | (uint32_t)u.psize[i][1] << 16;
    dp.pad_ = 0;
    for (int c = 0; c < 3; ++c) {
        dp.rec[c] = dbase + u.o_rec + u.pic_plane_bytes * i + u.plane_off[c];
        dp.out[c] = u.lf ? dbase + u.o_out + u.pic_plane_bytes * i + u.plane_off[c] : dp.rec[c];
        if (u.mono && c) dp.rec[c] = dp.out[c] = nullptr;            // no chroma planes exist
    }
    if (pic.nofilter) {
        std::memcpy(stage + u.s_nf + u.nf_at[i] * u.nf_bytes, pic.nofilter, u.pnf[i]);   // (slot of the context size)
        dp.nofilter = dbase + u.o_nf + u.nf_at[i] * u.nf_bytes;
    } else {
        dp.nofilter = nullptr;
    }
}

void widen_plane(const UploadPlan& u, int i, int c, const p265r_picture* pics, unsigned char* stage) {
    const size_t n = (size_t)(u.psize[i][0] >> (c ? 1 : 0)) * (size_t)(u.psize[i][1] >> (c ? 1 : 0));
    const uint8_t* src = static_cast<const uint8_t*>(pics[i].recon[c]);
    uint16_t* dst = reinterpret_cast<uint16_t*>(stage + u.wide_at[i][c]);
    for (size_t k = 0; k < n; ++k) dst[k] = src[k];
}

void close_chunk(const UploadPlan& u, int k, unsigned char* stage) {
    uint32_t* h_beg = reinterpret_cast<uint32_t*>(stage + u.s_beg);
    for (int c = 0; c < RC_NUM; ++c) h_beg[u.beg_kc[k * RC_NUM + c + 1] - 1] = (uint32_t)u.ent_kc[k * RC_NUM + c + 1];
}

void pack_header(const UploadPlan& u, const DevPic* dev_pics, unsigned char* stage) {
    const size_t pics_end = u.o_pics + sizeof(DevPic) * u.n_pics;
    std::memcpy(stage + u.o_pics, dev_pics, sizeof(DevPic) * u.n_pics);
    std::memset(stage + pics_end, 0, u.o_ctus - pics_end);
}

}  // namespace p265r
