// mono_check.cpp -- stand-alone host check of the monochrome (chroma_format_idc 0) forms of the batch upload's
// planner / validation and of the device-side output's layout (make mono-check builds it with
// p265_amd/csrc/upload_host.cpp, sparse_host.cpp and export_host.cpp under -fsanitize=address,undefined and runs it
// on the CPU).  Every buffer is a heap allocation of exactly the advertised size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../p265_amd/csrc/export_host.h"
#include "../p265_amd/csrc/sparse_host.h"
#include "../p265_amd/csrc/upload_host.h"

using namespace p265r;

static int g_fail = 0;
static const char* g_case = "";
#define EXPECT(cond)                                                                                    \
    do {                                                                                                \
        if (!(cond)) { if (++g_fail <= 40) std::printf("FAIL %s:%d [%s]: %s\n", __FILE__, __LINE__, g_case, #cond); } \
    } while (0)

struct Ctx {
    p265r_params p{};
    Geo g{};
    int n_ctus = 0;
};

// parameters and geometry as p265r_create derives them (mono: cw = ch = 0, no chroma stride)
static Ctx make_ctx(int w, int h, int ctb_log2, int bit_depth, bool mono, bool sao) {
    Ctx c;
    c.p.version = P265R_ABI_VERSION;
    c.p.pic_width = (uint16_t)w;
    c.p.pic_height = (uint16_t)h;
    c.p.chroma_format_idc = mono ? 0 : 1;
    c.p.bit_depth_luma = c.p.bit_depth_chroma = (uint8_t)bit_depth;
    c.p.ctb_log2_size = (uint8_t)ctb_log2;
    c.p.min_tb_log2_size = 2;
    c.p.max_tb_log2_size = 5;
    c.p.sample_adaptive_offset = sao;
    Geo& g = c.g;
    g.w = w; g.h = h;
    g.mono = mono ? 1 : 0;
    g.cw = mono ? 0 : w / 2; g.ch = mono ? 0 : h / 2;
    g.stride[0] = (int)align_up(g.w, 64);
    g.stride[1] = g.stride[2] = (int)align_up(g.cw, 64);
    g.ctb_log2 = ctb_log2;
    g.wc = (w + (1 << ctb_log2) - 1) >> ctb_log2;
    g.hc = (h + (1 << ctb_log2) - 1) >> ctb_log2;
    g.bd[0] = g.bd[1] = g.bd[2] = bit_depth;
    g.pel16 = bit_depth > 8;
    g.nf_w = (w + 7) / 8;
    c.n_ctus = g.wc * g.hc;
    return c;
}

template <class T>
static void exact(std::vector<T>& v) { v = std::vector<T>(v); }      // capacity == size: ASan sees the true end

struct Pic {
    int w = 0, h = 0;
    std::vector<p265r_ctu> ctus;
    std::vector<p265r_tb> tbs;
    std::vector<int16_t> coef;
    std::vector<uint8_t> recon_y;
    uint32_t flags = 0;
    p265r_picture view(const Ctx& c) const {
        p265r_picture p{};
        p.ctus = ctus.data();
        p.tbs = tbs.empty() ? nullptr : tbs.data();
        p.n_tbs = (uint32_t)tbs.size();
        p.coef = coef.empty() ? nullptr : coef.data();
        p.n_coef = coef.size();
        p.flags = flags;
        if (flags & P265R_PIC_RECON_INPUT) p.recon[0] = const_cast<uint8_t*>(recon_y.data());
        if (w != c.p.pic_width || h != c.p.pic_height) { p.pic_width = (uint16_t)w; p.pic_height = (uint16_t)h; }
        return p;
    }
};

// a picture of 8x8 luma TBs (every third one coded), optionally with the 4x4 chroma pair a 4:2:0 picture has
static Pic make_pic(const Ctx& c, int w, int h, bool chroma, unsigned seed) {
    Pic pic;
    pic.w = w; pic.h = h;
    const int ctb = 1 << c.g.ctb_log2;
    const int wc = (w + ctb - 1) / ctb, hc = (h + ctb - 1) / ctb;
    pic.ctus.assign((size_t)wc * hc, p265r_ctu{});
    unsigned k = seed;
    for (int rs = 0; rs < wc * hc; ++rs) {
        p265r_ctu& u = pic.ctus[rs];
        u.tb_begin = (uint32_t)pic.tbs.size();
        u.flags = P265R_CTU_LF_ACROSS_SLICES | ((seed & 1) ? P265R_CTU_DEBLOCK : 0);
        u.deblock_offsets = (seed & 1) ? P265R_DEBLOCK_OFFSETS(0, 0) : 0;
        u.sao_type[0] = (uint8_t)(c.p.sample_adaptive_offset ? 1 + rs % 2 : 0);
        u.sao_class[0] = (uint8_t)(rs % 4);
        const int x0 = (rs % wc) * ctb, y0 = (rs / wc) * ctb;
        for (int y = y0; y < y0 + ctb && y < h; y += 8)
            for (int x = x0; x < x0 + ctb && x < w; x += 8) {
                for (int ci = 0; ci < (chroma ? 3 : 1); ++ci) {
                    p265r_tb t{};
                    t.x = (uint16_t)(ci ? x / 2 : x);
                    t.y = (uint16_t)(ci ? y / 2 : y);
                    t.log2_size = (uint8_t)(ci ? 2 : 3);
                    t.c_idx = (uint8_t)ci;
                    t.pred_mode = (uint8_t)(k % 35);
                    t.qp = (uint8_t)(20 + k % 20);
                    if (++k % 3 == 0) {
                        t.flags = P265R_TB_CBF;
                        t.coef_off = (uint32_t)pic.coef.size();
                        pic.coef.resize(pic.coef.size() + (ci ? 16 : 64), (int16_t)(k % 7 - 3));
                    }
                    pic.tbs.push_back(t);
                }
            }
        u.tb_count = (uint16_t)(pic.tbs.size() - u.tb_begin);
    }
    exact(pic.ctus); exact(pic.tbs); exact(pic.coef);
    return pic;
}

static int plan(const Ctx& c, const std::vector<Pic>& pics, UploadPlan* u, bool sparse = false) {
    std::vector<p265r_picture> v;
    for (const Pic& p : pics) v.push_back(p.view(c));
    exact(v);
    std::vector<p265r_sparse_coef> sp(sparse ? pics.size() : 0);
    return plan_upload(c.p, c.g, c.n_ctus, 4, true, 256, v.data(), sparse ? sp.data() : nullptr, (int)v.size(), u);
}

static void check_layout_and_pack() {
    for (int bd : {8, 10})
        for (int lg : {4, 5, 6}) {
            g_case = "plan";
            const Ctx m = make_ctx(136, 72, lg, bd, true, true), f = make_ctx(136, 72, lg, bd, false, true);
            std::vector<Pic> mp, fp;
            for (int i = 0; i < 5; ++i) {
                mp.push_back(make_pic(m, 136, 72, false, 17u * (unsigned)i + (unsigned)lg));
                fp.push_back(make_pic(f, 136, 72, true, 17u * (unsigned)i + (unsigned)lg));
            }
            UploadPlan um, uf;
            EXPECT(plan(m, mp, &um) == P265R_OK);
            EXPECT(plan(f, fp, &uf) == P265R_OK);
            const size_t pb = bd > 8 ? 2 : 1;
            // one luma plane per picture, nothing for chroma; the cross-group layout is not offered
            EXPECT(um.mono && !uf.mono);
            EXPECT(um.pic_plane_bytes == align_up((size_t)m.g.stride[0] * 72 * pb, 256));
            EXPECT(uf.pic_plane_bytes > um.pic_plane_bytes);
            EXPECT(um.plane_off[0] == 0 && um.plane_off[1] == um.pic_plane_bytes && um.plane_off[2] == um.pic_plane_bytes);
            EXPECT(!um.xg_ok && uf.xg_ok);
            EXPECT(um.total < uf.total);
            EXPECT(um.sao && um.lf && um.o_out == um.o_rec + um.pic_plane_bytes * 5);
            EXPECT(um.total >= um.o_out + um.pic_plane_bytes * 5);
            // pack every picture into a staging buffer of exactly stage_need bytes: the DevPic table has no chroma plane
            g_case = "pack";
            std::vector<unsigned char> stage(um.stage_need);
            std::vector<p265r_picture> v;
            for (const Pic& p : mp) v.push_back(p.view(m));
            unsigned char* dbase = reinterpret_cast<unsigned char*>((uintptr_t)1 << 32);   // (addresses only)
            std::vector<DevPic> dev(5);
            for (int i = 0; i < 5; ++i) pack_picture(um, i, v.data(), nullptr, stage.data(), dbase, &dev[i]);
            pack_header(um, dev.data(), stage.data());
            for (int i = 0; i < 5; ++i) {
                EXPECT(dev[i].rec[0] == dbase + um.o_rec + um.pic_plane_bytes * i);
                EXPECT(dev[i].out[0] == dbase + um.o_out + um.pic_plane_bytes * i);
                EXPECT(!dev[i].rec[1] && !dev[i].rec[2] && !dev[i].out[1] && !dev[i].out[2]);
                EXPECT(dev[i].wh == (136u | 72u << 16));
            }
            int jobs_m = 0, jobs_f = 0;
            for (int k = 0; k < RC_NUM; ++k) { jobs_m += um.n_jobs[k]; jobs_f += uf.n_jobs[k]; }
            EXPECT(jobs_m > 0 && jobs_m < jobs_f && um.n_jobs[RC_DCT4] == 0 && uf.n_jobs[RC_DCT4] > 0);
        }
}

static void check_refusals() {
    const Ctx m = make_ctx(136, 72, 5, 8, true, true), f = make_ctx(136, 72, 5, 8, false, true);
    UploadPlan u;
    g_case = "chroma TB";
    {   // the 4:2:0 picture in a monochrome context, dense and sparse; accepted in its own
        std::vector<Pic> p{make_pic(m, 136, 72, false, 3), make_pic(f, 136, 72, true, 4)};
        EXPECT(plan(m, p, &u) == P265R_EINVAL);
        EXPECT(plan(f, p, &u) == P265R_OK);
        EXPECT(plan(m, {p[0]}, &u) == P265R_OK);
    }
    {   // one chroma TB among the luma ones, listed by its CTU
        Pic p = make_pic(m, 136, 72, false, 5);
        p.tbs[7].c_idx = 1; p.tbs[7].x = 0; p.tbs[7].y = 0; p.tbs[7].log2_size = 2; p.tbs[7].flags = 0;
        EXPECT(plan(m, {p}, &u) == P265R_EINVAL);
        p.tbs[7].c_idx = 2;
        EXPECT(plan(m, {p}, &u) == P265R_EINVAL);
    }
    {   // a coded chroma TB that no CTU lists (the packing would still make a residual job of it)
        Pic p = make_pic(m, 136, 72, false, 6);
        p265r_tb t{};
        t.log2_size = 2; t.c_idx = 1; t.flags = P265R_TB_CBF; t.coef_off = 0; t.qp = 30;
        p.tbs.push_back(t);
        exact(p.tbs);
        EXPECT(plan(m, {p}, &u) == P265R_EINVAL);
        p.tbs.back().c_idx = 0;
        EXPECT(plan(m, {p}, &u) == P265R_OK);
    }
    g_case = "chroma SAO";
    for (int k = 1; k <= 2; ++k) {
        Pic p = make_pic(m, 136, 72, false, 7);
        p.ctus[2].sao_type[1] = p.ctus[2].sao_type[2] = (uint8_t)k;       // (Cb = Cr: legal in 4:2:0)
        EXPECT(plan(m, {p}, &u) == P265R_EINVAL);
        EXPECT(validate_picture(f.p, f.g, p.view(f), false) == P265R_OK);
        p.ctus[2].sao_type[1] = 0;                                        // Cr alone: refused by either rule
        EXPECT(plan(m, {p}, &u) == P265R_EINVAL);
    }
    g_case = "recon input";
    {
        Pic p = make_pic(m, 136, 72, false, 8);
        p.flags = P265R_PIC_RECON_INPUT;
        p.recon_y.assign((size_t)136 * 72, 128);
        exact(p.recon_y);
        EXPECT(plan(m, {p}, &u) == P265R_OK && u.recon_input);            // luma alone: recon[1..2] stay null
        EXPECT(plan(f, {p}, &u) == P265R_EINVAL);                         // 4:2:0 wants all three
        p265r_picture v = p.view(m);
        v.recon[0] = nullptr;
        EXPECT(validate_picture(m.p, m.g, v, false) == P265R_EINVAL);
    }
    g_case = "ragged";
    {
        const Ctx big = make_ctx(96, 96, 5, 8, true, false);
        std::vector<Pic> p{make_pic(big, 96, 96, false, 1), make_pic(big, 72, 40, false, 2), make_pic(big, 8, 96, false, 3)};
        EXPECT(plan(big, p, &u) == P265R_OK && u.ragged && u.mono);
        p.push_back(make_pic(big, 104, 96, false, 4));
        EXPECT(plan(big, p, &u) == P265R_EINVAL);
        p.back() = make_pic(big, 72, 44, false, 5);
        EXPECT(plan(big, p, &u) == P265R_EINVAL);
    }
    g_case = "malformed";
    {   // the ordinary checks hold in a monochrome context too
        Pic p = make_pic(m, 136, 72, false, 9);
        Pic q = p; q.tbs[3].x = 132; EXPECT(plan(m, {q}, &u) != P265R_OK);
        q = p; q.tbs[3].qp = 52; EXPECT(plan(m, {q}, &u) == P265R_EINVAL);
        q = p; q.tbs[2].flags = P265R_TB_CBF; q.tbs[2].coef_off = (uint32_t)q.coef.size() - 8; EXPECT(plan(m, {q}, &u) == P265R_ERANGE);
        q = p; q.ctus[1].tb_begin = (uint32_t)q.tbs.size(); EXPECT(plan(m, {q}, &u) == P265R_ERANGE);
        q = p; q.ctus[0].sao_type[0] = 3; EXPECT(plan(m, {q}, &u) == P265R_EINVAL);
    }
}

static int layout(const Ctx& c, p265r_export_desc* d, uint32_t align = 1, int w = 0, int h = 0) {
    return p265r_export_layout(&c.p, w, h, d, align);
}

static void check_export() {
    g_case = "export";
    for (int bd : {8, 10, 12}) {
        const Ctx m = make_ctx(72, 40, 4, bd, true, true), f = make_ctx(72, 40, 4, bd, false, true);
        const uint64_t es = bd > 8 ? 2 : 1;
        p265r_export_desc d{};
        d.format = P265R_FMT_PLANAR;
        d.crop_left = 1; d.crop_right = 3; d.crop_top = 1; d.crop_bottom = 1;
        EXPECT(layout(m, &d) == P265R_OK);
        EXPECT(d.pitch[0] == 68 * es && d.plane_off[0] == 0 && d.frame_bytes == 68 * es * 38);
        EXPECT(d.pitch[1] == 0 && d.pitch[2] == 0 && d.plane_off[1] == 0 && d.plane_off[2] == 0);
        EXPECT(layout(f, &d) == P265R_EINVAL);
        ExportShape s;
        uint64_t slot = 0;
        EXPECT(export_check_desc(d, bd, &s, true) == P265R_OK && s.n_planes == 1 && s.mono == 1);
        EXPECT(export_check_layout(d, s, 72, 40, &slot) == P265R_OK && slot == d.frame_bytes);
        EXPECT(export_check_layout(d, s, 64, 40, &slot) == P265R_OK && slot < d.frame_bytes);    // a smaller picture fits
        EXPECT(export_check_layout(d, s, 80, 40, &slot) == P265R_EINVAL);                        // a wider one does not
        EXPECT(export_check_desc(d, bd, &s, false) == P265R_EINVAL);
        p265r_export_desc bad = d;
        bad.pitch[0] = 68 * es - es; EXPECT(export_check_layout(bad, s, 72, 40, nullptr) == P265R_EINVAL);
        bad = d; bad.frame_bytes -= es; EXPECT(export_check_layout(bad, s, 72, 40, nullptr) == P265R_EINVAL);
        bad = d; bad.crop_left = 71; EXPECT(layout(m, &bad) == P265R_EINVAL);
        // semi-planar: Y + CbCr, even crops only
        p265r_export_desc n{};
        n.format = P265R_FMT_SEMIPLANAR;
        n.sample = bd > 8 ? P265R_SMP_MSB16 : P265R_SMP_NATIVE;
        n.crop_left = 2; n.crop_bottom = 4;
        EXPECT(layout(m, &n, 64) == P265R_OK);
        EXPECT(n.pitch[0] == n.pitch[1] && n.pitch[0] % 64 == 0 && n.pitch[0] >= 70 * es && n.plane_off[1] == n.pitch[0] * 36);
        EXPECT(n.frame_bytes == n.pitch[0] * (36 + 18));
        EXPECT(export_check_desc(n, bd, &s, true) == P265R_OK && s.n_planes == 2);
        for (int k = 0; k < 4; ++k) {
            p265r_export_desc o = n;
            (k == 0 ? o.crop_left : k == 1 ? o.crop_right : k == 2 ? o.crop_top : o.crop_bottom) = 1;
            EXPECT(layout(m, &o) == P265R_EINVAL);
            o.format = P265R_FMT_RGB_PACKED; o.sample = P265R_SMP_U8;
            EXPECT(layout(m, &o) == P265R_OK);
            EXPECT(layout(f, &o) == P265R_EINVAL);
        }
        // RGB: matrix / upsample / range still validated
        p265r_export_desc r{};
        r.format = P265R_FMT_RGB_PLANAR; r.sample = P265R_SMP_F16; r.crop_top = 3;
        EXPECT(layout(m, &r) == P265R_OK && r.pitch[0] == 72 * 2 && r.pitch[2] == 72 * 2 && r.frame_bytes == 3 * 72 * 2 * 37);
        r.matrix = 3; EXPECT(layout(m, &r) == P265R_EINVAL);
        r.matrix = 0; r.upsample = 2; EXPECT(layout(m, &r) == P265R_EINVAL);
        r.upsample = 1; r.full_range = 2; EXPECT(layout(m, &r) == P265R_EINVAL);
        r.full_range = 1; r.sample = P265R_SMP_MSB16; EXPECT(layout(m, &r) == P265R_EINVAL);
        // a chroma bit depth that differs is ignored for monochrome parameters only
        Ctx m2 = m, f2 = f;
        m2.p.bit_depth_chroma = (uint8_t)(bd == 8 ? 12 : 8);
        f2.p.bit_depth_chroma = m2.p.bit_depth_chroma;
        p265r_export_desc e{};
        EXPECT(layout(m2, &e) == P265R_OK && e.frame_bytes == 72 * 40 * es);
        EXPECT(layout(f2, &e) == P265R_EINVAL);
        EXPECT(layout(m, &e, 1, 0x10000, 8) == P265R_EINVAL);
        EXPECT(p265r_export_layout(nullptr, 0, 0, &e, 1) == P265R_EINVAL && p265r_export_layout(&m.p, 0, 0, nullptr, 1) == P265R_EINVAL);
    }
}

int main() {
    check_layout_and_pack();
    check_refusals();
    check_export();
    if (g_fail) { std::printf("mono_check: %d failures\n", g_fail); return 1; }
    std::printf("mono_check: ok\n");
    return 0;
}
