// upload_check.cpp -- stand-alone host check of the batch upload's planner and packer (make upload-check builds
// it with p265_amd/csrc/upload_host.cpp and sparse_host.cpp under -fsanitize=address,undefined and runs it on
// the CPU).  Builds small batches by hand -- every buffer a heap allocation of exactly the advertised size, the
// staging buffer of exactly stage_need bytes -- and checks the device layout, the DevPic table, the staged
// bytes, the chunk copy lists and the code of every malformed input.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../p265_amd/csrc/sparse_host.h"
#include "../p265_amd/csrc/upload_host.h"

using namespace p265r;

static int g_fail = 0;
static const char* g_case = "";
#define EXPECT(cond)                                                                                    \
    do {                                                                                                \
        if (!(cond)) { if (++g_fail <= 40) std::printf("FAIL %s:%d [%s]: %s\n", __FILE__, __LINE__, g_case, #cond); } \
    } while (0)

// ---- a context's parameters and geometry, as p265r_create derives them ---------------------------------
struct Ctx {
    p265r_params p{};
    Geo g{};
    int n_ctus = 0, xg = 4, num_cus = 256;
    bool split = true;
};

static Ctx make_ctx(int w, int h, int ctb_log2, int bit_depth, bool sao) {
    Ctx c;
    c.p.version = P265R_ABI_VERSION;
    c.p.pic_width = (uint16_t)w;
    c.p.pic_height = (uint16_t)h;
    c.p.chroma_format_idc = 1;
    c.p.bit_depth_luma = c.p.bit_depth_chroma = (uint8_t)bit_depth;
    c.p.ctb_log2_size = (uint8_t)ctb_log2;
    c.p.min_tb_log2_size = 2;
    c.p.max_tb_log2_size = 5;
    c.p.sample_adaptive_offset = sao;
    Geo& g = c.g;
    g.w = w; g.h = h;
    g.cw = w / 2; g.ch = h / 2;
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

// ---- pictures -------------------------------------------------------------------------------------------
template <class T>
static void exact(std::vector<T>& v) { v = std::vector<T>(v); }      // capacity == size: ASan sees the true end

struct Pic {
    int w = 0, h = 0;
    std::vector<p265r_ctu> ctus;
    std::vector<p265r_tb> tbs, stbs;      // dense records; their sparse form (p265r_sparsify)
    std::vector<int16_t> coef, raw;
    std::vector<uint32_t> nz;
    std::vector<uint8_t> nf;
    uint32_t flags = 0, reserved = 0;
    bool null_ctus = false;
    void* recon[3] = {nullptr, nullptr, nullptr};
    void sparsify() {
        p265r_picture p = view(false);
        uint64_t n_nz = 0, n_raw = 0;
        if (p265r_sparsify(&p, nullptr, nullptr, 0, &n_nz, nullptr, 0, &n_raw) != P265R_OK) { EXPECT(!"sparsify"); return; }
        stbs.assign(tbs.size(), p265r_tb{});
        nz.assign(n_nz, 0);
        raw.assign(n_raw, 0);
        EXPECT(p265r_sparsify(&p, stbs.data(), nz.data(), nz.size(), nullptr, raw.data(), raw.size(), nullptr) == P265R_OK);
    }
    p265r_picture view(bool sparse) const {
        p265r_picture p{};
        const auto& t = sparse ? stbs : tbs;
        const auto& c = sparse ? raw : coef;
        p.ctus = null_ctus ? nullptr : ctus.data();
        p.tbs = t.empty() ? nullptr : t.data();
        p.n_tbs = (uint32_t)t.size();
        p.flags = flags;
        p.coef = c.empty() ? nullptr : c.data();
        p.n_coef = c.size();
        p.nofilter = nf.empty() ? nullptr : nf.data();
        for (int k = 0; k < 3; ++k) p.recon[k] = recon[k];
        p.pic_width = (uint16_t)w;
        p.pic_height = (uint16_t)h;
        p.reserved = reserved;
        return p;
    }
};

enum Kind { MIXED, NONE_CODED, RAW_ONLY };
struct PicOpt { int w, h; bool nf, dbk; Kind kind; bool unlisted; };

static p265r_tb random_tb(std::mt19937& rng, const Ctx& cx, Kind kind, int cx0, int cy0, int rw, int rh, Pic* pic) {
    p265r_tb t{};
    t.c_idx = (uint8_t)(rng() % 3);
    const int sub = t.c_idx ? 1 : 0;
    int lg = 2 + (int)(rng() % 4);
    while (((1 << lg) << sub) > std::min(rw, rh) || (sub && lg > 4)) --lg;
    const int n = 1 << lg;
    t.log2_size = (uint8_t)lg;
    t.x = (uint16_t)((cx0 >> sub) + (int)(rng() % ((rw >> sub) / n)) * n);
    t.y = (uint16_t)((cy0 >> sub) + (int)(rng() % ((rh >> sub) / n)) * n);
    t.pred_mode = (uint8_t)(rng() % 35);
    t.qp = (uint8_t)(rng() % (52 + 6 * (cx.p.bit_depth_luma - 8)));
    const uint32_t r = rng() % 7;
    if (kind == MIXED)
        t.flags = r == 0 ? 0 : r == 1 ? P265R_TB_PCM : r == 2 ? (P265R_TB_CBF | P265R_TB_BYPASS) : r == 3 ? (P265R_TB_CBF | P265R_TB_TSKIP)
                : r == 4 ? P265R_TB_BYPASS : P265R_TB_CBF;
    else if (kind == RAW_ONLY)
        t.flags = r < 3 ? P265R_TB_PCM : r < 6 ? (P265R_TB_CBF | P265R_TB_BYPASS) : 0;
    if (t.flags & (P265R_TB_CBF | P265R_TB_PCM)) {
        t.coef_off = (uint32_t)pic->coef.size();
        for (int k = 0; k < n * n; ++k) pic->coef.push_back(rng() % 4 ? (int16_t)0 : (int16_t)(rng() | 1));
    }
    return t;
}

static Pic make_pic(const Ctx& cx, const PicOpt& o, uint32_t seed) {
    std::mt19937 rng(seed);
    Pic pic;
    pic.w = o.w; pic.h = o.h;
    const int ctb = 1 << cx.g.ctb_log2;
    const int wc = (o.w + ctb - 1) / ctb, hc = (o.h + ctb - 1) / ctb;
    for (int rs = 0; rs < wc * hc; ++rs) {
        const int cx0 = (rs % wc) * ctb, cy0 = (rs / wc) * ctb;
        p265r_ctu c{};
        c.tb_begin = (uint32_t)pic.tbs.size();
        c.tb_count = (uint16_t)(rng() % 5);
        c.tile_id = (uint16_t)rng();
        c.slice_addr = (uint32_t)rng();
        c.flags = (uint8_t)((o.dbk && rs % 2 == 0 ? P265R_CTU_DEBLOCK : 0) | (rng() & P265R_CTU_LF_ACROSS_SLICES));
        c.sao_type[0] = (uint8_t)(rng() % 3);
        c.sao_type[1] = c.sao_type[2] = (uint8_t)(rng() % 3);
        c.sao_class[0] = (uint8_t)(rng() % (c.sao_type[0] == 2 ? 4 : 32));
        c.sao_class[1] = c.sao_class[2] = (uint8_t)(rng() % (c.sao_type[1] == 2 ? 4 : 32));
        c.deblock_offsets = P265R_DEBLOCK_OFFSETS((int)(rng() % 13) - 6, (int)(rng() % 13) - 6);
        for (auto& row : c.sao_offset) for (auto& v : row) v = (int8_t)rng();
        for (int k = 0; k < c.tb_count; ++k)
            pic.tbs.push_back(random_tb(rng, cx, o.kind, cx0, cy0, std::min(ctb, o.w - cx0), std::min(ctb, o.h - cy0), &pic));
        pic.ctus.push_back(c);
    }
    if (o.unlisted) {                       // TBs of the array that no CTU lists: packed all the same
        for (int k = 0; k < 3; ++k) pic.tbs.push_back(random_tb(rng, cx, k == 2 ? NONE_CODED : MIXED, 0, 0, 8, 8, &pic));
        pic.tbs.back().qp = 255;            // (not coded: its fields are not read)
    }
    if (o.nf) for (int k = 0; k < ((o.w + 7) / 8) * ((o.h + 7) / 8); ++k) pic.nf.push_back((uint8_t)(rng() & 1));
    exact(pic.ctus); exact(pic.tbs); exact(pic.coef); exact(pic.nf);
    pic.sparsify();
    return pic;
}

struct Batch {
    std::vector<Pic> pics;
    std::vector<p265r_picture> views(bool sparse) const {
        std::vector<p265r_picture> v;
        for (const Pic& p : pics) v.push_back(p.view(sparse));
        exact(v);
        return v;
    }
    std::vector<p265r_sparse_coef> coefs() const {
        std::vector<p265r_sparse_coef> v;
        for (const Pic& p : pics) v.push_back(p265r_sparse_coef{p.nz.empty() ? nullptr : p.nz.data(), p.nz.size()});
        exact(v);
        return v;
    }
};

static int plan_of(const Ctx& cx, const Batch& b, bool sparse, UploadPlan* u) {
    const auto pv = b.views(sparse);
    const auto sc = b.coefs();
    return plan_upload(cx.p, cx.g, cx.n_ctus, cx.xg, cx.split, cx.num_cus, pv.data(), sparse ? sc.data() : nullptr, (int)pv.size(), u);
}

// ---- one good batch: plan, pack, and check everything ----------------------------------------------------
static void check_batch(const char* name, const Ctx& cx, const Batch& b, bool sparse, int want_chunks) {
    g_case = name;
    const int n = (int)b.pics.size();
    const auto pv = b.views(sparse);
    const auto sc = b.coefs();
    const p265r_sparse_coef* sp = sparse ? sc.data() : nullptr;
    UploadPlan u;
    EXPECT(plan_upload(cx.p, cx.g, cx.n_ctus, cx.xg, cx.split, cx.num_cus, pv.data(), sp, n, &u) == P265R_OK);
    if (u.n_pics != n) { EXPECT(!"plan"); return; }
    const Geo& g = cx.g;
    const size_t nc = (size_t)cx.n_ctus, pb = g.pel16 ? 2 : 1;

    // counts of our own, from the input records
    size_t pool_sz[N_POOLS] = {}, n_jobs[RC_NUM] = {}, n_tbs = 0, n_nf = 0, nz_total = 0, jobs_total = 0;
    bool dbk = false;
    for (const Pic& pic : b.pics) {
        n_tbs += pic.tbs.size();
        n_nf += !pic.nf.empty();
        for (const p265r_ctu& c : pic.ctus) dbk |= (c.flags & P265R_CTU_DEBLOCK) != 0;
        for (const p265r_tb& t : pic.stbs) {
            if (!(t.flags & (P265R_TB_CBF | P265R_TB_PCM))) continue;
            const int cls = tb_class(t);
            pool_sz[cls] += (size_t)1 << (2 * t.log2_size);
            if (cls < RC_NUM) { ++n_jobs[cls]; ++jobs_total; nz_total += tb_sparse_count(t); }
        }
    }
    size_t pool_total = 0;
    for (int c = 0; c < N_POOLS; ++c) { EXPECT(u.pool_base[c] == pool_total && u.pool_sz[c] == pool_sz[c]); pool_total += pool_sz[c]; }
    for (int c = 0; c < RC_NUM; ++c) EXPECT((size_t)u.n_jobs[c] == n_jobs[c]);
    const bool lf = cx.p.sample_adaptive_offset || dbk;
    EXPECT(u.pool_total == pool_total && u.n_tbs_total == n_tbs && u.n_nf == n_nf && u.dbk == dbk && u.lf == lf);
    EXPECT(u.sao == (cx.p.sample_adaptive_offset != 0) && u.sparse == sparse && !u.recon_input);
    EXPECT(u.n_chunks == want_chunks && u.chunk_lo(0) == 0 && u.chunk_lo(u.n_chunks) == n);
    const bool xg_ok = cx.xg > 0 && cx.split && 2 * n * cx.xg <= cx.num_cus;
    EXPECT(u.xg_ok == xg_ok);

    // layout: aligned, ordered, every range large enough, the pads of the two pools
    const size_t nf_bytes = (size_t)g.nf_w * ((g.h + 7) / 8);
    const size_t plane[3] = {(size_t)g.stride[0] * g.h * pb, (size_t)g.stride[1] * g.ch * pb, (size_t)g.stride[2] * g.ch * pb};
    EXPECT(u.plane_off[0] == 0 && u.plane_off[1] >= plane[0] && u.plane_off[2] >= u.plane_off[1] + plane[1] &&
           u.pic_plane_bytes >= u.plane_off[2] + plane[2] && u.plane_off[1] % 256 == 0 && u.plane_off[2] % 256 == 0 && u.pic_plane_bytes % 256 == 0);
    struct R { size_t off, size; };
    std::vector<R> rs = {{u.o_pics, sizeof(DevPic) * n},
                         {u.o_err, 256 + (size_t)kRowCuSlots * 16 + (xg_ok ? sizeof(int) * 2 * ((size_t)g.hc + 1) * n : 0)},
                         {u.o_xgl, xg_ok ? 2 * (size_t)g.hc * ((size_t)(g.wc + 2) << g.ctb_log2) * n : 0},
                         {u.o_ctus, sizeof(p265r_ctu) * nc * n}, {u.o_tbs, sizeof(p265r_tb) * n_tbs},
                         {u.o_pool, 2 * pool_total + 256}, {u.o_res, 2 * pool_total + 1024}};
    for (int c = 0; c < RC_NUM; ++c) rs.push_back({u.o_jobs[c], sizeof(ResJob) * n_jobs[c]});
    rs.push_back({u.o_ijobs, sizeof(IntraJob) * n_tbs});
    rs.push_back({u.o_jcount, 16 * nc * n});
    rs.push_back({u.o_nf, nf_bytes * n_nf});
    rs.push_back({u.o_map, dbk ? (nf_bytes << g.pel16) * n : 0});
    rs.push_back({u.o_rec, u.pic_plane_bytes * n});
    rs.push_back({u.o_out, lf ? u.pic_plane_bytes * n : 0});
    rs.push_back({u.total, 0});
    EXPECT(rs[0].off == 0);
    for (size_t k = 0; k + 1 < rs.size(); ++k) {
        EXPECT(rs[k].off % 256 == 0 && rs[k].off + rs[k].size <= rs[k + 1].off);
        EXPECT(rs[k].size == 0 || rs[k].off < rs[k + 1].off);
    }
    EXPECT(u.total % 256 == 0 && u.o_res - u.o_pool >= 2 * pool_total + 256 && u.o_jobs[0] - u.o_res >= 2 * pool_total + 1024);
    EXPECT(u.nf_bytes == nf_bytes && u.map_bytes == nf_bytes << g.pel16 && u.pel_bytes == pb);
    EXPECT(u.sp_need == 0 || sparse);
    EXPECT(u.nz_total == (sparse ? nz_total : 0));

    // pack chunk by chunk into sentinel-filled staging buffers of exactly stage_need bytes: a byte is written
    // iff it comes out the same over two different fills.  owner[i]: the chunk that wrote byte i (n_chunks: the
    // header, -1: nobody)
    unsigned char* dbase = reinterpret_cast<unsigned char*>((uintptr_t)1 << 40);
    std::vector<DevPic> dp(n);
    std::vector<unsigned char> stage(u.stage_need, 0xa5);       // (a byte nobody wrote does not read as zero)
    std::vector<int> owner(u.stage_need, -1);
    for (int k = 0; k <= u.n_chunks; ++k) {
        std::vector<unsigned char> a(u.stage_need, 0xa5), z(u.stage_need, 0x5a);
        for (unsigned char* s : {a.data(), z.data()}) {
            if (k == u.n_chunks) { pack_header(u, dp.data(), s); continue; }
            const int p0 = u.chunk_lo(k), p1 = u.chunk_lo(k + 1);
            parallel_for(p1 - p0, [&](int j) { pack_picture(u, p0 + j, pv.data(), sp, s, dbase, &dp[p0 + j]); });
            if (sparse) close_chunk(u, k, s);
        }
        for (size_t i = 0; i < u.stage_need; ++i)
            if (a[i] == z[i]) { EXPECT(owner[i] == -1); owner[i] = k; stage[i] = a[i]; }
    }

    // copy lists: inside both sides, no overlap on either, only the chunk's own bytes, every written byte once
    std::vector<unsigned char> host_hit(u.stage_need, 0), dev_hit(u.total, 0), land_hit(u.sp_need, 0);
    size_t bytes = 0;
    // the one thing copied unwritten: the rest of a no-filter slot (context size) behind a smaller picture's map
    std::vector<size_t> slot_map(n_nf, 0);
    for (int i = 0; i < n; ++i) if (!b.pics[i].nf.empty() && u.nf_at[i] < n_nf) slot_map[u.nf_at[i]] = b.pics[i].nf.size();
    auto slot_tail = [&](size_t off) {
        return off >= u.s_nf && off < u.s_nf + nf_bytes * n_nf && (off - u.s_nf) % nf_bytes >= slot_map[(off - u.s_nf) / nf_bytes];
    };
    auto take = [&](const H2dCopy& c, int k) {
        std::vector<unsigned char>& dst = c.to_landing ? land_hit : dev_hit;
        EXPECT(c.bytes > 0 && c.host_off + c.bytes <= u.stage_need && c.dst_off + c.bytes <= dst.size());
        if (c.host_off + c.bytes > u.stage_need || c.dst_off + c.bytes > dst.size()) return;
        for (size_t i = 0; i < c.bytes; ++i) {
            EXPECT(!host_hit[c.host_off + i]++ && !dst[c.dst_off + i]++);
            EXPECT(owner[c.host_off + i] == k || (owner[c.host_off + i] == -1 && slot_tail(c.host_off + i)));
        }
        bytes += c.bytes;
    };
    for (int k = 0; k < u.n_chunks; ++k) {
        const CopyList l = u.chunk_copies(k);
        EXPECT(l.n <= (int)(sizeof(l.v) / sizeof(l.v[0])));
        for (const H2dCopy& c : l) { EXPECT(c.to_landing ? sparse : c.dst_off >= u.o_ctus && c.dst_off + c.bytes <= u.o_rec); take(c, k); }
    }
    take(u.header_copy(), u.n_chunks);
    EXPECT(u.header_copy().bytes == u.o_ctus && !u.header_copy().to_landing);
    for (size_t i = 0; i < u.stage_need; ++i) EXPECT(owner[i] == -1 || host_hit[i] == 1);
    const size_t common = u.o_ctus + sizeof(p265r_ctu) * nc * n + sizeof(p265r_tb) * n_tbs + sizeof(ResJob) * jobs_total + nf_bytes * n_nf;
    EXPECT(bytes == common + (sparse ? 2 * pool_sz[RC_RAW] + 4 * nz_total + 4 * (jobs_total + (size_t)u.n_chunks * RC_NUM) : 2 * pool_total));
    // the gap memsets: inside the image, over bytes no copy writes, up to the next array
    const auto gaps = u.gap_zeros();
    EXPECT(gaps[0].off + gaps[0].bytes == u.o_tbs && gaps[1].off + gaps[1].bytes == u.o_pool && gaps[2].off + gaps[2].bytes == u.o_res);
    EXPECT(gaps[0].off == u.o_ctus + sizeof(p265r_ctu) * nc * n && gaps[1].off == u.o_tbs + sizeof(p265r_tb) * n_tbs && gaps[2].off == u.o_pool + 2 * pool_total);
    for (const ZeroRange& z : gaps)
        for (size_t i = 0; i < z.bytes; ++i) EXPECT(!dev_hit[z.off + i]);

    // the header and the DevPic table
    EXPECT(std::memcmp(stage.data() + u.o_pics, dp.data(), sizeof(DevPic) * n) == 0);
    for (size_t i = u.o_pics + sizeof(DevPic) * n; i < u.o_ctus; ++i) EXPECT(stage[i] == 0 && owner[i] == u.n_chunks);
    for (int i = 0; i < n; ++i) {
        const DevPic& d = dp[i];
        const Pic& pic = b.pics[i];
        EXPECT(d.pool_rel == -(int32_t)((u.o_res - u.o_pool) / 2) && d.zero_off == pool_total && d.pad_ == 0);
        EXPECT(d.wh == ((uint32_t)pic.w | (uint32_t)pic.h << 16));
        EXPECT((const unsigned char*)d.ctus == dbase + u.o_ctus + sizeof(p265r_ctu) * nc * i);
        EXPECT((const unsigned char*)d.tbs == dbase + u.o_tbs + sizeof(p265r_tb) * u.tb_at[i]);
        EXPECT((unsigned char*)d.jobs == dbase + u.o_ijobs + sizeof(IntraJob) * u.tb_at[i]);
        EXPECT((unsigned char*)d.jcount == dbase + u.o_jcount + 16 * nc * i);
        EXPECT(d.dbk_map == (dbk ? dbase + u.o_map + (nf_bytes << g.pel16) * i : nullptr));
        for (int c = 0; c < 3; ++c) {
            EXPECT(d.rec[c] == dbase + u.o_rec + u.pic_plane_bytes * i + u.plane_off[c]);
            EXPECT(d.rec[c] + plane[c] <= dbase + u.o_out);
            if (lf) EXPECT(d.out[c] == dbase + u.o_out + u.pic_plane_bytes * i + u.plane_off[c] && d.out[c] + plane[c] <= dbase + u.total);
            else EXPECT(d.out[c] == d.rec[c]);
        }
        // CTU records, the slots beyond a ragged picture's own zero; the no-filter map
        const p265r_ctu* hc = reinterpret_cast<const p265r_ctu*>(stage.data() + u.o_ctus) + nc * i;
        EXPECT(u.pnc[i] == (int)pic.ctus.size() && std::memcmp(hc, pic.ctus.data(), sizeof(p265r_ctu) * pic.ctus.size()) == 0);
        for (size_t k = sizeof(p265r_ctu) * pic.ctus.size(); k < sizeof(p265r_ctu) * nc; ++k)
            EXPECT(reinterpret_cast<const unsigned char*>(hc)[k] == 0 && owner[u.o_ctus + sizeof(p265r_ctu) * nc * i + k] != -1);
        if (pic.nf.empty()) EXPECT(d.nofilter == nullptr);
        else {
            EXPECT(d.nofilter == dbase + u.o_nf + nf_bytes * u.nf_at[i] && u.nf_at[i] < n_nf && pic.nf.size() <= nf_bytes);
            EXPECT(std::memcmp(stage.data() + u.s_nf + nf_bytes * u.nf_at[i], pic.nf.data(), pic.nf.size()) == 0);
        }
    }

    // TB records, pool slabs, jobs, entries: walk the input in packing order with counters of our own
    const int16_t* h_pool = reinterpret_cast<const int16_t*>(stage.data() + u.o_pool);
    const uint32_t* h_ent = sparse ? reinterpret_cast<const uint32_t*>(stage.data() + u.s_ent) : nullptr;
    const uint32_t* h_beg = sparse ? reinterpret_cast<const uint32_t*>(stage.data() + u.s_beg) : nullptr;
    size_t fill[N_POOLS], job[RC_NUM] = {}, tb_at = 0;
    for (int c = 0; c < N_POOLS; ++c) fill[c] = u.pool_base[c];
    for (int k = 0; k < u.n_chunks; ++k) {
        size_t beg[RC_NUM], ent[RC_NUM] = {};
        // a class range of the chunk: the pictures' begin words in job order; entries: class-major inside the chunk
        size_t e_run = sparse ? u.ent_kc[k * RC_NUM] : 0;
        for (int c = 0; c < RC_NUM; ++c) {
            beg[c] = sparse ? u.beg_kc[k * RC_NUM + c] : 0;
            if (!sparse) continue;
            EXPECT(u.ent_kc[k * RC_NUM + c] == e_run);
            ent[c] = e_run;
            for (int i = u.chunk_lo(k); i < u.chunk_lo(k + 1); ++i)
                for (const p265r_tb& t : b.pics[i].stbs)
                    if ((t.flags & (P265R_TB_CBF | P265R_TB_PCM)) && tb_class(t) == c) e_run += tb_sparse_count(t);
        }
        for (int i = u.chunk_lo(k); i < u.chunk_lo(k + 1); ++i) {
            const Pic& pic = b.pics[i];
            EXPECT(u.tb_at[i] == tb_at);
            const auto& in = sparse ? pic.stbs : pic.tbs;
            const p265r_tb* out = reinterpret_cast<const p265r_tb*>(stage.data() + u.o_tbs) + tb_at;
            for (size_t t = 0; t < in.size(); ++t) {
                const p265r_tb &a = in[t], &o = out[t];
                EXPECT(a.x == o.x && a.y == o.y && a.log2_size == o.log2_size && a.c_idx == o.c_idx && a.pred_mode == o.pred_mode &&
                       a.flags == o.flags && a.qp == o.qp);
                if (sparse) EXPECT(!o.reserved[0] && !o.reserved[1] && !o.reserved[2]);
                else EXPECT(std::memcmp(a.reserved, o.reserved, 3) == 0);
                if (!(a.flags & (P265R_TB_CBF | P265R_TB_PCM))) { EXPECT(o.coef_off == a.coef_off); continue; }
                const int cls = tb_class(a);
                const size_t nn = (size_t)1 << (2 * a.log2_size);
                EXPECT(o.coef_off == fill[cls] && fill[cls] + nn <= u.pool_base[cls] + u.pool_sz[cls]);
                const int16_t* levels = pic.coef.data() + pic.tbs[t].coef_off;          // the dense input
                if (!sparse) EXPECT(std::memcmp(h_pool + fill[cls], levels, 2 * nn) == 0);
                else if (cls == RC_RAW) EXPECT(std::memcmp(h_pool + (fill[cls] - u.pool_base[RC_RAW]), levels, 2 * nn) == 0);
                else {
                    const uint32_t cnt = tb_sparse_count(a);
                    EXPECT(h_beg[beg[cls]] == ent[cls] && h_beg[beg[cls] + 1] == ent[cls] + cnt);     // the next job's, or the closing word
                    EXPECT(cnt == 0 || std::memcmp(h_ent + ent[cls], pic.nz.data() + a.coef_off, 4 * (size_t)cnt) == 0);
                    ++beg[cls];
                    ent[cls] += cnt;
                }
                if (cls < RC_NUM) {
                    const ResJob* j = reinterpret_cast<const ResJob*>(stage.data() + u.s_jobs + (u.o_jobs[cls] - u.o_jobs[0])) + job[cls]++;
                    EXPECT(j->off == o.coef_off && j->qp == a.qp && j->flags == a.flags && j->log2 == a.log2_size && j->c_idx == a.c_idx);
                }
                fill[cls] += nn;
            }
            tb_at += in.size();
        }
        for (int c = 0; c < RC_NUM && sparse; ++c) {         // each class range closed by the index past its last entry
            EXPECT(beg[c] + 1 == u.beg_kc[k * RC_NUM + c + 1] && ent[c] == u.ent_kc[k * RC_NUM + c + 1] && h_beg[beg[c]] == ent[c]);
            EXPECT((size_t)u.job_at[u.chunk_lo(k + 1)][c] == job[c]);
        }
    }
    EXPECT(u.tb_at[n] == n_tbs);
    for (int c = 0; c < N_POOLS; ++c) EXPECT(fill[c] == u.pool_base[c] + u.pool_sz[c] && u.pool_at[n][c] == fill[c]);
    if (sparse) {
        EXPECT(u.ent_kc.back() == nz_total && u.beg_kc.back() == jobs_total + (size_t)u.n_chunks * RC_NUM);
        EXPECT(u.s_beg - u.s_ent >= 4 * nz_total && u.sp_need >= (u.s_beg - u.s_ent) + 4 * u.beg_kc.back() && u.stage_need == u.s_ent + u.sp_need);
    }
}

// ---- the good batches -------------------------------------------------------------------------------------
static Batch make_batch(const Ctx& cx, int n, uint32_t seed, bool nf, bool dbk, Kind kind = MIXED) {
    Batch b;
    for (int i = 0; i < n; ++i)       // (a few pictures without a map, one without a coded TB, one with unlisted TBs)
        b.pics.push_back(make_pic(cx, PicOpt{cx.g.w, cx.g.h, nf && i % 3 != 1, dbk, i == 2 ? NONE_CODED : kind, i % 4 == 0}, seed * 1000 + i));
    return b;
}

static void good_batches() {
    static const int counts[] = {1, 8, 16, 17, 20, 27}, chunks[] = {1, 1, 2, 2, 2, 3};
    uint32_t seed = 1;
    for (int ctb = 4; ctb <= 6; ++ctb)
        for (int k = 0; k < 6; ++k) {
            const int n = counts[k];
            // vary with the case: bit depth, SAO, deblocking, maps, the cross-group kernel's conditions
            Ctx cx = make_ctx(64, 64, ctb, (k + ctb) % 2 ? 10 : 8, (k + ctb) % 3 != 0);
            if (k % 3 == 1) cx.num_cus = 64;
            if (k == 2) cx.split = false;
            if (k == 5) cx.xg = 0;
            const Batch b = make_batch(cx, n, seed++, k % 2 == 0, (k + ctb) % 4 < 2);
            char name[96];
            for (int sparse = 0; sparse < 2; ++sparse) {
                std::snprintf(name, sizeof name, "%s n=%d ctb=%d bd=%d", sparse ? "sparse" : "dense", n, 1 << ctb, cx.p.bit_depth_luma);
                check_batch(name, cx, b, sparse, chunks[k]);
            }
        }
    {   // chunk bounds: 20 -> 10 / 10, 17 -> 8 / 9, 27 -> 9 / 9 / 9
        UploadPlan u;
        u.n_pics = 20; u.n_chunks = 2; EXPECT(u.chunk_lo(1) == 10 && u.chunk_lo(2) == 20);
        u.n_pics = 17; EXPECT(u.chunk_lo(1) == 8 && u.chunk_lo(2) == 17);
        u.n_pics = 27; u.n_chunks = 3; EXPECT(u.chunk_lo(1) == 9 && u.chunk_lo(2) == 18 && u.chunk_lo(3) == 27);
    }
    for (int ctb = 4; ctb <= 6; ++ctb)
        for (int variant = 0; variant < 4; ++variant) {
            // no SAO and no deblocking (out == rec); a ragged batch; only PCM / bypass TBs; no coded TB at all
            const Ctx cx = make_ctx(64, 64, ctb, variant == 1 ? 10 : 8, variant == 1);
            Batch b;
            if (variant == 1) {
                static const int sz[4][2] = {{64, 64}, {40, 64}, {64, 8}, {8, 8}};
                for (int i = 0; i < 4; ++i) b.pics.push_back(make_pic(cx, PicOpt{sz[i][0], sz[i][1], i != 2, i == 1, MIXED, i == 3}, 7000 + 10 * ctb + i));
            } else {
                b = make_batch(cx, variant == 0 ? 9 : 3, 900 + 10 * ctb + variant, variant == 0, false, variant == 2 ? RAW_ONLY : variant == 3 ? NONE_CODED : MIXED);
                if (variant == 2) b.pics[2] = make_pic(cx, PicOpt{64, 64, false, false, RAW_ONLY, true}, 77);
            }
            static const char* names[] = {"plain", "ragged", "raw only", "none coded"};
            for (int sparse = 0; sparse < 2; ++sparse) check_batch(names[variant], cx, b, sparse, 1);
        }
}

// ---- malformed inputs: the code of each, read off the validation's order of checks ------------------------
// A 64x64 context, CTB 32.  Picture 0 has, per CTU, one luma 8x8 TB (coded, transformed) at the CTU's origin;
// CTU 0 also one PCM luma 4x4 at (8, 0) and one uncoded Cb 4x4; an uncoded TB that no CTU lists ends the array.
static Pic plain_pic(int w = 64, int h = 64, int ctb = 32) {
    Pic pic;
    pic.w = w; pic.h = h;
    const int wc = (w + ctb - 1) / ctb, hc = (h + ctb - 1) / ctb;
    auto add = [&](int x, int y, int lg, int c_idx, uint8_t flags) {
        p265r_tb t{};
        t.x = (uint16_t)x; t.y = (uint16_t)y; t.log2_size = (uint8_t)lg; t.c_idx = (uint8_t)c_idx; t.flags = flags; t.qp = 30;
        if (flags & (P265R_TB_CBF | P265R_TB_PCM)) {
            t.coef_off = (uint32_t)pic.coef.size();
            for (int k = 0; k < 1 << (2 * lg); ++k) pic.coef.push_back((int16_t)(k % 5 == 0 ? k + 1 : 0));
        }
        pic.tbs.push_back(t);
    };
    for (int rs = 0; rs < wc * hc; ++rs) {
        p265r_ctu c{};
        c.tb_begin = (uint32_t)pic.tbs.size();
        add((rs % wc) * ctb, (rs / wc) * ctb, 3, 0, P265R_TB_CBF);
        if (rs == 0) { add(8, 0, 2, 0, P265R_TB_PCM); add(0, 0, 2, 1, 0); }
        c.tb_count = (uint16_t)(pic.tbs.size() - c.tb_begin);
        pic.ctus.push_back(c);
    }
    add(0, 0, 2, 0, 0);
    exact(pic.ctus); exact(pic.tbs); exact(pic.coef);
    return pic;
}

struct Bad {
    const char* name;
    int code;
    bool sparse;                                     // the upload it is given to
    std::function<void(Batch&)> dense_edit;          // applied before the sparse form is derived
    std::function<void(Batch&)> sparse_edit;         // applied to the sparse form
};

static void rejections() {
    const Ctx cx = make_ctx(64, 64, 5, 8, true);
    const int E = P265R_EINVAL, R = P265R_ERANGE, OK = P265R_OK;
    auto tb = [](Batch& b, size_t t, int pic = 0) -> p265r_tb& { return b.pics[pic].tbs[t]; };   // 0: 8x8 Y, 1: PCM, 2: Cb, 3.., last: unlisted
    auto ctu = [](Batch& b, size_t rs) -> p265r_ctu& { return b.pics[0].ctus[rs]; };
    const auto none = [](Batch&) {};
    std::vector<Bad> bad = {
        {"good", OK, false, none, none},
        {"good sparse", OK, true, none, none},
        // TB fields
        {"log2 6", E, false, [&](Batch& b) { tb(b, 0).log2_size = 6; }, none},
        {"log2 1", E, false, [&](Batch& b) { tb(b, 2).log2_size = 1; }, none},
        {"chroma 32x32", E, false, [&](Batch& b) { tb(b, 2).log2_size = 5; }, none},
        {"c_idx 3", E, false, [&](Batch& b) { tb(b, 0).c_idx = 3; }, none},
        {"pred_mode 35", E, false, [&](Batch& b) { tb(b, 0).pred_mode = 35; }, none},
        {"pred_mode 35 outside the picture", E, false, [&](Batch& b) { tb(b, 0).pred_mode = 35; tb(b, 0).x = 64; }, none},
        {"qp 51", OK, false, [&](Batch& b) { tb(b, 0).qp = 51; }, none},
        {"qp 52", E, false, [&](Batch& b) { tb(b, 0).qp = 52; }, none},
        {"qp 52 PCM", E, false, [&](Batch& b) { tb(b, 1).qp = 52; }, none},
        {"qp 52 uncoded listed", E, false, [&](Batch& b) { tb(b, 2).qp = 52; }, none},
        {"qp 52 unlisted uncoded", OK, false, [&](Batch& b) { b.pics[0].tbs.back().qp = 52; }, none},
        {"qp 52 unlisted coded", E, false, [&](Batch& b) { b.pics[0].tbs.back().qp = 52; b.pics[0].tbs.back().flags = P265R_TB_CBF; }, none},
        {"log2 6 unlisted uncoded", OK, false, [&](Batch& b) { b.pics[0].tbs.back().log2_size = 6; }, none},
        {"log2 6 unlisted uncoded, sparse", E, true, [&](Batch& b) { b.pics[0].tbs.back().log2_size = 6; }, none},
        {"log2 6 unlisted coded", E, false, [&](Batch& b) { b.pics[0].tbs.back().log2_size = 6; b.pics[0].tbs.back().flags = P265R_TB_PCM; }, none},
        {"c_idx 3 unlisted coded", E, false, [&](Batch& b) { b.pics[0].tbs.back().c_idx = 3; b.pics[0].tbs.back().flags = P265R_TB_CBF; }, none},
        {"flags 0x10", E, false, [&](Batch& b) { tb(b, 2).flags = 0x10; }, none},
        {"flags 0x11", E, false, [&](Batch& b) { tb(b, 0).flags |= 0x10; }, none},
        {"flags 0x11 past the coefficients", R, false, [&](Batch& b) { tb(b, 0).flags |= 0x10; tb(b, 0).coef_off = (uint32_t)b.pics[0].coef.size(); }, none},
        // position
        {"x not a multiple of 4", E, false, [&](Batch& b) { tb(b, 1).x = 10; }, none},
        {"8x8 at x = 4", E, false, [&](Batch& b) { tb(b, 0).x = 4; }, none},
        {"outside the picture", R, false, [&](Batch& b) { tb(b, 0).x = 64; }, none},
        {"misaligned and outside the picture", R, false, [&](Batch& b) { tb(b, 0).x = 60; }, none},
        {"inside another CTB", R, false, [&](Batch& b) { tb(b, 0).x = 32; }, none},
        {"chroma inside another CTB", R, false, [&](Batch& b) { tb(b, 2).y = 16; }, none},
        {"outside a smaller picture", R, false, [&](Batch& b) { b.pics[0] = plain_pic(40, 64); b.pics[0].tbs[3].x = 40; }, none},
        {"a smaller picture", OK, false, [&](Batch& b) { b.pics[0] = plain_pic(40, 64); }, none},
        // coefficient range
        {"coef_off last fit", OK, false, [&](Batch& b) { tb(b, 1).coef_off = (uint32_t)b.pics[0].coef.size() - 16; }, none},
        {"coef_off one past the last fit", R, false, [&](Batch& b) { tb(b, 1).coef_off = (uint32_t)b.pics[0].coef.size() - 15; }, none},
        {"coef_off = n_coef", R, false, [&](Batch& b) { tb(b, 0).coef_off = (uint32_t)b.pics[0].coef.size(); }, none},
        {"coef_off = 2^32 - 1", R, false, [&](Batch& b) { tb(b, 0).coef_off = 0xffffffffu; }, none},
        {"unlisted coded TB past the coefficients", R, false,
         [&](Batch& b) { b.pics[0].tbs.back().flags = P265R_TB_PCM; b.pics[0].tbs.back().coef_off = (uint32_t)b.pics[0].coef.size() - 15; }, none},
        {"coef NULL with n_coef = 0 and a coded TB", R, false, [&](Batch& b) { b.pics[0].coef.clear(); exact(b.pics[0].coef); }, none},
        // CTU records
        {"tb_begin + tb_count overflows", R, false, [&](Batch& b) { ctu(b, 1).tb_begin = 0xffffffffu; }, none},
        {"tb_begin + tb_count past n_tbs", R, false, [&](Batch& b) { ctu(b, 3).tb_count = 3; }, none},
        {"tb range past n_tbs and a bad SAO type", R, false, [&](Batch& b) { ctu(b, 3).tb_count = 3; ctu(b, 3).sao_type[0] = 3; }, none},
        {"sao_type 3", E, false, [&](Batch& b) { ctu(b, 0).sao_type[0] = 3; }, none},
        {"edge class 4", E, false, [&](Batch& b) { ctu(b, 0).sao_type[0] = 2; ctu(b, 0).sao_class[0] = 4; }, none},
        {"edge class 3", OK, false, [&](Batch& b) { ctu(b, 0).sao_type[0] = 2; ctu(b, 0).sao_class[0] = 3; }, none},
        {"band position 32", E, false, [&](Batch& b) { ctu(b, 0).sao_type[0] = 1; ctu(b, 0).sao_class[0] = 32; }, none},
        {"Cb / Cr SAO types differ", E, false, [&](Batch& b) { ctu(b, 2).sao_type[1] = 1; }, none},
        {"Cb / Cr edge classes differ", E, false, [&](Batch& b) { ctu(b, 2).sao_type[1] = ctu(b, 2).sao_type[2] = 2; ctu(b, 2).sao_class[2] = 1; }, none},
        {"beta offset 7", E, false, [&](Batch& b) { ctu(b, 0).deblock_offsets = P265R_DEBLOCK_OFFSETS(7, 0); }, none},
        {"tc offset -7", E, false, [&](Batch& b) { ctu(b, 0).deblock_offsets = P265R_DEBLOCK_OFFSETS(0, -7); }, none},
        {"offsets -6 / 6", OK, false, [&](Batch& b) { ctu(b, 0).deblock_offsets = P265R_DEBLOCK_OFFSETS(-6, 6); }, none},
        // picture fields
        {"wider than the context", E, false, [&](Batch& b) { b.pics[0].w = 72; }, none},
        {"width not a multiple of 8", E, false, [&](Batch& b) { b.pics[0].w = 20; }, none},
        {"reserved set", E, false, [&](Batch& b) { b.pics[0].reserved = 1; }, none},
        {"ctus NULL", E, false, [&](Batch& b) { b.pics[0].null_ctus = true; }, none},
        {"unknown picture flag", E, false, [&](Batch& b) { b.pics[0].flags = 2; }, none},
        {"RECON_INPUT without planes", E, false, [&](Batch& b) { b.pics[0].flags = b.pics[1].flags = P265R_PIC_RECON_INPUT; }, none},
        {"mixed RECON_INPUT", E, false, [&](Batch& b) { b.pics[1].flags = P265R_PIC_RECON_INPUT; b.pics[1].recon[0] = b.pics[1].recon[1] = b.pics[1].recon[2] = &b; }, none},
        {"mixed RECON_INPUT before a range error", E, false, [&](Batch& b) { tb(b, 0).x = 64; b.pics[1].flags = P265R_PIC_RECON_INPUT; }, none},
        // the first failing picture's code
        {"picture 0 ERANGE, picture 1 EINVAL", R, false, [&](Batch& b) { tb(b, 0).x = 64; tb(b, 0, 1).qp = 52; }, none},
        {"picture 0 EINVAL, picture 1 ERANGE", E, false, [&](Batch& b) { tb(b, 0).qp = 52; tb(b, 0, 1).x = 64; }, none},
        // sparse records (the TBs of the sparse form: 0 is the 8x8 luma TB with 13 entries, 1 the PCM TB)
        {"entries out of order", E, true, none, [&](Batch& b) { std::swap(b.pics[0].nz[1], b.pics[0].nz[2]); }},
        {"entry repeated", E, true, none, [&](Batch& b) { b.pics[0].nz[2] = b.pics[0].nz[1]; }},
        {"entry pos = N*N", R, true, none, [&](Batch& b) { b.pics[0].nz[12] = 64 | 1u << 16; }},
        {"entry out of range and out of order", R, true, none, [&](Batch& b) { b.pics[0].nz[3] = 64 | 1u << 16; }},
        {"a count on a PCM TB", E, true, none, [&](Batch& b) { b.pics[0].stbs[1].reserved[0] = 1; }},
        {"a count on an uncoded TB", E, true, none, [&](Batch& b) { b.pics[0].stbs.back().reserved[0] = 1; }},
        {"count N*N + 1", E, true, none, [&](Batch& b) { b.pics[0].stbs[0].reserved[0] = 65; }},
        {"reserved[2]", E, true, none, [&](Batch& b) { b.pics[0].stbs[0].reserved[2] = 1; }},
        {"entries past n_nz", R, true, none, [&](Batch& b) { b.pics[0].stbs[0].coef_off = (uint32_t)b.pics[0].nz.size() - 12; }},
        {"no entries at all", R, true, none, [&](Batch& b) { b.pics[1].nz.clear(); exact(b.pics[1].nz); }},
        {"raw TB past the samples", R, true, none, [&](Batch& b) { b.pics[0].stbs[1].coef_off = 1; }},
        {"position error before the sparse one", R, true, [&](Batch& b) { tb(b, 0).x = 64; }, [&](Batch& b) { b.pics[0].stbs[0].reserved[2] = 1; }},
        {"qp before the sparse error of a later TB", E, true, [&](Batch& b) { tb(b, 0).qp = 52; }, [&](Batch& b) { b.pics[0].stbs[1].coef_off = 1; }},
    };
    for (const Bad& c : bad) {
        g_case = c.name;
        Batch b;
        b.pics = {plain_pic(), plain_pic()};
        c.dense_edit(b);
        for (Pic& p : b.pics) { p.stbs = p.tbs; p.nz.clear(); p.raw = p.coef; }
        if (c.sparse) {                         // (the sparse form of the records as edited; sparsify reads no position)
            for (Pic& p : b.pics) p.sparsify();
            c.sparse_edit(b);
        }
        UploadPlan u;
        const int rc = plan_of(cx, b, c.sparse, &u);
        if (rc != c.code) std::printf("  [%s] returned %d, expected %d\n", c.name, rc, c.code);
        EXPECT(rc == c.code);
    }
    {   // too many TBs in a CTU (CTB 16: 24; 16 luma; 8 chroma), none of them coded
        const Ctx c16 = make_ctx(16, 16, 4, 8, false);
        for (int variant = 0; variant < 5; ++variant) {
            static const int count[] = {25, 24, 17, 16, 9}, c_idx[] = {0, 0, 0, 0, 1}, code[] = {P265R_EINVAL, P265R_EINVAL, P265R_EINVAL, P265R_OK, P265R_EINVAL};
            g_case = "TBs per CTU";
            Pic pic;
            pic.w = pic.h = 16;
            p265r_tb t{};
            t.log2_size = 2;
            t.c_idx = (uint8_t)c_idx[variant];
            pic.tbs.assign(25, t);
            p265r_ctu c{};
            c.tb_count = (uint16_t)count[variant];
            pic.ctus.assign(1, c);
            pic.stbs = pic.tbs;
            Batch b;
            b.pics.push_back(pic);
            UploadPlan u;
            EXPECT(plan_of(c16, b, false, &u) == code[variant]);
        }
    }
    {   // the argument checks: no picture is read for n_pics = 65536
        g_case = "arguments";
        Batch b;
        b.pics = {plain_pic()};
        for (Pic& p : b.pics) p.stbs = p.tbs;
        const auto pv = b.views(false);
        UploadPlan u;
        auto plan = [&](const p265r_picture* pics, int n, UploadPlan* out) { return plan_upload(cx.p, cx.g, cx.n_ctus, cx.xg, cx.split, cx.num_cus, pics, nullptr, n, out); };
        EXPECT(plan(pv.data(), 0, &u) == P265R_EINVAL);
        EXPECT(plan(pv.data(), -1, &u) == P265R_EINVAL);
        EXPECT(plan(nullptr, 1, &u) == P265R_EINVAL);
        EXPECT(plan(pv.data(), 1, nullptr) == P265R_EINVAL);
        EXPECT(plan(pv.data(), 65536, &u) == P265R_ERANGE);
        EXPECT(plan(pv.data(), 1, &u) == P265R_OK);
        const p265r_sparse_coef null_nz{nullptr, 1};         // entries announced, none given
        EXPECT(plan_upload(cx.p, cx.g, cx.n_ctus, cx.xg, cx.split, cx.num_cus, pv.data(), &null_nz, 1, &u) == P265R_EINVAL);
    }
    {   // 10-bit: qP up to 63
        g_case = "qp at 10 bits";
        const Ctx c10 = make_ctx(64, 64, 5, 10, true);
        for (int qp : {63, 64}) {
            Batch b;
            b.pics = {plain_pic()};
            b.pics[0].tbs[0].qp = (uint8_t)qp;
            b.pics[0].stbs = b.pics[0].tbs;
            UploadPlan u;
            EXPECT(plan_of(c10, b, false, &u) == (qp == 63 ? P265R_OK : P265R_EINVAL));
        }
    }
}

// ---- recon input at unequal bit depths: the 8-bit component goes up widened -------------------------------
// A wide context (p265r_params.split_bit_depth) keeps every device plane as uint16_t: the planner places each
// uint8_t recon-input plane's widened copy behind the rest of the staging buffer, widen_plane fills it.
static void wide_recon_input() {
    static const int depths[3][2] = {{8, 10}, {10, 8}, {10, 10}};
    for (const auto& d : depths) {
        g_case = d[0] == 8 ? "recon input (8, 10)" : d[1] == 8 ? "recon input (10, 8)" : "recon input (10, 10)";
        Ctx cx = make_ctx(72, 40, 4, 10, true);
        cx.p.bit_depth_luma = (uint8_t)d[0]; cx.p.bit_depth_chroma = (uint8_t)d[1];
        cx.p.split_bit_depth = d[0] != d[1];
        cx.g.bd[0] = d[0]; cx.g.bd[1] = cx.g.bd[2] = d[1];
        static const int sz[2][2] = {{72, 40}, {40, 24}};
        Batch b;
        std::vector<std::vector<uint8_t>> planes;                 // exact-size host planes, in the component's type
        const Ctx gen = make_ctx(72, 40, 4, 8, true);             // (records legal at either depth: qp <= 51)
        for (int i = 0; i < 2; ++i) b.pics.push_back(make_pic(gen, PicOpt{sz[i][0], sz[i][1], false, false, NONE_CODED, false}, 8100 + i));
        for (int i = 0; i < 2; ++i)
            for (int c = 0; c < 3; ++c) {
                const size_t n = (size_t)(sz[i][0] >> (c ? 1 : 0)) * (sz[i][1] >> (c ? 1 : 0));
                std::vector<uint8_t> v(n * (cx.g.bd[c] > 8 ? 2 : 1));
                for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)(37 * k + 11 * c + i);
                exact(v);
                planes.push_back(v);
            }
        for (int i = 0; i < 2; ++i) {
            b.pics[i].flags = P265R_PIC_RECON_INPUT;
            for (int c = 0; c < 3; ++c) b.pics[i].recon[c] = planes[3 * i + c].data();
        }
        UploadPlan base, u;
        if (plan_of(cx, b, false, &u) != P265R_OK) { EXPECT(!"plan of a recon-input batch"); continue; }
        EXPECT(u.recon_input && u.ragged && u.pel_bytes == 2);
        if (d[0] == d[1]) { EXPECT(u.wide_at.empty() && u.s_wide == 0); continue; }
        for (auto& pic : b.pics) pic.flags = 0;                   // the same batch without the recon input
        EXPECT(plan_of(cx, b, false, &base) == P265R_OK);
        for (auto& pic : b.pics) pic.flags = P265R_PIC_RECON_INPUT;
        EXPECT(u.s_wide == align_up(base.stage_need, 256) && u.total == base.total && u.wide_at.size() == 2);
        std::vector<unsigned char> stage(u.stage_need, 0xEE);
        exact(stage);
        const auto pv = b.views(false);
        size_t end = u.s_wide;
        for (int i = 0; i < 2; ++i)
            for (int c = 0; c < 3; ++c) {
                const size_t n = (size_t)(sz[i][0] >> (c ? 1 : 0)) * (sz[i][1] >> (c ? 1 : 0));
                if (cx.g.bd[c] > 8) { EXPECT(u.wide_at[i][c] == SIZE_MAX); continue; }
                EXPECT(u.wide_at[i][c] == end && end % 256 == 0);
                widen_plane(u, i, c, pv.data(), stage.data());
                const uint16_t* w = reinterpret_cast<const uint16_t*>(stage.data() + u.wide_at[i][c]);
                bool same = true;
                for (size_t k = 0; k < n; ++k) same = same && w[k] == planes[3 * i + c][k];
                EXPECT(same);
                end = align_up(end + 2 * n, 256);
            }
        EXPECT(end == u.stage_need);
        for (size_t k = 0; k < u.s_wide; ++k)
            if (stage[k] != 0xEE) { EXPECT(!"widen_plane wrote in front of its range"); break; }
    }
}

int main() {
    good_batches();
    rejections();
    wide_recon_input();
    if (g_fail) { std::printf("upload_check: %d check(s) failed\n", g_fail); return 1; }
    std::printf("upload_check ok\n");
    return 0;
}
