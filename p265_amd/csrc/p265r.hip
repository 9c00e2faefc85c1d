// p265r.hip -- host side of the C ABI declared in include/p265r.h.
//
// Build (see Makefile):  hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o p265_amd/libp265r.so
//
// One context = one HIP device + one non-blocking stream + one parameter set.
// A batch = one device allocation holding every picture's records, the re-packed
// coefficient pool, the residual job lists and the output planes.  Run order on the
// stream: residual kernels (one per job class) -> intra wavefront steps -> SAO.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/p265r.h"
#include "digest.h"
#include "export.h"
#include "export_host.h"
#include "resize.h"
#include "resize_host.h"
#include "grid.h"
#include "grid_host.h"
#include "grid_resize.h"
#include "grid_resize_host.h"
#include "intra.h"
#include "intra_prep.h"
#include "intra_rows.h"
#include "loopfilter.h"
#include "loopfilter16.h"
#include "narrow.h"
#include "pichash.h"
#include "sao16.h"
#include "residual.h"
#include "coef_expand.h"
#include "sao.h"
#include "sao_strip16.h"
#include "sao_rows.h"
#include "tables.h"
#include "upload_host.h"

using namespace p265r;

// The library reads only the environment knobs the GPU parity matrix sets (tests/test_gpu_parity.py), and
// P265R_DEBUG_SYNC in -DP265R_DEBUG_DIAG builds.  Retired experiment knobs: EXPERIMENTS.md, "Retired knobs".
//
// Stream plan of pipelined contexts (round 5: one interleaved A/B of round 3's head against every round-4
// step): the two round-4 schedules below each cost 5-8 % of the pipelined C3 step by adding
// streams -- a process's streams map round-robin onto GPU_MAX_HW_QUEUES hardware queues (4), so every
// extra stream changes which lanes' kernels queue behind which -- and are off (the check-variant builds only):
#ifndef P265R_EARLY_RESIDUAL
#define P265R_EARLY_RESIDUAL 0     // re-runs: residual + prep start when the batch's previous intra phase ends
#endif
#ifndef P265R_PHASE_ORDER
#define P265R_PHASE_ORDER 0        // pipelined contexts: one intra phase at a time; residual + prep overlap loop filters
#endif

namespace {

thread_local std::string g_last_hip_error;

int hip_fail(hipError_t e, const char* what) {
    g_last_hip_error = std::string(what) + ": " + hipGetErrorString(e);
    return P265R_EHIP;
}

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(_e, #expr);    \
    } while (0)

constexpr size_t kDlHalf = 24u << 20;   // download bounce buffer half (p265r_batch_download)

bool params_ok(const p265r_params& p) {
    return p.version == P265R_ABI_VERSION && p.chroma_format_idc <= 1 && p.pic_width > 0 && p.pic_height > 0 &&
           p.pic_width % 8 == 0 && p.pic_height % 8 == 0 && p.ctb_log2_size >= 4 && p.ctb_log2_size <= 6 &&
           p.min_tb_log2_size >= 2 && p.max_tb_log2_size <= 5 && p.min_tb_log2_size <= p.max_tb_log2_size;
}

}  // namespace

struct p265r_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    p265r_params params{};
    Geo geo{};
    int n_ctus = 0;
    bool timing = false;
    // per timed run: 4 events (start, after residual, after intra, after loop filter) + the
    // launch counts; kept for every run since p265r_set_timing(ctx, 1) so runs can be queued
    // back to back and read once (p265r_timings_total)
    struct Run { hipEvent_t ev[4]; p265r_timings counts; };
    std::vector<Run> runs;
    std::vector<hipEvent_t> spare;
    bool have_timing = false;
    p265r_batch* pending = nullptr;
    std::vector<p265r_picture> pending_pics;
    int schedule = 1;          // 0: one launch per anti-diagonal, 1: CU-local row pipeline
    int row_waves = 0;         // waves per workgroup of the row pipeline (P265R_ROW_WAVES 8, 12);
                               // 0 = by run: a batch alone 12 (6 per SIMD, 80 VGPRs:
                               // lowest latency), overlapping other lanes' batches 8 (80 VGPRs: room beside it)
    unsigned lane_busy = 0;    // lanes with a run enqueued since the API last synchronised them (p265r_sync,
                               // p265r_batch_download / p265r_batch_status of a batch on the lane): the row
                               // kernel build of a run follows from the call sequence, not from device timing
    int sao_rows = 1;          // SAO-only batches: 1 16-B strip kernel (CTB 32 / 64; 4-B strip kernel for
                               // CTB 16), 2 4-B strip kernel, 0 loop-filter window kernel (P265R_SAO_ROWS)
    int split = 1;            // component split of small batches (P265R_SPLIT=0: off; launch_rows_w)
    int xg = 4;                // workgroups per chain of the cross-group row kernel (P265R_XG; 0: off; launch_rows)
    bool last_split = false;   // the last row-kernel launch was split (p265r_describe)
    bool last_xg = false;      // ... was the cross-group kernel
    const char* last_layout = "none";   // row layout of the last run's intra phase: whole | split | xg | luma
                                        // (monochrome) | steps (per-diagonal kernel) | none (p265r_describe)
    int last_row_waves = 0;    // ... and the W of its row-kernel build (0: no row kernel ran)
    long long row_launches[4] = {0, 0, 0, 0};      // row-kernel launches per build: W = 12, W = 8, W = 16 split,
                                                   // cross-group -- p265r_describe
    int luma_lead = -1;        // rows the luma chain leads the chroma chain in the row queue (P265R_LUMA_LEAD);
                               // -1 = by run: 8 for a batch alone, 5 beside other lanes' batches (round 3,
                               // 2 reps: alone lead 5/7/8/10 -> 4.28/4.23/4.19/4.22 ms, pipelined
                               // 45.5/44.9/44.4/44.7 M CTU/s; round 1, W=8: lead 0/1/2/3/5/8/17 ->
                               // 10.40/10.10/10.40/10.09/10.07/10.35/10.38 ms)
    int num_cus = 256;
    bool debug_sync = false;   // P265R_DEBUG_DIAG builds, P265R_DEBUG_SYNC=1: synchronise + log after every phase,
                               // trace the row kernel's waves and print placement statistics
    // reused across batches: pinned host staging (grow-only) and one freed device allocation
    unsigned char* stage = nullptr;
    size_t stage_bytes = 0;
    bool stage_pinned = false;
    void* cache_mem = nullptr;
    size_t cache_bytes = 0;
    // batch pipelining (p265r_set_pipeline): batches are bound round-robin to `pipeline`
    // streams (lane 0 = stream), so one batch's residual / loop-filter phases run beside
    // another batch's intra kernel
    int pipeline = 1;
    int next_lane = 0;
    std::vector<hipStream_t> lanes;   // lanes[0] == stream
    // job prep forked onto a second stream per lane (P265R_FORK_PREP, default on): the prep
    // kernel (latency-bound, LDS/VGPR-limited occupancy) runs beside the residual kernels
    // (HBM-bound) instead of after them; the intra kernel waits for both
    int fork_prep = 1;
    std::vector<hipStream_t> aux;     // aux[i]: lane i's prep stream (created on first use)
    std::vector<hipEvent_t> fork_ev, join_ev;
    std::vector<hipStream_t> aux2;    // aux2[i]: lane i's residual stream (early residual phase)
    std::vector<hipEvent_t> join2_ev;
    // phase order of a pipelined context (P265R_PHASE_ORDER): the last intra launch and the last
    // loop-filter launch of ANY lane, recorded on their lane streams
    hipEvent_t last_intra_ev = nullptr, last_lf_ev = nullptr;
    bool last_intra_valid = false, last_lf_valid = false;
    std::string describe;             // p265r_describe text
    uint8_t* d_sf = nullptr;           // scaling lists: the intra ScalingFactor table (p265r_set_scaling_factors)
    unsigned char* dl_stage = nullptr;  // pinned download bounce buffer, 2 x kDlHalf (first download)
    hipEvent_t dl_ev[2] = {nullptr, nullptr};
    // sparse upload (p265r_batch_upload_sparse): device landing buffer of a batch's entries and per-job
    // entry begins (grow-only; an upload is complete when it returns, so the next one reuses it)
    void* sp_mem = nullptr;
    size_t sp_bytes = 0;
    std::vector<hipEvent_t> exp_ev;         // timed uploads: an event pair per chunk around its expand kernels
    double last_expand_ms = -1.0;           // expand kernels of the last sparse upload (timing on), p265r_describe
};

struct p265r_batch {
    int n_pics = 0;
    void* mem = nullptr;
    size_t bytes = 0;
    DevPic* d_pics = nullptr;
    int16_t* d_pool = nullptr;
    int16_t* d_res = nullptr;
    int* d_err = nullptr;
    ResJob* d_jobs[RC_NUM] = {};
    uint32_t slab[RC_NUM] = {};    // int16 offset of each class's packed TBs in the pool (fixed-size classes)
    BatchView view{};
    int n_jobs[RC_NUM] = {};
    std::vector<DevPic> h_pics;
    hipStream_t stream = nullptr;  // the context lane this batch runs on
    int lane = 0;
    bool sao = false;
    bool dbk = false;          // some CTU of the batch has deblocking on
    bool recon_input = false;  // P265R_PIC_RECON_INPUT: only the in-loop filters run
    bool ragged = false;       // some picture is smaller than the context size (Geo::ragged)
    int* d_xg_prog = nullptr;  // cross-group row kernel (intra_rows.h XgBuf): progress words (zeroed per run
    uint8_t* d_xg_lines = nullptr;  // with the CU slots), the rows' bottom lines; null: batch too large
    std::vector<std::array<int, 2>> size;   // per picture: luma width, height
    uint64_t h2d_bytes = 0;    // host-to-device bytes its upload enqueued (p265r_batch_upload_bytes)
    int runs = 0;              // p265r_batch_run calls so far
    std::vector<void*> exp_idx;        // p265r_batch_export: device copies of the pic_index lists of the exports
                                       // enqueued since the lane was last synchronised (p265r_batch_status)
    void* grid_stage = nullptr;        // p265r_batch_export_grid, quarter turns: the untransposed frames (allocated at the
    size_t grid_stage_bytes = 0;       // first such call and reused; grown when a later call needs more)
    unsigned long long* d_dig = nullptr;   // p265r_batch_digest_async slots: P265R_DIGEST_SLOTS x n_pics x 3
    uint8_t* d_hash = nullptr;         // p265r_batch_hash_async: 16 bytes per plane (the SEI form), then one 32-bit
                                       // accumulator per plane (checksum, CRC)
    // p265r_batch_download in a wide context with an 8-bit component (narrow.h): the staging area of the narrowed
    // planes, its items in front (allocated at the first such download, grown when a later one asks for more)
    unsigned char* d_narrow = nullptr;
    size_t narrow_bytes = 0;
    std::vector<NarrowItem> narrow_items;   // (host copy: lives until the batch is freed, the H2D copy reads it)
    hipEvent_t intra_done = nullptr;   // recorded after each run's intra phase (the last reader of the
                                       // residual pool and job lists): the next run's residual + prep
                                       // phase waits for it instead of for the whole previous run
};

namespace {

#ifdef P265R_DEBUG_DIAG
// Row-kernel diagnostics (P265R_DEBUG_DIAG builds with P265R_DEBUG_SYNC=1): wave trace of a hung
// launch, dependency-wait share, workgroup lifetimes and placement, per-job-class cycles
// (P265R_JOB_STATS builds).  Not compiled into the product library.
void rows_diag(hipStream_t st, const int* dbg, int grid, int W) {
    for (int it = 0; it < 100; ++it) {
        if (hipStreamQuery(st) == hipSuccess) break;
        struct timespec ts{0, 100000000};
        nanosleep(&ts, nullptr);
        if (it == 99) {
            fprintf(stderr, "[p265r] rows kernel still running after 10 s; wave trace:\n");
            for (int i = 0; i < grid * W && i < 64; ++i) fprintf(stderr, "  wg %d wave %d: code %d (0x%x)\n", i / W, i % W, dbg[i] & 0xff, dbg[i]);
            fflush(stderr);
            std::abort();
        }
    }
    double tot = 0, wt = 0;
    for (int i = 0; i < grid * W; ++i) { tot += dbg[grid * W + 2 * i]; wt += dbg[grid * W + 2 * i + 1]; }
    fprintf(stderr, "[p265r] rows kernel: %.1f%% of wave time in dependency waits (%d waves)\n", 100.0 * wt / (tot > 0 ? tot : 1), grid * W);
    std::vector<int> life(grid, 0);          // workgroup lifetimes (longest wave, 256-cycle units)
    for (int i = 0; i < grid * W; ++i) life[i / W] = std::max(life[i / W], dbg[grid * W + 2 * i]);
    double sx[16] = {}; int nx[16] = {};
    for (int i = 0; i < grid; ++i) { const int x = dbg[3 * grid * W + 2 * i] & 15; sx[x] += life[i]; ++nx[x]; }
    fprintf(stderr, "[p265r] mean workgroup lifetime per XCC (Mcycles):");
    for (int x = 0; x < 16; ++x) if (nx[x]) fprintf(stderr, " x%d:%.2f(%d)", x, sx[x] / nx[x] * 256e-6, nx[x]);
    fprintf(stderr, "\n");
    std::vector<std::pair<int, int>> byhw;
    for (int i = 0; i < grid; ++i) byhw.push_back({dbg[3 * grid * W + 2 * i] * 256 + ((dbg[3 * grid * W + 2 * i + 1] >> 8) & 255), life[i]});
    std::sort(byhw.begin(), byhw.end());
    int same = 0; double dsum = 0;
    for (size_t i = 1; i < byhw.size(); ++i)
        if (byhw[i].first == byhw[i - 1].first) { ++same; dsum += std::abs(byhw[i].second - byhw[i - 1].second); }
    fprintf(stderr, "[p265r] workgroups sharing a CU: %d pairs, mean lifetime difference %.2f Mcycles\n", same, same ? dsum / same * 256e-6 : 0.0);
    static const char* names[14] = {"luma quad", "chroma quad", "fast Y4", "fast Y8", "fast Y16", "fast C4 pair",
                                    "fast C8 pair", "gen Y4", "gen Y8", "gen Y16", "gen Y32", "gen C4", "gen C8", "gen C16"};
    const int* js = dbg + 3 * grid * W + 2 * grid;
    double jt = 0;
    for (int k = 0; k < 14; ++k) jt += 16.0 * (unsigned)js[2 * k];
    for (int k = 0; k < 14; ++k)
        if (js[2 * k + 1])
            fprintf(stderr, "[p265r] jobs %-13s %9d  %7.0f cycles/job  %5.1f %%\n", names[k], js[2 * k + 1],
                    16.0 * (unsigned)js[2 * k] / js[2 * k + 1], 100.0 * 16.0 * (unsigned)js[2 * k] / (jt > 0 ? jt : 1));
    std::sort(life.begin(), life.end());
    if (grid > 0)
        fprintf(stderr, "[p265r] rows kernel workgroup lifetime (Mcycles): min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f\n",
                life[0] * 256e-6, life[grid / 10] * 256e-6, life[grid / 2] * 256e-6, life[grid * 9 / 10] * 256e-6,
                life[grid - 1] * 256e-6);
}
#endif

// dynamic LDS of the row kernel with W waves and f picture slots (launch_rows_w)
template <typename T>
size_t rows_lds_bytes(const Geo& g, int W, int f) {
    return 256 + (size_t)((f * 2 * g.hc * 4 + 15) & ~15) + W * sizeof(WaveLdsT<T>) +
           (size_t)f * 2 * (g.w + 2 * g.cw) * sizeof(T) + kAngTabBytes;
}

template <int W, int WPE, bool XG = false, bool TRCHK = false, typename T = uint8_t>
int launch_rows_w(p265r_ctx* ctx, p265r_batch* b, hipStream_t st, bool alone) {
    Geo g = ctx->geo;
    // picture slots: the W rows in flight are consecutive in the queue, so they span at
    // most ceil(W / hc) + 1 pictures; a slot is reused only after its previous picture is
    // complete (the kernel waits for that, so fewer slots would still be correct)
    const int chains = g.mono ? 1 : 2;                              // row units per CTU row: luma, chroma (Cb + Cr)
    int fs = std::min(32, (W + chains * g.hc - 1) / (chains * g.hc) + 1);
    auto lds_of = [&](int f) { return rows_lds_bytes<T>(g, W, f); };
    while (fs > 2 && lds_of(fs) > 160 * 1024) --fs;
    auto fn = intra_rows_kernel<W, WPE, XG, TRCHK, T>;
    bool split = false;
    {
        // every workgroup resident at once and holding a single picture: one slot is enough
        // (a second picture would only wait for the first), and the smaller LDS footprint can
        // fit one more workgroup per CU
        int pc1 = 0;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(1)));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc1, fn, 64 * W, lds_of(1)));
        if (pc1 >= 1 && b->n_pics <= pc1 * ctx->num_cus) fs = 1;
        // component split: a picture's luma chain and its chroma chain on two workgroups of their own
        // (on different CUs) when all of them fit at once -- the latency regime of a few large
        // pictures / tile units, where one workgroup's W waves on one CU bound the picture's time
        // (monochrome has one chain per picture: nothing to split; its layout is `luma`, below)
        split = !g.mono && ctx->split && pc1 >= 1 && 2 * (long long)b->n_pics <= (long long)pc1 * ctx->num_cus;
        if (XG) { fs = 1; split = true; }
    }
    const size_t lds = lds_of(fs);
    if (lds > 160 * 1024) return P265R_EUNSUPPORTED;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * W, lds));
    if (per_cu < 1) return P265R_EUNSUPPORTED;
    const int grid = XG ? 2 * b->n_pics * ctx->xg : split ? 2 * b->n_pics : std::min(b->n_pics, per_cu * ctx->num_cus);
    // fair CU sharing pairs the two workgroups of a CU (rank = arrival order & 1): only valid
    // when exactly two fit per CU and all of them are resident for the whole launch (grid <= 2
    // per CU, no workgroup starts after another ends) -- and only worth it for a batch alone
    g.fair = g.fair && alone && per_cu == 2 && !split && !g.mono;     // (monochrome: the priority bands of the
                                                                      // one-chain row queue use s_setprio instead)
    // (XG: the progress words were cleared with the CU slots this run, so one tag serves every run)
    const XgBuf xb{XG ? b->d_xg_prog : nullptr, XG ? b->d_xg_lines : nullptr,
                   XG ? b->d_xg_prog + 2 * (size_t)g.hc * b->n_pics : nullptr, XG ? ctx->xg : 0, 1};
    g.ragged = b->ragged ? 1 : 0;
    int* dbg = nullptr;
#ifdef P265R_DEBUG_DIAG
    if (ctx->debug_sync) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&dbg), sizeof(int) * (grid * W * 3 + grid * 2 + 32), hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(dbg, 0, sizeof(int) * (grid * W * 3 + grid * 2 + 32));
        fprintf(stderr, "[p265r] rows kernel W=%d WPE=%d fair=%d grid=%d lds=%zu fs=%d per_cu=%d\n", W, WPE, g.fair, grid, lds, fs, per_cu);
    }
#endif
    const int lead = ctx->luma_lead >= 0 ? ctx->luma_lead : (alone ? 8 : 5);
    // layout (the kernel's `split` argument): 0 whole pictures (luma and chroma rows interleaved), 1 component
    // split (two workgroups per picture), 2 luma rows only (monochrome: one workgroup per picture slot)
    const int layout = g.mono ? 2 : (split ? 1 : 0);
    fn<<<grid, 64 * W, lds, st>>>(b->d_pics, b->d_pool, b->d_res, g, b->n_pics, fs, lead, b->d_err, dbg, layout, xb);
    ctx->last_split = split;
    ctx->last_xg = XG;
    ctx->last_layout = XG ? "xg" : (layout == 2 ? "luma" : (layout == 1 ? "split" : "whole"));
    ctx->last_row_waves = W;
    ++ctx->row_launches[XG ? 3 : (W == 16 ? 2 : (W == 8 ? 1 : 0))];
    HIP_TRY(hipGetLastError());
#ifdef P265R_DEBUG_DIAG
    if (dbg) {
        rows_diag(st, dbg, grid, W);
        (void)hipHostFree(dbg);
    }
#endif
    return P265R_OK;
}

// alone: no other lane of the context has a run enqueued (ctx->lane_busy), so this batch's kernels
// have the GPU to themselves: W = 12 with fair CU sharing; otherwise W = 8 (80 VGPRs, so the residual /
// prep / SAO waves of the neighbouring batches fit beside it on every SIMD)
int launch_rows(p265r_ctx* ctx, p265r_batch* b, hipStream_t st, bool alone) {
    // 16-bit samples (BitDepth 9..12): the same row pipeline on 16-bit LDS tiles and line buffers
    // (one workgroup per CU: twice the LDS of a wave); W = 12 alone, W = 8 beside other lanes' work
    if (ctx->geo.pel16) {
        // (wide pictures: W = 12 only while its two picture slots fit the 160 KB of LDS; p265r_create keeps
        // the per-diagonal schedule for pictures too wide for W = 8)
        int w = ctx->row_waves ? ctx->row_waves : (alone ? 12 : 8);
        if (w == 12 && rows_lds_bytes<uint16_t>(ctx->geo, 12, 2) > 160 * 1024) w = 8;
        if (ctx->geo.bd[1] > 10)                    // BitDepthC 11..12: int16_t tags the split angular sums (pang) of
                                                    // the Cb | Cr pairs; the luma jobs never read the tag
            return w == 12 ? launch_rows_w<12, 1, false, false, int16_t>(ctx, b, st, alone)
                           : launch_rows_w<8, 1, false, false, int16_t>(ctx, b, st, alone);
        return w == 12 ? launch_rows_w<12, 1, false, false, uint16_t>(ctx, b, st, alone)
                       : launch_rows_w<8, 1, false, false, uint16_t>(ctx, b, st, alone);
    }
    // the smallest batches (every chain on xg CUs of its own): the cross-group kernel, one wave per SIMD
    if (ctx->row_waves == 0 && !ctx->geo.mono && b->d_xg_prog && 2 * (long long)b->n_pics * ctx->xg <= ctx->num_cus)
        return ctx->geo.tr_check ? launch_rows_w<4, 1, true, true>(ctx, b, st, alone)     // (test build of it)
                                 : launch_rows_w<4, 1, true>(ctx, b, st, alone);
    // a batch small enough for the component split with one workgroup per CU (the latency regime:
    // tile units, the decoder's small batches): W = 16, so every CTU row of a picture's chain can
    // be in flight at once (a 2-CTU-lag wavefront of 17 rows needs 17 waves; with 12 the rows
    // after the 12th wait for a whole row to finish)
    // (monochrome: one chain per picture, so up to one picture per CU)
    if (ctx->row_waves == 0 && ctx->split && (ctx->geo.mono ? 1 : 2) * (long long)b->n_pics <= ctx->num_cus)
        return launch_rows_w<16, 4>(ctx, b, st, alone);
    const int w = ctx->row_waves ? ctx->row_waves : (alone ? 12 : 8);
    return w == 12 ? launch_rows_w<12, 6>(ctx, b, st, alone) : launch_rows_w<8, 6>(ctx, b, st, alone);
}

// grid of a strip kernel (sao.h strip_pos): one wave per unit, 4 waves per block, the block count
// rounded up to the 8 XCDs
int strip_grid(int units_per_pic, int n_pics, unsigned* blocks) {
    const long long waves = (long long)units_per_pic * n_pics;
    if (waves >= (1ll << 31) - 64) return P265R_ERANGE;
    *blocks = (unsigned)(((waves + 3) / 4 + 7) / 8 * 8);
    return P265R_OK;
}

// The in-loop filter pass of a batch (deblocking + SAO) on stream s; `launched` counts the kernel.
//   SAO only, 16-bit samples: sao16.h, 8 samples per lane, 496-sample strips
//   SAO only, CTB 32 / 64: sao_strip16.h, 16 samples per lane, 992-sample strips; it filters 2-row chunks
//     and takes plane heights in multiples of 4 (luma a multiple of MinCbSizeY >= 8 in a conforming
//     stream; anything else goes to the 4-B strip kernel)
//   SAO only, CTB 16 (or P265R_SAO_ROWS=2): sao_rows.h, 4 samples per lane, 248-sample strips
//   with deblocking (or P265R_SAO_ROWS=0): the window kernels, loopfilter.h / loopfilter16.h
// Strip kernels: one wave per (picture, CTB row, component, strip), 4 waves per block; window kernels:
// one workgroup per (picture, CTB).
int launch_loop_filters(p265r_ctx* ctx, p265r_batch* b, const Geo& g, hipStream_t s, int* launched) {
    if (!b->dbk && !b->sao) return P265R_OK;
    const bool sao_only = b->sao && !b->dbk;
    const int np = b->n_pics;
    unsigned blocks = 0;
    if (sao_only && g.pel16) {
        if (int rc = strip_grid(strip_units(g, strip_samples(8)), np, &blocks)) return rc;
        sao16_strip_kernel<<<blocks, 256, 0, s>>>(b->d_pics, g, b->view, np);
    } else if (sao_only && !g.pel16 && ctx->sao_rows == 1 && g.ctb_log2 >= 5 && g.h % 8 == 0) {
        if (int rc = strip_grid(strip_units(g, strip_samples(16)), np, &blocks)) return rc;
        if (g.ctb_log2 == 6) sao_strip16_kernel<6><<<blocks, 256, 0, s>>>(b->d_pics, g, b->view, np);
        else sao_strip16_kernel<5><<<blocks, 256, 0, s>>>(b->d_pics, g, b->view, np);
    } else if (sao_only && !g.pel16 && ctx->sao_rows) {
        if (int rc = strip_grid(strip_units(g, strip_samples(4)), np, &blocks)) return rc;
        sao_rows_kernel<<<blocks, 256, 0, s>>>(b->d_pics, g, np);
    } else {
        const long long units = (long long)ctx->n_ctus * np;
        if (units >= (1ll << 31) - 8) return P265R_ERANGE;
        blocks = (unsigned)((units + 7) / 8 * 8);
        const int so = b->sao ? 1 : 0;
        auto window = [&](auto ctbl, auto dbk) {
            constexpr int L = decltype(ctbl)::value;
            constexpr bool D = decltype(dbk)::value;
            if (g.pel16) loopfilter16_kernel<L, D><<<blocks, 256, 0, s>>>(b->d_pics, g, so, np);
            else loopfilter_kernel<L, D><<<blocks, LfShape<L>::threads(D), 0, s>>>(b->d_pics, g, so, np);
        };
        auto by_dbk = [&](auto ctbl) {
            if (b->dbk) window(ctbl, std::true_type{});
            else window(ctbl, std::false_type{});
        };
        if (g.ctb_log2 == 6) by_dbk(std::integral_constant<int, 6>{});
        else if (g.ctb_log2 == 5) by_dbk(std::integral_constant<int, 5>{});
        else by_dbk(std::integral_constant<int, 4>{});
    }
    ++*launched;
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// The one launch of p265r_batch_export on stream st: n slots; mw x mh = the largest cropped picture listed.
template <typename S>
int launch_export(const p265r_export_desc& d, const DevPic* d_pics, const Geo& g, const ExportArgs& a, int mw, int mh, int n,
                  hipStream_t st) {
    const auto grid = [&](int group, int row_units) {
        return dim3((unsigned)((mw / group + 2 + kExportLanes - 1) / kExportLanes),
                    (unsigned)((row_units + kExportRows - 1) / kExportRows), (unsigned)n);
    };
    if (g.mono) {
        // monochrome: luma rows alone (semi-planar: + the grey CbCr rows); RGB one row per unit, no upsampling
        const int grey = (1 << (g.bd[0] - 1)) << a.shift;
        if (d.format == P265R_FMT_PLANAR) {
            export_mono_yuv_kernel<S, false><<<grid(16 / (int)sizeof(S), mh), 256, 0, st>>>(d_pics, g, a, grey);
        } else if (d.format == P265R_FMT_SEMIPLANAR) {
            export_mono_yuv_kernel<S, true><<<grid(16 / (int)sizeof(S), mh + mh / 2), 256, 0, st>>>(d_pics, g, a, grey);
        } else {
            auto rgb = [&](auto dtag) {
                using D = typename decltype(dtag)::type;
                if (d.format == P265R_FMT_RGB_PACKED)
                    export_mono_rgb_kernel<S, D, true><<<grid(sizeof(D) == 1 ? 16 : 8, mh), 256, 0, st>>>(d_pics, g, a);
                else
                    export_mono_rgb_kernel<S, D, false><<<grid(sizeof(D) == 1 ? 16 : 8, mh), 256, 0, st>>>(d_pics, g, a);
            };
            switch (d.sample) {
                case P265R_SMP_U8: rgb(std::enable_if<true, uint8_t>{}); break;
                case P265R_SMP_F16: rgb(std::enable_if<true, _Float16>{}); break;
                case P265R_SMP_F32: rgb(std::enable_if<true, float>{}); break;
                default: rgb(std::enable_if<true, S>{}); break;                   // NATIVE
            }
        }
    } else if (d.format == P265R_FMT_PLANAR) {
        export_yuv_kernel<S, false><<<grid(16 / (int)sizeof(S), 2 * mh), 256, 0, st>>>(d_pics, g, a);
    } else if (d.format == P265R_FMT_SEMIPLANAR) {
        export_yuv_kernel<S, true><<<grid(16 / (int)sizeof(S), mh + mh / 2), 256, 0, st>>>(d_pics, g, a);
    } else {
        const bool bil = d.upsample == P265R_UP_BILINEAR;
        const int pairs = mh / 2 + (bil ? 1 : 0);
        auto rgb = [&](auto dtag, auto packed, auto bl) {
            using D = typename decltype(dtag)::type;
            constexpr bool PK = decltype(packed)::value, BL = decltype(bl)::value;
            export_rgb_kernel<S, D, PK, BL><<<grid(sizeof(D) == 1 ? 16 : 8, pairs), 256, 0, st>>>(d_pics, g, a);
        };
        auto by_shape = [&](auto dtag) {
            const bool pk = d.format == P265R_FMT_RGB_PACKED;
            if (pk && bil) rgb(dtag, std::true_type{}, std::true_type{});
            else if (pk) rgb(dtag, std::true_type{}, std::false_type{});
            else if (bil) rgb(dtag, std::false_type{}, std::true_type{});
            else rgb(dtag, std::false_type{}, std::false_type{});
        };
        switch (d.sample) {
            case P265R_SMP_U8: by_shape(std::enable_if<true, uint8_t>{}); break;
            case P265R_SMP_F16: by_shape(std::enable_if<true, _Float16>{}); break;
            case P265R_SMP_F32: by_shape(std::enable_if<true, float>{}); break;
            default: by_shape(std::enable_if<true, S>{}); break;                  // NATIVE
        }
    }
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// The one launch of p265r_batch_export_resized on stream st: n slots of a.ow x a.oh.
template <typename S>
int launch_resize(const p265r_export_desc& d, uint32_t filter, const DevPic* d_pics, const Geo& g, const ResizeArgs& a, int n,
                  hipStream_t st) {
    const auto blocks = [](int rows) { return (rows + kExportRows - 1) / kExportRows; };
    const auto grid = [&](int group, int row_blocks) {
        return dim3((unsigned)((a.ow / group + 2 + kExportLanes - 1) / kExportLanes), (unsigned)row_blocks, (unsigned)n);
    };
    const auto by_filter = [&](auto&& go) {
        if (filter == P265R_RS_NEAREST) go(std::integral_constant<int, (int)kRsNearest>{});
        else if (filter == P265R_RS_BILINEAR) go(std::integral_constant<int, (int)kRsBilinear>{});
        else go(std::integral_constant<int, (int)kRsArea>{});
    };
    if (d.format == P265R_FMT_PLANAR || d.format == P265R_FMT_SEMIPLANAR) {
        const int semi = d.format == P265R_FMT_SEMIPLANAR ? 1 : 0;
        const int chroma_blocks = semi ? blocks(a.oh / 2) : (g.mono ? 0 : 2 * blocks(a.oh / 2));
        by_filter([&](auto f) {
            resize_yuv_kernel<S, decltype(f)::value><<<grid(16 / (int)sizeof(S), blocks(a.oh) + chroma_blocks), 256, 0, st>>>(
                d_pics, g, a, semi);
        });
    } else {
        auto rgb = [&](auto dtag) {
            using D = typename decltype(dtag)::type;
            by_filter([&](auto f) {
                constexpr int F = decltype(f)::value;
                if (d.format == P265R_FMT_RGB_PACKED)
                    resize_rgb_kernel<S, D, true, F><<<grid(sizeof(D) == 1 ? 16 : 8, blocks(a.oh)), 256, 0, st>>>(d_pics, g, a);
                else
                    resize_rgb_kernel<S, D, false, F><<<grid(sizeof(D) == 1 ? 16 : 8, blocks(a.oh)), 256, 0, st>>>(d_pics, g, a);
            });
        };
        switch (d.sample) {
            case P265R_SMP_U8: rgb(std::enable_if<true, uint8_t>{}); break;
            case P265R_SMP_F16: rgb(std::enable_if<true, _Float16>{}); break;
            case P265R_SMP_F32: rgb(std::enable_if<true, float>{}); break;
            default: rgb(std::enable_if<true, S>{}); break;                       // NATIVE
        }
    }
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// Pass 1 of p265r_batch_export_grid on stream st: n frames of the a.W x a.H window.
template <typename S>
int launch_grid(const p265r_export_desc& d, const Geo& g, const GridArgs& a, int n, hipStream_t st) {
    const auto grid = [&](int group, int row_units) {
        return dim3((unsigned)((a.W / group + 2 + kExportLanes - 1) / kExportLanes),
                    (unsigned)((row_units + kExportRows - 1) / kExportRows), (unsigned)n);
    };
    if (d.format == P265R_FMT_PLANAR) {
        grid_yuv_kernel<S, false><<<grid(16 / (int)sizeof(S), g.mono ? a.H : 2 * a.H), 256, 0, st>>>(g, a);
    } else if (d.format == P265R_FMT_SEMIPLANAR) {
        grid_yuv_kernel<S, true><<<grid(16 / (int)sizeof(S), a.H + a.H / 2), 256, 0, st>>>(g, a);
    } else {
        const bool bil = d.upsample == P265R_UP_BILINEAR && !g.mono;    // (a monochrome source has nothing to upsample)
        const int pairs = bil ? a.H / 2 + 1 : (a.H + 1) / 2;
        auto rgb = [&](auto dtag, auto packed, auto bl) {
            using D = typename decltype(dtag)::type;
            constexpr bool PK = decltype(packed)::value, BL = decltype(bl)::value;
            grid_rgb_kernel<S, D, PK, BL><<<grid(sizeof(D) == 1 ? 16 : 8, pairs), 256, 0, st>>>(g, a);
        };
        auto by_shape = [&](auto dtag) {
            const bool pk = d.format == P265R_FMT_RGB_PACKED;
            if (pk && bil) rgb(dtag, std::true_type{}, std::true_type{});
            else if (pk) rgb(dtag, std::true_type{}, std::false_type{});
            else if (bil) rgb(dtag, std::false_type{}, std::true_type{});
            else rgb(dtag, std::false_type{}, std::false_type{});
        };
        switch (d.sample) {
            case P265R_SMP_U8: by_shape(std::enable_if<true, uint8_t>{}); break;
            case P265R_SMP_F16: by_shape(std::enable_if<true, _Float16>{}); break;
            case P265R_SMP_F32: by_shape(std::enable_if<true, float>{}); break;
            default: by_shape(std::enable_if<true, S>{}); break;                  // NATIVE
        }
    }
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// Pass 2 (quarter turns): every plane of n staged frames transposed into the destination.
int launch_grid_transpose(const p265r_export_desc& d, int es, const GridTransposeArgs& a, int n_planes, int n, hipStream_t st) {
    const dim3 grid((unsigned)((a.w[0] + kGridTile - 1) / kGridTile), (unsigned)(n_planes * a.tiles_y), (unsigned)n);
    auto go = [&](auto utag) {
        using U = typename decltype(utag)::type;
        if (d.format == P265R_FMT_RGB_PACKED) grid_transpose_kernel<U, 3, 3><<<grid, 256, 0, st>>>(a);
        else if (d.format == P265R_FMT_SEMIPLANAR) grid_transpose_kernel<U, 1, 2><<<grid, 256, 0, st>>>(a);
        else grid_transpose_kernel<U, 1, 1><<<grid, 256, 0, st>>>(a);
    };
    if (es == 1) go(std::enable_if<true, uint8_t>{});
    else if (es == 2) go(std::enable_if<true, uint16_t>{});
    else go(std::enable_if<true, uint32_t>{});
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// Pass 1 of p265r_batch_export_grid_resized on stream st: n frames, the largest R mw x mh.
template <typename S>
int launch_grid_resize(const p265r_export_desc& d, uint32_t filter, const Geo& g, const GridRsArgs& a, int mw, int mh, int n,
                       hipStream_t st) {
    const auto blocks = [](int rows) { return (rows + kExportRows - 1) / kExportRows; };
    const auto grid = [&](int group, int row_blocks) {
        return dim3((unsigned)((mw / group + 2 + kExportLanes - 1) / kExportLanes), (unsigned)row_blocks, (unsigned)n);
    };
    const auto by_filter = [&](auto&& go) {
        if (filter == P265R_RS_NEAREST) go(std::integral_constant<int, (int)kRsNearest>{});
        else if (filter == P265R_RS_BILINEAR) go(std::integral_constant<int, (int)kRsBilinear>{});
        else go(std::integral_constant<int, (int)kRsArea>{});
    };
    if (d.format == P265R_FMT_PLANAR || d.format == P265R_FMT_SEMIPLANAR) {
        const int semi = d.format == P265R_FMT_SEMIPLANAR ? 1 : 0;
        const int chroma_blocks = semi ? blocks(mh / 2) : (g.mono ? 0 : 2 * blocks(mh / 2));
        by_filter([&](auto f) {
            grid_resize_yuv_kernel<S, decltype(f)::value><<<grid(16 / (int)sizeof(S), blocks(mh) + chroma_blocks), 256, 0, st>>>(
                g, a, semi);
        });
    } else {
        auto rgb = [&](auto dtag) {
            using D = typename decltype(dtag)::type;
            by_filter([&](auto f) {
                constexpr int F = decltype(f)::value;
                if (d.format == P265R_FMT_RGB_PACKED)
                    grid_resize_rgb_kernel<S, D, true, F><<<grid(sizeof(D) == 1 ? 16 : 8, blocks(mh)), 256, 0, st>>>(g, a);
                else
                    grid_resize_rgb_kernel<S, D, false, F><<<grid(sizeof(D) == 1 ? 16 : 8, blocks(mh)), 256, 0, st>>>(g, a);
            });
        };
        switch (d.sample) {
            case P265R_SMP_U8: rgb(std::enable_if<true, uint8_t>{}); break;
            case P265R_SMP_F16: rgb(std::enable_if<true, _Float16>{}); break;
            case P265R_SMP_F32: rgb(std::enable_if<true, float>{}); break;
            default: rgb(std::enable_if<true, S>{}); break;                       // NATIVE
        }
    }
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// Pass 2: the staged frames of a ragged call transposed into their slots (the others' blocks return at once).
int launch_grid_resize_transpose(const p265r_export_desc& d, int es, const GridTransposeArgs& a, const GridRsFrame* frames,
                                 int n_planes, int n, hipStream_t st) {
    const dim3 grid((unsigned)((a.w[0] + kGridTile - 1) / kGridTile), (unsigned)(n_planes * a.tiles_y), (unsigned)n);
    auto go = [&](auto utag) {
        using U = typename decltype(utag)::type;
        if (d.format == P265R_FMT_RGB_PACKED) grid_resize_transpose_kernel<U, 3, 3><<<grid, 256, 0, st>>>(a, frames);
        else if (d.format == P265R_FMT_SEMIPLANAR) grid_resize_transpose_kernel<U, 1, 2><<<grid, 256, 0, st>>>(a, frames);
        else grid_resize_transpose_kernel<U, 1, 1><<<grid, 256, 0, st>>>(a, frames);
    };
    if (es == 1) go(std::enable_if<true, uint8_t>{});
    else if (es == 2) go(std::enable_if<true, uint16_t>{});
    else go(std::enable_if<true, uint32_t>{});
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

}  // namespace

extern "C" {

uint32_t p265r_abi_version(void) { return P265R_ABI_VERSION; }

const char* p265r_last_hip_error(void) { return g_last_hip_error.c_str(); }

const char* p265r_strerror(int code) {
    switch (code) {
        case P265R_OK: return "ok";
        case P265R_EINVAL: return "invalid argument or malformed record";
        case P265R_ENOMEM: return "out of memory";
        case P265R_EHIP: return "HIP runtime error";
        case P265R_EUNSUPPORTED: return "unsupported stream feature";
        case P265R_ERANGE: return "record points outside the picture or its buffers";
        case P265R_ESTATE: return "call out of order";
        case P265R_ENODEV: return "no such HIP device";
        default: return "unknown error";
    }
}

int p265r_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    return n;
}

int p265r_create(int device, const p265r_params* params, p265r_ctx** out) {
    if (!params || !out) return P265R_EINVAL;
    *out = nullptr;
    const p265r_params& p = *params;
    if (!params_ok(p)) return P265R_EINVAL;
    // BitDepth 8 (uint8_t planes) or 9..12 (uint16_t planes; 13..14 would need SaoOffsetVal beyond the int8 of the
    // CTU record), one depth for luma and chroma unless split_bit_depth allows two
    // (monochrome, chroma_format_idc 0: bit_depth_chroma, split_bit_depth, the chroma QP offsets and a scaling
    // table's chroma entries mean nothing and are ignored)
    const bool mono = p.chroma_format_idc == 0;
    if (!mono && p.split_bit_depth > 1) return P265R_EINVAL;
    const bool split_bd = !mono && p.split_bit_depth == 1;
    if (p.bit_depth_luma < 8 || p.bit_depth_luma > 12 || p.scaling_list_enabled > 1) return P265R_EUNSUPPORTED;
    if (!mono && (split_bd ? (p.bit_depth_chroma < 8 || p.bit_depth_chroma > 12) : p.bit_depth_chroma != p.bit_depth_luma))
        return P265R_EUNSUPPORTED;
    const int n = p265r_device_count();
    if (n < 0) return n;
    if (device < 0 || device >= n) return P265R_ENODEV;
    p265r_ctx* ctx = new (std::nothrow) p265r_ctx();
    if (!ctx) return P265R_ENOMEM;
    ctx->device = device;
    ctx->params = p;
    if (mono) {                                     // one depth from here on; no chroma QP
        ctx->params.bit_depth_chroma = p.bit_depth_luma;
        ctx->params.pps_cb_qp_offset = ctx->params.pps_cr_qp_offset = 0;
    }
    Geo& g = ctx->geo;
    g.w = p.pic_width; g.h = p.pic_height;
    g.mono = mono ? 1 : 0;
    g.cw = mono ? 0 : g.w / 2; g.ch = mono ? 0 : g.h / 2;
    g.stride[0] = (int)align_up(g.w, 64);
    g.stride[1] = g.stride[2] = (int)align_up(g.cw, 64);
    g.ctb_log2 = p.ctb_log2_size;
    g.wc = (g.w + (1 << g.ctb_log2) - 1) >> g.ctb_log2;
    g.hc = (g.h + (1 << g.ctb_log2) - 1) >> g.ctb_log2;
    g.bd[0] = p.bit_depth_luma; g.bd[1] = g.bd[2] = ctx->params.bit_depth_chroma;
    // wide context: either depth above 8 puts uint16_t samples in all three planes (one sample type per kernel)
    g.pel16 = (g.bd[0] > 8 || g.bd[1] > 8) ? 1 : 0;
    g.strong = p.strong_intra_smoothing;
    g.lf_tiles = p.loop_filter_across_tiles;
    g.nf_w = (g.w + 7) / 8;
    g.cqp[0] = ctx->params.pps_cb_qp_offset;
    g.cqp[1] = ctx->params.pps_cr_qp_offset;
    g.fair = 1;
    if (const char* v = std::getenv("P265R_FAIR")) g.fair = v[0] != '0';
    g.quad = 3;
    g.tr_check = 0;
    g.tr_info = 1;
    if (const char* v = std::getenv("P265R_QUAD")) g.quad = std::atoi(v) & 7;
    ctx->n_ctus = g.wc * g.hc;
    // test knobs of the GPU parity matrix (bench.py refuses to run with any P265R_* variable set)
    for (const char* k : {"P265R_FAIR", "P265R_QUAD", "P265R_SCHEDULE", "P265R_SAO_ROWS", "P265R_LUMA_LEAD", "P265R_ROW_WAVES",
                          "P265R_FORK_PREP", "P265R_SPLIT", "P265R_XG", "P265R_TR_CHECK"})
        if (std::getenv(k)) ctx->describe += std::string(ctx->describe.empty() ? "" : ", ") + "\"" + k + "\"";
    if (const char* v = std::getenv("P265R_SCHEDULE")) ctx->schedule = std::strcmp(v, "steps") == 0 ? 0 : 1;
    // 16-bit samples: the row pipeline while a W = 8 workgroup's LDS tiles and two line-buffer slots fit
    // 160 KB (pictures up to ≈ 4K wide), else the per-diagonal kernel (BitDepth 11..12 too: the row kernel's
    // packed Cb | Cr angular sums are split into 6-bit halves there, pang in intra_rows.h)
    if (g.pel16 && rows_lds_bytes<uint16_t>(g, 8, 2) > 160 * 1024) ctx->schedule = 0;
    if (const char* v = std::getenv("P265R_SAO_ROWS")) ctx->sao_rows = std::atoi(v) == 2 ? 2 : (v[0] != '0' ? 1 : 0);
    if (const char* v = std::getenv("P265R_LUMA_LEAD")) ctx->luma_lead = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("P265R_SPLIT")) ctx->split = v[0] != '0';
    if (const char* v = std::getenv("P265R_TR_CHECK")) g.tr_check = v[0] == '1';
    if (const char* v = std::getenv("P265R_XG")) { const int x = std::atoi(v); ctx->xg = (x == 2 || x == 4 || x == 8) ? x : 0; }
    if (const char* v = std::getenv("P265R_FORK_PREP")) ctx->fork_prep = std::atoi(v) != 0 ? 1 : 0;
    if (const char* v = std::getenv("P265R_ROW_WAVES")) {
        const int w = std::atoi(v);
        if (w == 8 || w == 12) ctx->row_waves = w;
    }
#ifdef P265R_DEBUG_DIAG
    if (const char* v = std::getenv("P265R_DEBUG_SYNC")) {
        ctx->debug_sync = v[0] == '1';
        ctx->describe += std::string(ctx->describe.empty() ? "" : ", ") + "\"P265R_DEBUG_SYNC\"";
    }
#endif
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) ctx->lanes.push_back(ctx->stream);
    if (e == hipSuccess) {
        int8_t ang[35];
        int16_t inv[35];
        for (int i = 0; i < 35; ++i) { ang[i] = (int8_t)kIntraPredAngle[i]; inv[i] = (int16_t)kInvAngle[i]; }
        uint32_t angw[35];
        for (int i = 0; i < 35; ++i) angw[i] = (uint32_t)(uint8_t)ang[i] | (uint32_t)(inv[i] ? -inv[i] : 256) << 8;
        e = hipMemcpyToSymbol(HIP_SYMBOL(c_angle), ang, sizeof(ang));
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_inv_angle), inv, sizeof(inv));
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_angw), angw, sizeof(angw));
        uint32_t ztab[64];
        for (int i = 0; i < 64; ++i) ztab[i] = avail_ztab_word(i >> 4, i & 15);
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_ztab), ztab, sizeof(ztab));
    }
    if (e != hipSuccess) {
        int rc = hip_fail(e, "p265r_create");
        p265r_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return P265R_OK;
}

void p265r_destroy(p265r_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t st : ctx->lanes) (void)hipStreamSynchronize(st);
    for (hipStream_t st : ctx->aux) if (st) (void)hipStreamSynchronize(st);
    for (hipStream_t st : ctx->aux2) if (st) (void)hipStreamSynchronize(st);
    if (ctx->pending) p265r_batch_free(ctx, ctx->pending);
    for (hipStream_t st : ctx->aux) if (st) (void)hipStreamDestroy(st);
    for (hipStream_t st : ctx->aux2) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : ctx->join2_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->last_intra_ev) (void)hipEventDestroy(ctx->last_intra_ev);
    if (ctx->last_lf_ev) (void)hipEventDestroy(ctx->last_lf_ev);
    for (hipEvent_t e : ctx->fork_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->join_ev) if (e) (void)hipEventDestroy(e);
    for (auto& r : ctx->runs) for (auto& e : r.ev) (void)hipEventDestroy(e);
    for (auto& e : ctx->spare) (void)hipEventDestroy(e);
    for (size_t i = 1; i < ctx->lanes.size(); ++i) (void)hipStreamDestroy(ctx->lanes[i]);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->cache_mem) (void)hipFree(ctx->cache_mem);
    if (ctx->d_sf) (void)hipFree(ctx->d_sf);
    if (ctx->dl_stage) (void)hipHostFree(ctx->dl_stage);
    if (ctx->sp_mem) (void)hipFree(ctx->sp_mem);
    for (hipEvent_t e : ctx->exp_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->dl_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->stage) { if (ctx->stage_pinned) (void)hipHostFree(ctx->stage); else std::free(ctx->stage); }
    delete ctx;
}

}  // extern "C"

namespace {

// The context's staging buffer (grow-only, reused across uploads) with room for `need` bytes: pinned, or
// pageable when pinning fails.
int stage_reserve(p265r_ctx* ctx, size_t need) {
    if (ctx->stage_bytes >= need) return P265R_OK;
    if (ctx->stage) { if (ctx->stage_pinned) (void)hipHostFree(ctx->stage); else std::free(ctx->stage); }
    ctx->stage = nullptr;
    ctx->stage_bytes = 0;
    const size_t want = need + need / 4;
    void* ptr = nullptr;
    if (hipHostMalloc(&ptr, want, hipHostMallocDefault) == hipSuccess) {
        ctx->stage_pinned = true;
    } else {
        (void)hipGetLastError();
        ptr = std::malloc(want);
        ctx->stage_pinned = false;
        if (!ptr) return P265R_ENOMEM;
    }
    ctx->stage = static_cast<unsigned char*>(ptr);
    ctx->stage_bytes = want;
    return P265R_OK;
}

// The batch's device allocation of `total` bytes: the context's cached one (the last freed) when it is large
// enough, else a new one -- dropping the cached one if that makes the room.
int batch_mem_take(p265r_ctx* ctx, p265r_batch* b, size_t total) {
    if (ctx->cache_mem && ctx->cache_bytes >= total) {
        b->mem = ctx->cache_mem;
        b->bytes = ctx->cache_bytes;
        ctx->cache_mem = nullptr;
        ctx->cache_bytes = 0;
        return P265R_OK;
    }
    hipError_t e = hipMalloc(&b->mem, total);
    if (e != hipSuccess && ctx->cache_mem) {
        (void)hipGetLastError();
        (void)hipFree(ctx->cache_mem);
        ctx->cache_mem = nullptr;
        ctx->cache_bytes = 0;
        e = hipMalloc(&b->mem, total);
    }
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? P265R_ENOMEM : hip_fail(e, "hipMalloc");
    b->bytes = total;
    return P265R_OK;
}

// The context's device landing buffer of a sparse upload's entries + begin words (grow-only).
int landing_reserve(p265r_ctx* ctx, size_t need) {
    if (ctx->sp_bytes >= need) return P265R_OK;
    if (ctx->sp_mem) (void)hipFree(ctx->sp_mem);
    ctx->sp_mem = nullptr;
    ctx->sp_bytes = 0;
    const size_t want = need + need / 4;
    const hipError_t e = hipMalloc(&ctx->sp_mem, want);
    if (e != hipSuccess) {
        ctx->sp_mem = nullptr;
        return e == hipErrorOutOfMemory ? P265R_ENOMEM : hip_fail(e, "hipMalloc");
    }
    ctx->sp_bytes = want;
    return P265R_OK;
}

// Sparse upload: expand the entries of nj jobs of class c (jobs, their begin words beg; their TBs start at pool
// element q0) into the coefficient pool, on stream xs.
hipError_t launch_expand(hipStream_t xs, int16_t* d_pool, int c, const ResJob* jobs, int nj, size_t q0,
                         const uint32_t* beg, const uint32_t* d_ent) {
    const int per_block = kExpandWaves * kExpandTile;    // int16 per block of a fixed-size class
    switch (c) {
        case RC_DST4: case RC_DCT4:
            coef_expand_kernel<2><<<(unsigned)(((size_t)nj * 16 + per_block - 1) / per_block), 64 * kExpandWaves, 0, xs>>>(d_pool, q0, beg, d_ent, nj); break;
        case RC_DCT8:
            coef_expand_kernel<3><<<(unsigned)(((size_t)nj * 64 + per_block - 1) / per_block), 64 * kExpandWaves, 0, xs>>>(d_pool, q0, beg, d_ent, nj); break;
        case RC_DCT16:
            coef_expand_kernel<4><<<(unsigned)(((size_t)nj * 256 + per_block - 1) / per_block), 64 * kExpandWaves, 0, xs>>>(d_pool, q0, beg, d_ent, nj); break;
        case RC_DCT32:
            coef_expand_kernel<5><<<(unsigned)(((size_t)nj * 1024 + per_block - 1) / per_block), 64 * kExpandWaves, 0, xs>>>(d_pool, q0, beg, d_ent, nj); break;
        default:
            coef_expand_jobs_kernel<<<(unsigned)((nj + kExpandWaves - 1) / kExpandWaves), 64 * kExpandWaves, 0, xs>>>(d_pool, jobs, beg, d_ent, nj); break;
    }
    return hipGetLastError();
}

// The upload of p265r_batch_upload (sp null: dense coefficients) and p265r_batch_upload_sparse (sp[i]: the
// entries of pics[i]'s transformed TBs): plan (upload_host.h: validation, layout, chunking), allocate, then per
// chunk pack, copy and -- sparse -- expand on the device (coef_expand.h), then the header and the join.
int upload_batch(p265r_ctx* ctx, const p265r_picture* pics, const p265r_sparse_coef* sp, int n_pics, p265r_batch** out) {
    if (!ctx || !pics || n_pics <= 0 || !out) return P265R_EINVAL;
    *out = nullptr;
    UploadPlan plan;
    if (const int rc = plan_upload(ctx->params, ctx->geo, ctx->n_ctus, ctx->xg, ctx->split != 0, ctx->num_cus, pics, sp, n_pics, &plan))
        return rc;
    (void)hipSetDevice(ctx->device);
    if (const int rc = stage_reserve(ctx, plan.stage_need)) return rc;
    unsigned char* host = ctx->stage;
    p265r_batch* b = new (std::nothrow) p265r_batch();
    if (!b) return P265R_ENOMEM;
    if (const int rc = batch_mem_take(ctx, b, plan.total)) { delete b; return rc; }
    if (const int rc = landing_reserve(ctx, plan.sp_need)) { (void)hipFree(b->mem); delete b; return rc; }
    b->n_pics = n_pics;
    b->stream = ctx->stream;
    if (ctx->pipeline > 1) {
        b->lane = ctx->next_lane++ % ctx->pipeline;
        b->stream = ctx->lanes[b->lane];
    }
    b->sao = plan.sao;
    b->dbk = plan.dbk;
    b->recon_input = plan.recon_input;
    b->ragged = plan.ragged;
    b->size = plan.psize;
    unsigned char* dbase = static_cast<unsigned char*>(b->mem);
    b->d_pics = reinterpret_cast<DevPic*>(dbase + plan.o_pics);
    b->d_pool = reinterpret_cast<int16_t*>(dbase + plan.o_pool);
    b->d_res = reinterpret_cast<int16_t*>(dbase + plan.o_res);
    b->d_err = reinterpret_cast<int*>(dbase + plan.o_err);
    b->d_xg_prog = plan.xg_ok ? b->d_err + 64 + kRowCuSlots * 4 : nullptr;
    b->d_xg_lines = plan.xg_ok ? dbase + plan.o_xgl : nullptr;
    for (int c = 0; c < RC_NUM; ++c) {
        b->d_jobs[c] = reinterpret_cast<ResJob*>(dbase + plan.o_jobs[c]);
        b->n_jobs[c] = plan.n_jobs[c];
        b->slab[c] = (uint32_t)plan.pool_base[c];
    }
    b->view.rec0 = dbase + plan.o_rec;
    b->view.out0 = plan.lf ? dbase + plan.o_out : dbase + plan.o_rec;
    b->view.pic_bytes = plan.pic_plane_bytes;
    for (int c = 0; c < 3; ++c) b->view.plane_off[c] = plan.plane_off[c];
    b->view.ctus0 = reinterpret_cast<const p265r_ctu*>(dbase + plan.o_ctus);
    b->view.err = b->d_err;
    b->h_pics.resize(n_pics);

    // Packing and H2D overlap: the pictures go in chunks, and a chunk's copies (UploadPlan::chunk_copies) are
    // enqueued as soon as it is packed, so the DMA engine copies chunk k while the host packs chunk k + 1.
    // The DevPic table and the error word follow last; the gaps between the arrays are zeroed on the device.
    hipError_t e = hipSuccess;
    hipStream_t st = b->stream;
    unsigned char* d_sp = static_cast<unsigned char*>(ctx->sp_mem);
    auto h2d = [&](const H2dCopy& c) {
        if (e != hipSuccess) return;
        e = hipMemcpyAsync((c.to_landing ? d_sp : dbase) + c.dst_off, host + c.host_off, c.bytes, hipMemcpyHostToDevice, st);
        b->h2d_bytes += c.bytes;
    };
    if (e == hipSuccess) e = hipMemsetAsync(dbase + plan.o_res, 0, plan.o_ijobs - plan.o_res, st);   // residual pool, job lists
    if (e == hipSuccess) e = hipMemsetAsync(dbase + plan.o_ijobs, 0, plan.o_rec - plan.o_ijobs, st);
    // sparse: the expand kernels of a chunk follow its copies on the same stream; with timing on, inside an
    // event pair per chunk
    const uint32_t* d_ent = reinterpret_cast<const uint32_t*>(d_sp);
    const uint32_t* d_beg = sp ? reinterpret_cast<const uint32_t*>(d_sp + (plan.s_beg - plan.s_ent)) : nullptr;
    const bool time_expand = sp && ctx->timing;
    auto expand_event = [&](int idx) -> hipEvent_t {             // [2 k], [2 k + 1]: chunk k's timed pair
        if (ctx->exp_ev.size() <= (size_t)idx) ctx->exp_ev.resize((size_t)idx + 1, nullptr);
        if (!ctx->exp_ev[idx] && e == hipSuccess) e = hipEventCreate(&ctx->exp_ev[idx]);
        return ctx->exp_ev[idx];
    };
    ctx->last_expand_ms = -1.0;
    for (int k = 0; k < plan.n_chunks; ++k) {
        const int p0 = plan.chunk_lo(k), p1 = plan.chunk_lo(k + 1);
        parallel_for(p1 - p0, [&](int j) { pack_picture(plan, p0 + j, pics, sp, host, dbase, &b->h_pics[p0 + j]); });
        if (sp) close_chunk(plan, k, host);
        for (const H2dCopy& c : plan.chunk_copies(k)) h2d(c);
        if (!sp) continue;
        if (time_expand) { hipEvent_t t0 = expand_event(2 * k); if (e == hipSuccess) e = hipEventRecord(t0, st); }
        for (int c = 0; c < RC_NUM && e == hipSuccess; ++c) {
            const size_t j0 = (size_t)plan.job_at[p0][c];
            const int nj = plan.job_at[p1][c] - plan.job_at[p0][c];
            if (nj) e = launch_expand(st, b->d_pool, c, b->d_jobs[c] + j0, nj, plan.pool_at[p0][c],
                                      d_beg + plan.beg_kc[k * RC_NUM + c], d_ent);
        }
        if (time_expand) { hipEvent_t t1 = expand_event(2 * k + 1); if (e == hipSuccess) e = hipEventRecord(t1, st); }
    }
    // alignment gaps between the arrays and the coefficient pool's pad: zero on the device, as the device
    // image always had them; then the DevPic table and the error word (complete before returning: the
    // staging buffer is refilled by the next upload)
    pack_header(plan, b->h_pics.data(), host);
    for (const ZeroRange& z : plan.gap_zeros())
        if (e == hipSuccess && z.bytes) e = hipMemsetAsync(dbase + z.off, 0, z.bytes, st);
    h2d(plan.header_copy());
    if (e == hipSuccess && plan.recon_input) {
        const Geo& g = ctx->geo;
        const size_t pb = plan.pel_bytes;
        // (a wide context's 8-bit component: its uint8_t planes are widened into the staging buffer first)
        if (!plan.wide_at.empty())
            parallel_for(n_pics, [&](int i) {
                for (int c = 0; c < (g.mono ? 1 : 3); ++c)
                    if (plan.wide_at[i][c] != SIZE_MAX) widen_plane(plan, i, c, pics, host);
            });
        for (int i = 0; i < n_pics && e == hipSuccess; ++i)
            for (int c = 0; c < (g.mono ? 1 : 3) && e == hipSuccess; ++c) {
                const size_t wd = (size_t)(plan.psize[i][0] >> (c ? 1 : 0)), ht = (size_t)(plan.psize[i][1] >> (c ? 1 : 0));
                const bool wide = !plan.wide_at.empty() && plan.wide_at[i][c] != SIZE_MAX;
                const void* src = wide ? static_cast<const void*>(host + plan.wide_at[i][c]) : pics[i].recon[c];
                e = hipMemcpy2DAsync(b->h_pics[i].rec[c], g.stride[c] * pb, src, wd * pb, wd * pb, ht, hipMemcpyHostToDevice, st);
                b->h2d_bytes += wd * pb * ht;
            }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (time_expand && e == hipSuccess) {
        double ms = 0;
        for (int k = 0; k < plan.n_chunks && e == hipSuccess; ++k) {
            float t = 0;
            e = hipEventElapsedTime(&t, ctx->exp_ev[2 * k], ctx->exp_ev[2 * k + 1]);
            ms += t;
        }
        if (e == hipSuccess) ctx->last_expand_ms = ms;
    }
    if (e != hipSuccess) {
        // copies (and expand kernels) enqueued before the failing call may still be in flight: let them end
        // before the allocation they write is freed
        int rc = hip_fail(e, "upload");
        (void)hipStreamSynchronize(st);
        (void)hipFree(b->mem);
        delete b;
        return rc;
    }
    *out = b;
    return P265R_OK;
}

// Stream plan of one run (no phase timing):
// * a batch smaller than the chip (< 1 picture per CU: tile units, decoder batches, a few workgroups
//   per launch) keeps every phase on its lane stream, and such batches run side by side: extra prep /
//   residual streams would outnumber the hardware queues (4 by default) and put one lane's kernels
//   behind another's (C5, 4 lanes: 2.3 M CTU/s forked vs 3.0 M unforked; 5.2 M unforked at
//   GPU_MAX_HW_QUEUES=8, round 4);
// * a chip-filling batch forks its prep kernel onto the lane's prep stream (P265R_FORK_PREP, default on);
// * P265R_PHASE_ORDER builds: a chip-filling batch in a pipelined context runs in PHASE ORDER: its residual +
//   prep phase (on two streams of the lane's own) waits for the last intra launch of ANY lane and runs beside
//   the previous batch's loop filters; its intra phase waits for the last loop-filter launch, so the row
//   kernel (W = 12, all of every CU's registers) always runs alone -- overlapping it with the other
//   phases cost as much as it hid (3 lanes unordered = serial, 43.0 vs 43.5 M CTU/s, round 4);
// * P265R_EARLY_RESIDUAL builds: otherwise (a lone lane's re-runs) the EARLY residual phase: residual + prep
//   start when this batch's previous intra phase ends, beside its previous loop filters.
struct RunPlan {
    bool recon;            // not a recon-input batch: the residual and intra phases run
    bool prep;             // ... on the row pipeline: the job prep kernel runs
    bool fork;             // ... on the lane's prep stream (ctx->aux) instead of the lane stream
    bool ordered, early;   // the two check-variant schedules
    hipEvent_t after;      // ordered / early: the event the residual + prep phase starts behind, on streams of
                           // its own (the residual kernels on ctx->aux2), instead of in the lane stream's order
};

RunPlan plan_run(const p265r_ctx* ctx, const p265r_batch* b) {
    RunPlan rp{};
    rp.recon = !b->recon_input;
    rp.prep = rp.recon && ctx->schedule == 1;
    const bool big = b->n_pics >= ctx->num_cus;
    rp.fork = rp.prep && big && ctx->fork_prep;
    rp.ordered = P265R_PHASE_ORDER && ctx->pipeline > 1 && rp.fork && !ctx->timing;
    rp.early = !rp.ordered && P265R_EARLY_RESIDUAL && rp.fork && !ctx->timing && b->intra_done;
    rp.after = rp.ordered ? (ctx->last_intra_valid ? ctx->last_intra_ev : nullptr) : (rp.early ? b->intra_done : nullptr);
    return rp;
}

// Entry li of a per-lane list of second streams (ctx->aux, ctx->aux2) exists, with its entry of each event list
// (created on first use).
int lane_stream_reserve(std::vector<hipStream_t>& streams, std::initializer_list<std::vector<hipEvent_t>*> events, size_t li) {
    if (streams.size() <= li) {
        streams.resize(li + 1, nullptr);
        for (auto* ev : events) ev->resize(li + 1, nullptr);
    }
    if (!streams[li]) {
        HIP_TRY(hipStreamCreateWithFlags(&streams[li], hipStreamNonBlocking));
        for (auto* ev : events) HIP_TRY(hipEventCreateWithFlags(&(*ev)[li], hipEventDisableTiming));
    }
    return P265R_OK;
}

// Phase 1 of a run: the residual kernels (one per job class), the intra job prep and the deblocking edge map;
// the lane stream s continues behind all of them.
int run_residual_prep(p265r_ctx* ctx, p265r_batch* b, const Geo& g, const RunPlan& rp, p265r_timings* tm) {
    hipStream_t s = b->stream;
    const size_t li = (size_t)b->lane;
    const int bdl = g.bd[0], bdc = g.bd[1];
    const uint8_t* sf = ctx->params.scaling_list_enabled ? ctx->d_sf : nullptr;
    // ordered / early: behind rp.after, and behind the batch's own previous intra phase (the last reader of its
    // residual pool and job lists): rp.after is the last intra launch of ANY lane, which only orders after it
    // when every intra launch of the context ran phase-ordered (a small or timed batch on another lane does not)
    auto start_after = [&](hipStream_t st) -> int {
        HIP_TRY(hipStreamWaitEvent(st, rp.after, 0));
        if (b->intra_done && rp.after != b->intra_done) HIP_TRY(hipStreamWaitEvent(st, b->intra_done, 0));
        return P265R_OK;
    };
    hipStream_t rs = s;                              // the residual kernels' stream
    if (rp.after) {
        if (int rc = lane_stream_reserve(ctx->aux2, {&ctx->join2_ev}, li)) return rc;
        rs = ctx->aux2[li];
        if (int rc = start_after(rs)) return rc;
    }
    hipStream_t ps = s;                              // the prep kernel's stream
    if (rp.fork) {
        if (int rc = lane_stream_reserve(ctx->aux, {&ctx->fork_ev, &ctx->join_ev}, li)) return rc;
        ps = ctx->aux[li];
        if (rp.after) {
            if (int rc = start_after(ps)) return rc;
        } else {
            HIP_TRY(hipEventRecord(ctx->fork_ev[li], s));
            HIP_TRY(hipStreamWaitEvent(ps, ctx->fork_ev[li], 0));
        }
    }
    if (rp.prep) {
        // intra job preparation (availability, filter decisions, Cb/Cr pairing): independent
        // of the residuals, timed with the residual phase; enqueued first so that, forked, its
        // waves start before the residual kernels fill the chip
        // (tr_info: launch_rows' latency layouts, the cross-group kernel and the W = 16 split, need 2 n_pics <= CUs)
        Geo gp = g;
        gp.tr_info = (g.mono ? 1 : 2) * (long long)b->n_pics <= ctx->num_cus ? 1 : 0;
        intra_prep_kernel<<<dim3(g.wc, g.hc, b->n_pics), 64, 0, ps>>>(b->d_pics, gp, b->view);
        ++tm->residual_launches;
        if (ps != s) HIP_TRY(hipEventRecord(ctx->join_ev[li], ps));
    }
    // (scaling lists: the SL instances, which read m from the context's ScalingFactor table)
#define P265R_RES_LAUNCH(K, KSL, blocks, ...)                                                                     \
    do {                                                                                                          \
        if (sf) KSL<<<(blocks), 256, 0, rs>>>(__VA_ARGS__, sf);                                                   \
        else K<<<(blocks), 256, 0, rs>>>(__VA_ARGS__, nullptr);                                                   \
        ++tm->residual_launches;                                                                                  \
    } while (0)
    if (rp.recon && b->n_jobs[RC_DST4])
        P265R_RES_LAUNCH((residual4_kernel<true, false>), (residual4_kernel<true, true>), (b->n_jobs[RC_DST4] + 255) / 256,
                         b->d_pool, b->d_res, b->d_jobs[RC_DST4], b->n_jobs[RC_DST4], bdl, b->slab[RC_DST4]);
    if (rp.recon && b->n_jobs[RC_DCT4])
        P265R_RES_LAUNCH((residual4_kernel<false, false>), (residual4_kernel<false, true>), (b->n_jobs[RC_DCT4] + 255) / 256,
                         b->d_pool, b->d_res, b->d_jobs[RC_DCT4], b->n_jobs[RC_DCT4], bdc, b->slab[RC_DCT4]);
    if (rp.recon && b->n_jobs[RC_DCT8])
        P265R_RES_LAUNCH((residualN_kernel<3, false>), (residualN_kernel<3, true>), (b->n_jobs[RC_DCT8] + 31) / 32,
                         b->d_pool, b->d_res, b->d_jobs[RC_DCT8], b->n_jobs[RC_DCT8], bdl, bdc, b->slab[RC_DCT8]);
    if (rp.recon && b->n_jobs[RC_DCT16])
        P265R_RES_LAUNCH((residualN_kernel<4, false>), (residualN_kernel<4, true>), (b->n_jobs[RC_DCT16] + 15) / 16,
                         b->d_pool, b->d_res, b->d_jobs[RC_DCT16], b->n_jobs[RC_DCT16], bdl, bdc, b->slab[RC_DCT16]);
    if (rp.recon && b->n_jobs[RC_DCT32])
        P265R_RES_LAUNCH((residualN_kernel<5, false>), (residualN_kernel<5, true>), (b->n_jobs[RC_DCT32] + 7) / 8,
                         b->d_pool, b->d_res, b->d_jobs[RC_DCT32], b->n_jobs[RC_DCT32], bdl, bdc, b->slab[RC_DCT32]);
#undef P265R_RES_LAUNCH
    if (rp.recon && b->n_jobs[RC_TSKIP]) {
        residual_tskip_kernel<<<(b->n_jobs[RC_TSKIP] + 255) / 256, 256, 0, rs>>>(b->d_pool, b->d_res, b->d_jobs[RC_TSKIP], b->n_jobs[RC_TSKIP], bdl, bdc, sf);
        ++tm->residual_launches;
    }
    if (ps != s) HIP_TRY(hipStreamWaitEvent(s, ctx->join_ev[li], 0));
    if (rs != s) {
        HIP_TRY(hipEventRecord(ctx->join2_ev[li], rs));
        HIP_TRY(hipStreamWaitEvent(s, ctx->join2_ev[li], 0));
    }
    if (b->dbk) {
        // deblocking edge / QpY map: depends on the records only
        if (g.pel16) dbk_map_kernel<uint16_t><<<dim3(ctx->n_ctus, b->n_pics), 64, 0, s>>>(b->d_pics, g);
        else dbk_map_kernel<uint8_t><<<dim3(ctx->n_ctus, b->n_pics), 64, 0, s>>>(b->d_pics, g);   // (context-size grid)
        ++tm->residual_launches;
    }
    HIP_TRY(hipGetLastError());
    return P265R_OK;
}

// Phase 2 of a run: the intra wavefront on the lane stream -- the row pipeline, or one launch per anti-diagonal.
int run_intra(p265r_ctx* ctx, p265r_batch* b, const Geo& g, const RunPlan& rp, p265r_timings* tm) {
    hipStream_t s = b->stream;
    if (rp.recon && ctx->schedule == 1) {
        // per-CU workgroup slots cleared per run; the error word (d_err[0]) is sticky from upload on,
        // so p265r_batch_status / p265r_batch_download report a give-up in ANY run of the batch
        // (and the cross-group kernel's progress words behind them)
        HIP_TRY(hipMemsetAsync(b->d_err + 64, 0, kRowCuSlots * 16 + (b->d_xg_prog ? sizeof(int) * 2 * ((size_t)g.hc + 1) * b->n_pics : 0), s));
        if (rp.ordered && ctx->last_lf_valid) HIP_TRY(hipStreamWaitEvent(s, ctx->last_lf_ev, 0));
        // does another lane have a run enqueued that the API has not synchronised since?  (host
        // state only, so the build a run gets is a function of the call sequence)
        // (phase order: the intra phase has the GPU to itself by construction)
        const bool alone = rp.ordered || (ctx->lane_busy & ~(1u << b->lane)) == 0u;
        if (int rc = launch_rows(ctx, b, s, alone)) return rc;
        ++tm->intra_launches;
    }
    const int n_steps = (rp.recon && ctx->schedule == 0) ? (g.wc - 1) + 2 * (g.hc - 1) + 1 : 0;
    if (n_steps) { ctx->last_layout = "steps"; ctx->last_row_waves = 0; }
    for (int step = 0; step < n_steps; ++step) {
        const int d = step - (g.wc - 1);
        const int cy_min = d > 0 ? (d + 1) / 2 : 0;
        const int cy_max = std::min(g.hc - 1, step / 2);
        if (cy_max < cy_min) continue;
        dim3 grid(cy_max - cy_min + 1, b->n_pics);
        if (g.pel16) intra_step_kernel<uint16_t><<<grid, 64, 0, s>>>(b->d_pics, b->d_pool, b->d_res, g, step, cy_min);
        else intra_step_kernel<uint8_t><<<grid, 64, 0, s>>>(b->d_pics, b->d_pool, b->d_res, g, step, cy_min);
        ++tm->intra_launches;
    }
    HIP_TRY(hipGetLastError());
    if (rp.recon) {                                  // the residual pool and job lists are free again
        if (!b->intra_done) HIP_TRY(hipEventCreateWithFlags(&b->intra_done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->intra_done, s));
        if (!ctx->last_intra_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->last_intra_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->last_intra_ev, s));
        ctx->last_intra_valid = true;
    }
    return P265R_OK;
}

// Phase 3 of a run: the in-loop filters (deblocking + SAO) on the lane stream.
int run_loop_filters(p265r_ctx* ctx, p265r_batch* b, const Geo& g, const RunPlan& rp, p265r_timings* tm) {
    hipStream_t s = b->stream;
    if (int rc = launch_loop_filters(ctx, b, g, s, &tm->sao_launches)) return rc;
    if (rp.ordered) {                                // the next batch's intra phase starts after this
        if (!ctx->last_lf_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->last_lf_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->last_lf_ev, s));
        ctx->last_lf_valid = true;
    }
    return P265R_OK;
}

}  // namespace

extern "C" {

int p265r_batch_upload(p265r_ctx* ctx, const p265r_picture* pics, int n_pics, p265r_batch** out) {
    return upload_batch(ctx, pics, nullptr, n_pics, out);
}

int p265r_batch_upload_sparse(p265r_ctx* ctx, const p265r_picture* pics, const p265r_sparse_coef* sp, int n_pics,
                              p265r_batch** out) {
    if (out) *out = nullptr;
    if (!sp) return P265R_EINVAL;
    return upload_batch(ctx, pics, sp, n_pics, out);
}

int p265r_batch_upload_bytes(p265r_ctx* ctx, p265r_batch* b, uint64_t* h2d_bytes) {
    if (!ctx || !b || !h2d_bytes) return P265R_EINVAL;
    *h2d_bytes = b->h2d_bytes;
    return P265R_OK;
}

int p265r_batch_run(p265r_ctx* ctx, p265r_batch* b) {
    if (!ctx || !b) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = b->stream;
    Geo g = ctx->geo;
    g.ragged = b->ragged ? 1 : 0;
    p265r_timings tm{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (ctx->timing) {
        for (auto& e : ev) {
            if (!ctx->spare.empty()) { e = ctx->spare.back(); ctx->spare.pop_back(); }
            else HIP_TRY(hipEventCreate(&e));
        }
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    if (ctx->params.scaling_list_enabled && !ctx->d_sf && !b->recon_input) return P265R_ESTATE;   // factors not set
    ++b->runs;
    ctx->lane_busy |= 1u << b->lane;
    const RunPlan rp = plan_run(ctx, b);
    if (int rc = run_residual_prep(ctx, b, g, rp, &tm)) return rc;
    if (ctx->debug_sync) { fprintf(stderr, "[p265r] residual phase enqueued\n"); HIP_TRY(hipStreamSynchronize(s)); fprintf(stderr, "[p265r] residual phase done\n"); }
    if (ctx->timing) HIP_TRY(hipEventRecord(ev[1], s));
    if (int rc = run_intra(ctx, b, g, rp, &tm)) return rc;
    if (ctx->debug_sync) { fprintf(stderr, "[p265r] intra phase enqueued\n"); HIP_TRY(hipStreamSynchronize(s)); fprintf(stderr, "[p265r] intra phase done\n"); }
    if (ctx->timing) HIP_TRY(hipEventRecord(ev[2], s));
    if (int rc = run_loop_filters(ctx, b, g, rp, &tm)) return rc;
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ev[3], s));
        p265r_ctx::Run run;
        for (int i = 0; i < 4; ++i) run.ev[i] = ev[i];
        run.counts = tm;
        ctx->runs.push_back(run);
        ctx->have_timing = true;
    }
    return P265R_OK;
}

int p265r_batch_download(p265r_ctx* ctx, p265r_batch* b, const p265r_picture* pics, int n_pics) {
    if (!ctx || !b || !pics || n_pics != b->n_pics) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    const Geo& g = ctx->geo;
    // planes to copy: (host destination, device source, row pitch, width, height)
    struct Item { void* dst; const unsigned char* src; int pitch, w, h; size_t bytes; };
    std::vector<Item> items;
    const int pb = g.pel16 ? 2 : 1;                          // bytes per sample on the device
    // a wide context's 8-bit component (unequal bit depths): the host planes are uint8_t, so the requested planes
    // are narrowed on the device first (narrow.h) and copied from the batch's staging area, rows tight
    b->narrow_items.clear();
    std::vector<size_t> narrow_of, narrow_off;               // per narrow item: its copy item, its offset in the area
    size_t narrow_need = 0;
    int nw_max = 0, nh_max = 0;
    for (int i = 0; i < n_pics; ++i)
        for (int c = 0; c < (g.mono ? 1 : 3); ++c) {      // (monochrome: out[1..2] / recon[1..2] are never touched)
            const int sub = c ? 1 : 0;
            const bool narrow = g.pel16 && g.bd[c] <= 8;
            const int ws = b->size[i][0] >> sub, h = b->size[i][1] >> sub;
            const int w = ws * (narrow ? 1 : pb);                                    // (w in bytes)
            const int pitch = (c ? g.stride[1] : g.stride[0]) * pb;
            auto add = [&](void* dst, const uint8_t* src) {
                if (narrow) {
                    narrow_of.push_back(items.size());
                    b->narrow_items.push_back({reinterpret_cast<const uint16_t*>(src), nullptr, ws, h, c ? g.stride[1] : g.stride[0],
                                               0});
                    narrow_off.push_back(narrow_need);
                    narrow_need += align_up((size_t)w * h, 256);
                    nw_max = std::max(nw_max, ws);
                    nh_max = std::max(nh_max, h);
                }
                items.push_back({dst, src, narrow ? w : pitch, w, h, (size_t)w * h});
            };
            if (pics[i].out[c]) add(pics[i].out[c], b->h_pics[i].out[c]);
            if (pics[i].recon[c] && !b->recon_input) add(pics[i].recon[c], b->h_pics[i].rec[c]);
        }
    if (!b->narrow_items.empty()) {
        const size_t n_it = b->narrow_items.size();
        const size_t head = align_up(sizeof(NarrowItem) * n_it, 256);
        const int segs = (nw_max + kNarrowSeg - 1) / kNarrowSeg;
        if ((unsigned long long)n_it * (unsigned)segs >= (1ull << 31)) return P265R_ERANGE;
        if (b->narrow_bytes < head + narrow_need) {          // (an earlier download's launch may still read the old one)
            if (b->d_narrow) { HIP_TRY(hipStreamSynchronize(b->stream)); (void)hipFree(b->d_narrow); }
            b->d_narrow = nullptr;
            b->narrow_bytes = 0;
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->d_narrow), head + narrow_need);
            if (e != hipSuccess) { b->d_narrow = nullptr; return e == hipErrorOutOfMemory ? P265R_ENOMEM : hip_fail(e, "hipMalloc"); }
            b->narrow_bytes = head + narrow_need;
        }
        for (size_t k = 0; k < n_it; ++k) {
            NarrowItem& it = b->narrow_items[k];
            it.dst = b->d_narrow + head + narrow_off[k];
            items[narrow_of[k]].src = it.dst;
        }
        HIP_TRY(hipMemcpyAsync(b->d_narrow, b->narrow_items.data(), sizeof(NarrowItem) * n_it, hipMemcpyHostToDevice, b->stream));
        narrow_kernel<<<dim3((unsigned)(n_it * segs), (unsigned)((nh_max + kNarrowWaves - 1) / kNarrowWaves)), 64 * kNarrowWaves, 0,
                        b->stream>>>(reinterpret_cast<const NarrowItem*>(b->d_narrow), segs);
        HIP_TRY(hipGetLastError());
    }
    // D2H through two halves of a pinned bounce buffer (DMA at pinned speed; the copy into the
    // caller's pageable planes runs on host threads while the next chunk's DMA is in flight)
    if (!ctx->dl_stage) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->dl_stage), 2 * kDlHalf, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            ctx->dl_stage = nullptr;
        }
    }
    if (!ctx->dl_stage) {                                   // no pinned memory: straight pageable copies
        for (const Item& it : items)
            HIP_TRY(hipMemcpy2DAsync(it.dst, it.w, it.src, it.pitch, it.w, it.h, hipMemcpyDeviceToHost, b->stream));
        return p265r_batch_status(ctx, b);
    }
    if (!ctx->dl_ev[0]) {
        HIP_TRY(hipEventCreateWithFlags(&ctx->dl_ev[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->dl_ev[1], hipEventDisableTiming));
    }
    // chunks: consecutive items of at most kDlHalf bytes (an item larger than that goes alone, direct)
    std::vector<std::pair<size_t, size_t>> chunks;          // [first, last) item
    for (size_t i = 0; i < items.size();) {
        size_t j = i, bytes = 0;
        while (j < items.size() && (j == i || bytes + items[j].bytes <= kDlHalf)) bytes += items[j++].bytes;
        chunks.push_back({i, j});
        i = j;
    }
    auto enqueue = [&](size_t k) -> hipError_t {
        unsigned char* st = ctx->dl_stage + (k & 1) * kDlHalf;
        size_t off = 0;
        for (size_t i = chunks[k].first; i < chunks[k].second; ++i) {
            const Item& it = items[i];
            hipError_t e = it.bytes > kDlHalf
                ? hipMemcpy2DAsync(it.dst, it.w, it.src, it.pitch, it.w, it.h, hipMemcpyDeviceToHost, b->stream)
                : hipMemcpy2DAsync(st + off, it.w, it.src, it.pitch, it.w, it.h, hipMemcpyDeviceToHost, b->stream);
            if (e != hipSuccess) return e;
            off += it.bytes;
        }
        return hipEventRecord(ctx->dl_ev[k & 1], b->stream);
    };
    if (!chunks.empty()) HIP_TRY(enqueue(0));
    for (size_t k = 0; k < chunks.size(); ++k) {
        if (k + 1 < chunks.size()) HIP_TRY(enqueue(k + 1));          // into the other half (its copy-out is done)
        HIP_TRY(hipEventSynchronize(ctx->dl_ev[k & 1]));
        const unsigned char* st = ctx->dl_stage + (k & 1) * kDlHalf;
        const size_t first = chunks[k].first, n = chunks[k].second - first;
        std::vector<size_t> offs(n);
        for (size_t i = 0, off = 0; i < n; ++i) { offs[i] = off; off += items[first + i].bytes; }
        parallel_for((int)n, [&](int i) {
            const Item& it = items[first + i];
            if (it.bytes <= kDlHalf) std::memcpy(it.dst, st + offs[i], it.bytes);
        });
    }
    return p265r_batch_status(ctx, b);
}

int p265r_batch_status(p265r_ctx* ctx, p265r_batch* b) {
    if (!ctx || !b) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    // the lane is idle now (every run on it, of any batch, has completed)
    ctx->lane_busy &= ~(1u << b->lane);
    for (void* p : b->exp_idx) (void)hipFree(p);
    b->exp_idx.clear();
    int err = 0;
    HIP_TRY(hipMemcpy(&err, b->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (err) {
        g_last_hip_error = (err & 1) ? "intra row pipeline: dependency wait timed out"
                                     : "job prep self-check (P265R_TR_CHECK): a job covering the bottom row's left half "
                                       "comes after the half-CTU publish point";
        return P265R_EHIP;
    }
    return P265R_OK;
}

int p265r_batch_digest(p265r_ctx* ctx, p265r_batch* b, int which, uint64_t* out, int n) {
    if (!ctx || !b || !out || n != 3 * b->n_pics || (which != 0 && which != 1)) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    // after every run enqueued on the batch's lane (stream order); one device buffer per call
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), sizeof(uint64_t) * (size_t)n));
    hipError_t e = hipMemsetAsync(d, 0, sizeof(uint64_t) * (size_t)n, b->stream);
    if (e == hipSuccess) {
        // (monochrome: no block for planes 1 and 2, whose entries stay zero)
        const dim3 grid((unsigned)((ctx->geo.h + kDigestRows - 1) / kDigestRows), ctx->geo.mono ? 1 : 3, (unsigned)b->n_pics);
        digest_kernel<<<grid, 256, 0, b->stream>>>(b->d_pics, ctx->geo, which == 0 ? 1 : 0, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "p265r_batch_digest");
    return p265r_batch_status(ctx, b);
}

int p265r_batch_digest_async(p265r_ctx* ctx, p265r_batch* b, int which, int slot) {
    if (!ctx || !b || (which != 0 && which != 1) || slot < 0 || slot >= P265R_DIGEST_SLOTS) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t per_slot = sizeof(uint64_t) * 3 * (size_t)b->n_pics;
    if (!b->d_dig) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->d_dig), per_slot * P265R_DIGEST_SLOTS));
        HIP_TRY(hipMemsetAsync(b->d_dig, 0, per_slot * P265R_DIGEST_SLOTS, b->stream));
    }
    unsigned long long* d = b->d_dig + 3 * (size_t)b->n_pics * slot;
    HIP_TRY(hipMemsetAsync(d, 0, per_slot, b->stream));
    const dim3 grid((unsigned)((ctx->geo.h + kDigestRows - 1) / kDigestRows), ctx->geo.mono ? 1 : 3, (unsigned)b->n_pics);
    digest_kernel<<<grid, 256, 0, b->stream>>>(b->d_pics, ctx->geo, which == 0 ? 1 : 0, d);
    HIP_TRY(hipGetLastError());
    ctx->lane_busy |= 1u << b->lane;
    return P265R_OK;
}

int p265r_batch_digest_slots(p265r_ctx* ctx, p265r_batch* b, uint64_t* out, int n_slots) {
    if (!ctx || !b || !out || n_slots < 1 || n_slots > P265R_DIGEST_SLOTS) return P265R_EINVAL;
    if (!b->d_dig) return P265R_ESTATE;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, b->d_dig, sizeof(uint64_t) * 3 * (size_t)b->n_pics * n_slots, hipMemcpyDeviceToHost,
                           b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return p265r_batch_status(ctx, b);
}

int p265r_batch_hash_async(p265r_ctx* ctx, p265r_batch* b, int hash_type) {
    if (!ctx || !b) return P265R_EINVAL;
    if (hash_type != P265R_HASH_MD5 && hash_type != P265R_HASH_CRC && hash_type != P265R_HASH_CHECKSUM) return P265R_EINVAL;
    // unequal bit depths: D.3.19 hashes each plane in its own sample width, the device planes have one (host hashing)
    if (ctx->geo.bd[0] != ctx->geo.bd[1]) return P265R_EUNSUPPORTED;
    if (b->runs == 0) return P265R_ESTATE;                  // (no output planes yet, as for p265r_batch_export)
    HIP_TRY(hipSetDevice(ctx->device));
    const int n_planes = 3 * b->n_pics;
    const size_t out_bytes = 16 * (size_t)n_planes, acc_bytes = sizeof(uint32_t) * (size_t)n_planes;
    if (!b->d_hash) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->d_hash), out_bytes + acc_bytes));
    uint4* out = reinterpret_cast<uint4*>(b->d_hash);
    uint32_t* acc = reinterpret_cast<uint32_t*>(b->d_hash + out_bytes);
    // monochrome: no chain or block for planes 1 and 2; their 16 bytes are zero
    const int hashed = ctx->geo.mono ? 1 : 3;
    if (ctx->geo.mono) HIP_TRY(hipMemsetAsync(out, 0, out_bytes, b->stream));
    if (hash_type == P265R_HASH_MD5) {
        hash_md5_kernel<<<dim3((unsigned)((hashed * b->n_pics + 63) / 64)), 64, 0, b->stream>>>(b->d_pics, ctx->geo, b->n_pics, out);
    } else {
        HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, b->stream));
        const dim3 grid((unsigned)((ctx->geo.h + kHashRows - 1) / kHashRows), (unsigned)hashed, (unsigned)b->n_pics);
        if (hash_type == P265R_HASH_CRC) hash_crc_kernel<<<grid, 256, 0, b->stream>>>(b->d_pics, ctx->geo, acc);
        else hash_checksum_kernel<<<grid, 256, 0, b->stream>>>(b->d_pics, ctx->geo, acc);
        HIP_TRY(hipGetLastError());
        hash_final_kernel<<<dim3((unsigned)((n_planes + 63) / 64)), 64, 0, b->stream>>>(
            b->d_pics, ctx->geo, hash_type == P265R_HASH_CRC ? 1 : 0, n_planes, acc, out);
    }
    HIP_TRY(hipGetLastError());
    ctx->lane_busy |= 1u << b->lane;
    return P265R_OK;
}

int p265r_batch_hash_read(p265r_ctx* ctx, p265r_batch* b, uint8_t* out, int n_bytes) {
    if (!ctx || !b || !out || (long long)n_bytes != 48ll * b->n_pics) return P265R_EINVAL;
    if (!b->d_hash) return P265R_ESTATE;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, b->d_hash, (size_t)n_bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return p265r_batch_status(ctx, b);
}

int p265r_batch_job_count(p265r_ctx* ctx, p265r_batch* b, uint64_t* luma, uint64_t* chroma) {
    if (!ctx || !b || !luma || !chroma) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    // per CTU slot: luma jobs | chroma jobs << 16, top-right indices (intra_prep.h), context-size slots
    const size_t n = (size_t)ctx->n_ctus * b->n_pics;
    std::vector<uint32_t> jc(4 * n);
    HIP_TRY(hipMemcpy(jc.data(), b->h_pics[0].jcount, 4 * sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    uint64_t l = 0, c = 0;
    for (size_t i = 0; i < n; ++i) { l += jc[4 * i] & 0xffffu; c += jc[4 * i] >> 16; }
    *luma = l;
    *chroma = c;
    return P265R_OK;
}

int p265r_batch_export(p265r_ctx* ctx, p265r_batch* b, const p265r_export_desc* desc, void* dev_dst, uint64_t dst_bytes,
                       const int32_t* pic_index, int n) {
    if (!ctx || !b || !desc || !dev_dst) return P265R_EINVAL;
    if (!pic_index) n = b->n_pics;
    if (n <= 0 || n > b->n_pics || n > 65535) return P265R_EINVAL;
    // ---- host checks: nothing is launched unless all of them pass ----------------------------
    const int B = ctx->params.bit_depth_luma;
    if (ctx->geo.bd[0] != ctx->geo.bd[1]) return P265R_EINVAL;      // unequal bit depths: as p265r_export_layout
    ExportShape shape;
    if (const int rc = export_check_desc(*desc, B, &shape, ctx->geo.mono != 0)) return rc;
    std::vector<char> seen(pic_index ? (size_t)b->n_pics : 0, 0);
    uint64_t slot_bytes = 0;
    int mw = 0, mh = 0;
    for (int i = 0; i < n; ++i) {
        const int pic = pic_index ? pic_index[i] : i;
        if (pic < 0 || pic >= b->n_pics) return P265R_EINVAL;
        if (pic_index) {
            if (seen[(size_t)pic]) return P265R_EINVAL;
            seen[(size_t)pic] = 1;
        }
        uint64_t sb = 0;
        if (const int rc = export_check_layout(*desc, shape, b->size[(size_t)pic][0], b->size[(size_t)pic][1], &sb)) return rc;
        slot_bytes = std::max(slot_bytes, sb);
        mw = std::max(mw, b->size[(size_t)pic][0] - desc->crop_left - desc->crop_right);
        mh = std::max(mh, b->size[(size_t)pic][1] - desc->crop_top - desc->crop_bottom);
    }
    if ((uint64_t)(uintptr_t)dev_dst % (uint64_t)shape.es) return P265R_EINVAL;
    const uint64_t need = (uint64_t)(n - 1) * desc->frame_bytes + slot_bytes;
    if (b->runs == 0) return P265R_ESTATE;                  // (a recon-input batch whose filters never ran: no planes yet)
    HIP_TRY(hipSetDevice(ctx->device));
    // the first byte of the destination (and, below, the last) is device memory of this context's device
    auto on_device = [&](const void* p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeDevice && at.device == ctx->device;
    };
    if (!on_device(dev_dst)) return P265R_EINVAL;
    if (need > dst_bytes) return P265R_ERANGE;
    if (!on_device(static_cast<const unsigned char*>(dev_dst) + need - 1)) return P265R_EINVAL;
    // ---- enqueue ---------------------------------------------------------------------------------
    ExportArgs a{};
    a.dst = static_cast<uint8_t*>(dev_dst);
    a.frame_bytes = desc->frame_bytes;
    for (int k = 0; k < 3; ++k) { a.plane_off[k] = desc->plane_off[k]; a.pitch[k] = desc->pitch[k]; }
    a.crop_l = desc->crop_left; a.crop_r = desc->crop_right; a.crop_t = desc->crop_top; a.crop_b = desc->crop_bottom;
    if (shape.rgb) {
        p265r_export_desc dc = *desc;                       // (the coefficients do not depend on the crop; a
        dc.crop_left = dc.crop_right = dc.crop_top = dc.crop_bottom = 0;   // monochrome one may be odd)
        if (const int rc = export_coefficients(dc, B, a.coef)) return rc;
        a.fscale = (float)(1.0 / (double)((1 << B) - 1));
    }
    a.shift = desc->sample == P265R_SMP_MSB16 ? 16 - B : 0;
    if (pic_index) {
        // the list's device copy lives until the lane is next synchronised (the kernel reads it in stream order)
        void* d_idx = nullptr;
        HIP_TRY(hipMalloc(&d_idx, sizeof(int32_t) * (size_t)n));
        b->exp_idx.push_back(d_idx);
        HIP_TRY(hipMemcpy(d_idx, pic_index, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        a.pic_index = static_cast<const int32_t*>(d_idx);
    }
    const int rc = ctx->geo.pel16 ? launch_export<uint16_t>(*desc, b->d_pics, ctx->geo, a, mw, mh, n, b->stream)
                                  : launch_export<uint8_t>(*desc, b->d_pics, ctx->geo, a, mw, mh, n, b->stream);
    if (rc) return rc;
    ctx->lane_busy |= 1u << b->lane;
    return P265R_OK;
}

int p265r_batch_export_resized(p265r_ctx* ctx, p265r_batch* b, const p265r_export_desc* desc, const p265r_resize_desc* rs,
                               void* dev_dst, uint64_t dst_bytes, const int32_t* pic_index, int n) {
    if (!ctx || !b || !desc || !rs || !dev_dst) return P265R_EINVAL;
    if (!pic_index) n = b->n_pics;
    if (n <= 0 || n > b->n_pics || n > 65535) return P265R_EINVAL;
    // ---- host checks: nothing is launched unless all of them pass ----------------------------
    const int B = ctx->params.bit_depth_luma;
    if (ctx->geo.bd[0] != ctx->geo.bd[1]) return P265R_EINVAL;      // unequal bit depths: as p265r_resize_layout
    ExportShape shape;
    if (const int rc = resize_check_desc(*desc, *rs, B, ctx->geo.mono != 0, &shape)) return rc;
    uint64_t slot_bytes = 0;
    if (const int rc = resize_check_layout(*desc, shape, *rs, &slot_bytes)) return rc;
    std::vector<char> seen(pic_index ? (size_t)b->n_pics : 0, 0);
    for (int i = 0; i < n; ++i) {
        const int pic = pic_index ? pic_index[i] : i;
        if (pic < 0 || pic >= b->n_pics) return P265R_EINVAL;
        if (pic_index) {
            if (seen[(size_t)pic]) return P265R_EINVAL;
            seen[(size_t)pic] = 1;
        }
        // every listed picture's own window against the filter (a ragged batch: per picture)
        if (const int rc = resize_check_window(*rs, b->size[(size_t)pic][0] - desc->crop_left - desc->crop_right,
                                               b->size[(size_t)pic][1] - desc->crop_top - desc->crop_bottom))
            return rc;
    }
    if ((uint64_t)(uintptr_t)dev_dst % (uint64_t)shape.es) return P265R_EINVAL;
    const uint64_t need = (uint64_t)(n - 1) * desc->frame_bytes + slot_bytes;
    if (b->runs == 0) return P265R_ESTATE;                  // (a recon-input batch whose filters never ran: no planes yet)
    HIP_TRY(hipSetDevice(ctx->device));
    auto on_device = [&](const void* p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeDevice && at.device == ctx->device;
    };
    if (!on_device(dev_dst)) return P265R_EINVAL;
    if (need > dst_bytes) return P265R_ERANGE;
    if (!on_device(static_cast<const unsigned char*>(dev_dst) + need - 1)) return P265R_EINVAL;
    // ---- enqueue ---------------------------------------------------------------------------------
    ResizeArgs a{};
    a.e.dst = static_cast<uint8_t*>(dev_dst);
    a.e.frame_bytes = desc->frame_bytes;
    for (int k = 0; k < 3; ++k) { a.e.plane_off[k] = desc->plane_off[k]; a.e.pitch[k] = desc->pitch[k]; }
    a.e.crop_l = desc->crop_left; a.e.crop_r = desc->crop_right; a.e.crop_t = desc->crop_top; a.e.crop_b = desc->crop_bottom;
    if (shape.rgb) {
        p265r_export_desc dc = *desc;                       // (the coefficients depend on neither crop nor upsample)
        dc.crop_left = dc.crop_right = dc.crop_top = dc.crop_bottom = 0;
        dc.upsample = P265R_UP_NEAREST;
        if (const int rc = export_coefficients(dc, B, a.e.coef)) return rc;
    }
    a.e.shift = desc->sample == P265R_SMP_MSB16 ? 16 - B : 0;
    a.ow = (int)rs->out_width; a.oh = (int)rs->out_height;
    a.grey = (1 << (B - 1)) << a.e.shift;
    resize_norm(*rs, B, a.scale, a.bias);
    if (pic_index) {
        // the list's device copy lives until the lane is next synchronised (the kernel reads it in stream order)
        void* d_idx = nullptr;
        HIP_TRY(hipMalloc(&d_idx, sizeof(int32_t) * (size_t)n));
        b->exp_idx.push_back(d_idx);
        HIP_TRY(hipMemcpy(d_idx, pic_index, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        a.e.pic_index = static_cast<const int32_t*>(d_idx);
    }
    const int rc = ctx->geo.pel16 ? launch_resize<uint16_t>(*desc, rs->filter, b->d_pics, ctx->geo, a, n, b->stream)
                                  : launch_resize<uint8_t>(*desc, rs->filter, b->d_pics, ctx->geo, a, n, b->stream);
    if (rc) return rc;
    ctx->lane_busy |= 1u << b->lane;
    return P265R_OK;
}

int p265r_batch_export_grid(p265r_ctx* ctx, p265r_batch* b, const p265r_export_desc* desc, const p265r_grid_desc* gd,
                            void* dev_dst, uint64_t dst_bytes, const int32_t* pic_index, int n_frames) {
    if (!ctx || !b || !desc || !gd || !dev_dst) return P265R_EINVAL;
    // ---- host checks: nothing is launched unless all of them pass ----------------------------
    if (gd->rows < 1 || gd->rows > 256 || gd->cols < 1 || gd->cols > 256) return P265R_EINVAL;
    const int tiles = (int)(gd->rows * gd->cols);
    // (NULL = the batch in order: n_frames must then account for every picture of it)
    if (!pic_index && (n_frames <= 0 || (int64_t)n_frames * tiles != b->n_pics)) return P265R_EINVAL;
    if (n_frames <= 0 || (int64_t)n_frames * tiles > 65535 || (int64_t)n_frames * tiles > b->n_pics) return P265R_EINVAL;
    const int n = n_frames * tiles;
    const int B = ctx->params.bit_depth_luma;
    if (ctx->geo.bd[0] != ctx->geo.bd[1]) return P265R_EUNSUPPORTED;   // unequal bit depths
    std::vector<char> seen(pic_index ? (size_t)b->n_pics : 0, 0);
    int tw = 0, th = 0;
    for (int i = 0; i < n; ++i) {
        const int pic = pic_index ? pic_index[i] : i;
        if (pic < 0 || pic >= b->n_pics) return P265R_EINVAL;
        if (pic_index) {
            if (seen[(size_t)pic]) return P265R_EINVAL;
            seen[(size_t)pic] = 1;
        }
        if (i == 0) { tw = b->size[(size_t)pic][0]; th = b->size[(size_t)pic][1]; }
        else if (b->size[(size_t)pic][0] != tw || b->size[(size_t)pic][1] != th) return P265R_EINVAL;
    }
    GridShape gs;
    if (const int rc = grid_check(*desc, *gd, B, ctx->geo.mono != 0, tw, th, &gs)) return rc;
    uint64_t slot_bytes = 0;
    if (const int rc = grid_check_layout(*desc, gs.e, gs.dw, gs.dh, &slot_bytes)) return rc;
    if ((uint64_t)(uintptr_t)dev_dst % (uint64_t)gs.e.es) return P265R_EINVAL;
    const uint64_t need = (uint64_t)(n_frames - 1) * desc->frame_bytes + slot_bytes;
    if (b->runs == 0) return P265R_ESTATE;                  // (a recon-input batch whose filters never ran: no planes yet)
    HIP_TRY(hipSetDevice(ctx->device));
    auto on_device = [&](const void* p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeDevice && at.device == ctx->device;
    };
    if (!on_device(dev_dst)) return P265R_EINVAL;
    if (need > dst_bytes) return P265R_ERANGE;
    if (!on_device(static_cast<const unsigned char*>(dev_dst) + need - 1)) return P265R_EINVAL;
    // ---- enqueue ---------------------------------------------------------------------------------
    // quarter turns: pass 1 writes F into the batch's staging area (tight, 16-byte pitches), pass 2 transposes it
    p265r_export_desc sd = *desc;
    if (gs.transpose) {
        grid_fill_layout(&sd, gs.e, gs.W, gs.H, 16);
        const uint64_t stage = sd.frame_bytes * (uint64_t)n_frames;
        if (stage > b->grid_stage_bytes) {
            if (b->grid_stage) {                            // (an earlier call's transpose may still read it)
                HIP_TRY(hipStreamSynchronize(b->stream));
                HIP_TRY(hipFree(b->grid_stage));
                b->grid_stage = nullptr;
                b->grid_stage_bytes = 0;
            }
            HIP_TRY(hipMalloc(&b->grid_stage, (size_t)stage));
            b->grid_stage_bytes = (size_t)stage;
        }
    }
    GridArgs a{};
    a.e.dst = gs.transpose ? static_cast<uint8_t*>(b->grid_stage) : static_cast<uint8_t*>(dev_dst);
    a.e.frame_bytes = sd.frame_bytes;
    for (int k = 0; k < 3; ++k) { a.e.plane_off[k] = sd.plane_off[k]; a.e.pitch[k] = sd.pitch[k]; }
    a.e.crop_l = gs.wl; a.e.crop_t = gs.wt;
    if (gs.e.rgb) {
        p265r_export_desc dc = *desc;                       // (the coefficients do not depend on the crop)
        dc.crop_left = dc.crop_right = dc.crop_top = dc.crop_bottom = 0;
        if (const int rc = export_coefficients(dc, B, a.e.coef)) return rc;
        a.e.fscale = (float)(1.0 / (double)((1 << B) - 1));
    }
    a.e.shift = desc->sample == P265R_SMP_MSB16 ? 16 - B : 0;
    a.grey = (1 << (B - 1)) << a.e.shift;
    a.rows = (int)gd->rows; a.cols = (int)gd->cols; a.tw = tw; a.th = th;
    a.W = gs.W; a.H = gs.H; a.fx = gs.fx; a.fy = gs.fy;
    {
        // the tiles' plane addresses; the device copy lives until the lane is next synchronised, like a pic_index list
        std::vector<uint64_t> tab((size_t)n * 3);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k)
                tab[(size_t)i * 3 + k] = (uint64_t)(uintptr_t)b->h_pics[(size_t)(pic_index ? pic_index[i] : i)].out[k];
        void* d_tab = nullptr;
        HIP_TRY(hipMalloc(&d_tab, sizeof(uint64_t) * tab.size()));
        b->exp_idx.push_back(d_tab);
        HIP_TRY(hipMemcpy(d_tab, tab.data(), sizeof(uint64_t) * tab.size(), hipMemcpyHostToDevice));
        a.tab = static_cast<const uint64_t*>(d_tab);
    }
    int rc = ctx->geo.pel16 ? launch_grid<uint16_t>(*desc, ctx->geo, a, n_frames, b->stream)
                            : launch_grid<uint8_t>(*desc, ctx->geo, a, n_frames, b->stream);
    if (rc) return rc;
    ctx->lane_busy |= 1u << b->lane;
    if (gs.transpose) {
        GridTransposeArgs t{};
        t.src = static_cast<const uint8_t*>(b->grid_stage);
        t.dst = static_cast<uint8_t*>(dev_dst);
        t.src_frame = sd.frame_bytes; t.dst_frame = desc->frame_bytes;
        ExportPlane pl[3];
        grid_planes(*desc, gs.e, gs.W, gs.H, pl);
        for (int k = 0; k < gs.e.n_planes; ++k) {
            t.src_off[k] = sd.plane_off[k]; t.dst_off[k] = desc->plane_off[k];
            t.src_pitch[k] = sd.pitch[k]; t.dst_pitch[k] = desc->pitch[k];
            const int c = desc->format == P265R_FMT_RGB_PACKED ? 3 : (desc->format == P265R_FMT_SEMIPLANAR && k == 1 ? 2 : 1);
            t.w[k] = (int)(pl[k].row_bytes / (uint64_t)(gs.e.es * c));
            t.h[k] = pl[k].rows;
        }
        t.tiles_y = (t.h[0] + kGridTile - 1) / kGridTile;
        rc = launch_grid_transpose(*desc, gs.e.es, t, gs.e.n_planes, n_frames, b->stream);
        if (rc) return rc;
    }
    return P265R_OK;
}

int p265r_batch_export_grid_resized(p265r_ctx* ctx, p265r_batch* b, const p265r_export_desc* desc, const p265r_resize_desc* rs,
                                    const p265r_grid_frame* frames, int n_frames, void* dev_dst, uint64_t dst_bytes,
                                    const int32_t* pic_index) {
    if (!ctx || !b || !desc || !rs || !frames || !dev_dst) return P265R_EINVAL;
    // ---- host checks: nothing is launched unless all of them pass ----------------------------
    if (n_frames <= 0 || n_frames > 65535) return P265R_EINVAL;
    const int B = ctx->params.bit_depth_luma;
    if (ctx->geo.bd[0] != ctx->geo.bd[1]) return P265R_EUNSUPPORTED;   // unequal bit depths
    int64_t n64 = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (frames[f].rows < 1 || frames[f].rows > 256 || frames[f].cols < 1 || frames[f].cols > 256) return P265R_EINVAL;
        n64 += (int64_t)(frames[f].rows * frames[f].cols);
    }
    // (NULL = the batch in order: the frames must then account for every picture of it)
    if (n64 > 65535 || n64 > b->n_pics || (!pic_index && n64 != b->n_pics)) return P265R_EINVAL;
    const int n = (int)n64;
    std::vector<char> seen(pic_index ? (size_t)b->n_pics : 0, 0);
    int tw = 0, th = 0;
    for (int i = 0; i < n; ++i) {
        const int pic = pic_index ? pic_index[i] : i;
        if (pic < 0 || pic >= b->n_pics) return P265R_EINVAL;
        if (pic_index) {
            if (seen[(size_t)pic]) return P265R_EINVAL;
            seen[(size_t)pic] = 1;
        }
        if (i == 0) { tw = b->size[(size_t)pic][0]; th = b->size[(size_t)pic][1]; }
        else if (b->size[(size_t)pic][0] != tw || b->size[(size_t)pic][1] != th) return P265R_EINVAL;
    }
    GridRsPlan plan;
    if (const int rc = grid_resize_plan(*desc, *rs, frames, n_frames, B, ctx->geo.mono != 0, tw, th, &plan)) return rc;
    uint64_t slot_bytes = 0;
    if (const int rc = resize_check_layout(*desc, plan.e, *rs, &slot_bytes)) return rc;
    if ((uint64_t)(uintptr_t)dev_dst % (uint64_t)plan.e.es) return P265R_EINVAL;
    const uint64_t need = (uint64_t)(n_frames - 1) * desc->frame_bytes + slot_bytes;
    if (b->runs == 0) return P265R_ESTATE;                  // (a recon-input batch whose filters never ran: no planes yet)
    HIP_TRY(hipSetDevice(ctx->device));
    auto on_device = [&](const void* p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeDevice && at.device == ctx->device;
    };
    if (!on_device(dev_dst)) return P265R_EINVAL;
    if (need > dst_bytes) return P265R_ERANGE;
    if (!on_device(static_cast<const unsigned char*>(dev_dst) + need - 1)) return P265R_EINVAL;
    // ---- enqueue ---------------------------------------------------------------------------------
    // quarter turns: pass 1 writes those frames' R (ow rows of oh) into the batch's staging area (tight, 16-byte
    // pitches), pass 2 transposes them
    p265r_export_desc sd = *desc;
    if (plan.n_stage) {
        grid_fill_layout(&sd, plan.e, plan.oh, plan.ow, 16);
        const uint64_t stage = sd.frame_bytes * (uint64_t)plan.n_stage;
        if (stage > b->grid_stage_bytes) {
            if (b->grid_stage) {                            // (an earlier call's transpose may still read it)
                HIP_TRY(hipStreamSynchronize(b->stream));
                HIP_TRY(hipFree(b->grid_stage));
                b->grid_stage = nullptr;
                b->grid_stage_bytes = 0;
            }
            HIP_TRY(hipMalloc(&b->grid_stage, (size_t)stage));
            b->grid_stage_bytes = (size_t)stage;
        }
    }
    GridRsArgs a{};
    a.r.e.dst = static_cast<uint8_t*>(dev_dst);
    a.r.e.frame_bytes = desc->frame_bytes;
    for (int k = 0; k < 3; ++k) {
        a.r.e.plane_off[k] = desc->plane_off[k]; a.r.e.pitch[k] = desc->pitch[k];
        a.st_off[k] = sd.plane_off[k]; a.st_pitch[k] = sd.pitch[k];
    }
    if (plan.e.rgb) {
        p265r_export_desc dc = *desc;                       // (the coefficients do not depend on upsample)
        dc.upsample = P265R_UP_NEAREST;
        if (const int rc = export_coefficients(dc, B, a.r.e.coef)) return rc;
    }
    a.r.e.shift = desc->sample == P265R_SMP_MSB16 ? 16 - B : 0;
    a.r.ow = plan.ow; a.r.oh = plan.oh;
    a.r.grey = (1 << (B - 1)) << a.r.e.shift;
    resize_norm(*rs, B, a.r.scale, a.r.bias);
    a.tw = tw; a.th = th;
    a.rcp_w[0] = grid_rs_rcp((uint32_t)tw); a.rcp_w[1] = grid_rs_rcp((uint32_t)tw >> 1);
    a.rcp_h[0] = grid_rs_rcp((uint32_t)th); a.rcp_h[1] = grid_rs_rcp((uint32_t)th >> 1);
    {
        // one device block: the tiles' plane addresses, then the frames' entries; it lives until the lane is next
        // synchronised, like a pic_index list
        const size_t tab_words = (size_t)n * 3;
        std::vector<uint64_t> blk(tab_words + (size_t)n_frames * (sizeof(GridRsFrame) / sizeof(uint64_t)));
        static_assert(sizeof(GridRsFrame) == 48, "six 64-bit words per table entry");
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k)
                blk[(size_t)i * 3 + k] = (uint64_t)(uintptr_t)b->h_pics[(size_t)(pic_index ? pic_index[i] : i)].out[k];
        for (int f = 0; f < n_frames; ++f) {
            GridRsFrame& o = plan.frames[(size_t)f];
            o.dst = plan.stage[(size_t)f] >= 0
                        ? (uint64_t)(uintptr_t)b->grid_stage + (uint64_t)plan.stage[(size_t)f] * sd.frame_bytes
                        : (uint64_t)(uintptr_t)dev_dst + (uint64_t)f * desc->frame_bytes;
        }
        std::memcpy(blk.data() + tab_words, plan.frames.data(), sizeof(GridRsFrame) * (size_t)n_frames);
        void* d_blk = nullptr;
        HIP_TRY(hipMalloc(&d_blk, sizeof(uint64_t) * blk.size()));
        b->exp_idx.push_back(d_blk);
        HIP_TRY(hipMemcpy(d_blk, blk.data(), sizeof(uint64_t) * blk.size(), hipMemcpyHostToDevice));
        a.tab = static_cast<const uint64_t*>(d_blk);
        a.frames = reinterpret_cast<const GridRsFrame*>(a.tab + tab_words);
    }
    int rc = ctx->geo.pel16
                 ? launch_grid_resize<uint16_t>(*desc, rs->filter, ctx->geo, a, plan.max_pw, plan.max_ph, n_frames, b->stream)
                 : launch_grid_resize<uint8_t>(*desc, rs->filter, ctx->geo, a, plan.max_pw, plan.max_ph, n_frames, b->stream);
    if (rc) return rc;
    ctx->lane_busy |= 1u << b->lane;
    if (plan.n_stage) {
        GridTransposeArgs t{};
        t.dst = static_cast<uint8_t*>(dev_dst);
        t.dst_frame = desc->frame_bytes;
        ExportPlane pl[3];
        grid_planes(*desc, plan.e, plan.oh, plan.ow, pl);   // the staged planes: R of a quarter turn
        for (int k = 0; k < plan.e.n_planes; ++k) {
            t.src_off[k] = sd.plane_off[k]; t.dst_off[k] = desc->plane_off[k];
            t.src_pitch[k] = sd.pitch[k]; t.dst_pitch[k] = desc->pitch[k];
            const int c = desc->format == P265R_FMT_RGB_PACKED ? 3 : (desc->format == P265R_FMT_SEMIPLANAR && k == 1 ? 2 : 1);
            t.w[k] = (int)(pl[k].row_bytes / (uint64_t)(plan.e.es * c));
            t.h[k] = pl[k].rows;
        }
        t.tiles_y = (t.h[0] + kGridTile - 1) / kGridTile;
        rc = launch_grid_resize_transpose(*desc, plan.e.es, t, a.frames, plan.e.n_planes, n_frames, b->stream);
        if (rc) return rc;
    }
    return P265R_OK;
}

int p265r_batch_free(p265r_ctx* ctx, p265r_batch* b) {
    if (!ctx || !b) return P265R_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->pending == b) ctx->pending = nullptr;
    // its lane may still run it: the allocation is reused by the next upload (another stream); the
    // lane stream's last run waited for every residual / prep kernel of the batch
    hipError_t e = b->stream ? hipStreamSynchronize(b->stream) : hipSuccess;
    if (b->intra_done) (void)hipEventDestroy(b->intra_done);
    if (b->d_dig) (void)hipFree(b->d_dig);
    if (b->d_hash) (void)hipFree(b->d_hash);
    if (b->d_narrow) (void)hipFree(b->d_narrow);
    if (b->grid_stage) (void)hipFree(b->grid_stage);
    for (void* p : b->exp_idx) (void)hipFree(p);
    if (b->mem) {
        // keep the larger of (cache, this allocation) for the next upload (its runs are complete)
        if (!ctx->cache_mem || b->bytes > ctx->cache_bytes) {
            if (ctx->cache_mem) e = hipFree(ctx->cache_mem);
            ctx->cache_mem = b->mem;
            ctx->cache_bytes = b->bytes;
        } else {
            e = hipFree(b->mem);
        }
    }
    delete b;
    return e == hipSuccess ? P265R_OK : hip_fail(e, "hipFree");
}

int p265r_submit(p265r_ctx* ctx, const p265r_picture* pics, int n_pics) {
    if (!ctx) return P265R_EINVAL;
    if (ctx->pending) return P265R_ESTATE;
    p265r_batch* b = nullptr;
    int rc = p265r_batch_upload(ctx, pics, n_pics, &b);
    if (rc) return rc;
    rc = p265r_batch_run(ctx, b);
    if (rc) { p265r_batch_free(ctx, b); return rc; }
    ctx->pending = b;
    ctx->pending_pics.assign(pics, pics + n_pics);
    return P265R_OK;
}

int p265r_wait(p265r_ctx* ctx) {
    if (!ctx) return P265R_EINVAL;
    if (!ctx->pending) return P265R_ESTATE;
    p265r_batch* b = ctx->pending;
    int rc = p265r_batch_download(ctx, b, ctx->pending_pics.data(), (int)ctx->pending_pics.size());
    ctx->pending = nullptr;
    ctx->pending_pics.clear();
    int rc2 = p265r_batch_free(ctx, b);
    return rc ? rc : rc2;
}

int p265r_sync(p265r_ctx* ctx) {
    if (!ctx) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    for (hipStream_t st : ctx->lanes) HIP_TRY(hipStreamSynchronize(st));
    for (hipStream_t st : ctx->aux) if (st) HIP_TRY(hipStreamSynchronize(st));
    for (hipStream_t st : ctx->aux2) if (st) HIP_TRY(hipStreamSynchronize(st));
    ctx->lane_busy = 0;
    return P265R_OK;
}

int p265r_set_pipeline(p265r_ctx* ctx, int depth) {
    if (!ctx || depth < 1 || depth > 16) return P265R_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    while ((int)ctx->lanes.size() < depth) {
        hipStream_t st = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        ctx->lanes.push_back(st);
    }
    ctx->pipeline = depth;
    ctx->next_lane = 0;
    return P265R_OK;
}

// GPU_MAX_HW_QUEUES as the HIP runtime read it at initialisation (HIP's default 4 when unset)
static const char* hwq_env() {
    const char* v = std::getenv("GPU_MAX_HW_QUEUES");
    return (v && std::strlen(v) < 8 && std::strspn(v, "0123456789") == std::strlen(v)) ? v : "default";
}

int p265r_describe(p265r_ctx* ctx, char* buf, int size) {
    if (!ctx || size < 0 || (size > 0 && !buf)) return P265R_EINVAL;
    const Geo& g = ctx->geo;
    char tmp[2048];
    const int n = snprintf(tmp, sizeof(tmp),
        "{\"schedule\": \"%s\", \"row_waves\": %d, \"row_waves_by_run\": \"%s\", \"lean\": %d, "
        "\"fair\": %d, \"quad\": %d, \"luma_lead\": %d, \"sao_rows\": %d, \"skip\": %d, \"debug_sync\": %d, "
        "\"pipeline\": %d, \"fork_prep\": %d, \"pipe_waves\": %d, \"hw_queues\": \"%s\", \"num_cus\": %d, \"diag_build\": %d, "
        "\"experiments_build\": %d, \"split\": %d, \"last_launch_split\": %d, \"xg\": %d, \"last_launch_xg\": %d, "
        "\"phase_order\": %d, \"early_residual\": %d, \"bit_depth\": %d, \"bit_depth_chroma\": %d, \"row_launches\": {\"w12\": %lld, \"w8\": %lld, \"w16_split\": %lld, \"xg\": %lld, \"other\": %lld}, "
        "\"sparse_expand\": \"%s\", \"sparse_expand_stream\": %d, \"last_sparse_expand_ms\": %.4f, "
        "\"chroma_format_idc\": %d, \"last_launch_layout\": \"%s\", \"last_launch_row_waves\": %d, "
        "\"env_overrides\": [%s]}",
        ctx->schedule ? "rows" : "steps", ctx->row_waves,
        ctx->row_waves ? "fixed" : (P265R_PHASE_ORDER
                                   ? "batches of >= 1 picture per CU in a pipelined context: W=12, one intra launch at a time "
                                     "(phase order); small batches (< 1 picture per CU: component split, W=16): side by side; "
                                     "otherwise W=12 while no other lane has a run enqueued since the API synchronised it, "
                                     "else pipe_waves"
                                   : "batches of <= CUs / (2 xg) pictures: every luma / chroma chain on xg workgroups of W=4 "
                                     "(cross-group rows, progress and lines in global memory); small batches (< 1 picture per "
                                     "CU: component split, W=16); otherwise W=12 while no other "
                                     "lane has a run enqueued since the API synchronised it, else pipe_waves (W=8, 80 VGPRs: "
                                     "the other lanes' residual / prep / SAO waves fit beside it)"),
        // (the keys of retired knobs stay, with the value that was kept: lean 1, skip 0, pipe_waves 8,
        // experiments_build 0, row_launches.other 0, sparse_expand "lds tile", sparse_expand_stream 0)
        1, g.fair, g.quad, ctx->luma_lead, ctx->sao_rows, 0, ctx->debug_sync ? 1 : 0,
        ctx->pipeline, ctx->fork_prep, 8, hwq_env(), ctx->num_cus,
#ifdef P265R_DEBUG_DIAG
        1,
#else
        0,
#endif
        0, ctx->split, ctx->last_split ? 1 : 0, ctx->xg, ctx->last_xg ? 1 : 0, P265R_PHASE_ORDER, P265R_EARLY_RESIDUAL,
        (int)ctx->params.bit_depth_luma, (int)ctx->params.bit_depth_chroma, ctx->row_launches[0], ctx->row_launches[1], ctx->row_launches[2], ctx->row_launches[3], 0ll,
        "lds tile", 0, ctx->last_expand_ms,
        (int)ctx->params.chroma_format_idc, ctx->last_layout, ctx->last_row_waves,
        ctx->describe.c_str());
    if (n < 0) return P265R_EINVAL;
    if (size > 0) {
        const int k = std::min(n, size - 1);
        std::memcpy(buf, tmp, (size_t)k);
        buf[k] = 0;
    }
    return n;
}

int p265r_set_scaling_factors(p265r_ctx* ctx, const uint8_t* factors, int n_bytes) {
    if (!ctx || !factors || n_bytes != P265R_SCALING_FACTOR_BYTES) return P265R_EINVAL;
    if (!ctx->params.scaling_list_enabled) return P265R_ESTATE;
    for (int i = 0; i < n_bytes; ++i)
        if (factors[i] == 0) return P265R_EINVAL;              // ScalingFactor is 1..255 (7.4.5)
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = p265r_sync(ctx)) return rc;                    // no run in flight reads the old table
    if (!ctx->d_sf) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->d_sf), P265R_SCALING_FACTOR_BYTES));
    HIP_TRY(hipMemcpy(ctx->d_sf, factors, P265R_SCALING_FACTOR_BYTES, hipMemcpyHostToDevice));
    return P265R_OK;
}

int p265r_set_row_waves(p265r_ctx* ctx, int waves) {
    if (!ctx || (waves != 0 && waves != 8 && waves != 12)) return P265R_EINVAL;
    ctx->row_waves = waves;
    return P265R_OK;
}

int p265r_set_timing(p265r_ctx* ctx, int enable) {
    if (!ctx) return P265R_EINVAL;
    ctx->timing = enable != 0;
    if (enable) {                               // start a new accumulation
        for (auto& r : ctx->runs) for (auto& e : r.ev) ctx->spare.push_back(e);
        ctx->runs.clear();
        ctx->have_timing = false;
    }
    return P265R_OK;
}

namespace {
int run_times(const p265r_ctx::Run& r, p265r_timings* t) {
    HIP_TRY(hipEventSynchronize(r.ev[3]));
    float a = 0, b = 0, c = 0, tt = 0;
    HIP_TRY(hipEventElapsedTime(&a, r.ev[0], r.ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, r.ev[1], r.ev[2]));
    HIP_TRY(hipEventElapsedTime(&c, r.ev[2], r.ev[3]));
    HIP_TRY(hipEventElapsedTime(&tt, r.ev[0], r.ev[3]));
    *t = r.counts;
    t->residual_ms = a; t->intra_ms = b; t->sao_ms = c; t->total_ms = tt;
    return P265R_OK;
}
}  // namespace

int p265r_last_timings(p265r_ctx* ctx, p265r_timings* out) {
    if (!ctx || !out) return P265R_EINVAL;
    if (!ctx->have_timing || ctx->runs.empty()) return P265R_ESTATE;
    HIP_TRY(hipSetDevice(ctx->device));
    return run_times(ctx->runs.back(), out);
}

int p265r_timings_total(p265r_ctx* ctx, p265r_timings* out, int* n_runs) {
    if (!ctx || !out) return P265R_EINVAL;
    if (!ctx->have_timing || ctx->runs.empty()) return P265R_ESTATE;
    HIP_TRY(hipSetDevice(ctx->device));
    p265r_timings sum{};
    for (const auto& r : ctx->runs) {
        p265r_timings t{};
        int rc = run_times(r, &t);
        if (rc) return rc;
        sum.total_ms += t.total_ms; sum.residual_ms += t.residual_ms; sum.intra_ms += t.intra_ms; sum.sao_ms += t.sao_ms;
        sum.intra_launches += t.intra_launches; sum.residual_launches += t.residual_launches;
        sum.sao_launches += t.sao_launches;
    }
    if (n_runs) *n_runs = (int)ctx->runs.size();
    *out = sum;
    return P265R_OK;
}

}  // extern "C"
