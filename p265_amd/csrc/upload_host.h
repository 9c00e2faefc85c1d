// upload_host.h -- the host-only part of the batch upload (upload_host.cpp; plain C++, no HIP): record
// validation, the layout of the device image and of the staging buffer, the chunking, and the packing of
// each picture.  p265r.hip allocates what the plan asks for and enqueues the copies it lists; every offset
// the kernels depend on is decided here, and checked on the CPU by tools/upload_check.cpp (make upload-check).
#pragma once

#include <algorithm>
#include <array>
#include <atomic>
#include <cstddef>
#include <thread>
#include <vector>

#include "batch_types.h"

namespace p265r {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Run fn(i) for i in [0, n) on up to 16 host threads (picture-level packing work).
template <class F>
void parallel_for(int n, F fn) {
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int nt = std::min(std::min(hw, 16), n);
    if (nt <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&]() {
            for (int i; (i = next.fetch_add(1)) < n;) fn(i);
        });
    for (auto& t : th) t.join();
}

// a picture's luma size: its own (p265r_picture.pic_width / pic_height) or the context's
std::array<int, 2> pic_size(const p265r_params& p, const p265r_picture& pic);

// (sparse: the picture of a sparse upload -- its transformed TBs' coef_off index entries, checked by
// sparse_validate_tb in the upload's counting pass)
int validate_picture(const p265r_params& p, const Geo& g, const p265r_picture& pic, bool sparse = false);

// One host-to-device copy of an upload: bytes from the staging buffer at host_off to dst_off of the batch
// image, or (to_landing) of the context's landing buffer of the sparse entries and begin words.
struct H2dCopy {
    bool to_landing;
    size_t dst_off, host_off, bytes;
};
struct CopyList {          // a chunk's copies, in enqueue order (empty ranges are left out)
    int n = 0;
    H2dCopy v[2 + N_POOLS + RC_NUM + 1 + 2];
    void add(bool to_landing, size_t dst_off, size_t host_off, size_t bytes) {
        if (bytes) v[n++] = H2dCopy{to_landing, dst_off, host_off, bytes};
    }
    const H2dCopy* begin() const { return v; }
    const H2dCopy* end() const { return v + n; }
};
struct ZeroRange { size_t off, bytes; };

// Everything an upload decides before it touches the device.  o_*: byte offsets in the device image (256-B
// aligned, in this order); s_*: byte offsets in the staging buffer, which holds
//   [0, o_res) as on the device | jobs [o_jobs[0], o_ijobs) at s_jobs | no-filter maps, compact, at s_nf
// (sparse: of the pool only the raw slab is staged, at o_pool; behind the no-filter maps follow, per chunk,
// the entries [class][job order] at s_ent and the begin words [class][job + 1 closing word] at s_beg).
struct UploadPlan {
    int n_pics = 0;
    int nc = 0;                        // per-picture CTU slots (the context size)
    bool sparse = false, recon_input = false, ragged = false, sao = false, dbk = false, lf = false, xg_ok = false;
    bool mono = false;            // Geo::mono: a picture's planes are its luma plane alone
    // per picture: luma size, CTUs, no-filter map bytes (a ragged batch mixes sizes)
    std::vector<std::array<int, 2>> psize;
    std::vector<int> pnc;
    std::vector<size_t> pnf;
    size_t pool_sz[N_POOLS] = {}, pool_base[N_POOLS] = {}, pool_total = 0;    // int16 elements
    int n_jobs[RC_NUM] = {};
    size_t n_tbs_total = 0, n_nf = 0, nz_total = 0;
    size_t plane_off[3] = {}, pic_plane_bytes = 0, nf_bytes = 0, map_bytes = 0, pel_bytes = 1;
    size_t o_pics = 0, o_err = 0, o_xgl = 0, o_ctus = 0, o_tbs = 0, o_pool = 0, o_res = 0, o_jobs[RC_NUM] = {}, o_ijobs = 0,
           o_jcount = 0, o_nf = 0, o_map = 0, o_rec = 0, o_out = 0, total = 0;
    size_t s_jobs = 0, s_nf = 0, s_ent = 0, s_beg = 0, stage_need = 0, sp_need = 0;
    // (16 chunks of 32 pictures at 512: the first H2D starts after 1/16 of the packing; 4 chunks measured
    // 78 ms per 512 1080p pictures, H2D-bound from the first chunk on)
    int n_chunks = 1;
    int chunk_lo(int k) const { return (int)((long long)n_pics * k / n_chunks); }
    // per-picture start offsets in every pool / job list / TB array / no-filter slot; row n_pics: the ends
    std::vector<std::array<size_t, N_POOLS>> pool_at;
    std::vector<std::array<int, RC_NUM>> job_at;
    std::vector<size_t> tb_at, nf_at;
    // sparse: where each picture's entries and begin words of every class go (chunk-major, then class, then
    // picture), and where each chunk's class ranges start (ent_kc / beg_kc [k * RC_NUM + c]; [n_chunks * RC_NUM]
    // closes the last)
    std::vector<std::array<size_t, RC_NUM>> ent_at, beg_at;
    std::vector<size_t> ent_kc, beg_kc;
    // recon-input planes of an 8-bit component in a wide context (unequal bit depths: every device plane is
    // uint16_t): widened into the staging buffer behind everything else (s_wide; wide_at[i][c]: plane c of
    // picture i, tight rows of its own width, SIZE_MAX: the plane is copied from the caller's memory as it is)
    size_t s_wide = 0;
    std::vector<std::array<size_t, 3>> wide_at;

    // Chunk k's copies, to enqueue once its pictures are packed: its ranges of the CTU and TB records, of each
    // class slab of the coefficient pool, of each residual job list and of the no-filter maps; sparse: its
    // entries and begin words.  The staging ranges of different chunks are disjoint, so the copies of chunk k
    // run while the host packs chunk k + 1.
    CopyList chunk_copies(int k) const;
    // last: the DevPic table and the error word (+ row-kernel slots), [0, o_ctus) of both sides (pack_header)
    H2dCopy header_copy() const { return H2dCopy{false, 0, 0, o_ctus}; }
    // the alignment gaps after the CTU records and the TB records and the coefficient pool's pad: zeroed on
    // the device, as the device image always had them (bytes 0: no gap)
    std::array<ZeroRange, 3> gap_zeros() const;
};

// Validates every record (on up to 16 host threads; the first failing picture's code is returned), counts the
// coded TBs per class and lays the upload out.  sp null: dense coefficients; else sp[i] holds the entries of
// pics[i]'s transformed TBs.  n_ctus: CTUs of a picture of the context size; xg, split, num_cus: whether the
// batch gets the cross-group row kernel's ranges (xg_ok).  P265R_OK, P265R_EINVAL or P265R_ERANGE.
int plan_upload(const p265r_params& p, const Geo& g, int n_ctus, int xg, bool split, int num_cus, const p265r_picture* pics,
                const p265r_sparse_coef* sp, int n_pics, UploadPlan* plan);

// Picture i's share of the staging buffer (stage_need bytes at `stage`) and its DevPic, whose pointers are
// offsets from dbase, the device image's address.  Pictures are independent: callable from parallel_for.
void pack_picture(const UploadPlan& plan, int i, const p265r_picture* pics, const p265r_sparse_coef* sp, unsigned char* stage,
                  unsigned char* dbase, DevPic* out);
// sparse, after chunk k's pictures are packed: each class range's closing begin word (the index past its
// last entry)
void close_chunk(const UploadPlan& plan, int k, unsigned char* stage);
// recon-input plane c of picture i, uint8_t samples at the caller's, as uint16_t into its staging range
// (UploadPlan::wide_at, which is not SIZE_MAX)
void widen_plane(const UploadPlan& plan, int i, int c, const p265r_picture* pics, unsigned char* stage);
// [0, o_ctus) of the staging buffer: the DevPic table, then zeros (alignment, error word, row-kernel slots)
void pack_header(const UploadPlan& plan, const DevPic* dev_pics, unsigned char* stage);

}  // namespace p265r
