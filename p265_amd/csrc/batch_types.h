// batch_types.h -- the records of a batch's device image that the host writes and the kernels read.
// No HIP: the upload planner (upload_host.cpp) and its CPU check (tools/upload_check.cpp) include it too.
#pragma once
#include <stdint.h>
#include "../../include/p265r.h"

namespace p265r {

// Intra job record written by intra_prep_kernel (layout: intra_prep.h).
struct IntraJob {                // 24 bytes (intra_prep.h documents the words)
    uint32_t w[6];
};
static_assert(sizeof(IntraJob) == 24, "IntraJob is 24 bytes");

struct DevPic {                 // per picture, device-resident table
    const p265r_ctu* ctus;
    const p265r_tb*  tbs;       // coef_off rewritten to pool offsets
    uint8_t* rec[3];            // pre-SAO planes (padded stride)
    uint8_t* out[3];            // SAO output planes (== rec when SAO is off)
    const uint8_t* nofilter;    // per 8x8 luma block or nullptr
    IntraJob* jobs;             // same index space as tbs (jobs of a CTU start at tb_begin)
    uint32_t* jcount;           // per CTU four words: luma jobs | chroma jobs << 16 (chroma listed first), the
                                // index of the first job of each list that reads the top-right CTU, the index of
                                // one past the last job in the CTB's bottom-left quadrant, 0 (intra_prep.h)
    uint8_t* dbk_map;           // per 8x8 luma block (loopfilter.h), nullptr without deblocking
    int32_t  pool_rel;          // residual pool element index of coefficient pool element 0 (<= 0)
    uint32_t zero_off;          // residual pool element index of a 256-sample zero block
    uint32_t wh;                // this picture's luma size, width | height << 16 (Geo::ragged batches)
    uint32_t pad_;
};

// Batch-uniform layout of the per-picture arrays (upload_host.cpp plan_upload places them at fixed
// strides), so a kernel computes a picture's plane and CTU-record addresses without loading its
// DevPic first: one dependent memory round trip less
struct BatchView {
    uint8_t* rec0;              // picture 0's reconstruction planes (Y at plane_off[0])
    uint8_t* out0;              // picture 0's output planes (== rec0 without in-loop filters)
    uint64_t pic_bytes;         // bytes of one picture's three planes
    uint64_t plane_off[3];      // Y, Cb, Cr offsets inside a picture's planes
    const p265r_ctu* ctus0;     // picture 0's CTU records (PicSizeInCtbsY per picture)
    int* err;                   // the batch's sticky error word (bit 0: a row-kernel wait gave up; bit 1: the
                                // prep kernel's half-CTU self-check failed, Geo::tr_check)
};

struct Geo {                    // batch-uniform geometry
    int w, h;                   // luma size
    int cw, ch;                 // chroma size (4:2:0: w / 2, h / 2; monochrome: 0, 0)
    int stride[3];
    int ctb_log2, wc, hc;
    int bd[3];
    int strong;
    int lf_tiles;
    int nf_w;                   // nofilter / deblocking map width (ceil(w/8))
    int cqp[2];                 // pps_cb_qp_offset, pps_cr_qp_offset (chroma deblocking)
    int fair;                   // intra_rows_kernel: the workgroup behind its CU partner raises its priority
                                // (P265R_FAIR, default 1)
    int quad;                   // intra_prep_kernel merges 4x4 quads into one job: bit 0 luma, bit 1 chroma;
                                // bit 2 (A/B only): Cb+Cr 8x8 pairs take the general path
                                // (P265R_QUAD, default 3)
    int ragged;                 // some picture of the batch is smaller than w x h (DevPic::wh): kernels
                                // take that picture's size from pic_geo().  Per-picture arrays keep the
                                // context-size slots (CTU records, job counts, maps, planes) -- a
                                // picture's CTU raster and map rows use ITS width in CTUs / 8x8 blocks
    int tr_info;                // intra_prep_kernel: compute the top-right / bottom-left job indices (jcount words 1
                                // and 2) -- set for batches that may run a latency layout (2 pictures per CU or
                                // fewer), whose row kernels read them; the throughput builds never do
    int tr_check;               // P265R_TR_CHECK (tests): the host launches the cross-group row kernel's checking
                                // instance, which poisons the top-right part of a CTU's row-above copy until its
                                // wait and serves the left half of every CTU's bottom line from the half-CTU
                                // publish alone (checks prep's `tr` and `br` deterministically); the prep kernel
                                // checks `br` against the TBs' extents (error word bit 1)
    int pel16;                  // samples are 16-bit (BitDepth 9..12): planes of stride[] samples of 2
                                // bytes, the per-diagonal intra kernel and loopfilter16.h (else uint8_t)
    int mono;                   // chroma_format_idc 0: cw = ch = 0, no chroma plane, record, job or row exists
                                // (DevPic::rec[1..2] / out[1..2] are null); every kernel's chroma work is behind
                                // a bounds test against cw / ch or is not launched
};

struct ResJob {          // 8 bytes, one per coded TB, in pool order within its class
    uint32_t off;        // int16 offset of the TB in the pool
    uint8_t  qp;         // qP (incl. QpBdOffset)
    uint8_t  flags;      // P265R_TB_*
    uint8_t  log2;
    uint8_t  c_idx;
};
static_assert(sizeof(ResJob) == 8, "ResJob is 8 bytes");

enum ResClass { RC_DST4 = 0, RC_DCT4, RC_DCT8, RC_DCT16, RC_DCT32, RC_TSKIP, RC_NUM };
// the coefficient pool's slabs: one per job class, then the raw (PCM / bypass) samples, which have no job
enum { RC_RAW = RC_NUM, N_POOLS = RC_NUM + 1 };

inline int tb_class(const p265r_tb& t) {
    if (t.flags & (P265R_TB_BYPASS | P265R_TB_PCM)) return RC_RAW;
    if (t.flags & P265R_TB_TSKIP) return RC_TSKIP;
    switch (t.log2_size) {
        case 2: return t.c_idx == 0 ? RC_DST4 : RC_DCT4;
        case 3: return RC_DCT8;
        case 4: return RC_DCT16;
        default: return RC_DCT32;
    }
}

// the row kernel's per-CU workgroup slots (intra_rows.h RowCuSlot, 16 B each) follow the batch's error word
constexpr int kRowCuSlots = 2048;

}  // namespace p265r
