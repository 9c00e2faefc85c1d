// Sparse coefficient upload: expand the non-zero entries of a chunk of pictures into the dense class
// slabs of the coefficient pool (p265r_batch_upload_sparse, p265r.hip).  Runs once per upload; the
// pool is afterwards what the dense upload copies there, so the residual and row kernels are unchanged.
//
// Transport per class slab, in job order: the entries (pos | (uint16_t)level << 16, pos raster inside
// the TB, strictly increasing per TB, checked on the host: sparse_host.cpp) and one uint32 per job, the
// index of its first entry (begin[j], begin[n_jobs] closing the last job).
//
// Shape: a wave owns 1024 consecutive int16 of a fixed-size class slab (2 KB: one 32x32 TB, 4 16x16,
// 16 8x8 or 64 4x4 -- slab offsets are job index x N*N), zeroes a 2 KB LDS tile, scatters its TBs'
// entries into it with 16-bit LDS writes (a lane per 4x4 TB, 4 lanes per 8x8, 16 per 16x16, the wave per
// 32x32, striding the TB's entries) and streams the tile out with 16 B per lane, coalesced: the pool is
// written exactly once, with no memset of the slabs and no 2-byte global stores.  The transform-skip
// slab mixes TB sizes: a wave per TB there, placed by its job record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "residual.h"

namespace p265r {

constexpr int kExpandTile = 1024;        // int16 per wave tile
constexpr int kExpandWaves = 4;          // waves per block

// Fixed-size class (N = 1 << LOG2): job j lives at pool[base + j * N*N ...].
template <int LOG2>
__global__ __launch_bounds__(64 * kExpandWaves) void coef_expand_kernel(int16_t* __restrict__ pool, size_t base,
                                                                       const uint32_t* __restrict__ begin,
                                                                       const uint32_t* __restrict__ ent, int n_jobs) {
    constexpr int NN = 1 << (2 * LOG2);
    constexpr int T = kExpandTile / NN;          // TBs per wave
    constexpr int LPT = 64 / T;                  // lanes per TB
    __shared__ __attribute__((aligned(16))) int16_t tiles[kExpandWaves][kExpandTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int16_t* tile = tiles[wave];
    const long long j0 = ((long long)blockIdx.x * kExpandWaves + wave) * T;     // the wave's first job
    reinterpret_cast<uint4*>(tile)[lane] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4*>(tile)[lane + 64] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const long long j = j0 + lane / LPT;
    if (j < n_jobs) {
        int16_t* t = tile + (lane / LPT) * NN;
        const uint32_t e1 = begin[j + 1];
        for (uint32_t e = begin[j] + lane % LPT; e < e1; e += LPT) {
            const uint32_t v = ent[e];
            t[v & (NN - 1)] = (int16_t)(v >> 16);          // (pos < N*N by the host's check; masked all the same)
        }
    }
    __syncthreads();
    const long long left = ((long long)n_jobs - j0) * NN;  // int16 of the wave's range that belong to jobs
    uint4* dst = reinterpret_cast<uint4*>(pool + base + j0 * NN);
    for (int k = lane; k < kExpandTile / 8; k += 64)
        if ((long long)k * 8 < left) dst[k] = reinterpret_cast<const uint4*>(tile)[k];
}

// Any TB size (the transform-skip slab): a wave per job, placed and sized by its job record.
__global__ __launch_bounds__(64 * kExpandWaves) void coef_expand_jobs_kernel(int16_t* __restrict__ pool,
                                                                            const ResJob* __restrict__ jobs,
                                                                            const uint32_t* __restrict__ begin,
                                                                            const uint32_t* __restrict__ ent, int n_jobs) {
    __shared__ __attribute__((aligned(16))) int16_t tiles[kExpandWaves][kExpandTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int16_t* tile = tiles[wave];
    const long long j = (long long)blockIdx.x * kExpandWaves + wave;
    reinterpret_cast<uint4*>(tile)[lane] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4*>(tile)[lane + 64] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    ResJob job{};
    int nn = 0;
    if (j < n_jobs) {
        job = jobs[j];
        nn = 1 << (2 * min(max((int)job.log2, 2), 5));
        const uint32_t e1 = begin[j + 1];
        for (uint32_t e = begin[j] + lane; e < e1; e += 64) {
            const uint32_t v = ent[e];
            tile[v & (uint32_t)(nn - 1)] = (int16_t)(v >> 16);
        }
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(pool + job.off);
    for (int k = lane; k * 8 < nn; k += 64) dst[k] = reinterpret_cast<const uint4*>(tile)[k];
}

}  // namespace p265r
