// narrow.h -- the download of a wide context's 8-bit component (p265r_params.split_bit_depth: BitDepthY !=
// BitDepthC with one of them 8).  Every device plane of such a context holds uint16_t samples; the host sees
// the 8-bit component as uint8_t planes, so its planes are narrowed on the device before the D2H copy and cross
// PCIe at one byte per sample.
//
// One launch per p265r_batch_download, on the batch's stream behind its runs: item k = one requested plane (source:
// the picture's own width and height against the context stride; destination: tight uint8_t rows in the batch's
// staging area).  A wave takes one 1024-sample segment of one row, a lane 16 samples: two 16-byte loads, one 16-byte
// store.  Plane widths are multiples of 4 (4:2:0 planes of pictures whose sizes are multiples of 8), so a lane whose
// 16 samples cross the row's end stores the 4-sample groups inside it.  A sample of an 8-bit component is at most
// 255 (every kernel clips to its component's depth), so the low bytes are the samples.
//
// The reference has no counterpart (it keeps Python integers per sample).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p265r {

struct NarrowItem {             // 32 bytes
    const uint16_t* src;        // plane origin; rows `stride` samples apart (a multiple of 64: 16-byte aligned loads)
    uint8_t* dst;               // w * h bytes, rows tight (4-byte aligned: w is a multiple of 4)
    int w, h, stride;
    int pad_;
};
static_assert(sizeof(NarrowItem) == 32, "NarrowItem is 32 bytes");

constexpr int kNarrowLane = 16;                    // samples per lane
constexpr int kNarrowSeg = 64 * kNarrowLane;       // samples per wave
constexpr int kNarrowWaves = 4;                    // waves (rows) per block

// low bytes of four uint16_t samples (two dwords) as one dword
__device__ __forceinline__ uint32_t narrow4(uint32_t lo, uint32_t hi) {
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u);
}

// grid (n_items * segs, ceil(max h / kNarrowWaves)), 64 * kNarrowWaves threads; segs = ceil(max w / kNarrowSeg)
__global__ __launch_bounds__(64 * kNarrowWaves) void narrow_kernel(const NarrowItem* __restrict__ items, int segs) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
    typedef u4v u4v_a4 __attribute__((aligned(4)));         // a tight row starts at any multiple of 4 bytes
    const int item = (int)(blockIdx.x / (unsigned)segs), seg = (int)(blockIdx.x - (unsigned)item * (unsigned)segs);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const NarrowItem it = items[item];
    const int y = (int)blockIdx.y * kNarrowWaves + wave;
    const int x = seg * kNarrowSeg + lane * kNarrowLane;
    if (y >= it.h || x >= it.w) return;                      // (no barrier below)
    const uint16_t* s = it.src + (size_t)y * it.stride + x;
    uint8_t* d = it.dst + (size_t)y * it.w + x;
    if (x + kNarrowLane <= it.w) {
        const u4v a = *reinterpret_cast<const u4v*>(s), b = *reinterpret_cast<const u4v*>(s + 8);
        *reinterpret_cast<u4v_a4*>(d) = u4v{narrow4(a.x, a.y), narrow4(a.z, a.w), narrow4(b.x, b.y), narrow4(b.z, b.w)};
    } else {
        for (int k = 0; x + 4 * k < it.w; ++k) {             // at most three groups
            const u2v a = *reinterpret_cast<const u2v*>(s + 4 * k);
            *reinterpret_cast<uint32_t*>(d + 4 * k) = narrow4(a.x, a.y);
        }
    }
}

}  // namespace p265r
