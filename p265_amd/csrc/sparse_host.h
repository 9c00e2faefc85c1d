// sparse_host.h -- host-only helpers of the sparse coefficient upload (sparse_host.cpp; plain C++, no HIP).
#pragma once

#include <cstdint>

#include "../../include/p265r.h"

namespace p265r {

// a TB whose coefficients travel as entries (p265r_batch_upload_sparse): coded, neither PCM nor bypass
inline bool tb_is_sparse(const p265r_tb& t) {
    return (t.flags & P265R_TB_CBF) && !(t.flags & (P265R_TB_PCM | P265R_TB_BYPASS));
}
// a TB whose N*N samples / levels stay dense (the pool's raw slab): coded PCM or bypass
inline bool tb_is_raw(const p265r_tb& t) {
    return (t.flags & (P265R_TB_CBF | P265R_TB_PCM)) && (t.flags & (P265R_TB_PCM | P265R_TB_BYPASS));
}
inline uint32_t tb_sparse_count(const p265r_tb& t) { return (uint32_t)t.reserved[0] | (uint32_t)t.reserved[1] << 8; }

// One TB record of a sparse picture against its entry array (nz, n_nz) and the picture's dense (PCM /
// bypass) samples (n_coef of them): P265R_OK, P265R_EINVAL or P265R_ERANGE (include/p265r.h).  After it
// every entry's pos is inside the TB, which is what keeps the expand kernel's stores inside the
// coefficient pool.  (The entry loop carries no dependency but two OR-reductions: a range error wins.)
inline int sparse_validate_tb(const p265r_tb& tb, const uint32_t* nz, uint64_t n_nz, uint64_t n_coef) {
    if (tb.log2_size < 2 || tb.log2_size > 5) return P265R_EINVAL;
    const uint32_t nn = 1u << (2 * tb.log2_size);
    const uint32_t count = tb_sparse_count(tb);
    if (tb.reserved[2]) return P265R_EINVAL;
    if (!tb_is_sparse(tb)) {
        if (count) return P265R_EINVAL;                          // entries on a TB that has none
        if (tb_is_raw(tb) && (uint64_t)tb.coef_off + nn > n_coef) return P265R_ERANGE;
        return P265R_OK;
    }
    if (count > nn) return P265R_EINVAL;
    if ((uint64_t)tb.coef_off + count > n_nz) return P265R_ERANGE;
    if (!count) return P265R_OK;
    const uint32_t* e = nz + tb.coef_off;
    uint32_t bad_range = (e[0] & 0xffffu) >= nn, bad_order = 0;
    for (uint32_t k = 1; k < count; ++k) {
        const uint32_t pos = e[k] & 0xffffu;
        bad_range |= pos >= nn;
        bad_order |= pos <= (e[k - 1] & 0xffffu);                // strictly increasing
    }
    return bad_range ? P265R_ERANGE : (bad_order ? P265R_EINVAL : P265R_OK);
}

// Every TB record of a sparse picture (sparse_validate_tb), and the array pointers themselves.
// n_entries (optional) gets the entries of the picture's sparse TBs, summed.
int sparse_validate(const p265r_picture& pic, const p265r_sparse_coef* sp, uint64_t* n_entries);

}  // namespace p265r
