// sparse_host.cpp -- host side of the sparse coefficient upload: p265r_sparsify (dense picture ->
// entries) and the validation of sparse records (p265r_batch_upload_sparse runs it before anything
// reaches the device).  Plain C++ without HIP, so that it also builds stand-alone under the host
// sanitizers (make sparse-check, tools/sparse_check.cpp).
#include "sparse_host.h"

#include <cstring>

namespace p265r {

int sparse_validate(const p265r_picture& pic, const p265r_sparse_coef* sp, uint64_t* n_entries) {
    if (!sp || (!sp->nz && sp->n_nz)) return P265R_EINVAL;
    if ((!pic.tbs && pic.n_tbs) || (!pic.coef && pic.n_coef)) return P265R_EINVAL;
    uint64_t total = 0;
    for (uint32_t t = 0; t < pic.n_tbs; ++t) {
        const p265r_tb& tb = pic.tbs[t];
        if (const int rc = sparse_validate_tb(tb, sp->nz, sp->n_nz, pic.n_coef)) return rc;
        if (tb_is_sparse(tb)) total += tb_sparse_count(tb);
    }
    if (n_entries) *n_entries = total;
    return P265R_OK;
}

}  // namespace p265r

extern "C" int p265r_sparsify(const p265r_picture* pic, p265r_tb* tbs_out, uint32_t* nz_out, uint64_t nz_cap,
                              uint64_t* n_nz, int16_t* raw_out, uint64_t raw_cap, uint64_t* n_raw) {
    using namespace p265r;
    if (!pic || (!pic->tbs && pic->n_tbs) || (!pic->coef && pic->n_coef)) return P265R_EINVAL;
    const bool count_only = !tbs_out && !nz_out && !raw_out;
    if (!count_only && !tbs_out) return P265R_EINVAL;
    uint64_t nz = 0, raw = 0;
    for (uint32_t t = 0; t < pic->n_tbs; ++t) {
        p265r_tb tb = pic->tbs[t];
        std::memset(tb.reserved, 0, sizeof(tb.reserved));
        if (tb.flags & (P265R_TB_CBF | P265R_TB_PCM)) {
            if (tb.log2_size < 2 || tb.log2_size > 5) return P265R_EINVAL;
            const uint32_t nn = 1u << (2 * tb.log2_size);
            if ((uint64_t)tb.coef_off + nn > pic->n_coef) return P265R_ERANGE;
            const int16_t* src = pic->coef + tb.coef_off;
            if (tb_is_sparse(tb)) {
                uint32_t count = 0;
                for (uint32_t pos = 0; pos < nn; ++pos) {
                    if (!src[pos]) continue;
                    if (!count_only) {
                        if (!nz_out || nz + count >= nz_cap) return P265R_ERANGE;
                        nz_out[nz + count] = pos | (uint32_t)(uint16_t)src[pos] << 16;
                    }
                    ++count;
                }
                if (nz > UINT32_MAX) return P265R_ERANGE;          // coef_off is 32 bits
                tb.coef_off = (uint32_t)nz;
                tb.reserved[0] = (uint8_t)(count & 0xff);
                tb.reserved[1] = (uint8_t)(count >> 8);
                nz += count;
            } else {
                if (!count_only) {
                    if (!raw_out || raw + nn > raw_cap) return P265R_ERANGE;
                    std::memcpy(raw_out + raw, src, sizeof(int16_t) * nn);
                }
                if (raw > UINT32_MAX) return P265R_ERANGE;
                tb.coef_off = (uint32_t)raw;
                raw += nn;
            }
        }
        if (!count_only) tbs_out[t] = tb;
    }
    if (n_nz) *n_nz = nz;
    if (n_raw) *n_raw = raw;
    return P265R_OK;
}
