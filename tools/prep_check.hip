// Host-side exhaustive check of the job preparation's short cuts (intra_prep.h):
//   prep_avail_clear()  == ref_avail_mask32() and the generic run bounds, for every TB place of a clear CTU
//                          (flags 15; the picture's right / bottom edge exactly at, and beyond, the stated limits);
//   prep_filter_min_lg() == the rule of 8.4.4.2.3, for every size and mode.
// Build + run (CPU only): hipcc --offload-arch=gfx950 -O2 tools/prep_check.hip -o /tmp/prep_check && /tmp/prep_check
#include <cstdio>
#include <cstdlib>
#include "../p265_amd/csrc/intra_prep.h"
using namespace p265r;

int main() {
    long long checked = 0, bad = 0;
    for (int ctb_log2 = 4; ctb_log2 <= 6; ++ctb_log2) {
        const int ctb = 1 << ctb_log2;
        for (int c = 0; c < 3; ++c)
            for (int lg = 2; lg <= 5; ++lg) {
                const int n = 1 << lg, sub = c ? 1 : 0;
                if ((n << sub) > ctb || (c && lg == 5)) continue;
                for (int yr = 0; (yr << sub) < ctb; yr += 4)          // (every 4-sample place: a 4x4 chroma TB of an
                    for (int xr = 0; (xr << sub) < ctb; xr += 4) {    // 8x8 CU split into four sits at multiples of 4)
                        if (((xr | yr) & (n - 1)) && !(c && lg == 2)) continue;
                        if (((xr + n) << sub) > ctb || ((yr + n) << sub) > ctb) continue;
                        for (int ex = 0; ex < 3; ++ex)
                            for (int ey = 0; ey < 3; ++ey) {
                                const int x0 = 2 * ctb, y0 = 3 * ctb;
                                const int w = x0 + 2 * ctb + 8 * ex, h = y0 + ctb + 8 * ey;
                                const int xc = xr << sub, yc = yr << sub;
                                const int s = __builtin_ctz((unsigned)(n << sub)) - 2;
                                const uint32_t zw = avail_ztab_word(s, yc >> 2);
                                // the generic record computation of intra_prep_kernel, restated
                                uint32_t mhi = 0;
                                const uint32_t mlo = ref_avail_mask32(c, xr, yr, n, x0, y0, w, h, ctb, 15u, zw, mhi);
                                const int L = (2 * n) >> (c ? 1 : 2), US = c ? 1 : 2;
                                const uint32_t full_lo = L == 16 ? 0xffffffffu : (1u << (2 * L + 1)) - 1u;
                                const bool m_full = (mlo == full_lo) & (mhi == (L == 16 ? 1u : 0u)), m_none = (mlo | mhi) == 0u;
                                const int ulo = mlo ? __builtin_ctz(mlo) : 32;
                                const int uhi = mhi ? 32 : 31 - __builtin_clz(mlo | 1u);
                                const uint32_t lo_cut = ulo >= 32 ? 0u : (0xffffffffu << ulo);
                                const bool contig = mlo == (mhi ? lo_cut : (lo_cut & (uhi >= 31 ? 0xffffffffu : ((2u << uhi) - 1u))));
                                const int fa = ulo < L ? (ulo << US) : (ulo == L ? 2 * n : 2 * n + 1 + ((ulo - L - 1) << US));
                                const int la = uhi < L ? ((uhi + 1) << US) - 1 : (uhi == L ? 2 * n : 2 * n + ((uhi - L) << US));
                                const PrepAvail a = prep_avail_clear(c, xr, yr, n, ctb, zw);
                                ++checked;
                                if (a.mlo != mlo || a.mhi != mhi || a.full != m_full || m_none || !contig || a.fa != fa || a.la != la) {
                                    if (bad++ < 10)
                                        printf("MISMATCH ctb %d c %d n %d xr %d yr %d w %d h %d: mask %x|%x vs %x|%x full %d vs %d "
                                               "none %d run %d fa %d vs %d la %d vs %d\n", ctb, c, n, xr, yr, w, h, a.mhi, a.mlo, mhi,
                                               mlo, (int)a.full, (int)m_full, (int)m_none, (int)contig, a.fa, fa, a.la, la);
                                }
                            }
                    }
            }
    }
    for (int lg = 2; lg <= 5; ++lg)
        for (int mode = 0; mode < 35; ++mode) {
            const int n = 1 << lg;
            const int da = abs(mode - 26), db = abs(mode - 10), dist = da < db ? da : db;
            const bool fon = (n != 4) & (mode != 1) & (dist > (n == 8 ? 7 : (n == 16 ? 1 : 0)));
            ++checked;
            if ((lg >= prep_filter_min_lg(mode)) != fon && bad++ < 20) printf("MISMATCH filter lg %d mode %d\n", lg, mode);
        }
    printf("checked %lld, mismatches %lld\n", checked, bad);
    return bad ? 1 : 0;
}
