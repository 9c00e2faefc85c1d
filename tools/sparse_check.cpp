// sparse_check.cpp -- stand-alone host check of the sparse upload's host code (make sparse-check builds
// it with p265_amd/csrc/sparse_host.cpp under -fsanitize=address,undefined and runs it on the CPU).
// Drives p265r_sparsify and the sparse record validation with good and malformed inputs: every buffer
// is a heap allocation of exactly the advertised size, so a read or write past one is reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../p265_amd/csrc/sparse_host.h"

using namespace p265r;

static int g_fail = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Dense {
    std::vector<p265r_tb> tbs;
    std::vector<int16_t> coef;
    p265r_picture pic() const {
        p265r_picture p{};
        p.tbs = tbs.empty() ? nullptr : tbs.data();
        p.n_tbs = (uint32_t)tbs.size();
        p.coef = coef.empty() ? nullptr : coef.data();
        p.n_coef = coef.size();
        return p;
    }
};

struct Sparse {
    std::vector<p265r_tb> tbs;
    std::vector<uint32_t> nz;
    std::vector<int16_t> raw;
    p265r_picture pic() const {
        p265r_picture p{};
        p.tbs = tbs.empty() ? nullptr : tbs.data();
        p.n_tbs = (uint32_t)tbs.size();
        p.coef = raw.empty() ? nullptr : raw.data();
        p.n_coef = raw.size();
        return p;
    }
    p265r_sparse_coef sc() const { return p265r_sparse_coef{nz.empty() ? nullptr : nz.data(), nz.size()}; }
    int validate() const { const p265r_picture p = pic(); const p265r_sparse_coef s = sc(); return sparse_validate(p, &s, nullptr); }
};

static Dense random_dense(uint32_t seed, int n_tbs) {
    std::mt19937 rng(seed);
    Dense d;
    for (int t = 0; t < n_tbs; ++t) {
        p265r_tb tb{};
        tb.log2_size = (uint8_t)(2 + rng() % 4);
        const uint32_t kind = rng() % 8;
        tb.flags = kind == 0 ? 0 : kind == 1 ? P265R_TB_PCM : kind == 2 ? (P265R_TB_CBF | P265R_TB_BYPASS)
                 : kind == 3 ? (P265R_TB_CBF | P265R_TB_TSKIP) : kind == 4 ? P265R_TB_BYPASS : P265R_TB_CBF;
        const uint32_t nn = 1u << (2 * tb.log2_size);
        if (tb.flags & (P265R_TB_CBF | P265R_TB_PCM)) {
            tb.coef_off = (uint32_t)d.coef.size();
            const uint32_t dens = rng() % 4;                          // 0: all zero, 3: all non-zero
            for (uint32_t k = 0; k < nn; ++k) {
                int16_t v = (int16_t)(rng() & 0xffff);
                if (dens == 0 || (dens < 3 && rng() % 6)) v = 0;
                if (dens == 3 && v == 0) v = -32768;
                d.coef.push_back(v);
            }
        }
        d.tbs.push_back(tb);
    }
    return d;
}

static int sparsify(const Dense& d, Sparse* s) {
    const p265r_picture p = d.pic();
    uint64_t n_nz = 0, n_raw = 0;
    int rc = p265r_sparsify(&p, nullptr, nullptr, 0, &n_nz, nullptr, 0, &n_raw);
    if (rc) return rc;
    s->tbs.assign(d.tbs.size(), p265r_tb{});
    s->nz.assign(n_nz, 0);
    s->raw.assign(n_raw, 0);
    uint64_t a = 0, b = 0;
    rc = p265r_sparsify(&p, s->tbs.data(), s->nz.data(), s->nz.size(), &a, s->raw.data(), s->raw.size(), &b);
    EXPECT(rc != 0 || (a == n_nz && b == n_raw));
    return rc;
}

// the dense coefficients a sparse picture stands for, TB by TB, against the dense picture
static void check_equal(const Dense& d, const Sparse& s) {
    for (size_t t = 0; t < d.tbs.size(); ++t) {
        const p265r_tb &a = d.tbs[t], &b = s.tbs[t];
        EXPECT(a.flags == b.flags && a.log2_size == b.log2_size);
        if (!(a.flags & (P265R_TB_CBF | P265R_TB_PCM))) continue;
        const uint32_t nn = 1u << (2 * a.log2_size);
        std::vector<int16_t> got(nn, 0);
        if (tb_is_sparse(b)) {
            for (uint32_t k = 0; k < tb_sparse_count(b); ++k) {
                const uint32_t e = s.nz[b.coef_off + k];
                got[e & 0xffff] = (int16_t)(e >> 16);
                EXPECT((e >> 16) != 0);
            }
        } else {
            EXPECT(tb_sparse_count(b) == 0);
            std::memcpy(got.data(), s.raw.data() + b.coef_off, sizeof(int16_t) * nn);
        }
        EXPECT(std::memcmp(got.data(), d.coef.data() + a.coef_off, sizeof(int16_t) * nn) == 0);
    }
}

// one sparse TB of log2 size lg with the given entries
static Sparse one_tb(int lg, std::vector<uint32_t> entries, uint8_t flags = P265R_TB_CBF) {
    Sparse s;
    p265r_tb tb{};
    tb.log2_size = (uint8_t)lg;
    tb.flags = flags;
    tb.reserved[0] = (uint8_t)(entries.size() & 0xff);
    tb.reserved[1] = (uint8_t)(entries.size() >> 8);
    s.tbs.push_back(tb);
    s.nz = std::move(entries);
    return s;
}

int main() {
    // good inputs: sparsify, validate what it wrote, compare with the dense picture
    for (uint32_t seed = 1; seed <= 40; ++seed) {
        const Dense d = random_dense(seed, (int)(seed * 7 % 90));
        Sparse s;
        EXPECT(sparsify(d, &s) == P265R_OK);
        EXPECT(s.validate() == P265R_OK);
        check_equal(d, s);
    }
    {   // an empty picture; a picture with n_nz = 0 and nz = NULL
        Dense d;
        Sparse s;
        EXPECT(sparsify(d, &s) == P265R_OK && s.validate() == P265R_OK);
        Sparse z = one_tb(3, {});
        EXPECT(z.validate() == P265R_OK);
    }
    {   // sparsify: capacities one short, a TB past the coefficients, a bad size, NULL arguments
        const Dense d = random_dense(99, 60);
        Sparse s;
        EXPECT(sparsify(d, &s) == P265R_OK);
        const p265r_picture p = d.pic();
        if (!s.nz.empty()) {
            std::vector<uint32_t> nz(s.nz.size() - 1);
            EXPECT(p265r_sparsify(&p, s.tbs.data(), nz.data(), nz.size(), nullptr, s.raw.data(), s.raw.size(), nullptr) == P265R_ERANGE);
        }
        if (!s.raw.empty()) {
            std::vector<int16_t> raw(s.raw.size() - 1);
            EXPECT(p265r_sparsify(&p, s.tbs.data(), s.nz.data(), s.nz.size(), nullptr, raw.data(), raw.size(), nullptr) == P265R_ERANGE);
        }
        Dense cut = d;
        cut.coef.pop_back();
        cut.coef.shrink_to_fit();
        const p265r_picture pc = cut.pic();
        EXPECT(p265r_sparsify(&pc, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == P265R_ERANGE);
        Dense bad = d;
        for (auto& tb : bad.tbs) if (tb.flags & P265R_TB_CBF) { tb.log2_size = 6; break; }
        const p265r_picture pb = bad.pic();
        EXPECT(p265r_sparsify(&pb, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == P265R_EINVAL);
        EXPECT(p265r_sparsify(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == P265R_EINVAL);
        EXPECT(p265r_sparsify(&p, nullptr, s.nz.data(), s.nz.size(), nullptr, nullptr, 0, nullptr) == P265R_EINVAL);
    }
    // malformed sparse records, each with the documented code
    for (int lg = 2; lg <= 5; ++lg) {
        const uint32_t nn = 1u << (2 * lg);
        EXPECT(one_tb(lg, {(nn - 1) | 0x7fffu << 16}).validate() == P265R_OK);          // last position
        EXPECT(one_tb(lg, {nn | 1u << 16}).validate() == P265R_ERANGE);               // pos >= N*N
        EXPECT(one_tb(lg, {0xffffu | 1u << 16}).validate() == P265R_ERANGE);
        EXPECT(one_tb(lg, {3 | 1u << 16, 3 | 2u << 16}).validate() == P265R_EINVAL);  // not strictly increasing
        EXPECT(one_tb(lg, {5 | 1u << 16, 2 | 2u << 16}).validate() == P265R_EINVAL);
        EXPECT(one_tb(lg, {0, 1, 2}).validate() == P265R_OK);                         // level 0 is allowed
        std::vector<uint32_t> full(nn);
        for (uint32_t k = 0; k < nn; ++k) full[k] = k | 0x8000u << 16;
        EXPECT(one_tb(lg, full).validate() == P265R_OK);                              // count = N*N
        Sparse over = one_tb(lg, full);                                               // count = N*N + 1
        over.nz.push_back(0);
        over.tbs[0].reserved[0] = (uint8_t)((nn + 1) & 0xff);
        over.tbs[0].reserved[1] = (uint8_t)((nn + 1) >> 8);
        EXPECT(over.validate() == P265R_EINVAL);
        Sparse shortnz = one_tb(lg, full);                                            // coef_off + count > n_nz
        shortnz.nz.pop_back();
        shortnz.nz.shrink_to_fit();
        EXPECT(shortnz.validate() == P265R_ERANGE);
        Sparse off = one_tb(lg, {1 | 1u << 16});
        off.tbs[0].coef_off = 1;
        EXPECT(off.validate() == P265R_ERANGE);
        off.tbs[0].coef_off = 0xffffffffu;
        EXPECT(off.validate() == P265R_ERANGE);
        Sparse r2 = one_tb(lg, {1 | 1u << 16});
        r2.tbs[0].reserved[2] = 1;
        EXPECT(r2.validate() == P265R_EINVAL);
        EXPECT(one_tb(lg, {1 | 1u << 16}, 0).validate() == P265R_EINVAL);             // a count without CBF
        EXPECT(one_tb(lg, {1 | 1u << 16}, P265R_TB_TSKIP).validate() == P265R_EINVAL);
        Sparse pcm = one_tb(lg, {}, P265R_TB_PCM);                                    // dense TB past the samples
        pcm.raw.assign(nn - 1, 7);
        EXPECT(pcm.validate() == P265R_ERANGE);
        pcm.raw.assign(nn, 7);
        EXPECT(pcm.validate() == P265R_OK);
        pcm.tbs[0].coef_off = 1;
        EXPECT(pcm.validate() == P265R_ERANGE);
    }
    {   // sp NULL; nz NULL with entries announced; a TB size outside 2..5
        Sparse s = one_tb(2, {1 | 1u << 16});
        const p265r_picture p = s.pic();
        EXPECT(sparse_validate(p, nullptr, nullptr) == P265R_EINVAL);
        const p265r_sparse_coef null_nz{nullptr, 1};
        EXPECT(sparse_validate(p, &null_nz, nullptr) == P265R_EINVAL);
        s.tbs[0].log2_size = 6;
        EXPECT(s.validate() == P265R_EINVAL);
        s.tbs[0].log2_size = 1;
        EXPECT(s.validate() == P265R_EINVAL);
    }
    if (g_fail) { std::printf("sparse_check: %d check(s) failed\n", g_fail); return 1; }
    std::printf("sparse_check ok\n");
    return 0;
}
