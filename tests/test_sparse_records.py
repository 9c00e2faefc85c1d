"""Sparse coefficient records (no GPU): records.sparsify / densify, and the C p265r_sparsify against them.

The sparse form (include/p265r.h p265r_sparse_coef): a transformed TB's coefficients are its non-zero
levels as entries pos | (uint16)level << 16, PCM / bypass TBs keep their dense samples."""
import ctypes

import numpy as np
import pytest

from p265_amd import _lib, frontend, recon, synth
from p265_amd import records as R


def _synthetic():
    """Feature pictures: PCM + bypass + transform skip, tiles + slices, a ragged size, Main 10."""
    out = []
    p = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    out.append(synth.make_picture(p, 11, perf=False, tiles=(3, 2), n_slices=4, tskip_rate=0.2, bypass_rate=0.1,
                                  pcm_rate=0.1, deblocking="random"))
    p = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=6)
    out.append(synth.make_picture(p, 12, perf=False, tskip_rate=0.1, bypass_rate=0.05, pcm_rate=0.05))
    p = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4, bit_depth_luma=10, bit_depth_chroma=10)
    out.append(synth.make_picture(p, 13, perf=False, pcm_rate=0.2, tskip_rate=0.3))
    p = R.make_params(pic_width=352, pic_height=288)
    out.append(synth.make_picture(p, 14, perf=True))
    return out


PICS = _synthetic()


def _one_tb_picture(log2, coef, flags=R.TB_CBF):
    """A picture record set holding one luma TB (records only: nothing decodes it here)."""
    tbs = np.zeros(1, R.TB_DTYPE)
    tbs["log2_size"], tbs["flags"], tbs["qp"] = log2, flags, 30
    ctus = np.zeros(1, R.CTU_DTYPE)
    ctus["tb_count"] = 1
    return R.Picture(ctus=ctus, tbs=tbs, coef=np.asarray(coef, np.int16).reshape(-1))


def _count(tbs):
    return tbs["reserved"][:, 0].astype(int) | (tbs["reserved"][:, 1].astype(int) << 8)


@pytest.mark.parametrize("k", range(len(PICS)))
def test_round_trip(k):
    pic = PICS[k]
    sp = R.sparsify(pic)
    back = R.densify(sp)
    assert np.array_equal(back.tbs, pic.tbs)
    assert np.array_equal(back.coef, pic.coef)
    assert back.ctus is pic.ctus and back.nofilter is pic.nofilter
    # entries: non-zero levels only, strictly increasing inside every TB, counts within N*N
    assert sp.nz.dtype == np.uint32 and ((sp.nz >> 16) != 0).all()
    sparse, raw = R._tb_kinds(sp.tbs)
    cnt = _count(sp.tbs)
    assert (cnt[~sparse] == 0).all() and (cnt <= 1 << (2 * sp.tbs["log2_size"].astype(int))).all()
    assert int(cnt.sum()) == len(sp.nz) == int(np.count_nonzero(R.densify(sp).coef)) - int(np.count_nonzero(sp.coef))
    for t in np.flatnonzero(sparse)[:200]:
        pos = sp.nz[sp.tbs["coef_off"][t]:sp.tbs["coef_off"][t] + cnt[t]] & 0xffff
        assert (np.diff(pos.astype(int)) > 0).all() and (pos < 1 << (2 * int(sp.tbs["log2_size"][t]))).all()
    assert len(sp.coef) == int(np.sum(1 << (2 * sp.tbs["log2_size"][raw].astype(int))))


@pytest.mark.parametrize("k", range(len(PICS)))
def test_densify_without_the_recorded_layout_packs_in_tb_order(k):
    """A sparse picture that never was dense (the C sparsify keeps no layout): every coded TB's block in TB
    order -- the same picture, and the same arrays when the dense one was laid out that way (no tiles)."""
    pic = PICS[k]
    sp = recon.sparsify(pic)
    assert sp.dense_off is None
    back = R.densify(sp)
    coded = (pic.tbs["flags"] & (R.TB_CBF | R.TB_PCM)) != 0
    nn = 1 << (2 * pic.tbs["log2_size"].astype(np.int64))
    assert np.array_equal(back.tbs["coef_off"][coded], (np.cumsum(nn[coded]) - nn[coded]))
    for name in R.TB_DTYPE.names:
        if name != "coef_off":
            assert np.array_equal(back.tbs[name], pic.tbs[name]), name
    a, _, _ = R._ranges(pic.tbs["coef_off"][coded], nn[coded])
    b, _, _ = R._ranges(back.tbs["coef_off"][coded], nn[coded])
    assert np.array_equal(pic.coef[a], back.coef[b])
    if pic.meta.get("tiles", (1, 1)) == (1, 1):
        assert np.array_equal(back.tbs, pic.tbs) and np.array_equal(back.coef, pic.coef)


def test_feature_pictures_cover_the_kinds():
    f = np.concatenate([p.tbs["flags"] for p in PICS])
    for bit in (R.TB_PCM, R.TB_BYPASS, R.TB_TSKIP):
        assert (f & bit).any()
    assert ((f & R.TB_BYPASS) != 0)[(f & R.TB_CBF) != 0].any()        # coded bypass TBs: dense by nature


@pytest.mark.parametrize("k", range(len(PICS)))
def test_c_sparsify_equals_numpy(k):
    pic = PICS[k]
    a, b = R.sparsify(pic), recon.sparsify(pic)
    assert np.array_equal(a.tbs, b.tbs)
    assert np.array_equal(a.nz, b.nz)
    assert np.array_equal(a.coef, b.coef)


def test_all_zero_cbf_tb_has_no_entries():
    pic = _one_tb_picture(3, np.zeros(64))
    for sp in (R.sparsify(pic), recon.sparsify(pic)):
        assert len(sp.nz) == 0 and _count(sp.tbs)[0] == 0 and len(sp.coef) == 0
        assert np.array_equal(R.densify(sp).coef, pic.coef)


def test_full_32x32_has_1024_entries():
    co = np.arange(1, 1025).astype(np.int16)
    pic = _one_tb_picture(5, co)
    for sp in (R.sparsify(pic), recon.sparsify(pic)):
        assert len(sp.nz) == 1024 and _count(sp.tbs)[0] == 1024
        assert np.array_equal(sp.nz & 0xffff, np.arange(1024))
        assert np.array_equal(R.densify(sp).coef, co)


def test_extreme_levels_survive():
    co = np.zeros(16, np.int16)
    co[3], co[15] = -32768, 32767
    pic = _one_tb_picture(2, co)
    for sp in (R.sparsify(pic), recon.sparsify(pic)):
        assert sp.nz.tolist() == [3 | 0x8000 << 16, 15 | 0x7fff << 16]
        assert np.array_equal(R.densify(sp).coef, co)


def test_pcm_and_bypass_stay_dense():
    co = np.arange(16).astype(np.int16)
    for flags in (R.TB_PCM, R.TB_CBF | R.TB_BYPASS, R.TB_CBF | R.TB_PCM):
        pic = _one_tb_picture(2, co, flags)
        for sp in (R.sparsify(pic), recon.sparsify(pic)):
            assert len(sp.nz) == 0 and np.array_equal(sp.coef, co) and _count(sp.tbs)[0] == 0


def test_c_sparsify_sizes_and_errors():
    lib = _lib.load()
    pic = PICS[0]
    ref = R.sparsify(pic)
    tbs = np.ascontiguousarray(pic.tbs)
    c = _lib.PictureC()
    c.tbs, c.n_tbs, c.coef, c.n_coef = tbs.ctypes.data, len(tbs), pic.coef.ctypes.data, len(pic.coef)
    n_nz, n_raw = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.p265r_sparsify(ctypes.byref(c), None, None, 0, ctypes.byref(n_nz), None, 0, ctypes.byref(n_raw)) == 0
    assert (n_nz.value, n_raw.value) == (len(ref.nz), len(ref.coef))
    out = np.zeros(len(tbs), R.TB_DTYPE)
    nz = np.zeros(len(ref.nz), np.uint32)
    raw = np.zeros(len(ref.coef), np.int16)
    # capacities one short: refused, nothing written past them
    assert lib.p265r_sparsify(ctypes.byref(c), out.ctypes.data, nz.ctypes.data, len(nz) - 1, None,
                              raw.ctypes.data, len(raw), None) == _lib.ERANGE
    assert lib.p265r_sparsify(ctypes.byref(c), out.ctypes.data, nz.ctypes.data, len(nz), None,
                              raw.ctypes.data, len(raw) - 1, None) == _lib.ERANGE
    c.n_coef = len(pic.coef) - 1                                       # a TB reaching past the coefficients
    assert lib.p265r_sparsify(ctypes.byref(c), None, None, 0, None, None, 0, None) == _lib.ERANGE
    assert lib.p265r_sparsify(None, None, None, 0, None, None, 0, None) == _lib.EINVAL


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    for name in ("p265r_batch_upload_sparse", "p265r_sparsify", "p265r_batch_upload_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.SparseCoefC) == 16 and ctypes.sizeof(_lib.PictureC) == 104
    assert lib.p265r_abi_version() == 2
    h = ctypes.c_void_p()
    assert lib.p265r_batch_upload_sparse(None, None, None, 1, ctypes.byref(h)) == _lib.EINVAL
    assert lib.p265r_batch_upload_bytes(None, None, None) == _lib.EINVAL


def test_sparse_form_is_smaller_at_the_bench_mix():
    """4 n_nz + 2 n_raw < 2 n_coef on a perf=True picture (the benchmark's mix: about one level in six
    is non-zero)."""
    pic = PICS[3]
    sp = R.sparsify(pic)
    assert 4 * len(sp.nz) + 2 * len(sp.coef) < 2 * pic.n_coded_coef
    assert pic.n_coded_coef == len(pic.coef)
