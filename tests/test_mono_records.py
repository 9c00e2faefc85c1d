"""Monochrome (4:0:0) records on the host: what the builder emits, what validation refuses, the independence
of the luma decode from every chroma record (the ground the GPU tests' expectations stand on, tests/mono.py),
and the one-plane forms of the host-only export layout."""
import ctypes
import dataclasses

import numpy as np
import pytest

import mono as M
import planted as P
import planted_lf as L
import planted_sao as S
import planted_struct as PS
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import _lib, recon, synth
from p265_amd import records as R

TILES_KW = dict(perf=False, tiles=(2, 2), n_slices=3, lf_across_slices=None, deblocking="random", bypass_rate=0.05,
                pcm_rate=0.03, tskip_rate=0.3)
SEEDED = [(lg, bd) for lg in (4, 5, 6) for bd in (8, 10)]


def _params(lg, bd, **kw):
    return R.make_params(pic_width=136, pic_height=72, ctb_log2_size=lg, bit_depth_luma=bd, bit_depth_chroma=bd,
                         loop_filter_across_tiles=0, **kw)


def test_builder_emits_no_chroma_records():
    """synth.make_picture with monochrome params: the same luma records as the 4:2:0 picture of the same seed
    (the builder ignores the chroma arguments, so the random draws are the same), no chroma TB, no chroma SAO,
    no chroma coefficient stored."""
    for lg, bd in SEEDED:
        p420 = _params(lg, bd)
        pm = M.mono_params(p420)
        full = synth.make_picture(p420, 900 + lg, **TILES_KW)
        got = synth.make_picture(pm, 900 + lg, **TILES_KW)
        want = M.to_mono(full)
        assert (got.tbs["c_idx"] == 0).all() and len(got.tbs) == int((full.tbs["c_idx"] == 0).sum())
        assert not got.ctus["sao_type"][:, 1:].any() and not got.ctus["sao_offset"][:, 1:].any()
        assert full.ctus["sao_type"][:, 1:].any()                       # (the twin does have chroma SAO)
        np.testing.assert_array_equal(got.ctus, want.ctus)
        for f in ("x", "y", "log2_size", "c_idx", "pred_mode", "flags", "qp"):
            np.testing.assert_array_equal(got.tbs[f], want.tbs[f], err_msg=f)
        # the coefficients of every coded luma TB, at the builder's own (tighter) offsets
        coded = np.flatnonzero(got.tbs["flags"] & (R.TB_CBF | R.TB_PCM))
        assert got.n_coded_coef == len(got.coef) < len(full.coef)
        for t in coded[:: max(1, len(coded) // 64)]:
            n = 1 << (2 * int(got.tbs["log2_size"][t]))
            a, b = int(got.tbs["coef_off"][t]), int(want.tbs["coef_off"][t])
            np.testing.assert_array_equal(got.coef[a:a + n], want.coef[b:b + n])
        assert (got.nofilter is None) == (want.nofilter is None)
        if got.nofilter is not None:
            np.testing.assert_array_equal(got.nofilter, want.nofilter)
        R.validate(pm, got)
        R.validate(pm, want)
        assert R.plane_dtypes(pm) == [np.uint8 if bd == 8 else np.uint16] and R.plane_shapes(pm) == [(72, 136)]
        assert recon.plane_shapes(pm) == [(72, 136)] and len(recon.plane_shapes(p420)) == 3


def test_validate_refuses_chroma_records():
    p420 = _params(5, 8)
    pm = M.mono_params(p420)
    full = synth.make_picture(p420, 31, **TILES_KW)
    with pytest.raises(R.RecordError, match="chroma TB"):
        R.validate(pm, full)
    ok = M.to_mono(full)
    R.validate(pm, ok)
    for k in (1, 2):
        bad = dataclasses.replace(ok, ctus=ok.ctus.copy())
        bad.ctus["sao_type"][3, 1:] = k                     # (Cb = Cr: the 4:2:0 rule alone would pass it)
        with pytest.raises(R.RecordError, match="chroma SaoTypeIdx"):
            R.validate(pm, bad)
        R.validate(p420, bad)
    one = dataclasses.replace(ok, tbs=ok.tbs.copy())
    one.tbs["c_idx"][len(one.tbs) // 2] = 2
    one.tbs["x"][len(one.tbs) // 2] = 0
    one.tbs["y"][len(one.tbs) // 2] = 0
    with pytest.raises(R.RecordError):
        R.validate(pm, one)


def _independent(params, pic, label, expect_filtered, c_twin=True):
    """Luma reconstruction and decoded luma of ``pic`` with and without its chroma records, both under the 4:2:0
    params the oracles take."""
    thin = M.to_mono(pic)
    assert len(thin.tbs) < len(pic.tbs) and (thin.tbs["c_idx"] == 0).all(), label
    pp = R.pic_params(params, pic)
    R.validate(pp, thin)
    pd = R.params_dict(pp)
    rec_f, out_f = O.decode_picture(pd, pic.as_oracle_dict())
    rec_t, out_t = O.decode_picture(pd, thin.as_oracle_dict())
    np.testing.assert_array_equal(rec_t[0], rec_f[0], err_msg=label + " recon")
    np.testing.assert_array_equal(out_t[0], out_f[0], err_msg=label + " out")
    if expect_filtered:
        assert (np.asarray(out_f[0]) != np.asarray(rec_f[0])).sum() > 100, label
    if c_twin:
        (crec_f, cout_f), = c_oracle.decode(params, [pic], threads=2)
        (crec_t, cout_t), = c_oracle.decode(params, [thin], threads=2)
        np.testing.assert_array_equal(crec_f[0], rec_f[0], err_msg=label + " C recon")
        np.testing.assert_array_equal(crec_t[0], rec_f[0], err_msg=label + " C recon, no chroma records")
        np.testing.assert_array_equal(cout_t[0], out_f[0], err_msg=label + " C out, no chroma records")
        np.testing.assert_array_equal(cout_f[0], out_f[0], err_msg=label + " C out")


@pytest.mark.parametrize("lg,bd", SEEDED)
def test_luma_is_independent_of_chroma_records_seeded(lg, bd):
    """136 x 72, CTB 16 / 32 / 64, 8 and 10 bits; tiles 2 x 2, 3 slices, random deblocking, PCM, bypass,
    transform skip, SAO.  The Python oracle and its C twin (which accepts records without chroma TBs: its chroma
    planes are then what prediction from nothing gives, and nobody reads them here) return the same luma
    reconstruction and the same decoded luma with and without the chroma records, and the filters change luma."""
    params = _params(lg, bd)
    _independent(params, synth.make_picture(params, 7000 + 10 * lg + bd, **TILES_KW), "seeded ctb%d bd%d" % (1 << lg, bd), True)


def _family_pictures():
    sp = PS.struct_set(8, 5, "counts")[0]
    lf = L.lf_set(8, 5, "b", sao=True)[0]
    sa = S.sao_set(10, 4, 0)[-1]
    return [("planted", P.set_params(8), P.planted_set(8)[40][1]),
            ("planted_struct", PS.set_params(8, 5), sp),
            ("planted_lf", L.params_of(8, 5, "b", True, lf.spec.w, lf.spec.h), lf),
            ("planted_sao", S.params_of(10, 4, 0, *sa.size), dataclasses.replace(sa, size=None))]


@pytest.mark.parametrize("k", range(4))
def test_luma_is_independent_of_chroma_records_planted(k):
    """One picture of each planted family (planted, planted_struct `counts`, planted_lf with SAO, planted_sao's
    last `strips` picture) through both oracles, with and without its chroma records."""
    name, params, pic = _family_pictures()[k]
    _independent(params, pic, name, False)


def test_tile_halo_and_rank_paths_refuse_monochrome_params():
    from p265_amd import dist, halo, tiles
    pm = M.mono_params(_params(5, 8))
    pic = synth.make_picture(pm, 5, perf=True)
    for call in (lambda: tiles.tile_grid(pm, pic), lambda: tiles.split(pm, pic, recon_only=True),
                 lambda: tiles.stitch(pm, [], []), lambda: halo.TileGrid(pm, [0, 5], [0, 3]),
                 lambda: dist.broadcast_params(pm)):
        with pytest.raises(ValueError, match="monochrome"):
            call()


# ---- host-only export layout and coefficients -------------------------------------------------------------------------

def _layout(params, **kw):
    return recon.export_layout(params, recon.ExportSpec(**kw))


@pytest.mark.parametrize("bd", [8, 10])
def test_export_layout_of_monochrome_params(bd):
    p420 = R.make_params(pic_width=72, pic_height=40, bit_depth_luma=bd, bit_depth_chroma=bd)
    pm = M.mono_params(p420)
    es = 1 if bd == 8 else 2
    # planar: one plane, plane_off[1..2] = pitch[1..2] = 0; odd crops are legal
    lay = _layout(pm, format="planar", crop=(1, 3, 1, 1))
    assert lay.n_planes == 1 and lay.plane_off == [0] and lay.pitch == [68 * es] and lay.frame_bytes == 68 * es * 38
    assert [int(lay.desc.plane_off[k]) for k in (1, 2)] == [0, 0] and [int(lay.desc.pitch[k]) for k in (1, 2)] == [0, 0]
    assert lay.plane_view(0, (72, 40)) == ((38, 68), (68 * es, es))
    assert _layout(p420, format="planar").n_planes == 3
    with pytest.raises(_lib.P265RError):
        _layout(p420, format="planar", crop=(1, 3, 1, 1))               # 4:2:0 keeps its even rule
    # semi-planar: Y + a CbCr plane (written grey), even crops only
    lay = _layout(pm, format="semiplanar", crop=(2, 2, 0, 4), pitch_align=64)
    assert lay.n_planes == 2
    assert lay.pitch[0] == lay.pitch[1] == -(-68 * es // 64) * 64 and lay.plane_off[1] == lay.pitch[0] * 36
    assert lay.frame_bytes == lay.pitch[0] * (36 + 18)
    for crop in ((1, 1, 0, 0), (0, 0, 1, 1), (0, 1, 0, 0)):
        with pytest.raises(_lib.P265RError) as ei:
            _layout(pm, format="semiplanar", crop=crop)
        assert ei.value.code == _lib.EINVAL
    # RGB: three planes / one packed plane of the cropped size, odd crops legal; matrix and upsample still validated
    for fmt, sample, npl, row in (("rgb_planar", "f16", 3, 68 * 2), ("rgb_packed", "u8", 1, 68 * 3), ("rgb_planar", "native", 3, 68 * es)):
        lay = _layout(pm, format=fmt, sample=sample, crop=(1, 3, 1, 1), upsample="bilinear", matrix="bt601")
        assert lay.n_planes == npl and lay.pitch == [row] * npl and lay.frame_bytes == npl * row * 38
    with pytest.raises(_lib.P265RError):
        _layout(pm, format="rgb_packed", sample="u8", matrix=7)
    with pytest.raises(_lib.P265RError):
        _layout(pm, format="rgb_packed", sample="u8", crop=(36, 36, 0, 0))      # no sample left
    # an SPS bit_depth_chroma that differs from luma means nothing for monochrome params
    kw = R.params_dict(pm)
    kw["bit_depth_chroma"] = 8 if bd != 8 else 12
    assert _layout(R.make_params(**kw), format="planar").frame_bytes == 72 * 40 * es
    # the coefficients: the 4:2:0 ones (R = G = B follows from Cb = Cr = 1 << (B - 1))
    spec = recon.ExportSpec(format="rgb_packed", sample="u8", matrix="bt709")
    c = recon.export_coefficients(spec, bd)
    assert c[5] == 16 << (bd - 8) and c[6] == 1 << (bd - 1) and c[7] == 8
    y = np.arange(1 << bd)
    grey = np.clip((c[0] * (y - c[5]) + 8192) >> 14, 0, 255)
    assert grey[16 << (bd - 8)] == 0 and grey[235 << (bd - 8)] == 255 and (np.diff(grey) >= 0).all()


def test_export_layout_c_abi_fields():
    """p265r_export_layout through ctypes: chroma_format_idc 0 and the crop parity rule per format."""
    lib = _lib.load()

    def rc(fmt, mono, **crop):
        p = R.make_params(pic_width=72, pic_height=40)
        pc = recon._params_c(M.mono_params(p) if mono else p)
        d = _lib.ExportDesc()
        d.format = fmt
        if fmt >= _lib.FMT_RGB_PLANAR:
            d.sample = _lib.SMP_U8
        for k, v in crop.items():
            setattr(d, k, v)
        return lib.p265r_export_layout(ctypes.byref(pc), 0, 0, ctypes.byref(d), 1)

    for f in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
        for fmt in (_lib.FMT_PLANAR, _lib.FMT_RGB_PLANAR, _lib.FMT_RGB_PACKED):
            assert rc(fmt, True, **{f: 3}) == _lib.OK
            assert rc(fmt, False, **{f: 3}) == _lib.EINVAL
        assert rc(_lib.FMT_SEMIPLANAR, True, **{f: 3}) == _lib.EINVAL
        assert rc(_lib.FMT_SEMIPLANAR, True, **{f: 2}) == _lib.OK
