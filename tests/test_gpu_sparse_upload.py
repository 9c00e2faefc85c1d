"""Sparse coefficient upload on the GPU (p265r_batch_upload_sparse: non-zero levels up, expanded into the
dense coefficient pool by the expand kernels of coef_expand.h), bit-exact against BOTH the oracle on the
dense picture (the C oracle, oracle/c_oracle.py) and the dense upload of the same picture."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from oracle import c_oracle
from p265_amd import _lib, frontend, synth
from p265_amd import records as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _same(a, b, what):
    for i, (pa, pb) in enumerate(zip(a, b)):
        for c in range(3):
            np.testing.assert_array_equal(pa[c], pb[c], err_msg="%s pic %d c%d" % (what, i, c))


def _check(recon_mod, params, pics, label="", scaling=None, sparse_pics=None):
    """Sparse decode == dense decode == oracle, reconstruction and output planes."""
    with recon_mod.ReconContext(params, scaling=scaling) as ctx:
        d_outs, d_recs = ctx.decode(pics, with_recon=True)
        s_outs, s_recs = ctx.decode(sparse_pics if sparse_pics is not None else pics, with_recon=True, sparse=True)
    ref = c_oracle.decode(params, pics, scaling=scaling)
    _same(s_recs, [r[0] for r in ref], label + " sparse recon vs oracle")
    _same(s_outs, [r[1] for r in ref], label + " sparse out vs oracle")
    _same(s_recs, d_recs, label + " sparse recon vs dense upload")
    _same(s_outs, d_outs, label + " sparse out vs dense upload")


# ---- 1. feature mix ---------------------------------------------------------------------------
@pytest.mark.parametrize("sao", [1, 0])
@pytest.mark.parametrize("ctb_log2", [4, 5, 6])
@pytest.mark.parametrize("w,h", [(136, 72), (264, 200)])
def test_feature_mix(recon_mod, w, h, ctb_log2, sao):
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, sample_adaptive_offset=sao)
    pics = [synth.make_picture(params, 7100 + 10 * ctb_log2 + s, perf=bool(s), tiles=(3, 2), n_slices=4, sao=bool(sao),
                               pcm_rate=0.06, bypass_rate=0.06, tskip_rate=0.2, deblocking="random") for s in range(2)]
    f = np.concatenate([p.tbs["flags"] for p in pics])
    assert all((f & bit).any() for bit in (R.TB_PCM, R.TB_BYPASS, R.TB_TSKIP))
    _check(recon_mod, params, pics, "mix %dx%d ctb %d sao %d" % (w, h, ctb_log2, sao))


# ---- 2. edge coefficient shapes, hand-built -----------------------------------------------------
def _zorder(x, y, log2, leaf):
    if log2 == leaf:
        yield x, y
        return
    h = 1 << (log2 - 1)
    for i in range(4):
        yield from _zorder(x + h * (i % 2), y + h * (i // 2), log2 - 1, leaf)


def _hand_picture(params, coef_fn, cbf=1):
    """One 64x64 CTB with every TB size: a 32x32 CU (luma 32, chroma 16), four 16x16 CUs (16 / 8), sixteen
    8x8 CUs (8 / 4) and sixteen 8x8 NxN CUs (four luma 4x4 + the chroma 4x4 pair).  coef_fn(log2, c_idx, k)
    gives TB number k's coefficients (an [N][N] array, or None for all zero)."""
    b = frontend.PictureBuilder(params)
    k = [0]

    def tu(x, y, log2, blk):
        clog2 = max(2, log2 - 1)
        coef = []
        for c in range(3):
            coef.append(coef_fn(log2 if c == 0 else clog2, c, k[0]) if cbf else None)
            k[0] += 1
        return dict(x=x, y=y, log2=log2, blk=blk, cbf=[cbf] * 3, tskip=[0, 0, 0], coef=coef)

    b.add_cu(0, 0, 5, 0, [26, 0, 0, 0], 1, 30, 29, 29, [tu(0, 0, 5, 0)])
    for x, y in _zorder(32, 0, 5, 4):
        b.add_cu(x, y, 4, 0, [10, 0, 0, 0], 0, 30, 29, 29, [tu(x, y, 4, 0)])
    for x, y in _zorder(0, 32, 5, 3):
        b.add_cu(x, y, 3, 0, [1, 0, 0, 0], 26, 30, 29, 29, [tu(x, y, 3, 0)])
    for x, y in _zorder(32, 32, 5, 3):
        b.add_cu(x, y, 3, 1, [0, 1, 10, 26], 34, 30, 29, 29, [tu(x + 4 * (i % 2), y + 4 * (i // 2), 2, i) for i in range(4)])
    b.add_ctu(0, sao_type=(2, 2, 2), sao_abs=np.ones((3, 4), int), sao_sign=np.zeros((3, 4), int), sao_eo=(0, 1, 1))
    return b.finish()


def _last_pos(log2, c_idx, k):
    n = 1 << log2
    co = np.zeros((n, n), np.int16)
    co[n - 1, n - 1] = 32767 if k % 2 else -32768          # pos = N*N - 1, the extreme levels
    return co


def _full32(log2, c_idx, k):
    if log2 != 5:
        return None
    rng = np.random.default_rng(5)
    co = rng.integers(1, 4, (32, 32)) * rng.choice(np.array([-1, 1]), (32, 32))
    co[0, 0], co[0, 1], co[31, 31], co[17, 5] = 32767, -32768, -32768, 32767
    return co.astype(np.int16)


def test_edge_coefficient_shapes(recon_mod):
    params = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=6)
    pics = [_hand_picture(params, lambda *a: None),             # every TB coded, no entry at all
            _hand_picture(params, _last_pos),                   # one entry at N*N - 1 per TB, N = 4, 8, 16, 32
            _hand_picture(params, _full32),                     # one 32x32 with all 1024 positions non-zero
            _hand_picture(params, None, cbf=0)]                 # no coded TB
    sps = [R.sparsify(p) for p in pics]
    assert len(sps[0].nz) == 0 and len(sps[3].nz) == 0 and (sps[0].tbs["flags"] & R.TB_CBF).all()
    sizes = sorted(set(sps[1].tbs["log2_size"].tolist()))
    assert sizes == [2, 3, 4, 5] and len(sps[1].nz) == len(pics[1].tbs)
    assert (sps[1].nz & 0xffff == (1 << (2 * sps[1].tbs["log2_size"].astype(np.int64))) - 1).all()
    cnt = sps[2].tbs["reserved"][:, 0].astype(int) | (sps[2].tbs["reserved"][:, 1].astype(int) << 8)
    assert cnt.max() == 1024 and len(sps[2].nz) == 1024
    _check(recon_mod, params, pics, "edge", sparse_pics=sps)
    # a picture alone whose entry array is NULL (n_nz = 0): through the C sparsify path too
    _check(recon_mod, params, pics[:1], "edge nz NULL")
    _check(recon_mod, params, pics[3:], "edge no cbf")


# ---- 3. chunking ------------------------------------------------------------------------------
def _digests_equal(recon_mod, params, pics):
    with recon_mod.ReconContext(params) as ctx:
        got = []
        for sparse in (False, True):
            b = ctx.upload(pics, sparse=sparse)
            ctx.run(b)
            got.append((ctx.digest(b), ctx.digest(b, recon=True)))
            b.free()
    assert np.array_equal(got[0][0], got[1][0]), "output digests differ"
    assert np.array_equal(got[0][1], got[1][1]), "reconstruction digests differ"
    assert got[0][0].any()


def test_two_upload_chunks(recon_mod):
    params = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=5)
    pics = [synth.make_picture(params, 7300 + s, perf=bool(s % 2), tskip_rate=0.1, pcm_rate=0.05 * (s % 3), bypass_rate=0.03,
                               deblocking=bool(s % 2)) for s in range(20)]
    _digests_equal(recon_mod, params, pics)


def test_ragged_batch(recon_mod):
    big = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=5)
    pics = []
    for k, (w, h) in enumerate([(264, 200), (128, 72), (40, 200), (264, 8)]):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 7350 + k, perf=bool(k % 2), deblocking=True, pcm_rate=0.05, tskip_rate=0.1)
        pic.size = (w, h)
        pics.append(pic)
    _digests_equal(recon_mod, big, pics)


# ---- 4. bit depth and scaling lists ------------------------------------------------------------
@pytest.mark.parametrize("bd", [10, 12])
def test_bit_depth(recon_mod, bd):
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = [synth.make_picture(params, 7400 + bd + s, perf=bool(s), tskip_rate=0.2, pcm_rate=0.05, bypass_rate=0.05,
                               deblocking="random") for s in range(2)]
    _check(recon_mod, params, pics, "bd %d" % bd)


def test_scaling_lists(recon_mod):
    from oracle import recon_oracle as O
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=6, scaling_list_enabled=1)
    rng = np.random.default_rng(74)
    sf = O.scaling_factor_bytes({k: rng.integers(1, 256, (4 << k[0], 4 << k[0])) for k in O.SF_OFFSETS})
    pics = [synth.make_picture(params, 7450 + s, perf=bool(s), tskip_rate=0.3, deblocking=True) for s in range(2)]
    _check(recon_mod, params, pics, "scaling", scaling=sf)


# ---- 5. lanes -----------------------------------------------------------------------------------
def test_dense_and_sparse_batches_on_two_lanes(recon_mod):
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    sets = [[synth.make_picture(params, 7500 + 10 * k + s, perf=bool(s), tskip_rate=0.1, deblocking=True) for s in range(3)]
            for k in range(2)]
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        bd = ctx.upload(sets[0])
        bs = ctx.upload(sets[1], sparse=True)
        for _ in range(2):
            ctx.run(bd)
            ctx.run(bs)
        got = [ctx.download(b, with_recon=True) for b in (bd, bs)]
        bd.free()
        bs.free()
    for k in range(2):
        ref = c_oracle.decode(params, sets[k])
        _same(got[k][1], [r[0] for r in ref], "lane %d recon" % k)
        _same(got[k][0], [r[1] for r in ref], "lane %d out" % k)


# ---- 6. rejection (host side: nothing malformed reaches the device) ------------------------------
def _count(tbs):
    return tbs["reserved"][:, 0].astype(int) | (tbs["reserved"][:, 1].astype(int) << 8)


def _malformed(sp):
    """(name, SparsePicture, expected code) for each malformed input of the sparse upload."""
    sparse, raw = R._tb_kinds(sp.tbs)
    cnt = _count(sp.tbs)
    nn = 1 << (2 * sp.tbs["log2_size"].astype(int))
    out = []

    def variant(name, code, **kw):
        d = dict(ctus=sp.ctus, tbs=sp.tbs.copy(), nz=sp.nz.copy(), coef=sp.coef.copy(), nofilter=sp.nofilter)
        d.update(kw)
        out.append((name, R.SparsePicture(**d), code))
        return out[-1][1]

    variant("entries past n_nz", _lib.ERANGE, nz=sp.nz[:-1].copy())
    t4 = int(np.flatnonzero(sparse & (sp.tbs["log2_size"] == 2) & (cnt >= 2))[0])
    v = variant("pos >= N*N", _lib.ERANGE)
    v.nz[sp.tbs["coef_off"][t4] + cnt[t4] - 1] = 16 | (1 << 16)
    v = variant("count > N*N", _lib.EINVAL)
    v.tbs["reserved"][t4, 0] = 17
    v = variant("positions not increasing", _lib.EINVAL)
    o = int(sp.tbs["coef_off"][t4])
    v.nz[o], v.nz[o + 1] = sp.nz[o + 1], sp.nz[o]
    v = variant("repeated position", _lib.EINVAL)
    v.nz[o + 1] = sp.nz[o]
    v = variant("reserved[2] set", _lib.EINVAL)
    v.tbs["reserved"][t4, 2] = 1
    tz = int(np.flatnonzero((sp.tbs["flags"] & (R.TB_CBF | R.TB_PCM)) == 0)[0])
    v = variant("count without CBF", _lib.EINVAL)
    v.tbs["reserved"][tz, 0] = 1
    assert raw.any() and len(sp.coef)
    variant("PCM / bypass samples past coef", _lib.ERANGE, coef=sp.coef[:-1].copy())
    return out


def test_malformed_sparse_records_are_rejected(recon_mod):
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    pic = synth.make_picture(params, 7600, perf=False, tskip_rate=0.1, pcm_rate=0.1, bypass_rate=0.05, deblocking=True)
    good = R.sparsify(pic)
    with recon_mod.ReconContext(params) as ctx:
        for name, bad, code in _malformed(good):
            with pytest.raises(_lib.P265RError) as ei:
                ctx.upload([good, bad], sparse=True)
            assert ei.value.code == code, name
        # sp NULL, and nz NULL with entries announced: straight through the C ABI
        arr, keep = ctx._pictures_c([good])
        h = ctypes.c_void_p()
        assert ctx.lib.p265r_batch_upload_sparse(ctx.handle, arr, None, 1, ctypes.byref(h)) == _lib.EINVAL and not h.value
        sc = (_lib.SparseCoefC * 1)()
        sc[0].nz, sc[0].n_nz = None, len(good.nz)
        assert ctx.lib.p265r_batch_upload_sparse(ctx.handle, arr, sc, 1, ctypes.byref(h)) == _lib.EINVAL and not h.value
        del keep
        # the context still decodes a good upload afterwards
        outs, recs = ctx.decode([good], with_recon=True, sparse=True)
    ref = c_oracle.decode(params, [pic])
    _same(recs, [ref[0][0]], "after rejection recon")
    _same(outs, [ref[0][1]], "after rejection out")


# ---- 7. bytes -----------------------------------------------------------------------------------
def test_sparse_upload_moves_fewer_bytes(recon_mod):
    params = R.make_params(pic_width=352, pic_height=288)
    pics = [synth.make_picture(params, 7700 + s, perf=True) for s in range(4)]
    sps = [R.sparsify(p) for p in pics]
    with recon_mod.ReconContext(params) as ctx:
        bd = ctx.upload(pics)
        D = ctx.upload_bytes(bd)
        bd.free()
        bs = ctx.upload(sps, sparse=True)
        S = ctx.upload_bytes(bs)
        bs.free()
    n_nz = sum(len(s.nz) for s in sps)
    J = sum(int(R._tb_kinds(s.tbs)[0].sum()) for s in sps)
    C_s = sum(int(np.sum(1 << (2 * s.tbs["log2_size"][R._tb_kinds(s.tbs)[0]].astype(np.int64)))) for s in sps)
    print("upload bytes: dense %d sparse %d (C_s %d n_nz %d J %d)" % (D, S, C_s, n_nz, J))
    assert D >= 2 * C_s
    assert S < D
    assert S <= D - 2 * C_s + 4 * n_nz + 8 * J + 65536


def _bytes_case(name):
    """(params, pictures) of a tiny batch whose upload_bytes are pinned below."""
    if name == "ragged":
        big = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=5)
        pics = []
        for k, (w, h) in enumerate([(264, 200), (128, 72), (40, 200), (264, 8)]):        # test_ragged_batch's
            pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
            pic = synth.make_picture(pp, 7350 + k, perf=bool(k % 2), deblocking=True, pcm_rate=0.05, tskip_rate=0.1)
            pic.size = (w, h)
            pics.append(pic)
        return big, pics
    n, ctb_log2, kw = {"1 x ctb 64": (1, 6, {}),
                       "16 x ctb 32": (16, 5, dict(pcm_rate=0.1, bypass_rate=0.05, deblocking=True)),    # no-filter maps
                       "27 x ctb 16": (27, 4, dict(tskip_rate=0.1))}[name]
    params = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=ctb_log2)
    return params, [synth.make_picture(params, 7800 + s, perf=bool(s % 2), **kw) for s in range(n)]


# p265r_batch_upload_bytes (dense, sparse) of each case, recorded from the library of commit 2a96b6f (before
# the upload was split into the host planner of upload_host.cpp and the enqueue loop): the count is integer
# arithmetic over the layout and the chunk copy lists, so any change of either shows here.
_UPLOAD_BYTES = {"1 x ctb 64": (45304, 39944), "16 x ctb 32": (234288, 165096), "27 x ctb 16": (381704, 254268),
                 "ragged": (266748, 186868)}


@pytest.mark.parametrize("name", list(_UPLOAD_BYTES))
def test_upload_bytes_are_pinned(recon_mod, name):
    params, pics = _bytes_case(name)
    if name == "16 x ctb 32":
        assert any(p.nofilter is not None for p in pics) and any((p.ctus["flags"] & R.CTU_DEBLOCK).any() for p in pics)
    got = []
    with recon_mod.ReconContext(params) as ctx:
        for sparse in (False, True):
            b = ctx.upload(pics, sparse=sparse)
            got.append(ctx.upload_bytes(b))
            b.free()
    print("upload bytes %s: dense %d sparse %d" % (name, got[0], got[1]))
    assert tuple(got) == _UPLOAD_BYTES[name]
    _digests_equal(recon_mod, params, pics)


# ---- 8. end to end ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_main10.bin", "synth_1080p_4pic.bin"])
def test_decoder_with_sparse_upload(recon_mod, name):
    from p265_amd import decoder
    data = open(os.path.join(GOLDEN, name), "rb").read()
    dense = decoder.decode_bytes(data)
    sparse = decoder.decode_bytes(data, sparse_upload=True)          # raises HashMismatch on any difference
    assert len(sparse) == len(dense) > 0
    for a, b in zip(sparse, dense):
        assert a.hash_ok is True and b.hash_ok is True
        assert a.poc == b.poc
        for c in range(3):
            assert hashlib.md5(a.planes[c].tobytes()).digest() == hashlib.md5(b.planes[c].tobytes()).digest()
            np.testing.assert_array_equal(a.planes[c], b.planes[c])
