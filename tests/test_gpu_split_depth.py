"""Unequal luma / chroma bit depths (p265r_params.split_bit_depth) on the GPU through the C ABI against the C oracle,
bit-exact, reconstruction and output.

A context is wide when either depth exceeds 8: all three device planes hold uint16_t samples, the row kernel clips
luma and chroma at their own limits (intra_rows_kernel<..., uint16_t>, int16_t when BitDepthC > 10), the in-loop
filters index the depth per component, an 8-bit component is narrowed on the device before the download (narrow.h)
and widened on the host during a recon-input upload.  The host sees every plane in its component's type.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import split_cases as S
from p265_amd import _lib, digest
from p265_amd import records as R

pytestmark = pytest.mark.gpu

SCHEDULES = {"rows": {"P265R_ROW_WAVES": "8"}, "rows12": {"P265R_ROW_WAVES": "12"}, "steps": {"P265R_SCHEDULE": "steps"}}
ALL = range(len(S.PAIRS))


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _dtypes(k):
    y, c = S.PAIRS[k]
    return [np.dtype(np.uint8 if y == 8 else np.uint16)] + [np.dtype(np.uint8 if c == 8 else np.uint16)] * 2


def _same(got, ref, k, label):
    for i in range(len(ref)):
        for c in range(3):
            assert got[i][c].dtype == _dtypes(k)[c], "%s pic %d c%d dtype %s" % (label, i, c, got[i][c].dtype)
            np.testing.assert_array_equal(got[i][c], ref[i][c], err_msg="%s pic %d c%d" % (label, i, c))


def _check(recon_mod, monkeypatch, name, k, schedule, sparse=False):
    for key, v in SCHEDULES[schedule].items():
        monkeypatch.setenv(key, v)
    params, pics, refs = S.case(name, k)
    with recon_mod.ReconContext(params) as ctx:
        outs, recs = ctx.decode(pics, with_recon=True, sparse=sparse)
        d = ctx.describe()
    assert (d["bit_depth"], d["bit_depth_chroma"]) == S.PAIRS[k]
    assert d["schedule"] == ("steps" if schedule == "steps" else "rows")
    if schedule == "steps":
        assert d["last_launch_layout"] == "steps" and d["last_launch_row_waves"] == 0
    else:
        assert d["row_waves"] == d["last_launch_row_waves"] == (12 if schedule == "rows12" else 8)
    _same(recs, [r[0] for r in refs], k, "%s %s %s recon" % (name, S.PAIRS[k], schedule))
    _same(outs, [r[1] for r in refs], k, "%s %s %s out" % (name, S.PAIRS[k], schedule))


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("k", ALL)
def test_tiles_slices_pcm_bypass_tskip(recon_mod, monkeypatch, k, schedule):
    _check(recon_mod, monkeypatch, "tiles", k, schedule)


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("k", ALL)
def test_uniform_modes_reach_both_clip_limits(recon_mod, monkeypatch, k, schedule):
    _, _, refs = S.case("uniform", k)
    y, c = S.PAIRS[k]
    lo = [min(int(rec[ci].min()) for rec, _ in refs) for ci in range(3)]
    hi = [max(int(rec[ci].max()) for rec, _ in refs) for ci in range(3)]
    assert lo[0] == 0 and hi[0] == (1 << y) - 1
    assert any(lo[ci] == 0 and hi[ci] == (1 << c) - 1 for ci in (1, 2))
    _check(recon_mod, monkeypatch, "uniform", k, schedule)


def _download_c(ctx, batch, n, shapes, dts, want_out, want_rec):
    """p265r_batch_download with exactly the planes asked for (the Python download always takes the output)."""
    outs = [[np.full(s, 0xA5, dt) for s, dt in zip(shapes[i], dts)] for i in range(n)] if want_out else None
    recs = [[np.full(s, 0xA5, dt) for s, dt in zip(shapes[i], dts)] for i in range(n)] if want_rec else None
    arr = (_lib.PictureC * n)()
    for i in range(n):
        for c in range(3):
            if outs is not None:
                arr[i].out[c] = outs[i][c].ctypes.data
            if recs is not None:
                arr[i].recon[c] = recs[i][c].ctypes.data
    _lib.check(ctx.lib.p265r_batch_download(ctx.handle, batch.handle, arr, n), "p265r_batch_download")
    return outs, recs


@pytest.mark.parametrize("k", [1, 0])
@pytest.mark.parametrize("name", ["narrow", "ragged"])
def test_narrowed_download_edges(recon_mod, k, name):
    """Chroma rows of 36 samples (two full 16-byte groups + 4 bytes) and a ragged batch, at (10, 8) and (8, 10): the
    output alone, the reconstruction alone, both, a partial download and a frame pool -- every download path."""
    params, pics, refs = S.case(name, k)
    n = len(pics)
    shapes = [R.plane_shapes(R.pic_params(params, p)) for p in pics]
    dts = R.plane_dtypes(params)
    rec_ref, out_ref = [r[0] for r in refs], [r[1] for r in refs]
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        outs, recs = _download_c(ctx, b, n, shapes, dts, True, False)
        _same(outs, out_ref, k, "%s out only" % name)
        outs, recs = _download_c(ctx, b, n, shapes, dts, False, True)
        _same(recs, rec_ref, k, "%s recon only" % name)
        outs, recs = _download_c(ctx, b, n, shapes, dts, True, True)
        _same(outs, out_ref, k, "%s both, out" % name)
        _same(recs, rec_ref, k, "%s both, recon" % name)
        part = ctx.download(b, only=[n - 1])
        assert all(part[i] is None for i in range(n - 1))
        _same([part[n - 1]], [out_ref[n - 1]], k, "%s partial" % name)
        pool = [[np.zeros(s, dt) for s, dt in zip(shapes[i], dts)] for i in range(n)]
        again = ctx.download(b, into=pool)
        assert all(again[i][c] is pool[i][c] for i in range(n) for c in range(3))
        _same(pool, out_ref, k, "%s frame pool" % name)
        b.free()
        outs, recs = ctx.decode(pics, with_recon=True)           # p265r_submit / p265r_wait
        _same(outs, out_ref, k, "%s wait, out" % name)
        _same(recs, rec_ref, k, "%s wait, recon" % name)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("name", ["sao_only", "narrow"])
def test_recon_input(recon_mod, k, name):
    """A P265R_PIC_RECON_INPUT batch at (8, 10) and (10, 8): the 8-bit component's planes go up widened, the filters
    run on 16-bit planes (sao_only: the streaming SAO kernel; narrow: the deblocking + SAO window kernel), and the
    output comes back narrowed."""
    params, pics, refs = S.case(name, k)
    given = [dataclasses.replace(p, recon_input=[np.array(pl) for pl in rec]) for p, (rec, _) in zip(pics, refs)]
    assert [pl.dtype for pl in given[0].recon_input] == _dtypes(k)
    with recon_mod.ReconContext(params) as ctx:
        _same(ctx.decode(given), [r[1] for r in refs], k, "%s recon input" % name)
        b = ctx.upload(given)
        ctx.run(b)
        _same(ctx.download(b), [r[1] for r in refs], k, "%s recon input, batch" % name)
        b.free()


@pytest.mark.parametrize("k", [0, 1, 2, 5])
@pytest.mark.parametrize("name", ["no_sao_dbk", "no_sao"])
def test_no_sao(recon_mod, monkeypatch, name, k):
    _check(recon_mod, monkeypatch, name, k, "rows12")


@pytest.mark.parametrize("k", [1, 2])
def test_sparse_upload_and_sao_only(recon_mod, monkeypatch, k):
    _check(recon_mod, monkeypatch, "sao_only" if k == 1 else "tiles", k, "rows", sparse=True)


def test_device_digest_is_of_the_wide_planes(recon_mod):
    params, pics, refs = S.case("ragged", 1)
    assert S.PAIRS[1] == (10, 8)
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        got, got_rec = ctx.digest(b), ctx.digest(b, recon=True)
        b.free()
    for i, (rec, out) in enumerate(refs):
        assert out[1].dtype == np.uint8
        assert np.array_equal(got[i], digest.picture_digest(out, wide=True)), "out %d" % i
        assert np.array_equal(got_rec[i], digest.picture_digest(rec, wide=True)), "recon %d" % i
        assert not np.array_equal(got[i][1:], digest.picture_digest(out)[1:])


@pytest.mark.parametrize("depths,kind", [((8, 10), "md5"), ((8, 10), "crc"), ((12, 10), "checksum"), ((12, 10), "md5"),
                                         ((8, 10), "checksum"), ((12, 10), "crc")])
def test_stream_end_to_end(recon_mod, tmp_path, depths, kind):
    """A generated stream through decoder.decode_bytes with host hashing, and through the command line."""
    from streamgen_split import StreamGenSplit
    from p265_amd import dec, decoder
    g = StreamGenSplit(60 + depths[0], depths=depths, width=136, height=72, ctb_log2=5, max_tb_log2=5, max_th_depth=2,
                       frames=3 if kind == "md5" else 2, hash_sei=kind, pcm=(3, 4, False), qp_delta_depth=1,
                       cb_qp_offset=-1, cr_qp_offset=2)
    data, pics, refs = g.stream()
    want = [np.dtype(np.uint8 if b == 8 else np.uint16) for b in (depths[0], depths[1], depths[1])]
    try:
        frames = decoder.decode_bytes(data)
        assert len(frames) == len(refs)
        for fr, (rec, out) in zip(frames, refs):
            assert fr.hash_ok is True and (fr.bit_depth, fr.bit_depth_chroma) == depths
            for c in range(3):
                assert fr.planes[c].dtype == want[c]
                np.testing.assert_array_equal(fr.planes[c], out[c])
        src, dst = tmp_path / "split.bin", tmp_path / "split.yuv"
        src.write_bytes(data)
        assert dec.main(["-b", str(src), "-o", str(dst)]) == 0
        raw = np.frombuffer(dst.read_bytes(), "<u2")            # one file sample width: 16-bit, values unscaled
        assert raw.size == len(refs) * 136 * 72 * 3 // 2
        np.testing.assert_array_equal(raw, np.concatenate([p.ravel().astype(np.uint16) for _, out in refs for p in out]))
        with pytest.raises(ValueError, match="unequal bit depths"):
            decoder.decode_bytes(data, hash_on="device")
        with pytest.raises(ValueError, match="unequal bit depths"):
            decoder.decode_bytes(data, export=recon_mod.ExportSpec.named("nv12"))
    finally:
        decoder.release_contexts()


def test_refusals(recon_mod):
    """What does not take unequal depths says so: the device-side output, the device-side hash, tiles and halo."""
    from p265_amd import halo, tiles
    params, pics, _ = S.case("narrow", 1)
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        for spec in (recon_mod.ExportSpec.named("nv12"), recon_mod.ExportSpec.named("rgb24", size=(32, 32))):
            with pytest.raises(_lib.P265RError) as ei:
                ctx.export(b, spec)
            assert ei.value.code == _lib.EINVAL
        d = recon_mod.ExportSpec.named("nv12").desc()            # the batch call itself, past the layout functions
        d.pitch[0] = d.pitch[1] = 72
        d.plane_off[1], d.frame_bytes = 72 * 40, 72 * 60
        assert ctx.lib.p265r_batch_export(ctx.handle, b.handle, ctypes.byref(d), ctypes.c_void_p(256), 1 << 20, None,
                                          len(pics)) == _lib.EINVAL
        with pytest.raises(_lib.P265RError) as ei:
            ctx.hash_async(b, _lib.HASH_MD5)
        assert ei.value.code == _lib.EUNSUPPORTED
        ctx.status(b)
        b.free()
    with pytest.raises(ValueError, match="unequal bit depths"):
        tiles.split(params, pics[0])
    with pytest.raises(ValueError, match="unequal bit depths"):
        halo.TileGrid(params, [0, 5], [0, 3])
