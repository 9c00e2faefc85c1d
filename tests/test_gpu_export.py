"""Device-side output on the GPU (p265r_batch_export): every export equals tests/export_ref.py applied to
``ctx.download`` of the same batch -- which the parity suites pin to the oracle -- bit for bit, floats and the
bytes around the planes included (every destination is pre-filled with 0xA5 and compared whole)."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import export_ref as X
from oracle import c_oracle
from p265_amd import _lib, hip, synth
from p265_amd import records as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 256                     # bytes behind the last slot that must stay untouched too


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


# every legal (format, sample) pair; RGB also by upsampling
YUV = [("planar", "native"), ("planar", "msb16"), ("semiplanar", "native"), ("semiplanar", "msb16")]
RGB = [(f, s, u) for f in ("rgb_planar", "rgb_packed") for s in ("native", "u8", "f16", "f32") for u in ("nearest", "bilinear")]
COLOUR = [(m, fr) for m in X.MATRICES for fr in (False, True)]


def specs_for(recon_mod, bd):
    """ExportSpecs of every legal pair at this bit depth; the k-th RGB one at colour (k + depth) mod 6, so each
    matrix x range occurs at every depth."""
    out = [recon_mod.ExportSpec(format=f, sample=s) for f, s in YUV if not (s == "msb16" and bd == 8)]
    for k, (f, s, u) in enumerate(RGB):
        m, fr = COLOUR[(k + bd // 2) % 6]
        out.append(recon_mod.ExportSpec(format=f, sample=s, upsample=u, matrix=m, full_range=fr))
    return out


def ref_planes(planes, bd, spec):
    return X.export(planes, bd, spec.format, spec.sample, spec.matrix, spec.full_range, spec.upsample, tuple(spec.crop))


class Target:
    """A device buffer pre-filled with 0xA5 and the expectation of its bytes."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes) + GUARD
        self.buf = hip.DeviceBuffer(self.nbytes)

    def fill(self):
        hip.check(hip.lib().hipMemset(self.buf.ptr, FILL, self.nbytes), "hipMemset")
        hip.synchronize()

    def read(self):
        host = np.empty(self.nbytes, np.uint8)
        hip.check(hip.lib().hipMemcpy(host.ctypes.data, self.buf.ptr, self.nbytes, hip.D2H), "hipMemcpy")
        return host

    def free(self):
        self.buf.free()


def check_export(ctx, batch, spec, sources, bd, target, only=None, refs=None):
    """Export into the pre-filled target and compare the WHOLE buffer with the expectation built on the host:
    0xA5 everywhere but the planes' samples.  ``sources``: the downloaded planes per exported slot."""
    lay = ctx.export_layout(spec)
    n = len(sources)
    assert lay.frame_bytes * n + GUARD <= target.nbytes
    target.fill()
    fr = ctx.export(batch, spec, dst=target.buf.ptr.value, dst_bytes=lay.frame_bytes * n, only=only)
    ctx.status(batch)
    got = target.read()
    want = np.full(target.nbytes, FILL, np.uint8)
    views = fr.host_views(want)
    for i, src in enumerate(sources):
        ref = refs[i] if refs is not None else ref_planes(src, bd, spec)
        assert len(ref) == len(views[i])
        for k, (v, r) in enumerate(zip(views[i], ref)):
            assert v.shape == r.shape and v.dtype == r.dtype, (spec, i, k, v.shape, r.shape)
            v[...] = r
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d bytes differ, first at %d of %d (slot bytes %d, plane offsets %s, pitches %s)"
                             % (spec, bad.size, bad[0], got.size, lay.frame_bytes, lay.plane_off, lay.pitch))
    return fr


def crops_of(w, h):
    return [(0, 0, 0, 0),
            (2, 0, 0, 0),               # source rows 2 bytes (samples) off alignment
            (6, 10, 2, 4),
            (16, 8, 8, 8),
            (w - 6, 4, h - 4, 2)]       # the largest crop: a 2 x 2 picture is left


# 72x40, 136x72: rows shorter than one wave's span, a partial last group; 520x40, 2008x72: rows over several
# workgroups; 1032x40: 8 samples past the column tile of a workgroup (64 lanes x 16 samples = 1024 for 1-byte
# output, 2 x 512 + 8 for the 8-sample groups) and, at 40 rows, past no row tile (4 rows) -- 72 - 2 - 4 = 66 rows
# of the (6, 10, 2, 4) crop leave a partial row tile
SIZES = [(72, 40), (136, 72), (520, 40), (2008, 72), (1032, 40)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ctb_log2", [4, 6])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_format_crop_and_pitch(recon_mod, w, h, ctb_log2, bd):
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, bit_depth_luma=bd, bit_depth_chroma=bd)
    pic = synth.make_picture(params, 4200 + w + ctb_log2 + bd, perf=True, deblocking=True, sao=True)
    target = Target(4 * 3 * w * h + 256 * (3 * h + 8))
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload([pic])
            ctx.run(b)
            src = ctx.download(b)
            for spec0 in specs_for(recon_mod, bd):
                for crop in crops_of(w, h):
                    spec = dataclasses.replace(spec0, crop=crop)
                    refs = [ref_planes(src[0], bd, spec)]
                    for align in (1, 256):
                        check_export(ctx, b, dataclasses.replace(spec, pitch_align=align), src, bd, target, refs=refs)
            b.free()
    finally:
        target.free()


def _ragged(recon_mod, bd=8, ctb_log2=5):
    big = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=ctb_log2, bit_depth_luma=bd, bit_depth_chroma=bd)
    sizes = [(264, 200), (128, 72), (200, 136), (264, 64), (32, 200), (96, 200)]
    pics = []
    for k, (w, h) in enumerate(sizes):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 8800 + 3 * k + bd, perf=bool(k % 2), deblocking=True)
        pic.size = (w, h)
        pics.append(pic)
    return big, pics


SOME = [dict(format="semiplanar", sample="native"), dict(format="planar", sample="native"),
        dict(format="rgb_packed", sample="u8", upsample="bilinear", matrix="bt601"),
        dict(format="rgb_planar", sample="f16", upsample="nearest", matrix="bt2020", full_range=True)]


@pytest.mark.parametrize("bd", [8, 10])
def test_ragged_batch_cropped_per_picture(recon_mod, bd):
    """Six picture sizes in one batch: the crop is relative to each picture's own size, the slots share the
    layout of the context's (largest) size."""
    big, pics = _ragged(recon_mod, bd)
    target = Target(6 * 4 * 3 * 264 * 200)
    try:
        with recon_mod.ReconContext(big) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            for kw in SOME:
                for crop, align in (((2, 4, 2, 6), 1), ((0, 0, 0, 0), 256), ((16, 8, 8, 8), 1)):
                    check_export(ctx, b, recon_mod.ExportSpec(crop=crop, pitch_align=align, **kw), src, bd, target)
            b.free()
    finally:
        target.free()


def test_subset_in_the_order_given(recon_mod):
    big, pics = _ragged(recon_mod)
    target = Target(2 * 4 * 3 * 264 * 200)
    try:
        with recon_mod.ReconContext(big) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            for kw in SOME:
                fr = check_export(ctx, b, recon_mod.ExportSpec(crop=(2, 0, 0, 2), **kw), [src[4], src[1]], 8, target, only=[4, 1])
                assert fr.sizes == [(32, 200), (128, 72)]
            b.free()
    finally:
        target.free()


def test_export_is_ordered_behind_its_own_batch_on_a_pipelined_context(recon_mod):
    """Run, export, then run another batch on the other lane: the export holds the first batch's frames."""
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    first = [synth.make_picture(params, 9100 + k, deblocking=True) for k in range(3)]
    other = [synth.make_picture(params, 9200 + k, deblocking=True) for k in range(3)]
    spec = recon_mod.ExportSpec(format="semiplanar", crop=(2, 2, 0, 2))
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        b1, b2 = ctx.upload(first), ctx.upload(other)
        ctx.run(b1)
        fr = ctx.export(b1, spec)                    # its own buffer
        ctx.run(b2)
        ctx.run(b1)                                  # (the same records: the same planes again)
        got = fr.to_host()
        src = ctx.download(b1)
        src2 = ctx.download(b2)
        for i in range(3):
            for g, r in zip(got[i], ref_planes(src[i], 8, spec)):
                np.testing.assert_array_equal(g, r)
            assert not np.array_equal(got[i][0], ref_planes(src2[i], 8, spec)[0])
        a = fr.plane(2, 1).__cuda_array_interface__
        assert a["data"][0] == fr.ptr + 2 * fr.layout.frame_bytes + fr.layout.plane_off[1] and a["shape"] == (35, 66, 2)
        fr.free()
        b1.free()
        b2.free()


def test_sanity_frame_as_nv12_equals_the_c_oracle(recon_mod):
    from p265_amd import bitstream
    dec = bitstream.decode_stream(open(os.path.join(GOLDEN, "sanity.bin"), "rb").read())
    params, pic = dec[0].params, dec[0].picture
    ref = c_oracle.decode(params, [pic], scaling=dec[0].scaling)[0][1]
    with recon_mod.ReconContext(params, scaling=dec[0].scaling) as ctx:
        b = ctx.upload([pic])
        ctx.run(b)
        fr = ctx.export(b, recon_mod.ExportSpec(format="semiplanar"))
        y, c = fr.to_host()[0]
        fr.free()
        b.free()
    np.testing.assert_array_equal(y, ref[0])
    np.testing.assert_array_equal(c, np.stack([ref[1], ref[2]], axis=-1))


def _nv12_bytes(frames):
    out = []
    for f in frames:
        y, cb, cr = f.cropped()
        out.append(np.ascontiguousarray(y).tobytes() + np.ascontiguousarray(np.stack([cb, cr], axis=-1)).tobytes())
    return out


def test_decoder_end_to_end_nv12(recon_mod, tmp_path):
    """synth_1080p_4pic.bin through the decoder and the command line (the stream codes 1920 x 1080 with an empty
    conformance window: test_decoder_applies_the_conformance_window below has a real one)."""
    from p265_amd import decoder
    path = os.path.join(GOLDEN, "synth_1080p_4pic.bin")
    data = open(path, "rb").read()
    spec = recon_mod.ExportSpec.named("nv12")
    frames = decoder.decode_bytes(data, export=spec)                 # verification on: raises on a hash mismatch
    assert len(frames) == 4
    want = _nv12_bytes(frames)
    for f, w in zip(frames, want):
        assert f.hash_ok is True and f.planes is not None
        y, c = f.device.to_host()
        assert y.shape == (1080, 1920) and c.shape == (540, 960, 2)
        assert f.device.tobytes() == w
        assert f.device.planes[0].__cuda_array_interface__["shape"] == (1080, 1920)
    # without verification nothing but the exported frames comes back
    quiet = decoder.decode_bytes(data, export=spec, verify_hash=False)
    assert [f.planes for f in quiet] == [None] * 4
    assert [f.device.tobytes() for f in quiet] == want
    for f in quiet + frames:
        f.device.release()
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = tmp_path / "x.nv12"
    subprocess.run([sys.executable, "-m", "p265_amd.dec", "-b", path, "-o", str(out), "--format", "nv12"], check=True,
                   env=env, cwd=ROOT, timeout=120)
    assert out.read_bytes() == b"".join(want)
    # the default format is the host path: the bytes decoder.write_yuv writes
    out2, ref2 = tmp_path / "x.yuv", tmp_path / "ref.yuv"
    subprocess.run([sys.executable, "-m", "p265_amd.dec", "-b", path, "-o", str(out2), "--format", "i420"], check=True,
                   env=env, cwd=ROOT, timeout=120)
    decoder.write_yuv(decoder.decode_bytes(data), str(ref2))
    assert out2.read_bytes() == ref2.read_bytes()


def test_decoder_applies_the_conformance_window(recon_mod):
    """A generated stream with conf_win offsets (1, 2, 3, 1) chroma units = (2, 4, 6, 2) luma samples and a
    picture-hash SEI: with verification on the uncropped host planes pass their MD5, and every frame's device
    view is the restatement applied to them under the stream's own window -- NV12 and bilinear RGB."""
    import streamgen
    from p265_amd import decoder
    g = streamgen.StreamGen(78, hash_sei="md5", conf_window=(1, 2, 3, 1), width=136, height=104, frames=3)
    data, pics = g.stream(planes_fn=lambda prm, pic, scaling=None: c_oracle.decode(prm, [pic], with_recon=False,
                                                                                   scaling=scaling)[0][1])
    for spec in (recon_mod.ExportSpec.named("nv12"), recon_mod.ExportSpec.named("rgb24", matrix="bt601", upsample="bilinear")):
        frames = decoder.decode_bytes(data, export=spec, batch=2)
        assert len(frames) == 3
        for f in frames:
            assert f.hash_ok is True and f.crop == (2, 4, 6, 2)
            want = ref_planes(f.planes, 8, dataclasses.replace(spec, crop=f.crop))
            got = f.device.to_host()
            assert got[0].shape[:2] == (104 - 8, 136 - 6)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
            f.device.release()


def _desc(ctx, recon_mod, **kw):
    return ctx.export_layout(recon_mod.ExportSpec(**kw)).desc


def test_refusals_launch_nothing(recon_mod):
    """Every refusal of p265r_batch_export that needs a batch; the target stays 0xA5 through all of them, and a
    good export on the same context succeeds afterwards."""
    params = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4, bit_depth_luma=10, bit_depth_chroma=10)
    pics = [synth.make_picture(params, 9300 + k, deblocking=True) for k in range(3)]
    target = Target(3 * 4 * 3 * 72 * 40)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            target.fill()
            lib, dst = ctx.lib, ctypes.c_void_p(target.buf.ptr.value)

            def rc(d, ptr=dst, nbytes=None, idx=None, n=3):
                arr = (ctypes.c_int32 * len(idx))(*idx) if idx is not None else None
                return lib.p265r_batch_export(ctx.handle, b.handle, ctypes.byref(d), ptr,
                                              3 * d.frame_bytes if nbytes is None else nbytes, arr, n)

            d = _desc(ctx, recon_mod, format="planar")                    # uint16: rows of 144, 72, 72 bytes
            for field, k, val in (("pitch", 0, 142), ("pitch", 1, 70), ("pitch", 2, 73), ("pitch", 0, 145),
                                  ("plane_off", 1, 1)):
                bad = _desc(ctx, recon_mod, format="planar")
                getattr(bad, field)[k] = val
                assert rc(bad) == _lib.EINVAL, (field, k, val)
            bad = _desc(ctx, recon_mod, format="planar")
            bad.plane_off[1] -= 2                                         # Cb starts inside Y
            assert rc(bad) == _lib.EINVAL
            bad = _desc(ctx, recon_mod, format="planar")
            bad.plane_off[2] = bad.plane_off[1]                           # Cr on Cb
            assert rc(bad) == _lib.EINVAL
            bad = _desc(ctx, recon_mod, format="planar")
            bad.frame_bytes -= 2                                          # smaller than a slot
            assert rc(bad) == _lib.EINVAL
            bad = _desc(ctx, recon_mod, format="planar")
            bad.crop_left = 3
            assert rc(bad) == _lib.EINVAL
            bad = _desc(ctx, recon_mod, format="planar")
            bad.sample = _lib.SMP_F16
            assert rc(bad) == _lib.EINVAL
            for idx in ([0, 3], [-1, 0], [1, 1], [0, 1, 2, 0]):
                assert rc(d, idx=idx, n=len(idx)) == _lib.EINVAL, idx
            host = np.zeros(3 * d.frame_bytes, np.uint8)
            assert rc(d, ptr=ctypes.c_void_p(host.ctypes.data)) == _lib.EINVAL      # a host pointer
            assert rc(d, nbytes=3 * d.frame_bytes - 1) == _lib.ERANGE               # one byte short
            assert rc(d, nbytes=2 * d.frame_bytes, idx=[2, 0], n=2) == _lib.OK      # (two slots do fit)
            ctx.status(b)
            target.fill()
            # a recon-input batch whose filters never ran has no output planes yet
            rb = ctx.upload([dataclasses.replace(pics[0], recon_input=src[0])])
            one = _desc(ctx, recon_mod, format="planar")
            assert lib.p265r_batch_export(ctx.handle, rb.handle, ctypes.byref(one), dst, one.frame_bytes, None, 1) == _lib.ESTATE
            ctx.status(b)
            assert np.all(target.read() == FILL)                          # nothing was launched
            ctx.run(rb)
            check_export(ctx, rb, recon_mod.ExportSpec(format="planar"), ctx.download(rb), 10, target)
            rb.free()
            # and the context still exports
            check_export(ctx, b, recon_mod.ExportSpec(format="semiplanar", sample="msb16"), src, 10, target)
            b.free()
    finally:
        target.free()
