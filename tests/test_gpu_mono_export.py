"""Device-side output and the end-to-end decoder for monochrome (4:0:0) pictures.

Export: every legal format x sample type of a monochrome batch equals the unmodified tests/export_ref.py given the
decoded Y and chroma planes of 1 << (BitDepth - 1) -- planar is its Y plane alone, semi-planar Y plus a grey CbCr
plane, RGB R = G = B -- the bytes around the planes included (tests/test_gpu_export.py check_export).  End to end:
tests/streamgen_mono.py streams through decoder.decode_bytes (hash on the host and on the device, NV12 export) and
the command line."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import export_ref as X
import mono as M
from oracle import c_oracle
from p265_amd import _lib, synth
from p265_amd import records as R
from streamgen_mono import StreamGenMono
from test_gpu_export import FILL, ROOT, Target, check_export, specs_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def mono_ref(y, bd, spec):
    """export_ref.export of (Y, grey, grey); planar keeps the Y plane alone.  Odd crops: the restatement slices the
    upsampled chroma by luma coordinates, and a constant plane is the same under any slicing."""
    h, w = y.shape
    planes = [y, M.grey({"bit_depth_luma": bd}, (h // 2, w // 2)), M.grey({"bit_depth_luma": bd}, (h // 2, w // 2))]
    if spec.format == "planar":
        l, r, t, b = spec.crop
        sh = 16 - bd if spec.sample == "msb16" else 0
        return [(y[t:h - b, l:w - r].astype(np.uint32) << sh).astype(X.sample_dtype(spec.sample, bd))]
    out = X.export(planes, bd, spec.format, spec.sample, spec.matrix, spec.full_range, spec.upsample, tuple(spec.crop))
    if spec.format in ("rgb_planar", "rgb_packed"):
        co = X.coefficients(spec.matrix, spec.full_range, bd, 8 if spec.sample == "u8" else bd)
        l, r, t, b = spec.crop
        g = np.clip((co[0] * (y[t:h - b, l:w - r].astype(np.int64) - co[5]) + 8192) >> 14, 0, (1 << co[7]) - 1)
        first = out[0][..., 0] if spec.format == "rgb_packed" else out[0]
        if spec.sample in ("f16", "f32"):
            g = (g.astype(np.float32) * np.float32(1 / (2 ** bd - 1))).astype(first.dtype)
        assert np.array_equal(first, g.astype(first.dtype))          # the issue's formula: R = G = B
    return out


def _batch(recon_mod, bd, lg=4, n=2, w=72, h=40):
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=lg, bit_depth_luma=bd, bit_depth_chroma=bd)
    full = [synth.make_picture(params, 7300 + bd + k, perf=True, deblocking=True, sao=True) for k in range(n)]
    want = [out[0] for _, out in c_oracle.decode(params, full, threads=4)]
    return M.mono_params(params), [M.to_mono(p) for p in full], want


@pytest.mark.parametrize("bd", [8, 10])
def test_every_format_sample_crop_and_pitch(recon_mod, bd):
    """72 x 40: every format x sample type legal at this depth (RGB under both upsampling values, which change nothing
    here); the crop (1, 3, 1, 1) for planar and RGB, (2, 4, 2, 6) for all; tight and 256-aligned pitches."""
    pm, pics, want = _batch(recon_mod, bd)
    target = Target(2 * (4 * 3 * 72 * 40 + 256 * (3 * 40 + 8)))
    try:
        with recon_mod.ReconContext(pm) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            for i in range(2):
                np.testing.assert_array_equal(src[i][0], want[i])
            seen = set()
            for spec0 in specs_for(recon_mod, bd):
                crops = [(0, 0, 0, 0), (2, 4, 2, 6)] + ([(1, 3, 1, 1)] if spec0.format != "semiplanar" else [])
                for crop in crops:
                    for align in (1, 256):
                        spec = dataclasses.replace(spec0, crop=crop, pitch_align=align)
                        lay = ctx.export_layout(spec)
                        assert lay.n_planes == {"planar": 1, "semiplanar": 2, "rgb_planar": 3, "rgb_packed": 1}[spec.format]
                        refs = [mono_ref(want[i], bd, spec) for i in range(2)]
                        check_export(ctx, b, spec, src, bd, target, refs=refs)
                        seen.add((spec.format, spec.sample))
            assert len(seen) == (10 if bd == 8 else 12)
            # the grey CbCr plane: 1 << (B - 1), shifted for MSB16
            fr = ctx.export(b, recon_mod.ExportSpec.named("nv12" if bd == 8 else "p010"))
            y, c = fr.to_host()[0]
            assert (c == ((1 << (bd - 1)) << (16 - bd if bd > 8 else 0))).all() and c.shape == (20, 36, 2)
            fr.free()
            b.free()
    finally:
        target.free()


def test_subset_and_ragged_batch(recon_mod):
    """Six picture sizes in a 3 x 3 CTB context, exported whole and as a ``pic_index`` subset in the order given; the
    crop is relative to each picture's own size."""
    ctb, bd = 32, 8
    big = R.make_params(pic_width=3 * ctb, pic_height=3 * ctb, ctb_log2_size=5)
    sizes = [(96, 96), (72, 40), (8, 96), (96, 8), (32, 32), (56, 88)]
    full = []
    for k, (w, h) in enumerate(sizes):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 7400 + k, perf=bool(k % 2), deblocking=True)
        pic.size = (w, h)
        full.append(pic)
    want = [out[0] for _, out in c_oracle.decode(big, full, threads=4)]
    target = Target(6 * 4 * 3 * 96 * 96)
    try:
        with recon_mod.ReconContext(M.mono_params(big)) as ctx:
            b = ctx.upload([M.to_mono(p) for p in full])
            ctx.run(b)
            src = ctx.download(b)
            for kw in (dict(format="planar", crop=(1, 2, 3, 0)), dict(format="semiplanar", crop=(2, 0, 0, 2), pitch_align=64),
                       dict(format="rgb_packed", sample="u8", crop=(3, 1, 1, 1)),
                       dict(format="rgb_planar", sample="f32", matrix="bt2020", full_range=True, crop=(0, 1, 0, 5))):
                spec = recon_mod.ExportSpec(**kw)
                check_export(ctx, b, spec, src, bd, target, refs=[mono_ref(y, bd, spec) for y in want])
                fr = check_export(ctx, b, spec, [src[4], src[1]], bd, target, only=[4, 1],
                                  refs=[mono_ref(want[4], bd, spec), mono_ref(want[1], bd, spec)])
                assert fr.sizes == [(32, 32), (72, 40)]
            b.free()
    finally:
        target.free()


def test_refusals_launch_nothing(recon_mod):
    pm, pics, want = _batch(recon_mod, 10)
    target = Target(2 * 4 * 3 * 72 * 40)
    try:
        with recon_mod.ReconContext(pm) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            target.fill()
            lib, dst = ctx.lib, ctypes.c_void_p(target.buf.ptr.value)

            def rc(d, nbytes=None):
                return lib.p265r_batch_export(ctx.handle, b.handle, ctypes.byref(d), dst,
                                              2 * d.frame_bytes if nbytes is None else nbytes, None, 2)

            nv = ctx.export_layout(recon_mod.ExportSpec(format="semiplanar", sample="msb16")).desc
            for f in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
                bad = ctx.export_layout(recon_mod.ExportSpec(format="semiplanar", sample="msb16")).desc
                setattr(bad, f, 1)
                assert rc(bad) == _lib.EINVAL, f                        # an odd crop on semi-planar
            assert rc(nv, nbytes=2 * nv.frame_bytes - 1) == _lib.ERANGE    # dev_dst one byte short
            pl = ctx.export_layout(recon_mod.ExportSpec(format="planar", crop=(1, 3, 1, 1))).desc
            assert rc(pl, nbytes=pl.frame_bytes) == _lib.ERANGE
            bad = ctx.export_layout(recon_mod.ExportSpec(format="planar")).desc
            bad.pitch[0] -= 2
            assert rc(bad) == _lib.EINVAL
            bad = ctx.export_layout(recon_mod.ExportSpec(format="rgb_packed", sample="u8")).desc
            bad.matrix = 3
            assert rc(bad) == _lib.EINVAL
            ctx.status(b)
            assert np.all(target.read() == FILL)                          # nothing was launched
            spec = recon_mod.ExportSpec(format="planar", crop=(1, 3, 1, 1))
            check_export(ctx, b, spec, src, 10, target, refs=[mono_ref(y, 10, spec) for y in want])
            b.free()
    finally:
        target.free()


# ---- end to end --------------------------------------------------------------------------------------------------------

def _luma(prm, pic, scaling=None):
    """The expected planes of a monochrome picture: Y of the C oracle's decode of the same records under
    chroma_format_idc 1 (its chroma planes, predicted from nothing, are dropped)."""
    kw = R.params_dict(prm)
    kw["chroma_format_idc"] = 1
    return c_oracle.decode(R.make_params(**kw), [pic], with_recon=False, scaling=scaling)[0][1][:1]


STREAMS = {
    "bd8_ctb16_tiles_slices_md5": dict(tiles=(2, 2), slices=[(0, False), (10, False), (20, True)], hash_sei="md5", frames=3,
                                       conf_window=(1, 3, 2, 5), width=136, height=104, pcm=(3, 4, True)),
    "bd10_ctb32_wpp_crc": dict(bit_depth=10, sps_bit_depth_chroma=8, ctb_log2=5, max_tb_log2=5, max_th_depth=2, wpp=True,
                               hash_sei="crc", frames=2, qp_delta_depth=1, width=136, height=72, conf_window=(2, 0, 0, 4)),
    "bd8_checksum_reordered": dict(hash_sei="checksum", frames=4, poc_order=[0, 3, 1, 2], max_reorder=2, bypass=True),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_decode_bytes(recon_mod, name):
    """streamgen_mono streams whose SEI carries the hash of the oracle's luma: decoded with the hash checked on the
    host and on the device, and exported as NV12 / P010 with no plane coming back."""
    from p265_amd import decoder
    cfg = STREAMS[name]
    g = StreamGenMono(77 + len(name), **cfg)
    data, pics = g.stream(planes_fn=_luma)
    bd = g.bd
    expect = {poc: _luma(prm, pic)[0] for prm, pic, poc in pics}
    frames = decoder.decode_bytes(data, batch=2)                      # raises on a hash mismatch
    assert len(frames) == len(pics) and [f.poc for f in frames] == sorted(f.poc for f in frames)
    crop = tuple(cfg.get("conf_window", (0, 0, 0, 0)))
    for f in frames:
        assert f.hash_ok is True and len(f.planes) == 1 and f.crop == crop and f.bit_depth == bd
        np.testing.assert_array_equal(f.planes[0], expect[f.poc])
        (y,) = f.cropped()
        assert y.shape == (g.H - crop[2] - crop[3], g.W - crop[0] - crop[1])
    dev = decoder.decode_bytes(data, batch=2, hash_on="device")
    assert [f.hash_ok for f in dev] == [True] * len(pics)
    if crop[0] % 2 == 0 and crop[1] % 2 == 0 and crop[2] % 2 == 0 and crop[3] % 2 == 0:
        spec = recon_mod.ExportSpec.named("nv12" if bd == 8 else "p010")
        quiet = decoder.decode_bytes(data, batch=2, export=spec, hash_on="device")
        for f, ref in zip(quiet, frames):
            assert f.hash_ok is True and f.planes is None
            y, c = f.device.to_host()
            np.testing.assert_array_equal(y, ref.cropped()[0].astype(y.dtype) << (16 - bd if bd > 8 else 0))
            assert (c == ((1 << (bd - 1)) << (16 - bd if bd > 8 else 0))).all()
            f.device.release()
    else:
        with pytest.raises(_lib.P265RError):                           # an odd window: semi-planar keeps its even rule
            decoder.decode_bytes(data, batch=2, export=recon_mod.ExportSpec.named("nv12"))
        rgb = decoder.decode_bytes(data, batch=2, export=recon_mod.ExportSpec.named("rgb24"), hash_on="device")
        for f, ref in zip(rgb, frames):
            (px,) = f.device.to_host()
            want = mono_ref(ref.planes[0], bd, recon_mod.ExportSpec.named("rgb24", crop=crop))[0]
            np.testing.assert_array_equal(px, want)
            f.device.release()
    # a corrupted hash is reported
    bad = bytearray(data)
    k = data.rfind(b"\x00\x00\x00\x01\x50")                           # the last suffix SEI
    assert k > 0
    bad[k + 9] ^= 0x40
    with pytest.raises(decoder.HashMismatch):
        decoder.decode_bytes(bytes(bad), batch=2, hash_on="device")


def test_command_line(recon_mod, tmp_path):
    """``-o`` writes luma-only frames of the cropped size; ``--mono-output i420`` appends grey chroma; ``--format
    rgb24`` goes through the one-plane export."""
    g = StreamGenMono(91, hash_sei="md5", frames=3, conf_window=(1, 3, 2, 5), width=136, height=104, tiles=(2, 2))
    data, pics = g.stream(planes_fn=_luma)
    path = tmp_path / "mono.bin"
    path.write_bytes(data)
    w, h = 136 - 4, 104 - 7
    ys = [_luma(prm, pic)[0][2:104 - 5, 1:136 - 3] for prm, pic, _ in pics]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in [k for k in env if k.startswith("P265R_")]:
        del env[k]

    def run(*args):
        out = tmp_path / ("out" + "_".join(a.strip("-") for a in args))
        subprocess.run([sys.executable, "-m", "p265_amd.dec", "-b", str(path), "-o", str(out)] + list(args), check=True,
                       env=env, cwd=ROOT, timeout=120)
        return out.read_bytes()

    got = run()
    assert len(got) == 3 * w * h and got == b"".join(np.ascontiguousarray(y).tobytes() for y in ys)
    got = run("--mono-output", "i420")
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert len(got) == 3 * (w * h + 2 * cw * ch)
    frame = w * h + 2 * cw * ch
    for i, y in enumerate(ys):
        assert got[i * frame:i * frame + w * h] == np.ascontiguousarray(y).tobytes()
        assert got[i * frame + w * h:(i + 1) * frame] == bytes([128]) * (2 * cw * ch)
    got = run("--format", "rgb24", "--hash-on", "device")
    assert len(got) == 3 * 3 * w * h
    co = X.coefficients("bt709", False, 8, 8)
    grey = np.clip((co[0] * (ys[0].astype(np.int64) - co[5]) + 8192) >> 14, 0, 255).astype(np.uint8)
    assert got[:3 * w * h] == np.repeat(grey[..., None], 3, axis=-1).tobytes()
