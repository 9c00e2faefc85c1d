"""Scaled grid export on the GPU (p265r_batch_export_grid_resized): every slot equals tests/grid_resize_ref.py applied
to ``ctx.download`` of the same batch -- which the parity suites pin to the oracle -- byte for byte, floats bit for
bit, and so do the bytes around the planes (every destination is pre-filled with 0xA5 and compared whole)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import grid_resize_ref as GRR
import mono as M
import planted_lf as PL
from p265_amd import _lib, hip, synth
from p265_amd import records as R
from test_gpu_grid import formats
from test_resize import PINNED_F16, PINNED_F32

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
FILTERS = ("nearest", "bilinear", "area")


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


class Target:
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


def ref_slot(tiles, f, bd, spec):
    return GRR.frame(tiles, f.rows, f.cols, (f.out_width, f.out_height), bd, spec.format, tuple(spec.size), spec.sample,
                     spec.matrix, spec.full_range, tuple(f.crop), f.orientation, spec.resize, spec.scale, spec.bias)


def call(ctx, batch, lay, gframes, ptr, nbytes, only=None, n=None):
    from p265_amd import recon
    arr = (ctypes.c_int32 * len(only))(*only) if only is not None else None
    return ctx.lib.p265r_batch_export_grid_resized(ctx.handle, batch.handle, ctypes.byref(lay.desc), ctypes.byref(lay.resize),
                                                   recon.grid_frames_c(gframes), len(gframes) if n is None else n,
                                                   ctypes.c_void_p(ptr), nbytes, arr)


def check(ctx, batch, spec, gframes, tiles, bd, target, only=None, offset=0, tweak=None):
    """Export into the pre-filled target (``offset`` bytes in) and compare the WHOLE buffer with the expectation: 0xA5
    everywhere but the planes' samples.  ``tiles``: per frame the downloaded planes of its tiles, in order."""
    from p265_amd import recon
    lay = ctx.export_layout(spec)
    if tweak is not None:
        tweak(lay)
    n = len(gframes)
    assert offset + lay.frame_bytes * n + GUARD <= target.nbytes
    target.fill()
    _lib.check(call(ctx, batch, lay, gframes, target.buf.ptr.value + offset, lay.frame_bytes * n, only),
               "p265r_batch_export_grid_resized")
    ctx.status(batch)
    got = target.read()
    want = np.full(target.nbytes, FILL, np.uint8)
    views = recon.DeviceFrames(0, lay.frame_bytes * n, lay, [lay.size] * n).host_views(want[offset:])
    for i, (f, t) in enumerate(zip(gframes, tiles)):
        ref = ref_slot(t, f, bd, spec)
        assert len(ref) == len(views[i])
        for k, (v, r) in enumerate(zip(views[i], ref)):
            assert v.shape == r.shape and v.dtype == r.dtype, (spec, f, i, k, v.shape, r.shape, v.dtype, r.dtype)
            v[...] = r
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s %s: %d bytes differ, first at %d of %d (slot bytes %d, plane offsets %s, pitches %s)"
                             % (spec, gframes, bad.size, bad[0], got.size, lay.frame_bytes, lay.plane_off, lay.pitch))


def decoded_tiles(ctx, params, n, seed, **kw):
    pics = [synth.make_picture(params, seed + k, deblocking=True, sao=True, **kw) for k in range(n)]
    b = ctx.upload(pics)
    ctx.run(b)
    return b, ctx.download(b)


def sized(spec, size, filt, **kw):
    return dataclasses.replace(spec, size=size, resize=filt, **kw)


# ---- 1. seams off every alignment -----------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_seams_off_every_alignment(recon_mod, bd):
    """2 x 3 tiles of 72 x 56 (chroma tiles 36 wide: no multiple of 8, a seam falls inside an 8-column load), item
    200 x 100, window 190 x 94 at (2, 2).  8 bits: every format, filter and orientation into 50 x 38; 10 bits: P010 and
    planar fp16, and bilinear up to 260 x 130."""
    params = R.make_params(pic_width=72, pic_height=56, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    crop = (2, 200 - 2 - 190, 2, 100 - 2 - 94)
    target = Target(4 * 3 * 272 * 136 + 4096)
    S = recon_mod.ExportSpec
    specs = formats(recon_mod, bd) if bd == 8 else [S(format="semiplanar", sample="msb16"),
                                                    S(format="rgb_planar", sample="f16", matrix="bt2020")]
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(ctx, params, 6, 6100 + bd)
            for spec0 in specs:
                for o in range(8):
                    f = recon_mod.GridFrame(2, 3, 200, 100, crop, o)
                    for filt in FILTERS:
                        check(ctx, b, sized(spec0, (50, 38), filt), [f], [src], bd, target)
                    if bd == 10:
                        check(ctx, b, sized(spec0, (260, 130), "bilinear"), [f], [src], bd, target)
            b.free()
    finally:
        target.free()


# ---- 2. a window above 2048 columns ---------------------------------------------------------------------------
@pytest.mark.parametrize("offset,odd_pitch", [(0, False), (4, False), (6, False), (0, True)])
def test_window_above_one_area_chunk(recon_mod, offset, odd_pitch):
    """1 x 3 tiles of 712 x 16, item 2130 x 16: the window spans two area chunks of 2048 columns, with a seam in each
    (712, 1424).  Area and bilinear to 300 x 8 and to 2130 x 16, packed uint8 and NV12, the destination 0 / 4 / 6
    bytes off a 16-byte boundary, and with a pitch that is no multiple of 16."""
    params = R.make_params(pic_width=712, pic_height=16, ctb_log2_size=4)
    target = Target(3 * 2136 * 16 + 4096)

    def tweak(lay):
        # every pitch 3 bytes longer (uint8 elements), the planes moved behind each other accordingly
        off = 0
        for k in range(lay.n_planes):
            rows = (lay.desc.plane_off[k + 1] - lay.desc.plane_off[k] if k + 1 < lay.n_planes
                    else lay.desc.frame_bytes - lay.desc.plane_off[k]) // lay.desc.pitch[k]
            lay.desc.pitch[k] += 3
            lay.desc.plane_off[k] = off
            off += lay.desc.pitch[k] * rows
        lay.desc.frame_bytes = off
        lay.plane_off = [int(lay.desc.plane_off[k]) for k in range(lay.n_planes)]
        lay.pitch = [int(lay.desc.pitch[k]) for k in range(lay.n_planes)]
        lay.frame_bytes = off

    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(ctx, params, 3, 6200)
            S = recon_mod.ExportSpec
            for spec0 in (S(format="rgb_packed", sample="u8", matrix="bt601"), S(format="semiplanar")):
                for size in ((300, 8), (2130, 16)):
                    for filt in ("area", "bilinear"):
                        for o in ((0, 4) if size[0] == 300 else (0, 2)):
                            f = recon_mod.GridFrame(1, 3, 2130, 16, (0, 0, 0, 0), o)
                            check(ctx, b, sized(spec0, size, filt), [f], [src], 8, target, offset=offset,
                                  tweak=tweak if odd_pitch else None)
            b.free()
    finally:
        target.free()


# ---- 3. the two identities -------------------------------------------------------------------------------------
def test_single_tile_equals_the_resized_export(recon_mod):
    """rows = cols = 1, orientation 0: byte for byte p265r_batch_export_resized with the crop the window implies."""
    params = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4)
    target = Target(4 * 3 * 80 * 48 + 256 * 140)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(ctx, params, 1, 6300)
            for kw in (dict(format="planar"), dict(format="semiplanar", pitch_align=256),
                       dict(format="rgb_packed", sample="u8"), dict(format="rgb_planar", sample="f32"),
                       dict(format="rgb_planar", sample="f16", pitch_align=64, scale=(2.0, 0.5, 3.0), bias=(0.1, 0.2, -1.0))):
                for size, filt in (((30, 18), "area"), ((30, 18), "nearest"), ((80, 44), "bilinear")):
                    target.fill()
                    plain = ctx.export(b, recon_mod.ExportSpec(crop=(2, 4 + 6, 2, 6 + 2), size=size, resize=filt, **kw),
                                       dst=target.buf.ptr.value, dst_bytes=target.nbytes - GUARD)
                    ctx.status(b)
                    want = target.read()
                    target.fill()
                    got_f = ctx.export_grid_resized(b, recon_mod.ExportSpec(size=size, resize=filt, **kw),
                                                    [recon_mod.GridFrame(1, 1, 66, 38, (2, 4, 2, 6))], dst=target.buf.ptr.value,
                                                    dst_bytes=target.nbytes - GUARD)
                    ctx.status(b)
                    got = target.read()
                    assert (got_f.layout.frame_bytes, got_f.layout.pitch, got_f.layout.plane_off) == \
                        (plain.layout.frame_bytes, plain.layout.pitch, plain.layout.plane_off)
                    assert np.any(want != FILL) and np.array_equal(got, want), (kw, size, filt)
            b.free()
    finally:
        target.free()


def test_nearest_at_the_window_size_equals_the_grid_export(recon_mod):
    """NEAREST with pw x ph = W x H, every orientation: byte for byte p265r_batch_export_grid with P265R_UP_NEAREST."""
    params = R.make_params(pic_width=40, pic_height=24, ctb_log2_size=4)
    target = Target(4 * 3 * 120 * 48 + 4096)
    crop = (2, 2, 4, 2)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(ctx, params, 6, 6350)
            for kw in (dict(format="planar"), dict(format="semiplanar"), dict(format="rgb_packed", sample="u8", matrix="bt601"),
                       dict(format="rgb_planar", sample="f16", full_range=True)):
                for o in range(8):
                    grid = recon_mod.GridSpec(2, 3, 100, 42, o)
                    target.fill()
                    g = ctx.export_grid(b, recon_mod.ExportSpec(crop=crop, upsample="nearest", **kw), grid,
                                        dst=target.buf.ptr.value, dst_bytes=target.nbytes - GUARD)
                    ctx.status(b)
                    want = target.read()
                    target.fill()
                    r = ctx.export_grid_resized(b, recon_mod.ExportSpec(size=grid.frame_size(crop), resize="nearest", **kw),
                                                [recon_mod.GridFrame(2, 3, 100, 42, crop, o)], dst=target.buf.ptr.value,
                                                dst_bytes=target.nbytes - GUARD)
                    ctx.status(b)
                    got = target.read()
                    assert (g.layout.frame_bytes, g.layout.pitch, g.layout.plane_off) == \
                        (r.layout.frame_bytes, r.layout.pitch, r.layout.plane_off)
                    assert np.any(want != FILL) and np.array_equal(got, want), (kw, o)
            b.free()
    finally:
        target.free()


# ---- 4. a ragged call -------------------------------------------------------------------------------------------
RAGGED = [(1, 1, 60, 50, (2, 4, 0, 2), 0), (2, 3, 190, 126, (0, 0, 0, 0), 1), (3, 2, 128, 180, (4, 2, 6, 4), 6),
          (2, 3, 150, 100, (10, 20, 2, 0), 3), (1, 1, 64, 64, (0, 6, 2, 0), 5)]


@pytest.mark.parametrize("filt", FILTERS)
def test_ragged_call_into_one_size(recon_mod, filt):
    """Five frames of tiles 64 x 64 -- 1 x 1, 2 x 3, 3 x 2, 2 x 3, 1 x 1; orientations 0, 1, 6, 3, 5; a window each -- out
    of a 21-picture batch listed in a shuffled order, ONE call into 48 x 32: every slot is the restatement's, the dense
    view is [5, 3, 32, 48], and the bytes before, between (pitch padding) and after the slots stay 0xA5."""
    params = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=4)
    gframes = [recon_mod.GridFrame(*f) for f in RAGGED]
    order = [int(v) for v in np.random.default_rng(64).permutation(21)][:20]        # one picture is not listed
    target = Target(64 + 5 * 3 * 32 * 128 + 4096)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(ctx, params, 21, 6400)
            tiles, at = [], 0
            for f in gframes:
                tiles.append([src[i] for i in order[at:at + f.tiles]])
                at += f.tiles
            spec = recon_mod.ExportSpec(format="rgb_planar", sample="f16", matrix="bt601", full_range=True, size=(48, 32),
                                        resize=filt, pitch_align=128, scale=(0.5, 0.25, 2.0), bias=(-1.0, 0.0, 3.0))
            check(ctx, b, spec, gframes, tiles, 8, target, only=order, offset=64)
            fr = ctx.export_grid_resized(b, spec, gframes, only=order)
            arr = fr.batch_array()
            assert arr.shape == (5, 3, 32, 48) and arr.strides == (3 * 32 * 128, 32 * 128, 128, 2)
            host = fr.to_host()
            for i, (f, t) in enumerate(zip(gframes, tiles)):
                for g, r in zip(host[i], ref_slot(t, f, 8, spec)):
                    np.testing.assert_array_equal(g.view(np.uint16), r.view(np.uint16))
            fr.free()
            # the YUV forms of the same call
            for spec in (recon_mod.ExportSpec(format="semiplanar", size=(48, 32), resize=filt, pitch_align=64),
                         recon_mod.ExportSpec(format="planar", size=(48, 32), resize=filt)):
                check(ctx, b, spec, gframes, tiles, 8, target, only=order, offset=16)
            b.free()
    finally:
        target.free()


# ---- 5. monochrome ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 12])
def test_monochrome_grid_odd_window_odd_size(recon_mod, bd):
    full = R.make_params(pic_width=40, pic_height=24, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = [M.to_mono(synth.make_picture(full, 6500 + bd + k, deblocking=True, sao=True)) for k in range(4)]
    target = Target(4 * 3 * 80 * 48 + 4096)
    try:
        with recon_mod.ReconContext(M.mono_params(full)) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = [[p[0]] for p in ctx.download(b)]
            S = recon_mod.ExportSpec
            for o in range(8):
                f = recon_mod.GridFrame(2, 2, 77, 45, (1, 3, 3, 1), o)                  # a 73 x 41 window
                for filt in FILTERS:
                    check(ctx, b, S(format="planar", size=(31, 17), resize=filt), [f], [src], bd, target)
                    check(ctx, b, S(format="rgb_packed", sample="u8", size=(31, 17), resize=filt), [f], [src], bd, target)
                check(ctx, b, S(format="rgb_planar", sample="f32", size=(31, 17), resize="area"), [f], [src], bd, target)
                check(ctx, b, S(format="semiplanar", size=(30, 16), resize="bilinear"),
                      [recon_mod.GridFrame(2, 2, 77, 45, (2, 1, 2, 1), o)], [src], bd, target)
            b.free()
    finally:
        target.free()


# ---- 6. P265R_RS_NORM -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample,bd", [("f32", 8), ("f16", 12)])
def test_normalised_float_outputs_through_a_grid(recon_mod, sample, bd):
    """The pinned triples of tests/test_resize.py -- values at which a fused multiply-add would differ from two rounded
    operations -- planted through PCM tiles (full range, grey chroma: R = G = B = Y) of a 2 x 2 grid."""
    w, h = 48, 32
    dt = np.uint16 if bd > 8 else np.uint8
    if bd == 8:
        vals, sc0, bi0 = (PINNED_F32[0],), PINNED_F32[1], PINNED_F32[2]
    else:
        vals, sc0, bi0 = PINNED_F16
    rng = np.random.default_rng(66 + bd)
    grey = np.full((h // 2, w // 2), 1 << (bd - 1), dt)
    planes_list = []
    for t in range(4):
        Y = rng.integers(0, 1 << bd, (h, w)).astype(dt)
        for k, v in enumerate(vals):
            Y[3 + k + t, 5:9] = v
        planes_list.append([Y, grey, grey])
    pcm = PL.params_of(bd, 4, "a", False, w, h)
    pics = []
    for planes in planes_list:
        sp = PL.Spec(bd, 4, 16, w, h)
        sp.dbk[:] = False
        pics.append(PL.build(sp, planes, "a", params=pcm))
    scale = (float(sc0), float(np.float32(1 / (((1 << bd) - 1) * 0.224))), float(np.float32(1 / (((1 << bd) - 1) * 0.225))))
    bias = (float(bi0), float(np.float32(-0.456 / 0.224)), float(np.float32(-0.406 / 0.225)))
    target = Target(4 * 3 * 2 * w * 2 * h + 4096)
    try:
        with recon_mod.ReconContext(pcm) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            np.testing.assert_array_equal(src[0][0], planes_list[0][0])
            for fmt in ("rgb_planar", "rgb_packed"):
                for size, filt, o in (((96, 64), "nearest", 0), ((64, 96), "nearest", 1), ((96, 64), "bilinear", 6),
                                      ((40, 24), "area", 0), ((24, 40), "area", 7)):
                    spec = recon_mod.ExportSpec(format=fmt, sample=sample, matrix="bt709", full_range=True, size=size, resize=filt,
                                                scale=scale, bias=bias)
                    f = recon_mod.GridFrame(2, 2, 96, 64, (0, 0, 0, 0), o)
                    if filt == "nearest":
                        ints = ref_slot(src, f, bd, dataclasses.replace(spec, sample="native", scale=None, bias=None))
                        r = ints[0] if fmt == "rgb_planar" else ints[0][..., 0]
                        assert all((r == v).any() for v in vals)         # the planted values reach channel 0
                    check(ctx, b, spec, [f], [src], bd, target)
            b.free()
    finally:
        target.free()


# ---- 7. ordering ------------------------------------------------------------------------------------------------
def test_ordered_behind_two_runs_of_a_pipelined_context(recon_mod):
    """run, run, export with no sync in between on a depth-2 pipeline: the slots are those of the batch's last run (a
    second batch on the other lane keeps the device busy beside it)."""
    params = R.make_params(pic_width=64, pic_height=48, ctb_log2_size=4)
    spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", size=(50, 36), resize="area")
    gframes = [recon_mod.GridFrame(2, 2, 120, 90, (0, 0, 0, 0), 1)]
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        first = [synth.make_picture(params, 6700 + k, deblocking=True) for k in range(4)]
        other = [synth.make_picture(params, 6750 + k, deblocking=True) for k in range(4)]
        b1, b2 = ctx.upload(first), ctx.upload(other)
        ctx.run(b1)
        ctx.run(b2)
        ctx.run(b1)
        fr = ctx.export_grid_resized(b1, spec, gframes)
        got = fr.to_host()[0]
        src = ctx.download(b1)
        for g, r in zip(got, ref_slot(src, gframes[0], 8, spec)):
            np.testing.assert_array_equal(g, r)
        assert got[0].shape == (36, 50, 3)
        fr.free()
        b1.free()
        b2.free()


# ---- 8. refusals ------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_batch_launch_nothing(recon_mod):
    big = R.make_params(pic_width=64, pic_height=48, ctb_log2_size=4)
    pics = [synth.make_picture(big, 6800 + k) for k in range(4)]
    small = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(48, 48)))
    odd = synth.make_picture(small, 6810)
    odd.size = (48, 48)
    target = Target(4 * 3 * 64 * 48)
    GF = recon_mod.GridFrame
    try:
        with recon_mod.ReconContext(big) as ctx:
            b = ctx.upload(pics + [odd])
            lay = ctx.export_layout(recon_mod.ExportSpec(format="rgb_packed", sample="u8", size=(64, 48), resize="area"))
            ptr = target.buf.ptr.value
            two = [GF(2, 2, 128, 96)]

            def rc(idx, gframes=two, nbytes=None, p=ptr, n=None):
                return call(ctx, b, lay, gframes, p, lay.frame_bytes * len(gframes) if nbytes is None else nbytes, idx, n)

            assert rc([0, 1, 2, 3]) == _lib.ESTATE                       # never run
            ctx.run(b)
            target.fill()
            assert rc([0, 1, 2, 4]) == _lib.EINVAL                       # pictures of differing own sizes
            assert rc([0, 1, 2, 2]) == _lib.EINVAL                       # a picture listed twice
            assert rc([0, 1, 2, 5]) == _lib.EINVAL                       # outside the batch
            assert rc(None) == _lib.EINVAL                               # NULL: 4 tiles do not account for 5 pictures
            assert rc([0, 1, 2, 3, 0, 1, 2, 3], gframes=two * 2) == _lib.EINVAL
            assert rc([0, 1, 2, 3], n=0) == _lib.EINVAL and rc([0, 1, 2, 3], n=65536) == _lib.EINVAL
            assert rc([0, 1, 2, 3], nbytes=lay.frame_bytes - 1) == _lib.ERANGE
            host = np.zeros(lay.frame_bytes, np.uint8)
            assert rc([0, 1, 2, 3], p=host.ctypes.data) == _lib.EINVAL
            assert rc([0, 1, 2, 3], gframes=[GF(2, 2, 128, 96, (0, 0, 0, 0), 8)]) == _lib.EINVAL     # orientation above 7
            assert rc([0, 1, 2, 3], gframes=[GF(2, 2, 128, 96, (0, 66, 0, 0))]) == _lib.EINVAL      # area: ow above W
            # area against the PRE-TURN size: a 128 x 60 window takes 64 x 48, but turned it would have to give 48 x 64
            assert rc([0, 1, 2, 3], gframes=[GF(2, 2, 128, 96, (0, 0, 0, 36), 1)]) == _lib.EINVAL
            assert rc([0, 1, 2, 3], gframes=[GF(2, 2, 127, 96)]) == _lib.EINVAL                       # an odd window, 4:2:0
            # the last frame of three fails (area: 46 rows for 48): nothing of the first two is written
            assert rc([0, 1, 2], gframes=[GF(1, 1, 64, 48), GF(1, 1, 64, 48), GF(1, 1, 64, 46)]) == _lib.EINVAL
            ctx.status(b)
            assert np.all(target.read() == FILL)
            assert rc([3, 1, 2, 0]) == _lib.OK
            ctx.status(b)
            b.free()
    finally:
        target.free()


def test_unequal_depths_are_unsupported(recon_mod):
    """A split_bit_depth context of unequal depths: P265R_EUNSUPPORTED from the batch call itself, nothing launched."""
    import split_cases as SC
    params, pics, _ = SC.case("narrow", 1)
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        d = recon_mod.ExportSpec.named("rgb24").desc()
        w, h = int(params["pic_width"]), int(params["pic_height"])
        d.pitch[0], d.frame_bytes = 3 * 16, 3 * 16 * 16
        rs = recon_mod.ExportSpec.named("rgb24", size=(16, 16)).resize_desc()
        fr = recon_mod.grid_frames_c([recon_mod.GridFrame(1, 1, w, h)] * len(pics))
        assert ctx.lib.p265r_batch_export_grid_resized(ctx.handle, b.handle, ctypes.byref(d), ctypes.byref(rs), fr, len(pics),
                                                       ctypes.c_void_p(256), 1 << 20, None) == _lib.EUNSUPPORTED
        ctx.status(b)
        b.free()
