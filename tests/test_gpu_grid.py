"""Grid export on the GPU (p265r_batch_export_grid): every frame equals tests/grid_ref.py applied to ``ctx.download`` of
the same batch -- which the parity suites pin to the oracle -- bit for bit, floats and the bytes around the planes
included (every destination is pre-filled with 0xA5 and compared whole)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import grid_ref as GR
import mono as M
from p265_amd import _lib, hip, synth
from p265_amd import records as R

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256


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


def ref_frame(tiles, grid, bd, spec):
    return GR.frame(tiles, grid.rows, grid.cols, (grid.out_width, grid.out_height), bd, spec.format, spec.sample,
                    spec.matrix, spec.full_range, spec.upsample, tuple(spec.crop), grid.orientation)


def check_grid(ctx, batch, spec, grid, frames, bd, target, only=None, offset=0, tweak=None):
    """Export into the pre-filled target (``offset`` bytes in) and compare the WHOLE buffer with the expectation:
    0xA5 everywhere but the planes' samples.  ``frames``: per frame the downloaded planes of its tiles, in order."""
    lay = ctx.grid_layout(spec, grid, batch.pics[0 if only is None else only[0]])
    if tweak is not None:
        tweak(lay)
    n = len(frames)
    assert offset + lay.frame_bytes * n + GUARD <= target.nbytes
    target.fill()
    arr = (ctypes.c_int32 * len(only))(*only) if only is not None else None
    _lib.check(ctx.lib.p265r_batch_export_grid(ctx.handle, batch.handle, ctypes.byref(lay.desc), ctypes.byref(lay.grid),
                                               ctypes.c_void_p(target.buf.ptr.value + offset), lay.frame_bytes * n, arr, n),
               "p265r_batch_export_grid")
    ctx.status(batch)
    got = target.read()
    want = np.full(target.nbytes, FILL, np.uint8)
    from p265_amd import recon
    views = recon.DeviceFrames(0, lay.frame_bytes * n, lay, [lay.size] * n).host_views(want[offset:])
    for i, tiles in enumerate(frames):
        ref = ref_frame(tiles, grid, bd, spec)
        assert len(ref) == len(views[i])
        for k, (v, r) in enumerate(zip(views[i], ref)):
            assert v.shape == r.shape and v.dtype == r.dtype, (spec, grid, i, k, v.shape, r.shape, v.dtype, r.dtype)
            v[...] = r
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s %s: %d bytes differ, first at %d of %d (slot bytes %d, plane offsets %s, pitches %s)"
                             % (spec, grid, bad.size, bad[0], got.size, lay.frame_bytes, lay.plane_off, lay.pitch))


def formats(recon_mod, bd):
    S = recon_mod.ExportSpec
    out = [S(format="planar"), S(format="semiplanar")]
    if bd > 8:
        out.append(S(format="semiplanar", sample="msb16"))
    out += [S(format="rgb_packed", sample="u8", upsample="nearest", matrix="bt601"),
            S(format="rgb_packed", sample="u8", upsample="bilinear", matrix="bt709", full_range=True),
            S(format="rgb_planar", sample="f16", upsample="bilinear", matrix="bt2020"),
            S(format="rgb_planar", sample="f32", upsample="nearest")]
    return out


def is_rgb(spec):
    return spec.format.startswith("rgb")


def decoded_tiles(recon_mod, ctx, params, n, seed, **kw):
    pics = [synth.make_picture(params, seed + k, deblocking=True, sao=True, **kw) for k in range(n)]
    b = ctx.upload(pics)
    ctx.run(b)
    return b, ctx.download(b)


@pytest.mark.parametrize("bd", [8, 10])
def test_basic_grid_every_format_and_orientation(recon_mod, bd):
    """2 x 3 tiles of 40 x 24 at CTB 16: the tile width is no multiple of 16 bytes, so every seam falls inside a lane's
    group.  RGB: 101 x 43 (odd, inside the last tile), crop (2, 3, 4, 1); YUV: 100 x 42, crop (2, 2, 4, 2)."""
    params = R.make_params(pic_width=40, pic_height=24, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    target = Target(4 * 3 * 120 * 48 + 4096)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(recon_mod, ctx, params, 6, 5100 + bd)
            for spec0 in formats(recon_mod, bd):
                rgb = is_rgb(spec0)
                spec = dataclasses.replace(spec0, crop=(2, 3, 4, 1) if rgb else (2, 2, 4, 2))
                for o in range(8):
                    grid = recon_mod.GridSpec(2, 3, 101 if rgb else 100, 43 if rgb else 42, o)
                    check_grid(ctx, b, spec, grid, [src], bd, target)
            b.free()
    finally:
        target.free()


def test_seam_picture_bilinear_taps_cross_the_seams(recon_mod):
    """Tiles whose chroma alternates 0 / max from tile to tile (recon-input pictures: the planes are given, only the
    filters run -- off here), RGB bilinear: the taps at every seam read the neighbouring tile."""
    params = R.make_params(pic_width=32, pic_height=32, ctb_log2_size=4)
    tiles = GR.seam_tiles(2, 3, 32, 32)
    with recon_mod.ReconContext(params) as ctx:
        pics = [dataclasses.replace(synth.make_picture(params, 5200 + k, sao=False), recon_input=t) for k, t in enumerate(tiles)]
        b = ctx.upload(pics)
        ctx.run(b)
        src = ctx.download(b)
        target = Target(3 * 96 * 64 + 1024)
        try:
            spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", upsample="bilinear", matrix="bt601", full_range=True)
            for o in (0, 3, 6):
                check_grid(ctx, b, spec, recon_mod.GridSpec(2, 3, 96, 64, o), [src], 8, target)
        finally:
            target.free()
        b.free()
    # (the decoded tiles are what was put in wherever no filter touched them: the teeth test uses the same picture)
    for s, t in zip(src, tiles):
        assert s[1].min() == s[1].max() == t[1][0, 0]


@pytest.mark.parametrize("align,odd_pitch", [(1, False), (256, False), (1, True)])
def test_wide_row_crosses_the_column_tile(recon_mod, align, odd_pitch):
    """1 x 3 tiles of 520 x 16 at 8 bits: a 1560-sample row is longer than one workgroup's 64 groups and than the
    transposing pass's 64-element tiles.  Also with pitch_align 256, and with a destination pitch that is no multiple
    of 16 (the element-wise store path)."""
    params = R.make_params(pic_width=520, pic_height=16, ctb_log2_size=4)
    target = Target(4 * 3 * 1560 * 16 + 256 * 1600 * 3 + 4096)

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
            b, src = decoded_tiles(recon_mod, ctx, params, 3, 5300)
            S = recon_mod.ExportSpec
            for spec in (S(format="planar", pitch_align=align), S(format="semiplanar", pitch_align=align),
                         S(format="rgb_packed", sample="u8", upsample="bilinear", pitch_align=align),
                         S(format="rgb_planar", sample="f16", pitch_align=align)):
                if odd_pitch and spec.sample == "f16":
                    continue                                     # (a pitch of 2-byte elements cannot be odd)
                for o in (0, 1, 2, 5):
                    check_grid(ctx, b, spec, recon_mod.GridSpec(1, 3, 1556, 16, o), [src], 8, target,
                               tweak=tweak if odd_pitch else None, offset=16 if odd_pitch else 0)
            b.free()
    finally:
        target.free()


def test_several_frames_shuffled_and_nothing_else_written(recon_mod):
    """Two 2 x 2 frames in one call out of a 9-picture batch, the pictures listed in a shuffled order: the unlisted
    picture influences nothing, and every byte outside the written planes is still 0xA5."""
    params = R.make_params(pic_width=48, pic_height=32, ctb_log2_size=4, bit_depth_luma=10, bit_depth_chroma=10)
    order = [7, 2, 5, 0, 3, 8, 1, 6]                             # picture 4 is not listed
    target = Target(2 * 4 * 3 * 96 * 64 + 4096)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(recon_mod, ctx, params, 9, 5400)
            frames = [[src[i] for i in order[:4]], [src[i] for i in order[4:]]]
            S = recon_mod.ExportSpec
            for spec in (S(format="semiplanar", sample="msb16", crop=(2, 0, 0, 2), pitch_align=64),
                         S(format="rgb_packed", sample="native", upsample="bilinear", crop=(0, 1, 2, 3))):
                for o in (0, 7):
                    check_grid(ctx, b, spec, recon_mod.GridSpec(2, 2, 90, 62, o), frames, 10, target, only=order)
            b.free()
    finally:
        target.free()


def test_single_tile_equals_the_plain_export(recon_mod):
    """1 x 1, orientation 0: byte for byte what p265r_batch_export writes under the crop the window implies -- both into
    the same pre-filled buffer, the whole buffer compared (padding and guard included)."""
    params = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4)
    target = Target(4 * 3 * 72 * 40 + 256 * 140)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b, src = decoded_tiles(recon_mod, ctx, params, 1, 5500)
            for kw in (dict(format="planar"), dict(format="semiplanar", pitch_align=256),
                       dict(format="rgb_packed", sample="u8", upsample="bilinear"), dict(format="rgb_planar", sample="f32"),
                       dict(format="rgb_planar", sample="f16", upsample="bilinear", pitch_align=64)):
                target.fill()
                plain = ctx.export(b, recon_mod.ExportSpec(crop=(2, 4 + 6, 2, 6 + 2), **kw), dst=target.buf.ptr.value,
                                   dst_bytes=target.nbytes - GUARD)
                ctx.status(b)
                want = target.read()
                target.fill()
                grid = ctx.export_grid(b, recon_mod.ExportSpec(crop=(2, 4, 2, 6), **kw), recon_mod.GridSpec(1, 1, 66, 38),
                                       dst=target.buf.ptr.value, dst_bytes=target.nbytes - GUARD)
                ctx.status(b)
                got = target.read()
                assert (grid.layout.frame_bytes, grid.layout.pitch, grid.layout.plane_off) == \
                    (plain.layout.frame_bytes, plain.layout.pitch, plain.layout.plane_off)
                assert np.any(want != FILL) and np.array_equal(got, want), kw
            b.free()
    finally:
        target.free()


@pytest.mark.parametrize("bd", [8, 12])
def test_monochrome_grid_odd_window_every_orientation(recon_mod, bd):
    full = R.make_params(pic_width=40, pic_height=24, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = [M.to_mono(synth.make_picture(full, 5600 + bd + k, deblocking=True, sao=True)) for k in range(4)]
    target = Target(4 * 3 * 80 * 48 + 4096)
    try:
        with recon_mod.ReconContext(M.mono_params(full)) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = [[p[0]] for p in ctx.download(b)]
            S = recon_mod.ExportSpec
            for o in range(8):
                check_grid(ctx, b, S(format="planar", crop=(1, 2, 3, 0)), recon_mod.GridSpec(2, 2, 77, 45, o), [src], bd, target)
            for o in (0, 3, 4):
                check_grid(ctx, b, S(format="rgb_packed", sample="u8", crop=(1, 2, 3, 0)), recon_mod.GridSpec(2, 2, 77, 45, o),
                           [src], bd, target)
                check_grid(ctx, b, S(format="semiplanar", crop=(2, 1, 2, 1)), recon_mod.GridSpec(2, 2, 77, 45, o), [src], bd,
                           target)
            b.free()
    finally:
        target.free()


def test_ordered_behind_two_runs_of_a_pipelined_context(recon_mod):
    """run, run, export with no sync in between on a depth-2 pipeline: the frame is that of the batch's last run (a
    second batch on the other lane keeps the device busy beside it)."""
    params = R.make_params(pic_width=64, pic_height=48, ctb_log2_size=4)
    spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", upsample="bilinear")
    grid = recon_mod.GridSpec(2, 2, 120, 90, 1)
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        first = [synth.make_picture(params, 5700 + k, deblocking=True) for k in range(4)]
        other = [synth.make_picture(params, 5750 + k, deblocking=True) for k in range(4)]
        b1, b2 = ctx.upload(first), ctx.upload(other)
        ctx.run(b1)
        ctx.run(b2)
        ctx.run(b1)
        fr = ctx.export_grid(b1, spec, grid)
        got = fr.to_host()[0]
        src = ctx.download(b1)
        for g, r in zip(got, ref_frame(src, grid, 8, spec)):
            np.testing.assert_array_equal(g, r)
        assert got[0].shape == (120, 90, 3)
        fr.free()
        b1.free()
        b2.free()


def test_refusals_that_need_a_batch_launch_nothing(recon_mod):
    big = R.make_params(pic_width=64, pic_height=48, ctb_log2_size=4)
    pics = [synth.make_picture(big, 5800 + k) for k in range(4)]
    small = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(48, 48)))
    odd = synth.make_picture(small, 5810)
    odd.size = (48, 48)
    target = Target(2 * 3 * 128 * 96)
    try:
        with recon_mod.ReconContext(big) as ctx:
            b = ctx.upload(pics + [odd])
            lay = ctx.grid_layout(recon_mod.ExportSpec(format="rgb_packed", sample="u8"), recon_mod.GridSpec(2, 2, 128, 96))
            dst = ctypes.c_void_p(target.buf.ptr.value)

            def rc(idx, n=1, nbytes=None, grid=None, ptr=dst):
                arr = (ctypes.c_int32 * len(idx))(*idx) if idx is not None else None
                return ctx.lib.p265r_batch_export_grid(ctx.handle, b.handle, ctypes.byref(lay.desc),
                                                       ctypes.byref(grid if grid is not None else lay.grid), ptr,
                                                       lay.frame_bytes * n if nbytes is None else nbytes, arr, n)

            assert rc([0, 1, 2, 3]) == _lib.ESTATE                       # never run
            ctx.run(b)
            target.fill()
            assert rc([0, 1, 2, 4]) == _lib.EINVAL                       # pictures of differing own sizes
            assert rc([0, 1, 2, 2]) == _lib.EINVAL                       # a picture listed twice
            assert rc([0, 1, 2, 5]) == _lib.EINVAL                       # outside the batch
            assert rc(None) == _lib.EINVAL                               # 5 pictures are no whole number of 2 x 2 frames
            assert rc([0, 1, 2, 3, 0, 1, 2, 3], n=2) == _lib.EINVAL
            # n_frames * rows * cols above 65535 (refused before the list is read), and a NULL list whose n_frames does
            # not account for the whole batch
            assert rc([0, 1, 2, 3], n=16384) == _lib.EINVAL
            one = recon_mod.GridSpec(1, 1, 64, 48).desc()
            assert rc(None, n=4, grid=one) == _lib.EINVAL and rc(None, n=6, grid=one) == _lib.EINVAL
            assert rc([0, 1, 2, 3], nbytes=lay.frame_bytes - 1) == _lib.ERANGE
            host = np.zeros(lay.frame_bytes, np.uint8)
            assert rc([0, 1, 2, 3], ptr=ctypes.c_void_p(host.ctypes.data)) == _lib.EINVAL
            g = recon_mod.GridSpec(2, 2, 128, 96, 8).desc()
            assert rc([0, 1, 2, 3], grid=g) == _lib.EINVAL               # orientation above 7
            ctx.status(b)
            assert np.all(target.read() == FILL)
            assert rc([3, 1, 2, 0]) == _lib.OK
            ctx.status(b)
            b.free()
    finally:
        target.free()


def test_unequal_depths_are_unsupported(recon_mod):
    """A split_bit_depth context of unequal depths: P265R_EUNSUPPORTED from the batch call itself, nothing launched."""
    import split_cases as S
    params, pics, _ = S.case("narrow", 1)
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        d = recon_mod.ExportSpec.named("rgb24").desc()
        w, h = int(params["pic_width"]), int(params["pic_height"])
        d.pitch[0], d.frame_bytes = 3 * w, 3 * w * h
        g = recon_mod.GridSpec(1, 1, w, h).desc()
        assert ctx.lib.p265r_batch_export_grid(ctx.handle, b.handle, ctypes.byref(d), ctypes.byref(g), ctypes.c_void_p(256),
                                               1 << 20, None, len(pics)) == _lib.EUNSUPPORTED
        with pytest.raises(_lib.P265RError) as ei:
            ctx.grid_layout(recon_mod.ExportSpec.named("rgb24"), recon_mod.GridSpec(1, 1, w, h))
        assert ei.value.code == _lib.EUNSUPPORTED
        ctx.status(b)
        b.free()
