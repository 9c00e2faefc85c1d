"""Scaled device-side output on the GPU (p265r_batch_export_resized): every export equals tests/resize_ref.py applied to
``ctx.download`` of the same batch, bit for bit, floats and the bytes around the planes included -- the whole-buffer
method of tests/test_gpu_export.py: the target is pre-filled with 0xA5 and compared whole, guard included.  With the
output size equal to the window, the nearest filter must equal the PLAIN export byte for byte."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import mono as M
import planted_lf as PL
import resize_ref as RR
from p265_amd import _lib, synth
from p265_amd import records as R
from test_gpu_export import COLOUR, FILL, GOLDEN, RGB, YUV, Target, _ragged, check_export
from test_resize import PINNED_F16, PINNED_F32

pytestmark = pytest.mark.gpu

FILTERS = RR.FILTERS
PAIRS = YUV + sorted({(f, s) for f, s, _ in RGB})


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def specs_for(recon_mod, bd):
    """ExportSpecs of every legal (format, sample) pair at this depth, the k-th RGB one at colour (k + depth) mod 6 as
    test_gpu_export.specs_for rotates them."""
    out = []
    for k, (f, s) in enumerate(PAIRS):
        if s == "msb16" and bd == 8:
            continue
        if f.startswith("rgb"):
            m, fr = COLOUR[(k + bd // 2) % 6]
            out.append(recon_mod.ExportSpec(format=f, sample=s, matrix=m, full_range=fr))
        else:
            out.append(recon_mod.ExportSpec(format=f, sample=s))
    return out


def half_chroma(spec, mono=False):
    return spec.format == "semiplanar" or (spec.format == "planar" and not mono)


def ref_of(src, bd, spec, cache=None):
    return RR.resize(src, bd, spec.format, spec.sample, spec.matrix, spec.full_range, tuple(spec.crop), tuple(spec.size),
                     spec.resize, spec.scale, spec.bias, cache=cache)


def even(v):
    return max(2, v & ~1)


def sizes_of(W, H):
    """(out_w, out_h, filters) for a W x H window."""
    both, gathered = FILTERS, ("nearest", "bilinear")
    out = [(W, H, both), (1, 1, both), (2, 2, both)]
    if W >= 2 and H >= 2:
        out.append((W // 2, H // 2, both))
    if (W, H) == (72, 40):
        out += [(34, 18, both), (31, 17, both), (100, 56, gathered)]
    else:
        out += [(even(W * 15 // 32), even(H * 7 // 16), both), (max(1, (W * 7 // 16) | 1), max(1, (H * 3 // 8) | 1), both),
                (even(W * 25 // 18), even(H * 7 // 5), gathered)]
    out.append((2 * W, 2 * H, gathered))
    out.append((even(W * 3 // 2), even(H // 2), ("bilinear",)))          # one axis up, the other down
    if W > 1000:
        out += [(520, 8, both), (16, 8, both)]        # a 64.5 : 1 box (one chunk of the area kernel's 2048 source columns:
                                                      # test_area_over_several_source_chunks has the wider source)
    seen, res = set(), []
    for w, h, fs in out:
        fs = tuple(f for f in fs if f != "area" or (w <= W and h <= H))
        if (w, h) not in seen and fs:
            seen.add((w, h))
            res.append((w, h, fs))
    return res


def crops_of(w, h):
    return [(0, 0, 0, 0), (2, 0, 0, 0), (6, 10, 2, 4), (w - 6, 4, h - 4, 2)]      # the last leaves 2 x 2


def run_matrix(recon_mod, ctx, b, src, bd, target, crops, specs, sizes_fn=sizes_of, aligns=(1, 256), mono=False):
    """Every spec x crop x output size x filter x pitch alignment; nearest at the window's own size against the plain
    export too.  Returns the number of exports checked."""
    n = 0
    caches = [{} for _ in src]                      # the filtered planes of each source, shared by the formats
    h, w = src[0][0].shape
    for crop in crops:
        W, H = w - crop[0] - crop[1], h - crop[2] - crop[3]
        for mw, mh, filters in sizes_fn(W, H):
            for spec0 in specs:
                if half_chroma(spec0, mono) and (mw % 2 or mh % 2):
                    continue
                if (crop[0] | crop[1] | crop[2] | crop[3]) & 1 and not (mono and spec0.format != "semiplanar"):
                    continue
                for filt in filters:
                    if filt == "area" and (mw > W or mh > H):
                        continue                                      # downscale only
                    spec = dataclasses.replace(spec0, crop=crop, size=(mw, mh), resize=filt)
                    refs = [ref_of(s, bd, spec, c) for s, c in zip(src, caches)]
                    for align in aligns:
                        check_export(ctx, b, dataclasses.replace(spec, pitch_align=align), src, bd, target, refs=refs)
                        n += 1
                    if filt == "nearest" and (mw, mh) == (W, H):
                        # no reference in between: the plain export's bytes
                        plain = ctx.export(b, dataclasses.replace(spec0, crop=crop, upsample="nearest"))
                        for got, want in zip(plain.to_host()[0], refs[0]):
                            assert np.array_equal(got, want), (spec, "plain export")
                        plain.free()
    return n


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", [(72, 40), (136, 72), (1032, 40)])
def test_every_format_filter_crop_size_and_pitch(recon_mod, w, h, bd):
    """72 x 40: a row shorter than a wave's span; 136 x 72; 1032 x 40: 8 samples past a workgroup's column tile."""
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pic = synth.make_picture(params, 5200 + w + bd, perf=True, deblocking=True, sao=True)
    target = Target(4 * 3 * (2 * w) * (2 * h) + 256 * (3 * 2 * h + 8))
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload([pic])
            ctx.run(b)
            src = ctx.download(b)
            specs = specs_for(recon_mod, bd)
            assert len(specs) == (10 if bd == 8 else 12)
            assert run_matrix(recon_mod, ctx, b, src, bd, target, crops_of(w, h), specs) > 500
            b.free()
    finally:
        target.free()


@pytest.mark.parametrize("bd", [8, 10])
def test_area_over_several_source_chunks(recon_mod, bd):
    """4104 x 8: the area kernel walks the source columns under a workgroup in chunks of 2048, so here a workgroup runs
    three chunks of luma and two of chroma (2052 columns): later passes, the LDS tile reused between them, and outputs
    whose box straddles a chunk boundary and is summed from two chunks (16 outputs of 256.5 columns; 1000 and 342
    outputs whose edges do not fall on column 2048 or 4096)."""
    w, h = 4104, 8
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pic = synth.make_picture(params, 6100 + bd, perf=True, deblocking=True, sao=True)
    target = Target(4 * 3 * w * h + 256 * (3 * h + 8))
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload([pic])
            ctx.run(b)
            src = ctx.download(b)
            sizes = lambda W, H: [(16, 8, FILTERS), (1000, 6, FILTERS), (342, 4, FILTERS), (2050, 8, FILTERS), (3, 1, FILTERS),
                                  (W, H, FILTERS)]
            n = run_matrix(recon_mod, ctx, b, src, bd, target, [(0, 0, 0, 0), (6, 10, 0, 2)], specs_for(recon_mod, bd), sizes_fn=sizes)
            assert n > 500
            b.free()
    finally:
        target.free()


def check_export_at(ctx, batch, spec, sources, target, off, refs):
    """check_export with the destination ``off`` bytes into the target: the whole buffer again."""
    lay = ctx.export_layout(spec)
    n = len(sources)
    assert off + lay.frame_bytes * n <= target.nbytes
    target.fill()
    fr = ctx.export(batch, spec, dst=target.buf.ptr.value + off, dst_bytes=lay.frame_bytes * n)
    ctx.status(batch)
    got = target.read()
    want = np.full(target.nbytes, FILL, np.uint8)
    views = fr.host_views(want[off:])
    for i in range(n):
        assert len(refs[i]) == len(views[i])
        for v, r in zip(views[i], refs[i]):
            assert v.shape == r.shape and v.dtype == r.dtype
            v[...] = r
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s at +%d: %d bytes differ, first at %d" % (spec, off, bad.size, bad[0]))


@pytest.mark.parametrize("bd", [8, 10])
def test_plane_base_off_a_16_byte_boundary_with_aligned_pitches(recon_mod, bd):
    """The head-shifted store path: pitches that are multiples of 16 (pitch_align 256) and a destination one or three
    elements past a 16-byte boundary, so the first lane of a row writes a partial head and the groups after it take
    16-byte stores."""
    w, h = 136, 72
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = [synth.make_picture(params, 6200 + bd + k, perf=True, deblocking=True, sao=True) for k in range(2)]
    target = Target(2 * (4 * 3 * 2 * w * 2 * h + 256 * (3 * 2 * h + 8)) + 64)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            caches = [{} for _ in src]
            n = 0
            for spec0 in specs_for(recon_mod, bd):
                for size, filters in (((66, 36), FILTERS), ((190, 100), ("nearest", "bilinear")), ((w, h), FILTERS)):
                    for filt in filters:
                        spec = dataclasses.replace(spec0, size=size, resize=filt, pitch_align=256)
                        refs = [ref_of(s_, bd, spec, c) for s_, c in zip(src, caches)]
                        es = ctx.export_layout(spec).dtype.itemsize
                        for off in (es, 3 * es):
                            check_export_at(ctx, b, spec, src, target, off, refs)
                            n += 1
            assert n > 100
            b.free()
    finally:
        target.free()


def _pcm_batch(bd, planes_list, w=48, h=32):
    """PCM pictures carrying the given planes exactly (deblocking off, no SAO)."""
    params = PL.params_of(bd, 4, "a", False, w, h)
    pics = []
    for planes in planes_list:
        spec = PL.Spec(bd, 4, 16, w, h)
        spec.dbk[:] = False
        pics.append(PL.build(spec, planes, "a", params=params))
    return params, pics


@pytest.mark.parametrize("bd", [8, 12])
def test_value_edges(recon_mod, bd):
    """All 0, all max, a 0 / max checkerboard and one of 2 x 2 cells, in every plane: the area and bilinear sums reach
    both ends and the clip after the RGB conversion fires."""
    w, h, top = 48, 32, (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    dt = np.uint16 if bd > 8 else np.uint8

    def tri(f):
        return [f(yy, xx).astype(dt), f(yy[:h // 2, :w // 2], xx[:h // 2, :w // 2]).astype(dt),
                f(yy[:h // 2, :w // 2] + 1, xx[:h // 2, :w // 2]).astype(dt)]

    planes_list = [tri(lambda y, x: 0 * x), tri(lambda y, x: 0 * x + top), tri(lambda y, x: ((x + y) & 1) * top),
                   tri(lambda y, x: (((x >> 1) + (y >> 1)) & 1) * top)]
    params, pics = _pcm_batch(bd, planes_list, w, h)
    target = Target(4 * (4 * 3 * 2 * w * 2 * h + 4096))
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            for got, want in zip(src, planes_list):
                for g, p in zip(got, want):
                    np.testing.assert_array_equal(g, p)              # the planted planes, exactly
            sizes = lambda W, H: [(W, H, FILTERS), (24, 16, FILTERS), (18, 10, FILTERS), (13, 7, FILTERS), (2, 2, FILTERS),
                                  (66, 44, ("nearest", "bilinear"))]
            specs = specs_for(recon_mod, bd)
            run_matrix(recon_mod, ctx, b, src, bd, target, [(0, 0, 0, 0), (2, 4, 2, 0)], specs, sizes_fn=sizes, aligns=(1,))
            # the ends are reached: the clip fires both ways, and a 2 : 1 box of a checkerboard is (2 top + 2) >> 2
            spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", matrix="bt601", size=(24, 16), resize="area")
            refs = [ref_of(s, bd, spec)[0] for s in src]
            assert refs[1].max() == 255 and refs[0].min() == 0
            spec = recon_mod.ExportSpec(format="planar", size=(24, 16), resize="area")
            for k in (2, 3):
                y = ref_of(src[k], bd, spec)[0]
                assert (y == ((2 * top + 2) >> 2)).all() if k == 2 else set(np.unique(y)) == {0, top}
            b.free()
    finally:
        target.free()


@pytest.mark.parametrize("sample,bd", [("f32", 8), ("f16", 12), ("f32", 10), ("f16", 8)])
def test_normalised_float_outputs(recon_mod, sample, bd):
    """P265R_RS_NORM: per-channel scale and bias, two separately rounded fp32 operations.  The pinned triples whose
    fused result differs are planted through a PCM picture (full range, grey chroma: R = G = B = Y); a synthetic
    picture beside it."""
    w, h = 48, 32
    dt = np.uint16 if bd > 8 else np.uint8
    if bd == 8:
        vals, sc0, bi0 = (PINNED_F32[0],), PINNED_F32[1], PINNED_F32[2]
    elif bd == 12:
        vals, sc0, bi0 = PINNED_F16
    else:
        vals, sc0, bi0 = (), np.float32(1 / (1023 * 0.229)), np.float32(-0.485 / 0.229)
    rng = np.random.default_rng(77 + bd)
    Y = rng.integers(0, 1 << bd, (h, w)).astype(dt)
    for k, v in enumerate(vals):
        Y[3 + k, 5:9] = v
    grey = np.full((h // 2, w // 2), 1 << (bd - 1), dt)
    noise = [Y, rng.integers(0, 1 << bd, grey.shape).astype(dt), rng.integers(0, 1 << bd, grey.shape).astype(dt)]
    params, pics = _pcm_batch(bd, [[Y, grey, grey], noise], w, h)
    scale = (float(sc0), float(np.float32(1 / (((1 << bd) - 1) * 0.224))), float(np.float32(1 / (((1 << bd) - 1) * 0.225))))
    bias = (float(bi0), float(np.float32(-0.456 / 0.224)), float(np.float32(-0.406 / 0.225)))
    target = Target(2 * 4 * 3 * 2 * w * 2 * h + 4096)
    try:
        with recon_mod.ReconContext(params) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            np.testing.assert_array_equal(src[0][0], Y)
            for fmt in ("rgb_planar", "rgb_packed"):
                for size, filt in (((w, h), "nearest"), ((w, h), "bilinear"), ((24, 16), "area"), ((34, 18), "bilinear"),
                                   ((31, 17), "area"), ((66, 40), "nearest")):
                    for align in (1, 256):
                        spec = recon_mod.ExportSpec(format=fmt, sample=sample, matrix="bt709", full_range=True, size=size, resize=filt,
                                                    scale=scale, bias=bias, pitch_align=align)
                        refs = [ref_of(s, bd, spec) for s in src]
                        if size == (w, h) and vals:
                            # the planted values are among the pixels of channel 0, and fusing would show there
                            ints = RR.resize(src[0], bd, fmt, "native", "bt709", True, size=size, filt=filt)
                            r = ints[0] if fmt == "rgb_planar" else ints[0][..., 0]
                            assert all((r == v).any() for v in vals)
                        check_export(ctx, b, spec, src, bd, target, refs=refs)
            # scale alone / bias alone
            for kw in (dict(scale=(2.0, 0.5, 3.0)), dict(bias=(-1.0, 0.25, 100.0))):
                spec = recon_mod.ExportSpec(format="rgb_planar", sample=sample, size=(34, 18), resize="area", **kw)
                check_export(ctx, b, spec, src, bd, target, refs=[ref_of(s, bd, spec) for s in src])
            b.free()
    finally:
        target.free()


SOME = [dict(format="semiplanar", sample="native"), dict(format="planar", sample="native"),
        dict(format="rgb_packed", sample="u8", matrix="bt601"),
        dict(format="rgb_planar", sample="f16", matrix="bt2020", full_range=True)]


@pytest.mark.parametrize("bd", [8, 10])
def test_ragged_batch_to_one_size(recon_mod, bd):
    """Six picture sizes in one context, every slot 64 x 48; area is refused, nothing written, when one listed picture's
    window is smaller than the output; batch_array views all slots as one array."""
    big, pics = _ragged(recon_mod, bd)
    target = Target(6 * 4 * 3 * 264 * 200)
    try:
        with recon_mod.ReconContext(big) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            for kw in SOME:
                for filt in FILTERS:
                    for crop, align, size in (((2, 4, 2, 6), 1, (24, 48)), ((0, 0, 0, 0), 256, (32, 64)), ((16, 8, 8, 8), 1, (8, 6))):
                        spec = recon_mod.ExportSpec(crop=crop, pitch_align=align, size=size, resize=filt, **kw)
                        fr = check_export(ctx, b, spec, src, bd, target, refs=[ref_of(s, bd, spec) for s in src])
                        # batch_array: shape and strides against the bytes
                        host = target.read()
                        for k in range(fr.layout.n_planes if spec.format != "rgb_planar" else 1):
                            a = fr.batch_array(k).__cuda_array_interface__
                            view = np.ndarray(a["shape"], np.dtype(a["typestr"]), host, a["data"][0] - fr.ptr, a["strides"])
                            per_slot = fr.host_views(host)
                            for i in range(6):
                                want = np.stack(per_slot[i]) if spec.format == "rgb_planar" else per_slot[i][k]
                                assert np.array_equal(view[i], want)
            # (264, 64) is 64 rows high, (32, 200) 32 columns wide
            target.fill()
            for size in ((24, 66), (34, 48)):
                spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", size=size, resize="area")
                lay = ctx.export_layout(spec)
                rc = ctx.lib.p265r_batch_export_resized(ctx.handle, b.handle, ctypes.byref(lay.desc), ctypes.byref(lay.resize),
                                                        ctypes.c_void_p(target.buf.ptr.value), 6 * lay.frame_bytes, None, 6)
                assert rc == _lib.EINVAL
            ctx.status(b)
            assert np.all(target.read() == FILL)
            # ... the same sizes are legal without those pictures, and for the gathered filters
            spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", size=(24, 66), resize="area")
            check_export(ctx, b, spec, [src[0], src[2], src[4]], bd, target, only=[0, 2, 4],
                         refs=[ref_of(src[i], bd, spec) for i in (0, 2, 4)])
            spec = dataclasses.replace(spec, resize="bilinear")
            check_export(ctx, b, spec, src, bd, target, refs=[ref_of(s, bd, spec) for s in src])
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
                for filt in FILTERS:
                    spec = recon_mod.ExportSpec(crop=(2, 0, 0, 2), size=(30, 40), resize=filt, **kw)
                    fr = check_export(ctx, b, spec, [src[4], src[1]], 8, target, only=[4, 1],
                                      refs=[ref_of(src[i], 8, spec) for i in (4, 1)])
                    assert fr.sizes == [(32, 200), (128, 72)]
            b.free()
    finally:
        target.free()


def test_resized_export_is_ordered_behind_its_own_batch_on_a_pipelined_context(recon_mod):
    """Run, export, then run another batch on the other lane: the export holds the first batch's frames."""
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    first = [synth.make_picture(params, 9100 + k, deblocking=True) for k in range(3)]
    other = [synth.make_picture(params, 9200 + k, deblocking=True) for k in range(3)]
    spec = recon_mod.ExportSpec(format="semiplanar", crop=(2, 2, 0, 2), size=(64, 34), resize="area")
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
            for g, r in zip(got[i], ref_of(src[i], 8, spec)):
                np.testing.assert_array_equal(g, r)
            assert not np.array_equal(got[i][0], ref_of(src2[i], 8, spec)[0])
        a = fr.plane(2, 1).__cuda_array_interface__
        assert a["data"][0] == fr.ptr + 2 * fr.layout.frame_bytes + fr.layout.plane_off[1] and a["shape"] == (17, 32, 2)
        assert fr.batch_array(0).__cuda_array_interface__["shape"] == (3, 34, 64)
        fr.free()
        b1.free()
        b2.free()


@pytest.mark.parametrize("bd", [8, 10])
def test_monochrome_source(recon_mod, bd):
    """Planar (the Y plane alone), semi-planar with a grey CbCr plane, RGB with R = G = B; odd crops and odd sizes."""
    params = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = [M.to_mono(synth.make_picture(params, 7300 + bd + k, perf=True, deblocking=True, sao=True)) for k in range(2)]
    target = Target(2 * (4 * 3 * 144 * 80 + 256 * (3 * 80 + 8)))
    try:
        with recon_mod.ReconContext(M.mono_params(params)) as ctx:
            b = ctx.upload(pics)
            ctx.run(b)
            src = ctx.download(b)
            assert len(src[0]) == 1
            sizes = lambda W, H: [(W, H, FILTERS), (34, 18, FILTERS), (31, 17, FILTERS), (1, 1, FILTERS), (2, 2, FILTERS),
                                  (100, 56, ("nearest", "bilinear"))]
            n = run_matrix(recon_mod, ctx, b, src, bd, target, [(0, 0, 0, 0), (1, 3, 1, 1), (2, 4, 2, 6)], specs_for(recon_mod, bd),
                           sizes_fn=sizes, mono=True)
            assert n > 300
            spec = recon_mod.ExportSpec.named("nv12" if bd == 8 else "p010", size=(34, 18), resize="area")
            fr = ctx.export(b, spec)
            y, c = fr.to_host()[1]
            assert (c == ((1 << (bd - 1)) << (16 - bd if bd > 8 else 0))).all() and c.shape == (9, 17, 2)
            fr.free()
            b.free()
    finally:
        target.free()


def test_decoder_end_to_end_224(recon_mod, tmp_path):
    """synth_1080p_4pic.bin -> four 224 x 224 planar fp16 RGB frames, area-averaged, the picture hash checked on the
    device: equal to the restatement applied to the host decode; no plane comes back."""
    from p265_amd import decoder
    path = os.path.join(GOLDEN, "synth_1080p_4pic.bin")
    spec = recon_mod.ExportSpec.named("rgb-planar-f16", size=(224, 224), resize="area")
    out = tmp_path / "x.rgb"
    st = decoder.decode_file(path, str(out), export=spec, hash_on="device")
    assert st["pictures"] == 4 and st["hash_mismatch"] == 0 and st["hash_checked"] == 4
    got = np.frombuffer(out.read_bytes(), np.float16).reshape(4, 3, 224, 224)
    host = decoder.decode_bytes(open(path, "rb").read())
    for i, f in enumerate(host):
        want = ref_of(f.planes, 8, dataclasses.replace(spec, crop=tuple(f.crop)))
        assert np.array_equal(got[i].view(np.uint16), np.stack(want).view(np.uint16))
    frames = decoder.decode_bytes(open(path, "rb").read(), export=spec, hash_on="device")
    assert [f.planes for f in frames] == [None] * 4 and all(f.hash_ok is True for f in frames)
    a = frames[0].device.frames.batch_array().__cuda_array_interface__
    assert a["shape"][1:] == (3, 224, 224) and a["typestr"] == "<f2"
    assert frames[0].device.planes[0].__cuda_array_interface__["shape"] == (224, 224)
    for f in frames:
        f.device.release()


def test_refusals_launch_nothing(recon_mod):
    """Every refusal of p265r_batch_export_resized that needs a batch; the target stays 0xA5 through all of them, and a
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

            def lay_of(**kw):
                kw.setdefault("size", (34, 18))
                return ctx.export_layout(recon_mod.ExportSpec(**kw))

            def rc(lay, d=None, rs=None, ptr=dst, nbytes=None, idx=None, n=3, batch=b):
                d = lay.desc if d is None else d
                rs = lay.resize if rs is None else rs
                arr = (ctypes.c_int32 * len(idx))(*idx) if idx is not None else None
                return lib.p265r_batch_export_resized(ctx.handle, batch.handle, ctypes.byref(d), ctypes.byref(rs), ptr,
                                                      3 * d.frame_bytes if nbytes is None else nbytes, arr, n)

            def changed(obj, **kw):
                c = type(obj).from_buffer_copy(obj)
                for k, v in kw.items():
                    setattr(c, k, v)
                return c

            good = lay_of(format="planar")                               # uint16: rows of 68, 34, 34 bytes
            # the resize descriptor
            for kw in (dict(filter=3), dict(flags=2), dict(flags=_lib.RS_NORM), dict(out_width=0), dict(out_height=16385),
                       dict(out_width=33), dict(out_height=17), dict(out_width=36), dict(out_height=20)):
                assert rc(good, rs=changed(good.resize, **kw)) == _lib.EINVAL, kw       # (36 x 18: the layout is 34 wide)
            f32 = lay_of(format="rgb_planar", sample="f32", scale=(1, 1, 1))
            bad = changed(f32.resize)
            bad.bias[1] = float("nan")
            assert rc(f32, rs=bad) == _lib.EINVAL
            bad = changed(f32.resize)
            bad.scale[2] = float("inf")
            assert rc(f32, rs=bad) == _lib.EINVAL
            # area above the window: 72 x 40 pictures, crop (6, 10, 2, 4) leaves 56 x 34
            area = lay_of(format="rgb_packed", sample="u8", size=(58, 34), resize="area", crop=(6, 10, 2, 4))
            assert rc(area) == _lib.EINVAL
            area = lay_of(format="rgb_packed", sample="u8", size=(56, 36), resize="area", crop=(6, 10, 2, 4))
            assert rc(area) == _lib.EINVAL
            # the plain export's refusals, against the output size
            for field, k, val in (("pitch", 0, 66), ("pitch", 1, 32), ("pitch", 2, 35), ("pitch", 0, 69), ("plane_off", 1, 1)):
                d = changed(good.desc)
                getattr(d, field)[k] = val
                assert rc(good, d=d) == _lib.EINVAL, (field, k, val)
            d = changed(good.desc)
            d.plane_off[1] -= 2                                           # Cb starts inside Y
            assert rc(good, d=d) == _lib.EINVAL
            d = changed(good.desc)
            d.frame_bytes -= 2
            assert rc(good, d=d) == _lib.EINVAL
            assert rc(good, d=changed(good.desc, crop_left=3)) == _lib.EINVAL
            assert rc(good, d=changed(good.desc, crop_left=72)) == _lib.EINVAL          # no sample left
            assert rc(good, d=changed(good.desc, sample=_lib.SMP_F16)) == _lib.EINVAL
            for idx in ([0, 3], [-1, 0], [1, 1], [0, 1, 2, 0]):
                assert rc(good, idx=idx, n=len(idx)) == _lib.EINVAL, idx
            host = np.zeros(3 * good.frame_bytes, np.uint8)
            assert rc(good, ptr=ctypes.c_void_p(host.ctypes.data)) == _lib.EINVAL       # a host pointer
            assert rc(good, nbytes=3 * good.frame_bytes - 1) == _lib.ERANGE             # one byte short
            assert lib.p265r_batch_export_resized(ctx.handle, b.handle, ctypes.byref(good.desc), None, dst, 3 * good.frame_bytes,
                                                  None, 3) == _lib.EINVAL
            # a recon-input batch whose filters never ran has no output planes yet
            rb = ctx.upload([dataclasses.replace(pics[0], recon_input=src[0])])
            assert rc(good, nbytes=good.frame_bytes, n=1, batch=rb) == _lib.ESTATE
            ctx.status(b)
            assert np.all(target.read() == FILL)                          # nothing was launched
            assert rc(good, nbytes=2 * good.frame_bytes, idx=[2, 0], n=2) == _lib.OK    # (two slots do fit)
            ctx.status(b)
            rb.free()
            # and the context still exports, upsample ignored
            spec = recon_mod.ExportSpec(format="rgb_packed", sample="u8", upsample="bilinear", size=(34, 18), resize="nearest")
            check_export(ctx, b, spec, src, 10, target, refs=[ref_of(s, 10, spec) for s in src])
            b.free()
    finally:
        target.free()
