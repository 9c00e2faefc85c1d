"""Device-side output, the parts that need no device: p265r_export_layout, the descriptor validation,
p265r_export_coefficients, the accuracy of the integer RGB arithmetic (tests/export_ref.py restates it),
hand-worked bilinear chroma upsampling, the DeviceFrames plane interfaces and the command line."""
import ctypes
import itertools

import numpy as np
import pytest

import export_ref as X
from p265_amd import _lib, dec, recon
from p265_amd import records as R

YUV = [("planar", "native"), ("planar", "msb16"), ("semiplanar", "native"), ("semiplanar", "msb16")]
RGB = [(f, s) for f in ("rgb_planar", "rgb_packed") for s in ("native", "u8", "f16", "f32")]


def _legal(sample, bd):
    return not (sample == "msb16" and bd == 8)


def _planes(fmt, es, w, h):
    """(row bytes, rows) of every destination plane of a cropped w x h picture."""
    return {"planar": [(w * es, h), (w // 2 * es, h // 2), (w // 2 * es, h // 2)],
            "semiplanar": [(w * es, h), (w * es, h // 2)],
            "rgb_planar": [(w * es, h)] * 3, "rgb_packed": [(3 * w * es, h)]}[fmt]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("size,crop", [((72, 40), (2, 4, 2, 6)), ((1920, 1088), (0, 0, 0, 8))])
def test_layout_tight_and_aligned(bd, size, crop):
    params = R.make_params(pic_width=size[0], pic_height=size[1], bit_depth_luma=bd, bit_depth_chroma=bd)
    w, h = size[0] - crop[0] - crop[1], size[1] - crop[2] - crop[3]
    for fmt, sample in YUV + RGB:
        if not _legal(sample, bd):
            continue
        es = np.dtype(X.sample_dtype(sample, bd)).itemsize
        for align in (1, 256):
            lay = recon.export_layout(params, recon.ExportSpec(format=fmt, sample=sample, crop=crop, pitch_align=align))
            assert lay.dtype == np.dtype(X.sample_dtype(sample, bd))
            up = lambda v: (v + align - 1) // align * align
            off = 0
            planes = _planes(fmt, es, w, h)
            assert lay.n_planes == len(planes)
            for k, (row, rows) in enumerate(planes):
                assert lay.plane_off[k] == off, (fmt, sample, align, k)
                assert lay.pitch[k] == up(row), (fmt, sample, align, k)
                off = up(off + up(row) * rows)
            assert lay.frame_bytes == off
            # the explicit size of the picture gives the same layout as the params' size
            lay2 = recon.export_layout(params, recon.ExportSpec(format=fmt, sample=sample, crop=crop, pitch_align=align), size)
            assert (lay2.plane_off, lay2.pitch, lay2.frame_bytes) == (lay.plane_off, lay.pitch, lay.frame_bytes)


def _layout_rc(bd=8, size=(72, 40), align=1, **fields):
    lib = _lib.load()
    pc = recon._params_c(R.make_params(pic_width=size[0], pic_height=size[1], bit_depth_luma=bd, bit_depth_chroma=bd))
    d = _lib.ExportDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    return lib.p265r_export_layout(ctypes.byref(pc), 0, 0, ctypes.byref(d), align)


def test_validation_without_a_device():
    assert _layout_rc() == _lib.OK
    # unknown enum values
    assert _layout_rc(format=4) == _lib.EINVAL
    assert _layout_rc(sample=5) == _lib.EINVAL
    assert _layout_rc(format=_lib.FMT_RGB_PLANAR, matrix=3) == _lib.EINVAL
    assert _layout_rc(format=_lib.FMT_RGB_PACKED, upsample=2) == _lib.EINVAL
    assert _layout_rc(format=_lib.FMT_RGB_PACKED, full_range=2) == _lib.EINVAL
    # sample types that do not go with the format or the bit depth
    for smp in (_lib.SMP_U8, _lib.SMP_F16, _lib.SMP_F32):
        assert _layout_rc(format=_lib.FMT_PLANAR, sample=smp) == _lib.EINVAL
        assert _layout_rc(format=_lib.FMT_SEMIPLANAR, sample=smp, bd=10) == _lib.EINVAL
        assert _layout_rc(format=_lib.FMT_RGB_PLANAR, sample=smp, bd=10) == _lib.OK
    assert _layout_rc(format=_lib.FMT_SEMIPLANAR, sample=_lib.SMP_MSB16, bd=8) == _lib.EINVAL
    assert _layout_rc(format=_lib.FMT_SEMIPLANAR, sample=_lib.SMP_MSB16, bd=10) == _lib.OK
    assert _layout_rc(format=_lib.FMT_RGB_PACKED, sample=_lib.SMP_MSB16, bd=10) == _lib.EINVAL
    # odd crops, and crops that leave no sample
    for f in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
        assert _layout_rc(**{f: 3}) == _lib.EINVAL
        assert _layout_rc(**{f: 2}) == _lib.OK
    assert _layout_rc(crop_left=36, crop_right=36) == _lib.EINVAL
    assert _layout_rc(crop_left=70) == _lib.OK
    assert _layout_rc(crop_top=40) == _lib.EINVAL
    assert _layout_rc(crop_top=20, crop_bottom=18) == _lib.OK
    # an alignment that breaks the element size, null arguments
    assert _layout_rc(bd=10, align=5) == _lib.EINVAL                 # pitch 145: no multiple of 2
    lib = _lib.load()
    d = _lib.ExportDesc()
    assert lib.p265r_export_layout(None, 0, 0, ctypes.byref(d), 1) == _lib.EINVAL
    out = (ctypes.c_int32 * 8)()
    assert lib.p265r_export_coefficients(None, 8, out) == _lib.EINVAL
    assert lib.p265r_export_coefficients(ctypes.byref(d), 8, out) == _lib.EINVAL        # a YUV format has none
    d.format = _lib.FMT_RGB_PACKED
    assert lib.p265r_export_coefficients(ctypes.byref(d), 13, out) == _lib.EINVAL
    assert lib.p265r_batch_export(None, None, ctypes.byref(d), None, 0, None, 0) == _lib.EINVAL


def test_coefficients_equal_the_restatement():
    for matrix, full, B in itertools.product(X.MATRICES, (False, True), (8, 10, 12)):
        for D, sample in ((8, "u8"), (B, "native"), (B, "f16"), (B, "f32")):
            got = recon.export_coefficients(recon.ExportSpec(format="rgb_packed", sample=sample, matrix=matrix,
                                                             full_range=full), B)
            assert got == X.coefficients(matrix, full, B, D), (matrix, full, B, D)
    # BT.601 limited 8 bit: the familiar 1.164 / 1.596 / 0.392 / 0.813 / 2.017 at 14 fractional bits
    assert X.coefficients("bt601", False, 8, 8) == [19077, 26149, 6419, 13320, 33050, 16, 128, 8]


def _accuracy(Y, Cb, Cr, B):
    worst = 0.0
    for matrix, full in itertools.product(X.MATRICES, (False, True)):
        for D in sorted({8, B}):
            got = X.rgb_int(Y, Cb, Cr, X.coefficients(matrix, full, B, D))
            exact = X.rgb_exact(Y, Cb, Cr, matrix, full, B, D)
            for g, e in zip(got, exact):
                worst = max(worst, float(np.abs(g - np.clip(e, 0, 2 ** D - 1)).max()))
    return worst


def test_integer_rgb_is_within_its_bound_of_the_exact_conversion():
    """Each integer coefficient is within 0.5 of its real value c * 2^14, and |y| <= 2^B, |cb|, |cr| <= 2^(B-1)
    <= 2^B, so the up to three products of a sum are together within 3 * 0.5 * 2^B of the exact sum scaled by
    2^14: 3 * 2^(B-15) after the shift.  (s + 8192) >> 14 is floor(s / 2^14 + 0.5), at most 0.5 from s / 2^14, and
    clipping both sides to 0 .. 2^D - 1 moves them no further apart.  Hence |integer - exact| < 0.5 + 3 * 2^(B-15):
    0.875 at 12 bits.  All 2^24 triples at 8 bits, a seeded million at 10 and 12."""
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0.0
    for y0 in range(0, 256, 32):
        y = np.arange(y0, y0 + 32)[:, None, None]
        worst = max(worst, _accuracy(np.broadcast_to(y, (32, 256, 256)), cb[None], cr[None], 8))
    assert worst < 0.5 + 3 * 2.0 ** (8 - 15)
    for B in (10, 12):
        rng = np.random.default_rng(1000 + B)
        Y, Cb, Cr = (rng.integers(0, 1 << B, 1_000_000) for _ in range(3))
        assert _accuracy(Y, Cb, Cr, B) < 0.5 + 3 * 2.0 ** (B - 15)


def _bilinear_scalar(C, x, y):
    """The specification's bilinear rule for ONE luma position, in plain Python."""
    ch, cw = len(C), len(C[0])
    at = lambda j, i: C[min(max(j, 0), ch - 1)][min(max(i, 0), cw - 1)]
    j, i = y >> 1, x >> 1
    v = (lambda k: at(j - 1, k) + 3 * at(j, k)) if y % 2 == 0 else (lambda k: 3 * at(j, k) + at(j + 1, k))
    return (v(i) + 2) >> 2 if x % 2 == 0 else (v(i) + v(i + 1) + 4) >> 3


def test_bilinear_upsampling_hand_worked():
    """A 4 x 4 chroma ramp C[j][i] = 16 j + 4 i under an 8 x 8 luma grid: all four (x, y) parities and the clamps
    on all four sides, values worked by hand from the rule."""
    C = np.array([[16 * j + 4 * i for i in range(4)] for j in range(4)], np.uint8)
    up = X.upsample(C, "bilinear")
    hand = {(0, 0): 0,      # top-left: row -1 -> 0, v[0] = 0 + 3 * 0
            (1, 0): 2,      # v[0] = 0, v[1] = 4 + 3 * 4 = 16 -> (0 + 16 + 4) >> 3
            (7, 0): 12,     # right edge, odd x: v[3] = 48, v[4] -> v[3] -> (48 + 48 + 4) >> 3
            (0, 1): 4,      # odd y: v[0] = 3 * 0 + 16 -> (16 + 2) >> 2
            (1, 1): 6,      # v[0] = 16, v[1] = 3 * 4 + 20 = 32 -> (16 + 32 + 4) >> 3
            (2, 2): 16,     # even y, j = 1: v[1] = 4 + 3 * 20 = 64 -> (64 + 2) >> 2
            (3, 7): 54,     # bottom edge, odd y: row 4 -> 3, v[1] = 208, v[2] = 224 -> (432 + 4) >> 3
            (6, 7): 60,     # v[3] = 4 * 60 = 240 -> (240 + 2) >> 2
            (0, 7): 48}     # v[0] = 4 * 48 = 192 -> (192 + 2) >> 2
    for (x, y), want in hand.items():
        assert up[y, x] == want, (x, y)
    for y in range(8):
        for x in range(8):
            assert up[y, x] == _bilinear_scalar(C.tolist(), x, y), (x, y)
    near = X.upsample(C, "nearest")
    assert near[5, 7] == C[2, 3] and near[0, 0] == C[0, 0] and near[7, 6] == C[3, 3]


def test_device_frames_plane_interfaces():
    """The __cuda_array_interface__ of every plane of a DeviceFrames over a fake address (nothing is touched)."""
    params = R.make_params(pic_width=72, pic_height=40, bit_depth_luma=10, bit_depth_chroma=10)
    base = 0x7F0000000000
    spec = recon.ExportSpec(format="semiplanar", sample="msb16", crop=(2, 4, 2, 6), pitch_align=256)
    lay = recon.export_layout(params, spec)
    fr = recon.DeviceFrames(base, 2 * lay.frame_bytes, lay, [(72, 40), (72, 40)])
    assert len(fr) == 2 and fr.nbytes == 2 * lay.frame_bytes and fr.ptr == base
    y, c = fr.plane(1, 0).__cuda_array_interface__, fr.plane(1, 1).__cuda_array_interface__
    assert y == {"shape": (32, 66), "typestr": "<u2", "data": (base + lay.frame_bytes, False), "strides": (256, 2),
                 "version": 3}
    assert c == {"shape": (16, 33, 2), "typestr": "<u2", "data": (base + lay.frame_bytes + 32 * 256, False),
                 "strides": (256, 4, 2), "version": 3}
    with pytest.raises(IndexError):
        fr.plane(2, 0)
    with pytest.raises(IndexError):
        fr.plane(0, 2)
    p8 = R.make_params(pic_width=72, pic_height=40)
    lay = recon.export_layout(p8, recon.ExportSpec(format="rgb_packed", sample="f32"))
    a = recon.DeviceFrames(base, lay.frame_bytes, lay, [(72, 40)]).plane(0, 0).__cuda_array_interface__
    assert a["shape"] == (40, 72, 3) and a["typestr"] == "<f4" and a["strides"] == (72 * 12, 12, 4)
    lay = recon.export_layout(p8, recon.ExportSpec(format="rgb_planar", sample="f16"))
    fr = recon.DeviceFrames(base, lay.frame_bytes, lay, [(72, 40)])
    for k in range(3):
        a = fr.plane(0, k).__cuda_array_interface__
        assert a == {"shape": (40, 72), "typestr": "<f2", "data": (base + k * 72 * 40 * 2, False), "strides": (144, 2),
                     "version": 3}
    lay = recon.export_layout(p8, recon.ExportSpec(format="planar"))
    a = recon.DeviceFrames(base, lay.frame_bytes, lay, [(72, 40)]).plane(0, 2).__cuda_array_interface__
    assert a == {"shape": (20, 36), "typestr": "|u1", "data": (base + 72 * 40 + 36 * 20, False), "strides": (36, 1),
                 "version": 3}
    # host views of a host copy use the same geometry
    host = np.arange(lay.frame_bytes, dtype=np.uint8)
    v = recon.DeviceFrames(base, lay.frame_bytes, lay, [(72, 40)]).host_views(host)
    assert v[0][1][3, 5] == host[72 * 40 + 3 * 36 + 5]


def test_cli_flags():
    a = dec.parse_cmd(["-b", "x.bin"])
    assert a.format == "i420" and a.matrix == "bt709" and not a.full_range and a.upsample == "nearest"
    assert dec.export_spec(a) is None                      # the default keeps the host path
    a = dec.parse_cmd(["-b", "x.bin", "-o", "y", "--format", "rgb24", "--matrix", "bt601", "--full-range",
                       "--upsample", "bilinear"])
    s = dec.export_spec(a)
    assert (s.format, s.sample, s.matrix, s.full_range, s.upsample) == ("rgb_packed", "u8", "bt601", True, "bilinear")
    for name, fs in (("nv12", ("semiplanar", "native")), ("p010", ("semiplanar", "msb16")),
                     ("rgb-planar-f16", ("rgb_planar", "f16"))):
        s = dec.export_spec(dec.parse_cmd(["-b", "x.bin", "--format", name]))
        assert (s.format, s.sample) == fs
    with pytest.raises(SystemExit):
        dec.parse_cmd(["-b", "x.bin", "--format", "yuy2"])
