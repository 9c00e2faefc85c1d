"""Grid export, the parts that need no device: p265r_grid_layout and every refusal that needs no batch through ctypes,
and the teeth of the seam test on the reference alone (tests/grid_ref.py against per-tile exports pasted together)."""
import ctypes

import numpy as np
import pytest

import export_ref as X
import grid_ref as GR
from p265_amd import _lib, recon
from p265_amd import records as R


def _rc(tile=(40, 24), bd=8, mono=False, align=1, grid=(2, 3, 100, 42, 0), reserved=None, split=False, bdc=None, **fields):
    lib = _lib.load()
    p = R.make_params(pic_width=tile[0], pic_height=tile[1], bit_depth_luma=bd, bit_depth_chroma=bd if bdc is None else bdc,
                      chroma_format_idc=0 if mono else 1, split_bit_depth=int(split))
    pc = recon._params_c(p)
    d = _lib.ExportDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    g = _lib.GridDesc()
    g.rows, g.cols, g.out_width, g.out_height, g.orientation = grid
    if reserved is not None:
        g.reserved[reserved] = 1
    return lib.p265r_grid_layout(ctypes.byref(pc), 0, 0, ctypes.byref(g), ctypes.byref(d), align), d


def test_refusals_without_a_device():
    E = _lib.EINVAL
    assert _rc()[0] == _lib.OK
    for grid in ((0, 3, 100, 42, 0), (2, 0, 100, 42, 0), (257, 3, 100, 42, 0), (2, 257, 100, 42, 0), (2, 3, 100, 42, 8)):
        assert _rc(grid=grid)[0] == E, grid
    for k in range(3):
        assert _rc(reserved=k)[0] == E
    # the HEIF rule: the output ends inside the last tile column / row
    assert _rc(grid=(2, 3, 80, 42, 0))[0] == E and _rc(grid=(2, 3, 82, 42, 0))[0] == _lib.OK
    assert _rc(grid=(2, 3, 122, 42, 0))[0] == E and _rc(grid=(2, 3, 120, 48, 0))[0] == _lib.OK
    assert _rc(grid=(2, 3, 100, 24, 0))[0] == E and _rc(grid=(2, 3, 100, 50, 0))[0] == E
    # an empty window
    assert _rc(crop_left=50, crop_right=50)[0] == E and _rc(crop_top=42)[0] == E
    # odd windows: YUV of a 4:2:0 source no, RGB yes, a monochrome planar source yes, monochrome semi-planar no
    assert _rc(grid=(2, 3, 101, 42, 0))[0] == E and _rc(grid=(2, 3, 100, 43, 0))[0] == E
    assert _rc(grid=(2, 3, 101, 43, 0), format=_lib.FMT_RGB_PACKED, sample=_lib.SMP_U8)[0] == _lib.OK
    assert _rc(grid=(2, 3, 101, 43, 0), mono=True)[0] == _lib.OK
    assert _rc(grid=(2, 3, 101, 43, 0), mono=True, format=_lib.FMT_SEMIPLANAR)[0] == E
    assert _rc(crop_right=1)[0] == E and _rc(crop_right=1, format=_lib.FMT_RGB_PLANAR)[0] == _lib.OK
    # odd crop_left / crop_top on a 4:2:0 source, whatever the format; legal on a monochrome planar / RGB source
    for f in (_lib.FMT_PLANAR, _lib.FMT_RGB_PACKED):
        assert _rc(crop_left=1, crop_right=1, format=f)[0] == E and _rc(crop_top=1, crop_bottom=1, format=f)[0] == E
        assert _rc(crop_left=1, crop_top=1, mono=True, format=f)[0] == _lib.OK
    # what p265r_batch_export refuses: enums, sample type against format and depth
    assert _rc(format=4)[0] == E and _rc(sample=_lib.SMP_F16)[0] == E and _rc(sample=_lib.SMP_MSB16)[0] == E
    assert _rc(sample=_lib.SMP_MSB16, format=_lib.FMT_SEMIPLANAR, bd=10)[0] == _lib.OK
    assert _rc(format=_lib.FMT_RGB_PACKED, matrix=3)[0] == E
    # a canvas above 65535 samples, an alignment that breaks the element size, null arguments
    assert _rc(tile=(512, 512), grid=(2, 129, 66000, 600, 0))[0] == E
    assert _rc(bd=10, align=5, grid=(2, 3, 102, 42, 0))[0] == E
    lib = _lib.load()
    assert lib.p265r_grid_layout(None, 0, 0, None, None, 1) == E
    assert lib.p265r_batch_export_grid(None, None, None, None, None, 0, None, 0) == E
    # unequal depths: unsupported, as the issue states
    assert _rc(bd=10, bdc=8, split=True)[0] == _lib.EUNSUPPORTED


@pytest.mark.parametrize("o", range(8))
def test_layout_of_the_oriented_frame(o):
    for fmt, sample, bd, n in (("planar", "native", 8, 3), ("semiplanar", "msb16", 10, 2), ("rgb_packed", "u8", 8, 1),
                               ("rgb_planar", "f32", 10, 3)):
        p = R.make_params(pic_width=40, pic_height=24, bit_depth_luma=bd, bit_depth_chroma=bd)
        es = np.dtype(X.sample_dtype(sample, bd)).itemsize
        for align in (1, 256):
            lay = recon.grid_layout(p, recon.ExportSpec(format=fmt, sample=sample, crop=(2, 2, 4, 2), pitch_align=align),
                                    recon.GridSpec(2, 3, 100, 42, o))
            w, h = (36, 96) if o & 1 else (96, 36)
            assert lay.size == (w, h) and lay.n_planes == n
            rows = {"planar": [(w * es, h), (w // 2 * es, h // 2), (w // 2 * es, h // 2)], "semiplanar": [(w * es, h), (w * es, h // 2)],
                    "rgb_planar": [(w * es, h)] * 3, "rgb_packed": [(3 * w * es, h)]}[fmt]
            up = lambda v: (v + align - 1) // align * align
            off = 0
            for k, (rb, r) in enumerate(rows):
                assert (lay.plane_off[k], lay.pitch[k]) == (off, up(rb)), (fmt, o, align, k)
                off = up(off + up(rb) * r)
            assert lay.frame_bytes == off
            assert lay.plane_view(0, None)[0][:2] == (h, w)


def test_size_extremes_stay_in_64_bits():
    # 256 x 256 tiles of 8 x 8; a 16384-wide canvas of 64 tiles of 256, planar fp32 RGB with a 2^20 alignment
    rc, d = _rc(tile=(8, 8), grid=(256, 256, 2048, 2048, 3), format=_lib.FMT_RGB_PLANAR, sample=_lib.SMP_F32)
    assert rc == _lib.OK and d.frame_bytes == 3 * 4 * 2048 * 2048
    rc, d = _rc(tile=(256, 256), grid=(64, 64, 16384, 16384, 1), format=_lib.FMT_RGB_PLANAR, sample=_lib.SMP_F32, align=1 << 20)
    assert rc == _lib.OK and d.frame_bytes == 3 * 16384 * (1 << 20) and d.plane_off[2] == 2 * 16384 * (1 << 20)


def test_the_seam_test_has_teeth():
    """On the seam picture, the canvas-wide bilinear conversion differs from per-tile conversions pasted together in
    at least one sample of every interior seam column (the last column left of a seam, whose odd-x tap reads the next
    tile) and of both rows at every interior seam row."""
    rows, cols, tw, th = 2, 3, 32, 32
    tiles = GR.seam_tiles(rows, cols, tw, th)
    kw = dict(sample="u8", matrix="bt601", full_range=True)
    whole = GR.frame(tiles, rows, cols, (cols * tw, rows * th), 8, "rgb_packed", upsample_mode="bilinear", **kw)[0]
    pasted = GR.pasted(tiles, rows, cols, 8, "rgb_packed", upsample_mode="bilinear", **kw)[0]
    diff = (whole != pasted).any(axis=2)
    for c in range(1, cols):
        assert diff[:, c * tw - 1].any(), c
    for r in range(1, rows):
        assert diff[r * th - 1].any() and diff[r * th].any(), r
    # and nowhere else than next to a seam
    far = np.ones_like(diff)
    for c in range(1, cols):
        far[:, c * tw - 1:c * tw + 1] = False
    for r in range(1, rows):
        far[r * th - 1:r * th + 1] = False
    assert not diff[far].any()
    # nearest upsampling needs no neighbour: pasted is right there
    near = GR.frame(tiles, rows, cols, (cols * tw, rows * th), 8, "rgb_packed", upsample_mode="nearest", **kw)[0]
    assert np.array_equal(near, GR.pasted(tiles, rows, cols, 8, "rgb_packed", upsample_mode="nearest", **kw)[0])
