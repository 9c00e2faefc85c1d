"""Scaled grid export, the parts that need no device: every refusal that needs no launch through ctypes, the struct
sizes, the restatement's two identities against tests/resize_ref.py and tests/grid_ref.py, the host planner's per-frame
constants against the restatement, heif.decode_many's argument handling with stand-in frames, and the host sanitizer
check (`make grid-resize-check`)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grid_ref as GR
import grid_resize_ref as GRR
import resize_ref as RZ
from p265_amd import _lib, recon
from p265_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rc(frames=((2, 3, 100, 42, (0, 0, 0, 0), 0),), size=(50, 38), filt=_lib.RS_BILINEAR, flags=0, tile=(40, 24), bd=8, mono=False,
        reserved=None, split=False, bdc=None, out=True, **fields):
    lib = _lib.load()
    p = R.make_params(pic_width=tile[0], pic_height=tile[1], bit_depth_luma=bd, bit_depth_chroma=bd if bdc is None else bdc,
                      chroma_format_idc=0 if mono else 1, split_bit_depth=int(split))
    pc = recon._params_c(p)
    d = _lib.ExportDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    rs = _lib.ResizeDesc()
    rs.out_width, rs.out_height, rs.filter, rs.flags = size[0], size[1], filt, flags
    arr = recon.grid_frames_c([recon.GridFrame(*f) for f in frames])
    if reserved is not None:
        arr[len(frames) - 1].reserved[reserved] = 1
    res = (ctypes.c_int32 * (12 * max(len(frames), 1)))()
    return lib.p265r_grid_resize_plan(ctypes.byref(pc), 0, 0, ctypes.byref(d), ctypes.byref(rs), arr, len(frames),
                                      res if out else None)


def F(rows=2, cols=3, w=100, h=42, crop=(0, 0, 0, 0), o=0):
    return (rows, cols, w, h, crop, o)


def test_struct_sizes_and_symbols():
    assert ctypes.sizeof(_lib.GridFrame) == 48 and ctypes.sizeof(_lib.GridDesc) == 32 and ctypes.sizeof(_lib.ResizeDesc) == 40
    assert ctypes.sizeof(_lib.ExportDesc) == 88
    assert _lib.GridFrame.orientation.offset == 32 and _lib.GridFrame.reserved.offset == 36
    lib = _lib.load()
    for name in ("p265r_batch_export_grid_resized", "p265r_grid_resize_plan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.p265r_abi_version() == 2                                  # additions only


def test_refusals_without_a_device():
    E = _lib.EINVAL
    assert _rc() == _lib.OK
    # what the grid export refuses, per frame -- also in the last frame of two
    for f in (F(rows=0), F(cols=0), F(rows=257, h=24 * 257 - 2), F(cols=257, w=40 * 257 - 2), F(o=8), F(w=80), F(w=122, h=48),
              F(h=24), F(h=50), F(crop=(50, 50, 0, 0)), F(crop=(0, 0, 42, 0)), F(crop=(65536, 0, 0, 0))):
        assert _rc(frames=(f,)) == E, f
        assert _rc(frames=(F(), f)) == E, f
    for k in range(3):
        assert _rc(reserved=k) == E and _rc(frames=(F(), F()), reserved=k) == E
    # odd window origins on a 4:2:0 source; odd windows: every format there, semi-planar only on a monochrome source
    rgb = dict(format=_lib.FMT_RGB_PACKED, sample=_lib.SMP_U8)
    assert _rc(frames=(F(crop=(1, 1, 0, 0)),), **rgb) == E and _rc(frames=(F(crop=(0, 0, 1, 1)),), **rgb) == E
    assert _rc(frames=(F(w=101),)) == E and _rc(frames=(F(h=43),), format=_lib.FMT_SEMIPLANAR) == E
    assert _rc(frames=(F(w=101),), **rgb) == E and _rc(frames=(F(crop=(0, 0, 0, 1)),), **rgb) == E
    assert _rc(frames=(F(w=101, h=43, crop=(1, 0, 1, 0)),), size=(51, 37), mono=True) == _lib.OK
    assert _rc(frames=(F(w=101, h=43),), size=(51, 37), mono=True, **rgb) == _lib.OK
    assert _rc(frames=(F(w=101, h=43),), mono=True, format=_lib.FMT_SEMIPLANAR) == E
    # desc->crop_* non-zero: the crop is per frame
    for k in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
        assert _rc(**{k: 2}) == E
    # what the scaled export refuses
    assert _rc(filt=3) == E and _rc(flags=2) == E and _rc(size=(0, 38)) == E and _rc(size=(50, 16386)) == E
    assert _rc(size=(51, 38)) == E and _rc(size=(51, 37), **rgb) == _lib.OK
    assert _rc(flags=_lib.RS_NORM, **rgb) == E
    assert _rc(format=4) == E and _rc(sample=_lib.SMP_F16) == E and _rc(sample=_lib.SMP_MSB16) == E
    assert _rc(sample=_lib.SMP_MSB16, format=_lib.FMT_SEMIPLANAR, bd=10) == _lib.OK
    # area: downscale only, measured at the PRE-TURN size, per frame
    A = _lib.RS_AREA
    assert _rc(filt=A) == _lib.OK and _rc(filt=A, frames=(F(o=1),)) == E and _rc(frames=(F(o=1),)) == _lib.OK
    assert _rc(filt=A, frames=(F(crop=(0, 52, 0, 0)),)) == E and _rc(filt=A, frames=(F(), F(1, 1, 40, 24))) == E
    # windows above 8192 (area) and above 32767 (every filter)
    big = dict(tile=(512, 512), size=(64, 64))
    assert _rc(filt=A, frames=(F(16, 16, 8192, 8192),), **big) == _lib.OK
    assert _rc(filt=A, frames=(F(16, 17, 8194, 8192),), **big) == E and _rc(frames=(F(16, 17, 8194, 8192),), **big) == _lib.OK
    assert _rc(frames=(F(16, 64, 32766, 8192),), **big) == _lib.OK and _rc(frames=(F(16, 64, 32768, 8192),), **big) == E
    # more than 65535 tiles or frames, no frame, null arguments
    assert _rc(frames=(F(256, 128, 1024, 2048),), tile=(8, 8)) == _lib.OK
    assert _rc(frames=(F(256, 128, 1024, 2048),) * 2, tile=(8, 8)) == E
    assert _rc(frames=()) == E and _rc(out=False) == E
    lib = _lib.load()
    assert lib.p265r_grid_resize_plan(None, 0, 0, None, None, None, 1, None) == E
    assert lib.p265r_batch_export_grid_resized(None, None, None, None, None, 0, None, 0, None) == E
    # unequal depths: unsupported
    assert _rc(bd=10, bdc=8, split=True) == _lib.EUNSUPPORTED


def _tiles(rows, cols, tw, th, bd=8, seed=3, mono=False):
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    out = []
    for _ in range(rows * cols):
        t = [rng.integers(0, 1 << bd, (th, tw)).astype(dt)]
        if not mono:
            t += [rng.integers(0, 1 << bd, (th // 2, tw // 2)).astype(dt) for _ in range(2)]
        out.append(t)
    return out


@pytest.mark.parametrize("fmt,sample", [("planar", "native"), ("semiplanar", "native"), ("rgb_packed", "u8"), ("rgb_planar", "f16")])
def test_identity_single_tile_is_the_scaled_export(fmt, sample):
    """rows = cols = 1, orientation 0: the restatement equals resize_ref with the crop the window implies."""
    tile = _tiles(1, 1, 72, 40)
    for size, filt in (((30, 18), "area"), ((30, 18), "nearest"), ((80, 44), "bilinear")):
        got = GRR.frame(tile, 1, 1, (66, 38), 8, fmt, size, sample, crop=(2, 4, 2, 6), filt=filt, scale=(2.0, 0.5, 3.0) if
                        sample == "f16" else None)
        want = RZ.resize(tile[0], 8, fmt, sample, crop=(2, 4 + 6, 2, 6 + 2), size=size, filt=filt,
                         scale=(2.0, 0.5, 3.0) if sample == "f16" else None)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))


@pytest.mark.parametrize("o", range(8))
def test_identity_nearest_at_the_window_size_is_the_grid_export(o):
    """NEAREST with pw x ph = W x H: the restatement equals grid_ref with nearest upsampling, every orientation."""
    tiles = _tiles(2, 3, 40, 24, seed=4 + o)
    crop = (2, 2, 4, 2)
    for fmt, sample in (("planar", "native"), ("semiplanar", "native"), ("rgb_packed", "u8"), ("rgb_planar", "f32")):
        want = GR.frame(tiles, 2, 3, (100, 42), 8, fmt, sample, upsample_mode="nearest", crop=crop, orientation=o)
        size = (36, 96) if o & 1 else (96, 36)
        got = GRR.frame(tiles, 2, 3, (100, 42), 8, fmt, size, sample, crop=crop, orientation=o, filt="nearest")
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (fmt, o)


def test_planner_constants_equal_the_restatement():
    """p265r_grid_resize_plan's per-frame constants -- first tile, window, pre-turn size, reversals, transpose, staging
    index -- against grid_resize_ref.expected_plan, which derives the reversals from numpy's rot90 itself; then R
    reversed and transposed as the planner says IS the restatement's slot."""
    p = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=4)
    frames = [(1, 1, 60, 50, (2, 4, 0, 2), 0), (2, 3, 190, 126, (0, 0, 0, 0), 1), (3, 2, 128, 180, (4, 2, 6, 4), 6),
              (2, 3, 150, 100, (10, 20, 2, 0), 3), (1, 1, 64, 64, (0, 6, 2, 0), 5)]
    frames += [(2, 2, 120, 100, (0, 0, 0, 0), o) for o in range(8)]
    spec = recon.ExportSpec(format="rgb_planar", sample="f16", size=(48, 32), resize="area")
    got = recon.grid_resize_plan(p, spec, [recon.GridFrame(*f) for f in frames])
    assert got == GRR.expected_plan(frames, (48, 32))
    tiles = _tiles(2, 2, 64, 64, seed=9)
    for o in range(8):
        c = got[5 + o]
        Rp = RZ.resize(GR.canvas(tiles, 2, 2), 8, "planar", crop=(0, 128 - 120, 0, 128 - 100), size=c["pre_turn"], filt="bilinear")
        for k, slot in enumerate(GRR.frame(tiles, 2, 2, (120, 100), 8, "planar", (48, 32), orientation=o, filt="bilinear")):
            u = Rp[k][::-1 if c["fy"] else 1, ::-1 if c["fx"] else 1]
            assert np.array_equal(u.T if c["transpose"] else u, slot), (o, k)


class _Info:
    def __init__(self, chroma_format):
        self.chroma_format = chroma_format


def test_decode_many_argument_handling(monkeypatch):
    """With stand-in parse and decode steps: a size no longer raises, an empty list stays empty, a 4:2:0 alpha image
    with an odd size is refused by name before anything is decoded, a monochrome one is not."""
    from p265_amd import heif
    calls = []

    def parse(chroma):
        def _parse(src, item, aux, apply_orientation):
            info = heif.ImageInfo(1, "grid", width=128, height=120, rows=2, cols=2, window=(0, 0, 128, 120), orientation=src)
            return None, info, (_Info(chroma) if aux else None)
        return _parse

    def items(jobs, export, *a):
        calls.append((len(jobs), export.size, export.format))
        return "frames%d" % len(calls), ("bt709", False)

    monkeypatch.setattr(heif, "_decode_items", items)
    monkeypatch.setattr(heif, "_parse", parse(0))
    spec = recon.ExportSpec.named("rgb24", size=(41, 31), resize="area")
    assert heif.decode_many([], export=spec) == []
    imgs = heif.decode_many([0, 1, 6], export=spec, aux=("alpha",))
    assert [(i.width, i.height, i.orientation, i.source_size, i.index) for i in imgs] == \
        [(41, 31, 0, (128, 120), 0), (41, 31, 1, (120, 128), 1), (41, 31, 6, (128, 120), 2)]
    assert calls == [(3, (41, 31), "rgb_packed"), (3, (41, 31), "planar")] and imgs[0].alpha == "frames2"
    monkeypatch.setattr(heif, "_parse", parse(1))
    del calls[:]
    with pytest.raises(heif.UnsupportedHeif, match="alpha auxiliary image coded 4:2:0 cannot be resized to an odd size 41 x 31"):
        heif.decode_many([0], export=spec, aux=("alpha",))
    assert calls == []
    assert heif.decode_many([0], export=spec)[0].alpha is None            # (no alpha asked for: no limit)
    even = heif.decode_many([0], export=recon.ExportSpec.named("rgb24", size=(40, 30)), aux=("alpha",))
    assert even[0].alpha is not None and calls[-1] == (1, (40, 30), "planar")
    # without a size: one shape for all, the slot is the oriented image
    plain = heif.decode_many([1], export=recon.ExportSpec.named("rgb24"))
    assert (plain[0].width, plain[0].height, plain[0].source_size) == (120, 128, (120, 128)) and calls[-1][1] is None


def test_export_grid_resized_needs_a_size():
    class Stub:
        pics = [None]
    with pytest.raises(ValueError, match="size"):
        recon.ReconContext.export_grid_resized(None, Stub(), recon.ExportSpec.named("rgb24"), [recon.GridFrame(1, 1, 64, 48)])


def test_host_sanitizer_check_builds_and_passes(tmp_path):
    """`make grid-resize-check`: the planner under ASan / UBSan, a stand-alone host program."""
    r = subprocess.run(["make", "-C", ROOT, "grid-resize-check", "GRID_RESIZE_CHECK=%s" % (tmp_path / "grid_resize_check")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grid_resize_check ok" in r.stdout
