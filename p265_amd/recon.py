"""Host API of the MI355X reconstruction back-end (Python side of the C ABI).

Mirrors what the reference's reconstruction hook would do per picture
(decoder/cu.py:483-494 -> decode_intra, decoder/sao.py), but per batch:

    ctx = ReconContext(params, device=0)
    frames = ctx.decode([pic0, pic1, ...])          # -> [(Y, Cb, Cr), ...] planes (uint8; uint16 > 8 bits)

or, keeping inputs resident in HBM (the benchmark path):

    batch = ctx.upload(pics); ctx.run(batch); ctx.sync(); frames = ctx.download(batch)

Errors raise ``P265RError`` (negative C return codes); there is no CPU fallback.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import records as R


def _params_c(p):
    c = _lib.Params()
    for name, _ in _lib.Params._fields_:
        if name == "reserved":
            continue
        setattr(c, name, int(p[name]))
    return c


def sparsify(pic):
    """records.SparsePicture of a dense Picture through the C p265r_sparsify (host only: needs the
    library, no context and no device; records.sparsify is the numpy statement of the same)."""
    lib = _lib.load()
    tbs_in = np.ascontiguousarray(pic.tbs, R.TB_DTYPE)
    coef = np.ascontiguousarray(pic.coef, np.int16)
    c = _lib.PictureC()
    c.tbs = tbs_in.ctypes.data if len(tbs_in) else None
    c.n_tbs = len(tbs_in)
    c.coef = coef.ctypes.data if len(coef) else None
    c.n_coef = len(coef)
    n_nz, n_raw = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(lib.p265r_sparsify(ctypes.byref(c), None, None, 0, ctypes.byref(n_nz), None, 0, ctypes.byref(n_raw)),
               "p265r_sparsify")
    tbs = np.zeros(len(tbs_in), R.TB_DTYPE)
    nz = np.zeros(n_nz.value, np.uint32)
    raw = np.zeros(n_raw.value, np.int16)
    _lib.check(lib.p265r_sparsify(ctypes.byref(c), tbs.ctypes.data, nz.ctypes.data, len(nz), ctypes.byref(n_nz),
                                  raw.ctypes.data, len(raw), ctypes.byref(n_raw)), "p265r_sparsify")
    return R.SparsePicture(ctus=pic.ctus, tbs=tbs, nz=nz, coef=raw, nofilter=pic.nofilter, size=pic.size,
                           recon_input=pic.recon_input, meta=dict(pic.meta))


def plane_shapes(params):
    return R.plane_shapes(params)


class DecodedPicture:
    """One decoded picture, served back to the reference's read-back surface.

    ``get_reconstructed_sample(x, y, c_idx)`` has the semantics of Cu.get_reconstructed_sample
    (decoder/cu.py:617-632): (x, y) in LUMA coordinates for every component (chroma: the
    sample at (x >> 1, y >> 1) of its plane, cu.py:624-630), returning the reconstruction
    before the in-loop filters (pu.reconstructed_samples, reconstruction.py:25), which is what
    intra prediction of later blocks reads.  ``get_output_sample`` returns the decoded
    (deblocked + SAO) sample that is written out.  ``planes`` / ``recon`` are [Y, Cb, Cr]
    arrays indexed [y][x] (the reference's arrays are x-major [x][y]): uint8 at BitDepth 8, uint16
    above (Main 10)."""

    def __init__(self, planes, recon):
        self.planes, self.recon = planes, recon

    @staticmethod
    def _at(planes, x, y, c_idx):
        sub = 1 if c_idx else 0
        return int(planes[c_idx][y >> sub, x >> sub])

    def get_reconstructed_sample(self, x, y, c_idx):
        return self._at(self.recon, x, y, c_idx)

    def get_output_sample(self, x, y, c_idx):
        return self._at(self.planes, x, y, c_idx)


# ---- device-side output (p265r_batch_export) ------------------------------------------------------
_FORMATS = {"planar": _lib.FMT_PLANAR, "semiplanar": _lib.FMT_SEMIPLANAR, "rgb_planar": _lib.FMT_RGB_PLANAR,
            "rgb_packed": _lib.FMT_RGB_PACKED}
_SAMPLES = {"native": _lib.SMP_NATIVE, "msb16": _lib.SMP_MSB16, "u8": _lib.SMP_U8, "f16": _lib.SMP_F16,
            "f32": _lib.SMP_F32}
_MATRICES = {"bt601": _lib.MAT_BT601, "bt709": _lib.MAT_BT709, "bt2020": _lib.MAT_BT2020}
_UPSAMPLES = {"nearest": _lib.UP_NEAREST, "bilinear": _lib.UP_BILINEAR}
_FILTERS = {"nearest": _lib.RS_NEAREST, "bilinear": _lib.RS_BILINEAR, "area": _lib.RS_AREA}


@dataclass(frozen=True)
class ExportSpec:
    """What p265r_batch_export writes: ``format`` planar | semiplanar | rgb_planar | rgb_packed, ``sample``
    native | msb16 | u8 | f16 | f32, and for RGB ``matrix`` bt601 | bt709 | bt2020, ``full_range`` and
    ``upsample`` nearest | bilinear (names, or the P265R_* integers).  ``crop`` = (left, right, top, bottom)
    in luma samples, relative to each picture's own size; ``pitch_align`` > 1 rounds every pitch and plane
    offset up to it.  ``size`` = (width, height): the scaled export (p265r_batch_export_resized) -- every frame slot
    has this size whatever its picture's, the crop window filtered by ``resize`` nearest | bilinear | area (area:
    downscale only; ``upsample`` is then ignored); ``scale`` / ``bias`` (3-tuples, f16 / f32 samples only): the
    float outputs are v * scale[c] + bias[c] instead of v / (2^BitDepth - 1)."""
    format: object = "planar"
    sample: object = "native"
    matrix: object = "bt709"
    full_range: bool = False
    upsample: object = "nearest"
    crop: tuple = (0, 0, 0, 0)
    pitch_align: int = 1
    size: object = None
    resize: object = "bilinear"
    scale: object = None
    bias: object = None

    @staticmethod
    def named(name, **kw):
        """The command line's format names: i420 (planar, native), nv12 (semi-planar, native), p010 (semi-planar,
        MSB-justified 16 bit), rgb24 (packed uint8), rgb-planar-f16."""
        table = {"i420": ("planar", "native"), "nv12": ("semiplanar", "native"), "p010": ("semiplanar", "msb16"),
                 "rgb24": ("rgb_packed", "u8"), "rgb-planar-f16": ("rgb_planar", "f16")}
        if name not in table:
            raise ValueError("unknown output format %r" % (name,))
        return ExportSpec(format=table[name][0], sample=table[name][1], **kw)

    def desc(self):
        """The p265r_export_desc of this spec, layout fields zero."""
        def enum(v, names, what):
            if isinstance(v, str):
                if v not in names:
                    raise ValueError("unknown %s %r" % (what, v))
                return names[v]
            return int(v)
        d = _lib.ExportDesc()
        d.format, d.sample = enum(self.format, _FORMATS, "format"), enum(self.sample, _SAMPLES, "sample")
        d.matrix, d.upsample = enum(self.matrix, _MATRICES, "matrix"), enum(self.upsample, _UPSAMPLES, "upsample")
        d.full_range = int(self.full_range)
        d.crop_left, d.crop_right, d.crop_top, d.crop_bottom = (int(v) for v in self.crop)
        return d

    def resize_desc(self):
        """The p265r_resize_desc of this spec (``size`` set)."""
        if self.size is None:
            raise ValueError("size: the (width, height) of the scaled export")
        r = _lib.ResizeDesc()
        r.out_width, r.out_height = int(self.size[0]), int(self.size[1])
        if isinstance(self.resize, str):
            if self.resize not in _FILTERS:
                raise ValueError("unknown resize filter %r" % (self.resize,))
            r.filter = _FILTERS[self.resize]
        else:
            r.filter = int(self.resize)
        if self.scale is not None or self.bias is not None:
            sc = (1.0, 1.0, 1.0) if self.scale is None else tuple(self.scale)
            bi = (0.0, 0.0, 0.0) if self.bias is None else tuple(self.bias)
            if len(sc) != 3 or len(bi) != 3:
                raise ValueError("scale / bias: one value per output channel (3)")
            r.flags = _lib.RS_NORM
            for c in range(3):
                r.scale[c], r.bias[c] = float(sc[c]), float(bi[c])
        return r


class ExportLayout:
    """A filled p265r_export_desc plus what Python needs to view a frame slot: the element dtype and, per
    picture size, the shape and byte strides of every destination plane."""

    def __init__(self, desc, bit_depth, mono=False, resize=None):
        self.desc = desc
        self.resize = resize                     # the p265r_resize_desc of a scaled export, else None
        self.size = (int(resize.out_width), int(resize.out_height)) if resize is not None else None
        native = np.dtype(np.uint16 if bit_depth > 8 else np.uint8)
        self.dtype = {_lib.SMP_NATIVE: native, _lib.SMP_MSB16: np.dtype(np.uint16), _lib.SMP_U8: np.dtype(np.uint8),
                      _lib.SMP_F16: np.dtype(np.float16), _lib.SMP_F32: np.dtype(np.float32)}[desc.sample]
        # (a monochrome source: planar is the Y plane alone; semi-planar keeps its CbCr plane, written mid-grey)
        self.n_planes = {_lib.FMT_PLANAR: 1 if mono else 3, _lib.FMT_SEMIPLANAR: 2, _lib.FMT_RGB_PLANAR: 3,
                         _lib.FMT_RGB_PACKED: 1}[desc.format]
        self.plane_off = [int(desc.plane_off[k]) for k in range(self.n_planes)]
        self.pitch = [int(desc.pitch[k]) for k in range(self.n_planes)]
        self.frame_bytes = int(desc.frame_bytes)
        self.crop = (desc.crop_left, desc.crop_right, desc.crop_top, desc.crop_bottom)

    def plane_view(self, k, size):
        """(shape, byte strides) of plane ``k`` of a picture of luma ``size`` = (width, height) before the crop; a
        scaled export: of its output size, whatever the picture's."""
        l, r, t, b = self.crop
        if self.size is not None:
            w, h = self.size
        else:
            w, h = int(size[0]) - l - r, int(size[1]) - t - b
        es, f = self.dtype.itemsize, self.desc.format
        if f == _lib.FMT_RGB_PACKED:
            return (h, w, 3), (self.pitch[0], 3 * es, es)
        if f == _lib.FMT_SEMIPLANAR and k == 1:
            return (h // 2, w // 2, 2), (self.pitch[1], 2 * es, es)
        if f == _lib.FMT_PLANAR and k > 0:
            return (h // 2, w // 2), (self.pitch[k], es)
        return (h, w), (self.pitch[k], es)


def export_layout(params, spec, size=None):
    """ExportLayout of ``spec`` for pictures of ``size`` = (width, height) (default: the params' size), through
    the C p265r_export_layout (host only: no context, no device); with ``spec.size`` the layout of a frame of that
    size, through p265r_resize_layout."""
    d = spec.desc()
    pc = _params_c(params)
    if spec.size is not None:
        rs = spec.resize_desc()
        _lib.check(_lib.load().p265r_resize_layout(ctypes.byref(pc), ctypes.byref(d), ctypes.byref(rs), int(spec.pitch_align)),
                   "p265r_resize_layout")
        return ExportLayout(d, int(params["bit_depth_luma"]), mono=R.is_mono(params), resize=rs)
    w, h = (0, 0) if size is None else (int(size[0]), int(size[1]))
    _lib.check(_lib.load().p265r_export_layout(ctypes.byref(pc), w, h, ctypes.byref(d), int(spec.pitch_align)),
               "p265r_export_layout")
    return ExportLayout(d, int(params["bit_depth_luma"]), mono=R.is_mono(params))


@dataclass(frozen=True)
class GridSpec:
    """A p265r_grid_desc: ``rows`` x ``cols`` pictures (row-major) form one canvas, of which ``out_width`` x
    ``out_height`` is the image; the ExportSpec's crop is taken inside that image.  ``orientation`` = k | m << 2: the
    frame is turned k quarter turns anticlockwise, then (m = 1) mirrored left-right -- np.rot90(F, k), then [:, ::-1]."""
    rows: int
    cols: int
    out_width: int
    out_height: int
    orientation: int = 0

    def desc(self):
        g = _lib.GridDesc()
        g.rows, g.cols, g.out_width, g.out_height = int(self.rows), int(self.cols), int(self.out_width), int(self.out_height)
        g.orientation = int(self.orientation)
        return g

    def frame_size(self, crop=(0, 0, 0, 0)):
        """(width, height) of the oriented frame under ``crop``."""
        w, h = self.out_width - crop[0] - crop[1], self.out_height - crop[2] - crop[3]
        return (h, w) if self.orientation & 1 else (w, h)


@dataclass(frozen=True)
class GridFrame:
    """A p265r_grid_frame, one frame of the scaled grid export (ReconContext.export_grid_resized): ``rows`` x ``cols``
    tiles (row-major) form the frame's canvas, of which ``out_width`` x ``out_height`` is the image; ``crop`` = (left,
    right, top, bottom) cuts the window inside that image; ``orientation`` = k | m << 2 as for GridSpec."""
    rows: int
    cols: int
    out_width: int
    out_height: int
    crop: tuple = (0, 0, 0, 0)
    orientation: int = 0

    def fill(self, f):
        f.rows, f.cols, f.out_width, f.out_height = int(self.rows), int(self.cols), int(self.out_width), int(self.out_height)
        f.crop_left, f.crop_right, f.crop_top, f.crop_bottom = (int(v) for v in self.crop)
        f.orientation = int(self.orientation)
        return f

    @property
    def tiles(self):
        return int(self.rows) * int(self.cols)


def grid_frames_c(frames):
    """The p265r_grid_frame array of a list of GridFrame."""
    arr = (_lib.GridFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        f.fill(arr[i])
    return arr


def grid_resize_plan(params, spec, frames, tile=None):
    """The per-frame constants of the scaled grid export's kernels (p265r_grid_resize_plan, host only): per frame a
    dict of tile0, cols, window (left, top, W, H), pre_turn (pw, ph), fx, fy, transpose, stage."""
    d, rs = spec.desc(), spec.resize_desc()
    pc = _params_c(params)
    tw, th = (0, 0) if tile is None else (int(tile[0]), int(tile[1]))
    out = (ctypes.c_int32 * (12 * max(len(frames), 1)))()
    _lib.check(_lib.load().p265r_grid_resize_plan(ctypes.byref(pc), tw, th, ctypes.byref(d), ctypes.byref(rs),
                                                  grid_frames_c(frames), len(frames), out), "p265r_grid_resize_plan")
    res = []
    for i in range(len(frames)):
        v = [int(x) for x in out[12 * i:12 * i + 12]]
        res.append({"tile0": v[0], "cols": v[1], "window": tuple(v[2:6]), "pre_turn": (v[6], v[7]), "fx": v[8], "fy": v[9],
                    "transpose": v[10], "stage": v[11]})
    return res


def grid_layout(params, spec, grid, tile=None):
    """ExportLayout of the frame a grid of ``tile`` = (width, height) pictures (default: the params' size) gives,
    through the C p265r_grid_layout (host only: no context, no device).  Every plane view has the oriented frame's
    size, whatever size is asked for."""
    if spec.size is not None:
        raise ValueError("a grid export is not scaled (ExportSpec.size)")
    d, g = spec.desc(), grid.desc()
    pc = _params_c(params)
    tw, th = (0, 0) if tile is None else (int(tile[0]), int(tile[1]))
    _lib.check(_lib.load().p265r_grid_layout(ctypes.byref(pc), tw, th, ctypes.byref(g), ctypes.byref(d), int(spec.pitch_align)),
               "p265r_grid_layout")
    lay = ExportLayout(d, int(params["bit_depth_luma"]), mono=R.is_mono(params))
    lay.size = grid.frame_size(tuple(int(v) for v in spec.crop))
    lay.grid = g
    return lay


def export_coefficients(spec, bit_depth):
    """The eight integers of the RGB conversion (p265r_export_coefficients, host only)."""
    d = spec.desc()
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load().p265r_export_coefficients(ctypes.byref(d), int(bit_depth), out), "p265r_export_coefficients")
    return [int(v) for v in out]


def plane_hash_host(plane, hash_type, seg_words=0):
    """decoded_picture_hash value (D.3.19) of one uint8 or uint16 plane (any row stride), as the SEI carries it,
    through p265r_plane_hash_host: the split arithmetic of the device kernels on the host, the message cut into
    segments of ``seg_words`` 32-bit words (0: one) that are combined last first.  Host only: no context."""
    p = np.asarray(plane)
    if p.ndim != 2 or p.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)) or p.strides[1] != p.itemsize:
        raise ValueError("plane: a 2-D uint8 or uint16 array with contiguous rows")
    if int(hash_type) not in _lib.HASH_BYTES:
        raise _lib.P265RError(_lib.EINVAL, "p265r_plane_hash_host")
    out = (ctypes.c_uint8 * 16)()
    _lib.check(_lib.load().p265r_plane_hash_host(p.ctypes.data, p.shape[1], p.shape[0], p.strides[0], p.itemsize,
                                                 int(hash_type), int(seg_words), out), "p265r_plane_hash_host")
    return bytes(out)[:_lib.HASH_BYTES[int(hash_type)]]


class DevicePlane:
    """One plane of one exported frame in device memory: a version-3 ``__cuda_array_interface__`` that array
    libraries on the same GPU wrap without a copy.  The memory belongs to the DeviceFrames it came from."""

    def __init__(self, owner, ptr, shape, strides, dtype):
        self.owner, self.ptr, self.shape, self.strides, self.dtype = owner, int(ptr), tuple(shape), tuple(strides), dtype

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "strides": self.strides,
                "version": 3}


class DeviceFrames:
    """The frame slots an export wrote (or will have written once its batch's lane is idle): ``ptr`` /
    ``nbytes`` of the whole buffer, ``layout``, ``sizes`` = the uncropped luma size of the picture in each slot.
    ``plane(i, k)`` views plane ``k`` of slot ``i`` on the device, ``to_host()`` copies everything back once."""

    def __init__(self, ptr, nbytes, layout, sizes, buffer=None, ctx=None, batch=None):
        self.ptr, self.nbytes, self.layout, self.sizes = int(ptr), int(nbytes), layout, [tuple(s) for s in sizes]
        self._buffer, self._ctx, self._batch = buffer, ctx, batch

    def __len__(self):
        return len(self.sizes)

    def plane(self, i, k):
        if not 0 <= i < len(self.sizes) or not 0 <= k < self.layout.n_planes:
            raise IndexError("slot %d plane %d" % (i, k))
        shape, strides = self.layout.plane_view(k, self.sizes[i])
        return DevicePlane(self, self.ptr + i * self.layout.frame_bytes + self.layout.plane_off[k], shape, strides,
                           self.layout.dtype)

    def batch_array(self, k=0):
        """Plane ``k`` of ALL slots as one ``__cuda_array_interface__``: (n, 3, H, W) for rgb_planar (k = 0: its three
        planes), (n, H, W, 3) for rgb_packed, (n, H, W) (semi-planar CbCr: (n, H / 2, W / 2, 2)) otherwise.  The strides
        come from frame_bytes, plane_off and pitch.  ValueError when the slots are not of one size (no ``size`` and a
        ragged batch) or the R, G, B plane offsets are not evenly spaced."""
        lay = self.layout
        if not 0 <= k < lay.n_planes:
            raise IndexError("plane %d" % k)
        if not self.sizes:
            raise ValueError("batch_array: no slots")
        views = {lay.plane_view(k, s) for s in self.sizes}
        if len(views) != 1:
            raise ValueError("batch_array: the slots are not of one size (export with ExportSpec(size=...))")
        shape, strides = views.pop()
        off = lay.plane_off[k]
        if lay.desc.format == _lib.FMT_RGB_PLANAR:
            if k != 0:
                raise IndexError("rgb_planar: batch_array(0) holds the three planes")
            step = lay.plane_off[1] - lay.plane_off[0]
            if lay.plane_off[2] - lay.plane_off[1] != step or step <= 0 or \
                    lay.pitch[1] != lay.pitch[0] or lay.pitch[2] != lay.pitch[0]:
                raise ValueError("batch_array: the R, G, B planes are not evenly spaced")
            shape, strides = (3,) + shape, (step,) + strides
        return DevicePlane(self, self.ptr + off, (len(self.sizes),) + shape, (lay.frame_bytes,) + strides, lay.dtype)

    def _download(self):
        from . import hip
        if self._ctx is not None:
            self._ctx.status(self._batch)
        host = np.empty(self.nbytes, np.uint8)
        hip.check(hip.lib().hipMemcpy(host.ctypes.data, ctypes.c_void_p(self.ptr), self.nbytes, hip.D2H), "hipMemcpy D2H")
        return host

    def to_host(self):
        """Wait for the batch, copy the buffer back in one piece; -> per slot a list of numpy views of its planes."""
        return self.host_views(self._download())

    def host_views(self, host):
        """numpy views per slot and plane of a host copy of the buffer (uint8, ``nbytes`` long)."""
        out = []
        for i, size in enumerate(self.sizes):
            planes = []
            for k in range(self.layout.n_planes):
                shape, strides = self.layout.plane_view(k, size)
                planes.append(np.ndarray(shape, self.layout.dtype, host, i * self.layout.frame_bytes + self.layout.plane_off[k],
                                         strides))
            out.append(planes)
        return out

    def detach(self):
        """The batch is complete (and may be freed): nothing left to wait for."""
        self._ctx = self._batch = None

    def host(self):
        """A host copy of the whole buffer, made once (one D2H copy) and kept with this object."""
        if getattr(self, "_host", None) is None:
            self._host = self._download()
        return self._host

    def slot(self, i):
        """DeviceFrame view of slot ``i`` (keeps this buffer alive)."""
        return DeviceFrame(self, i)

    def free(self):
        """Free the buffer if this object allocated it (a caller's ``dst`` stays the caller's)."""
        if self._buffer is not None:
            if self._ctx is not None and self._batch is not None and self._batch.handle and self._ctx.handle:
                self._ctx.status(self._batch)          # the export may still be writing it
            self._buffer.free()
            self._buffer = None
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceFrame:
    """One exported frame: slot ``index`` of a DeviceFrames, which stays allocated while any of its slot views
    lives (``release()`` drops this one's hold)."""

    def __init__(self, frames, index):
        self.frames, self.index = frames, int(index)

    @property
    def planes(self):
        return [self.frames.plane(self.index, k) for k in range(self.frames.layout.n_planes)]

    def to_host(self):
        """numpy views of this frame's planes in the buffer's host copy (DeviceFrames.host: one copy per batch)."""
        return self.frames.host_views(self.frames.host())[self.index]

    def tobytes(self):
        """The frame's planes back to back, rows tight: what a raw video file holds."""
        return b"".join(np.ascontiguousarray(p).tobytes() for p in self.to_host())

    def release(self):
        self.frames = None


class Batch:
    def __init__(self, ctx, handle, pics, keep):
        self.ctx, self.handle, self.pics, self._keep = ctx, handle, pics, keep
        self.device_frames = None            # decoder: the DeviceFrames exported from this batch

    def free(self):
        if self.handle:
            _lib.check(self.ctx.lib.p265r_batch_free(self.ctx.handle, self.handle), "p265r_batch_free")
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ReconContext:
    """One HIP device + stream + parameter set (p265r_ctx)."""

    def __init__(self, params, device=0, scaling=None):
        """``scaling``: the 2032-byte intra ScalingFactor table (p265r_set_scaling_factors) when
        params.scaling_list_enabled."""
        self.lib = _lib.load()
        self.params = params
        self._pc = _params_c(params)
        h = ctypes.c_void_p()
        _lib.check(self.lib.p265r_create(device, ctypes.byref(self._pc), ctypes.byref(h)), "p265r_create")
        self.handle = h
        self.device = device
        if scaling is not None:
            self.set_scaling_factors(scaling)

    def set_scaling_factors(self, factors):
        """The intra ScalingFactor table (2032 bytes, include/p265r.h) for every later run."""
        f = np.ascontiguousarray(factors, np.uint8).reshape(-1)
        _lib.check(self.lib.p265r_set_scaling_factors(self.handle, f.ctypes.data, int(f.size)),
                   "p265r_set_scaling_factors")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.p265r_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- marshalling ------------------------------------------------------------
    def _pictures_c(self, pics, outs=None, recons=None):
        keep = []
        arr = (_lib.PictureC * len(pics))()
        for i, p in enumerate(pics):
            R.check_shapes(self.params, p)      # record contents: validated by p265r_batch_upload
            pp = R.pic_params(self.params, p)
            if pp is not self.params:           # a smaller picture of a ragged batch
                arr[i].pic_width, arr[i].pic_height = int(pp["pic_width"]), int(pp["pic_height"])
            ctus = np.ascontiguousarray(p.ctus, R.CTU_DTYPE)
            tbs = np.ascontiguousarray(p.tbs, R.TB_DTYPE)
            coef = np.ascontiguousarray(p.coef, np.int16)
            keep += [ctus, tbs, coef]
            c = arr[i]
            c.ctus = ctus.ctypes.data
            c.tbs = tbs.ctypes.data if len(tbs) else None
            c.n_tbs = len(tbs)
            c.coef = coef.ctypes.data if len(coef) else None
            c.n_coef = len(coef)
            if p.nofilter is not None:
                nf = np.ascontiguousarray(p.nofilter, np.uint8)
                keep.append(nf)
                c.nofilter = nf.ctypes.data
            for k in range(R.n_planes(self.params)):
                if outs is not None:
                    c.out[k] = outs[i][k].ctypes.data
                if recons is not None:
                    c.recon[k] = recons[i][k].ctypes.data
            if p.recon_input is not None:
                c.flags = R.PIC_RECON_INPUT
                dts = R.plane_dtypes(self.params)
                planes = [np.ascontiguousarray(p.recon_input[k], dts[k]) for k in range(len(dts))]
                for k, (pl, shp) in enumerate(zip(planes, plane_shapes(pp))):
                    if pl.shape != shp:
                        raise R.RecordError("recon_input plane %d has shape %s, expected %s" % (k, pl.shape, shp))
                    c.recon[k] = pl.ctypes.data
                keep += planes
        return arr, keep

    def _alloc_planes(self, pics):
        dts = R.plane_dtypes(self.params)
        return [[np.empty(s, dt) for s, dt in zip(plane_shapes(R.pic_params(self.params, p)), dts)] for p in pics]

    # ---- batch API --------------------------------------------------------------
    def upload(self, pics, sparse=False):
        """Records -> a device-resident batch.  ``sparse``: the coefficients of the transformed TBs go up
        as their non-zero entries and are expanded on the device (p265r_batch_upload_sparse); ``pics`` are
        then records.SparsePicture, or Picture (sparsified here through p265r_sparsify).  The batch is the
        same either way."""
        if not sparse:
            arr, keep = self._pictures_c(pics)
            h = ctypes.c_void_p()
            _lib.check(self.lib.p265r_batch_upload(self.handle, arr, len(pics), ctypes.byref(h)), "p265r_batch_upload")
            return Batch(self, h, pics, keep)
        sps = [p if isinstance(p, R.SparsePicture) else sparsify(p) for p in pics]
        arr, keep = self._pictures_c(sps)
        sc = (_lib.SparseCoefC * len(sps))()
        for i, p in enumerate(sps):
            nz = np.ascontiguousarray(p.nz, np.uint32)
            keep.append(nz)
            sc[i].nz = nz.ctypes.data if len(nz) else None
            sc[i].n_nz = len(nz)
        h = ctypes.c_void_p()
        _lib.check(self.lib.p265r_batch_upload_sparse(self.handle, arr, sc, len(sps), ctypes.byref(h)),
                   "p265r_batch_upload_sparse")
        return Batch(self, h, pics, keep)

    def upload_bytes(self, batch):
        """Host-to-device bytes the batch's upload enqueued (p265r_batch_upload_bytes)."""
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.p265r_batch_upload_bytes(self.handle, batch.handle, ctypes.byref(n)),
                   "p265r_batch_upload_bytes")
        return int(n.value)

    def run(self, batch):
        _lib.check(self.lib.p265r_batch_run(self.handle, batch.handle), "p265r_batch_run")

    def download(self, batch, with_recon=False, only=None, into=None):
        """Planes of the batch's pictures (after its last run).  ``only``: indices of the pictures
        to copy back (the others are not transferred and come back as None).  ``into``: the output
        planes to fill instead of new arrays (a frame pool: per picture three C-contiguous arrays of the
        planes' shapes and dtype, e.g. a previous download's result) -- fresh host memory costs a page
        fault per 4 KB on its first write."""
        n = len(batch.pics)
        sel = set(range(n)) if only is None else {int(i) for i in only}
        shp = [plane_shapes(R.pic_params(self.params, p)) for p in batch.pics]
        dts = R.plane_dtypes(self.params)
        if into is not None:
            if len(into) != n:
                raise ValueError("into: one entry per picture")
            for i in sel:
                for k in range(len(dts)):
                    a = into[i][k]
                    if a.shape != tuple(shp[i][k]) or a.dtype != dts[k] or not a.flags.c_contiguous or not a.flags.writeable:
                        raise ValueError("into: picture %d plane %d does not match the plane layout" % (i, k))
            outs = [list(into[i]) if i in sel else None for i in range(n)]
        else:
            outs = [[np.empty(s, dt) for s, dt in zip(shp[i], dts)] if i in sel else None for i in range(n)]
        recs = ([[np.empty(s, dt) for s, dt in zip(shp[i], dts)] if i in sel else None for i in range(n)]
                if with_recon else None)
        arr = (_lib.PictureC * n)()
        for i in sel:
            for k in range(len(dts)):
                arr[i].out[k] = outs[i][k].ctypes.data
                if recs is not None:
                    arr[i].recon[k] = recs[i][k].ctypes.data
        _lib.check(self.lib.p265r_batch_download(self.handle, batch.handle, arr, n), "p265r_batch_download")
        return (outs, recs) if with_recon else outs

    def status(self, batch):
        """Wait for the batch and raise P265RError if any of its runs failed on the device
        (p265r_batch_status: the row kernel's sticky error word)."""
        _lib.check(self.lib.p265r_batch_status(self.handle, batch.handle), "p265r_batch_status")

    def digest(self, batch, recon=False):
        """Per-picture digests of the batch's planes after its last run, computed on the device
        (p265r_batch_digest; no plane download): uint64 array [n_pictures, 3] (Y, Cb, Cr), equal to
        digest.picture_digest() of the planes download() would return (recon: the reconstruction
        before the in-loop filters).  Raises P265RError like status()."""
        n = len(batch.pics)
        out = np.zeros(3 * n, np.uint64)
        _lib.check(self.lib.p265r_batch_digest(self.handle, batch.handle, 1 if recon else 0,
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 3 * n),
                   "p265r_batch_digest")
        return out.reshape(n, 3)

    def digest_async(self, batch, slot, recon=False):
        """Enqueue the device digest of the batch's planes after every run enqueued so far into digest
        slot ``slot`` (0 .. _lib.DIGEST_SLOTS - 1) and return at once (p265r_batch_digest_async)."""
        _lib.check(self.lib.p265r_batch_digest_async(self.handle, batch.handle, 1 if recon else 0, int(slot)),
                   "p265r_batch_digest_async")

    def digest_slots(self, batch, n_slots):
        """Wait for the batch's lane; -> uint64 array [n_slots, n_pictures, 3] of the digest slots
        (p265r_batch_digest_slots).  Raises P265RError like status()."""
        n = len(batch.pics)
        out = np.zeros(3 * n * n_slots, np.uint64)
        _lib.check(self.lib.p265r_batch_digest_slots(self.handle, batch.handle,
                                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(n_slots)),
                   "p265r_batch_digest_slots")
        return out.reshape(n_slots, n, 3)

    def job_count(self, batch):
        """(luma, chroma) intra jobs of the batch's last run (p265r_batch_job_count)."""
        lu, ch = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(self.lib.p265r_batch_job_count(self.handle, batch.handle, ctypes.byref(lu), ctypes.byref(ch)),
                   "p265r_batch_job_count")
        return int(lu.value), int(ch.value)

    # ---- device-side picture hash ------------------------------------------------------
    def hash_async(self, batch, hash_type):
        """Enqueue, behind every run and export of the batch so far, the decoded picture hash (D.3.19;
        _lib.HASH_MD5 / HASH_CRC / HASH_CHECKSUM) of its output planes on the device and return at once
        (p265r_batch_hash_async)."""
        _lib.check(self.lib.p265r_batch_hash_async(self.handle, batch.handle, int(hash_type)), "p265r_batch_hash_async")

    def hash_read(self, batch):
        """Wait for the batch's lane; -> uint8 array [n_pictures, 3, 16] of the last hash_async, each plane's
        16 bytes in the SEI's form (p265r_batch_hash_read: 48 bytes per picture).  Raises like status()."""
        n = len(batch.pics)
        out = np.zeros((n, 3, 16), np.uint8)
        _lib.check(self.lib.p265r_batch_hash_read(self.handle, batch.handle,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 48 * n),
                   "p265r_batch_hash_read")
        return out

    def picture_hash(self, batch, hash_type):
        """hash_async + hash_read: per picture three ``bytes`` (Y, Cb, Cr) of the SEI's length (16, 2 or 4);
        a monochrome context: one (Y)."""
        if int(hash_type) not in _lib.HASH_BYTES:
            raise _lib.P265RError(_lib.EINVAL, "p265r_batch_hash_async")
        self.hash_async(batch, hash_type)
        nb = _lib.HASH_BYTES[int(hash_type)]
        return [[h[c, :nb].tobytes() for c in range(R.n_planes(self.params))] for h in self.hash_read(batch)]

    # ---- device-side output -----------------------------------------------------------
    def export_layout(self, spec, pic=None):
        """ExportLayout of ``spec`` for a picture (a records Picture, a (width, height) pair, or None = the
        context's size; a ragged batch shares the layout of its largest picture)."""
        size = None
        if pic is not None:
            pp = R.pic_params(self.params, pic) if hasattr(pic, "ctus") else None
            size = (int(pp["pic_width"]), int(pp["pic_height"])) if pp is not None else (int(pic[0]), int(pic[1]))
        return export_layout(self.params, spec, size)

    def export(self, batch, spec, dst=None, dst_bytes=None, only=None):
        """Enqueue, after the batch's runs, the conversion of its pictures (``only``: these, in this order) into
        frame slots in device memory (p265r_batch_export) and return at once -> DeviceFrames.  ``dst`` None:
        the buffer is allocated here (hipMalloc) and owned by the result; an integer device address (with
        ``dst_bytes``): the caller's memory on this context's device, e.g. ``tensor.data_ptr()``.  The slots have
        the tight (or ``pitch_align``) layout of the context's picture size -- or, with ``spec.size``, of that size
        (p265r_batch_export_resized: every slot the same, whatever its picture's size)."""
        from . import hip
        lay = self.export_layout(spec)
        idx = list(range(len(batch.pics))) if only is None else [int(i) for i in only]
        sizes = []
        for i in idx:
            if not 0 <= i < len(batch.pics):
                raise _lib.P265RError(_lib.EINVAL, "p265r_batch_export")
            pp = R.pic_params(self.params, batch.pics[i])
            sizes.append((int(pp["pic_width"]), int(pp["pic_height"])))
        buf = None
        if dst is None:
            hip.set_device(self.device)
            dst_bytes = lay.frame_bytes * len(idx)
            buf = hip.DeviceBuffer(dst_bytes)
            dst = buf.ptr.value
        elif dst_bytes is None:
            raise ValueError("dst_bytes: the size of the caller's buffer")
        arr = (ctypes.c_int32 * len(idx))(*idx) if only is not None else None
        try:
            if lay.resize is not None:
                _lib.check(self.lib.p265r_batch_export_resized(self.handle, batch.handle, ctypes.byref(lay.desc),
                                                               ctypes.byref(lay.resize), ctypes.c_void_p(int(dst)),
                                                               int(dst_bytes), arr, len(idx)), "p265r_batch_export_resized")
            else:
                _lib.check(self.lib.p265r_batch_export(self.handle, batch.handle, ctypes.byref(lay.desc),
                                                       ctypes.c_void_p(int(dst)), int(dst_bytes), arr, len(idx)),
                           "p265r_batch_export")
        except BaseException:
            if buf is not None:
                buf.free()
            raise
        return DeviceFrames(dst, dst_bytes, lay, sizes, buffer=buf, ctx=self, batch=batch)

    def grid_layout(self, spec, grid, tile=None):
        """ExportLayout of the oriented frame of a grid of ``tile``-sized pictures (a records Picture, a (width,
        height) pair, or None = the context's size)."""
        if tile is not None and hasattr(tile, "ctus"):
            pp = R.pic_params(self.params, tile)
            tile = (int(pp["pic_width"]), int(pp["pic_height"]))
        return grid_layout(self.params, spec, grid, tile)

    def export_grid(self, batch, spec, grid, dst=None, dst_bytes=None, only=None):
        """Enqueue, after the batch's runs, the assembly of ``grid.rows * grid.cols`` pictures per frame into frame
        slots in device memory (p265r_batch_export_grid) and return at once -> DeviceFrames, one slot per frame.
        ``only`` lists the pictures, tile r * cols + c of frame f at f * rows * cols + r * cols + c (None: the batch in
        order); ``dst`` / ``dst_bytes`` as for ``export``."""
        from . import hip
        tiles = int(grid.rows) * int(grid.cols)
        idx = list(range(len(batch.pics))) if only is None else [int(i) for i in only]
        if tiles <= 0 or not idx or len(idx) % tiles or any(not 0 <= i < len(batch.pics) for i in idx):
            raise _lib.P265RError(_lib.EINVAL, "p265r_batch_export_grid")
        n_frames = len(idx) // tiles
        lay = self.grid_layout(spec, grid, batch.pics[idx[0]])
        buf = None
        if dst is None:
            hip.set_device(self.device)
            dst_bytes = lay.frame_bytes * n_frames
            buf = hip.DeviceBuffer(dst_bytes)
            dst = buf.ptr.value
        elif dst_bytes is None:
            raise ValueError("dst_bytes: the size of the caller's buffer")
        arr = (ctypes.c_int32 * len(idx))(*idx) if only is not None else None
        try:
            _lib.check(self.lib.p265r_batch_export_grid(self.handle, batch.handle, ctypes.byref(lay.desc), ctypes.byref(lay.grid),
                                                        ctypes.c_void_p(int(dst)), int(dst_bytes), arr, n_frames),
                       "p265r_batch_export_grid")
        except BaseException:
            if buf is not None:
                buf.free()
            raise
        return DeviceFrames(dst, dst_bytes, lay, [lay.size] * n_frames, buffer=buf, ctx=self, batch=batch)

    def export_grid_resized(self, batch, spec, frames, dst=None, dst_bytes=None, only=None):
        """Enqueue, after the batch's runs, the scaled grid export (p265r_batch_export_grid_resized) and return at once
        -> DeviceFrames, one slot of ``spec.size`` per GridFrame of ``frames``, whatever its grid, window or
        orientation: ``batch_array()`` is the dense view.  ``only`` lists the tiles frame after frame (None: the batch
        in order); ``dst`` / ``dst_bytes`` as for ``export``."""
        from . import hip
        if spec.size is None:
            raise ValueError("export_grid_resized: ExportSpec.size, the (width, height) of every slot")
        frames = list(frames)
        idx = list(range(len(batch.pics))) if only is None else [int(i) for i in only]
        if not frames or sum(f.tiles for f in frames) != len(idx) or any(not 0 <= i < len(batch.pics) for i in idx):
            raise _lib.P265RError(_lib.EINVAL, "p265r_batch_export_grid_resized")
        lay = self.export_layout(spec)
        buf = None
        if dst is None:
            hip.set_device(self.device)
            dst_bytes = lay.frame_bytes * len(frames)
            buf = hip.DeviceBuffer(dst_bytes)
            dst = buf.ptr.value
        elif dst_bytes is None:
            raise ValueError("dst_bytes: the size of the caller's buffer")
        arr = (ctypes.c_int32 * len(idx))(*idx) if only is not None else None
        try:
            _lib.check(self.lib.p265r_batch_export_grid_resized(self.handle, batch.handle, ctypes.byref(lay.desc),
                                                                ctypes.byref(lay.resize), grid_frames_c(frames), len(frames),
                                                                ctypes.c_void_p(int(dst)), int(dst_bytes), arr),
                       "p265r_batch_export_grid_resized")
        except BaseException:
            if buf is not None:
                buf.free()
            raise
        return DeviceFrames(dst, dst_bytes, lay, [lay.size] * len(frames), buffer=buf, ctx=self, batch=batch)

    def sync(self):
        _lib.check(self.lib.p265r_sync(self.handle), "p265r_sync")

    def set_pipeline(self, depth):
        """Bind batches uploaded from now on round-robin to `depth` streams (p265r_set_pipeline)."""
        _lib.check(self.lib.p265r_set_pipeline(self.handle, int(depth)), "p265r_set_pipeline")

    def set_row_waves(self, waves):
        """Force the row kernel's build (8 / 12 waves per workgroup) or 0 = by run (p265r_set_row_waves)."""
        _lib.check(self.lib.p265r_set_row_waves(self.handle, int(waves)), "p265r_set_row_waves")

    def set_timing(self, on=True):
        _lib.check(self.lib.p265r_set_timing(self.handle, int(bool(on))), "p265r_set_timing")

    def timings_total(self):
        """Sums of the per-phase times over every run since set_timing(True), and the run count."""
        t = _lib.Timings()
        n = ctypes.c_int(0)
        _lib.check(self.lib.p265r_timings_total(self.handle, ctypes.byref(t), ctypes.byref(n)), "p265r_timings_total")
        d = {f: getattr(t, f) for f, _ in _lib.Timings._fields_ if f != "reserved"}
        d["runs"] = n.value
        return d

    def describe(self):
        """Effective configuration of this context (p265r_describe) as a dict."""
        import json
        buf = ctypes.create_string_buffer(1024)
        n = _lib.check(self.lib.p265r_describe(self.handle, buf, len(buf)), "p265r_describe")
        if n >= len(buf):
            buf = ctypes.create_string_buffer(n + 1)
            _lib.check(self.lib.p265r_describe(self.handle, buf, len(buf)), "p265r_describe")
        return json.loads(buf.value.decode())

    def last_timings(self):
        t = _lib.Timings()
        _lib.check(self.lib.p265r_last_timings(self.handle, ctypes.byref(t)), "p265r_last_timings")
        return {f: getattr(t, f) for f, _ in _lib.Timings._fields_ if f != "reserved"}

    # ---- one-shot API (submit / wait) -------------------------------------------------
    def decode(self, pics, with_recon=False, sparse=False):
        """Upload, run and download in one call.  ``sparse``: through the sparse upload (the submit / wait
        pair of the C ABI is dense; this is upload(sparse=True) + run + download)."""
        if sparse:
            b = self.upload(pics, sparse=True)
            try:
                self.run(b)
                wr = with_recon and pics[0].recon_input is None
                res = self.download(b, with_recon=wr)
                return (res, None) if with_recon and not wr else res
            finally:
                b.free()
        outs = self._alloc_planes(pics)
        recs = self._alloc_planes(pics) if with_recon and pics[0].recon_input is None else None
        arr, keep = self._pictures_c(pics, outs, recs)
        _lib.check(self.lib.p265r_submit(self.handle, arr, len(pics)), "p265r_submit")
        _lib.check(self.lib.p265r_wait(self.handle), "p265r_wait")
        del keep
        return (outs, recs) if with_recon else outs


def decode_pictures(ctx, pics):
    """ReconContext.decode with the reconstruction too, as DecodedPicture objects (the
    read-back surface of decoder/cu.py:617-632)."""
    outs, recs = ctx.decode(pics, with_recon=True)
    return [DecodedPicture(o, r) for o, r in zip(outs, recs)]


def device_count():
    return _lib.check(_lib.load().p265r_device_count(), "p265r_device_count")
