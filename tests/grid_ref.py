"""numpy restatement of the grid export (include/p265r.h, "grid export"), written from the header's words and not
from the kernel: the canvas is assembled from the tiles, tests/export_ref.py converts it as ONE decoded picture whose
crop is the window, then numpy turns and mirrors every destination plane.

    canvas   cols tw x rows th; luma sample (x, y) = sample (x % tw, y % th) of tile (y / th) * cols + x / tw
    window   [crop_left, out_width - crop_right) x [crop_top, out_height - crop_bottom)
    F        export_ref.export(canvas, crop = the window)
    result   np.rot90(F, k), then [:, ::-1] when m      (orientation = k | m << 2)

A monochrome source (tiles of one plane) follows export_ref's rules for it, restated in tests/mono.py terms here:
planar = Y alone, semi-planar = Y + grey CbCr, RGB = the formula at Cb = Cr = 1 << (B - 1).
"""
import numpy as np

import export_ref as X


def canvas(tiles, rows, cols):
    """The canvas planes of rows * cols tiles (each a list of planes), row-major."""
    n = len(tiles[0])
    return [np.block([[tiles[r * cols + c][k] for c in range(cols)] for r in range(rows)]) for k in range(n)]


def orient(plane, orientation):
    k, m = orientation & 3, orientation >> 2
    out = np.rot90(plane, k)                     # (axes 0, 1: a trailing pair / triple axis moves with its element)
    return out[:, ::-1] if m else out


def frame(tiles, rows, cols, out_size, B, fmt, sample="native", matrix="bt709", full_range=False, upsample_mode="nearest",
          crop=(0, 0, 0, 0), orientation=0):
    """The tight destination planes of one grid frame."""
    cv = canvas(tiles, rows, cols)
    h, w = cv[0].shape
    l, r, t, b = crop
    win = (l, w - out_size[0] + r, t, h - out_size[1] + b)          # the window as a crop of the canvas
    if len(cv) == 1:
        planes = _mono(cv[0], B, fmt, sample, matrix, full_range, win)
    else:
        planes = X.export(cv, B, fmt, sample, matrix, full_range, upsample_mode, win)
    return [np.ascontiguousarray(orient(p, orientation)) for p in planes]


def _mono(Y, B, fmt, sample, matrix, full_range, win):
    h, w = Y.shape
    l, r, t, b = win
    dt = X.sample_dtype(sample, B)
    y = Y[t:h - b, l:w - r]
    if fmt in ("planar", "semiplanar"):
        sh = 16 - B if sample == "msb16" else 0
        out = [(y.astype(np.uint32) << sh).astype(dt)]
        if fmt == "semiplanar":
            out.append(np.full((y.shape[0] // 2, y.shape[1] // 2, 2), (1 << (B - 1)) << sh, dt))
        return out
    D = 8 if sample == "u8" else B
    half = np.full(y.shape, 1 << (B - 1))
    rgb = X.rgb_int(y, half, half, X.coefficients(matrix, full_range, B, D))
    if sample in ("f16", "f32"):
        k = np.float32(1 / (2 ** B - 1))
        rgb = [(c.astype(np.float32) * k).astype(dt) for c in rgb]
    else:
        rgb = [c.astype(dt) for c in rgb]
    return list(rgb) if fmt == "rgb_planar" else [np.stack(rgb, axis=-1)]


def pasted(tiles, rows, cols, B, fmt, **kw):
    """What assembling per-tile exports on the host gives (no crop, no orientation): the WRONG answer at every seam
    for bilinear RGB -- the teeth of the seam test."""
    per = [X.export(t, B, fmt, **kw) for t in tiles]
    return [np.block([[per[r * cols + c][k] for c in range(cols)] for r in range(rows)]) if per[0][k].ndim == 2 else
            np.concatenate([np.concatenate([per[r * cols + c][k] for c in range(cols)], axis=1) for r in range(rows)], axis=0)
            for k in range(len(per[0]))]


def seam_tiles(rows, cols, tw, th, bd=8):
    """The seam picture: luma noise, chroma constant per tile and alternating 0 / max like a chess board."""
    rng = np.random.default_rng(77)
    dt = np.uint16 if bd > 8 else np.uint8
    top = (1 << bd) - 1
    out = []
    for r in range(rows):
        for c in range(cols):
            v = top if (r + c) & 1 else 0
            out.append([rng.integers(0, top + 1, (th, tw)).astype(dt), np.full((th // 2, tw // 2), v, dt),
                        np.full((th // 2, tw // 2), top - v, dt)])
    return out
