"""numpy / Python-integer restatement of the scaled device-side output (include/p265r.h, "scaled device-side
output"), written from the header and not from the C code.  ``export_ref`` supplies the conversion after the filter.

The source of a frame is the crop window of its picture; ``resize`` takes the decoded, uncropped planes [Y, Cb, Cr]
([Y] for a monochrome source) and returns the tight destination planes of one out_width x out_height frame, in the
forms of export_ref.export.
"""
import numpy as np

import export_ref as X

FILTERS = ("nearest", "bilinear", "area")


def step(n, m):
    return (n << 16) // m


def u_of(h, n, m):
    """Source position x 2^16 in luma samples from the window's edge, for half-sample coordinate(s) h."""
    return (np.asarray(h, np.int64) * step(n, m)) >> 1


def grid_h(count, chroma_grid, vertical):
    """Half-sample coordinates of the ``count`` outputs of one axis."""
    i = np.arange(count, dtype=np.int64)
    if not chroma_grid:
        return 2 * i + 1
    return 4 * i + (2 if vertical else 1)


def nearest_index(n, m, h, chroma):
    u = u_of(h, n, m) >> 16
    return np.minimum(u >> 1, n // 2 - 1) if chroma else np.minimum(u, n - 1)


def bilinear_taps(n, m, h, chroma, vertical):
    """(i0, i1, f) for half-sample coordinate(s) h."""
    u = u_of(h, n, m)
    if not chroma:
        pos, n_p = u - 32768, n
    else:
        pos, n_p = (u - (65536 if vertical else 32768)) >> 1, n // 2          # (numpy's >> on int64 is arithmetic)
    pos = np.clip(pos, 0, (n_p - 1) << 16)
    i0 = pos >> 16
    return i0, np.minimum(i0 + 1, n_p - 1), (pos >> 8) & 255


def box(n, m, chroma_plane, chroma_grid):
    """(N, M): output i covers [i N, (i + 1) N), plane sample k covers [k M, (k + 1) M)."""
    if chroma_grid:
        return n // 2, m // 2
    return n, (2 * m if chroma_plane else m)


def area_weights(N, M, outputs, samples):
    """Dense [outputs, samples] int64 matrix of overlap lengths."""
    i = np.arange(outputs, dtype=np.int64)[:, None]
    k = np.arange(samples, dtype=np.int64)[None, :]
    return np.clip(np.minimum((k + 1) * M, (i + 1) * N) - np.maximum(k * M, i * N), 0, None)


def resize_plane(win, nw, nh, chroma_plane, chroma_grid, filt, mw, mh):
    """One plane window (its own samples: nw x nh luma, or nw/2 x nh/2 chroma) -> int64 output plane; nw, nh, mw, mh are
    the LUMA window and output sizes."""
    win = np.asarray(win, np.int64)
    ph, pw = (nh // 2, nw // 2) if chroma_plane else (nh, nw)
    assert win.shape == (ph, pw), (win.shape, ph, pw)
    oh, ow = (mh // 2, mw // 2) if chroma_grid else (mh, mw)
    hx, hy = grid_h(ow, chroma_grid, False), grid_h(oh, chroma_grid, True)
    if filt == "nearest":
        return win[nearest_index(nh, mh, hy, chroma_plane)[:, None], nearest_index(nw, mw, hx, chroma_plane)[None, :]]
    if filt == "bilinear":
        x0, x1, fx = bilinear_taps(nw, mw, hx, chroma_plane, False)
        y0, y1, fy = bilinear_taps(nh, mh, hy, chroma_plane, True)
        a, b = win[y0[:, None], x0[None, :]], win[y0[:, None], x1[None, :]]
        c, d = win[y1[:, None], x0[None, :]], win[y1[:, None], x1[None, :]]
        fx, fy = fx[None, :], fy[:, None]
        return (((256 - fx) * a + fx * b) * (256 - fy) + ((256 - fx) * c + fx * d) * fy + 32768) >> 16
    assert filt == "area" and mw <= nw and mh <= nh
    Nx, Mx = box(nw, mw, chroma_plane, chroma_grid)
    Ny, My = box(nh, mh, chroma_plane, chroma_grid)
    wx, wy = area_weights(Nx, Mx, ow, pw), area_weights(Ny, My, oh, ph)
    assert np.all(wx.sum(axis=1) == Nx) and np.all(wy.sum(axis=1) == Ny)
    total = wy @ win @ wx.T                                     # int64: below 2^38
    return (total + ((Nx * Ny) >> 1)) // (Nx * Ny)


def float_out(v, scale, bias, dt):
    """fl32(fl32(float(v) * scale) + bias), then the destination type: two separately rounded fp32 operations."""
    p = np.asarray(v).astype(np.float32) * np.float32(scale)
    return (p + np.float32(bias)).astype(dt)


def resize(planes, B, fmt, sample="native", matrix="bt709", full_range=False, crop=(0, 0, 0, 0), size=None, filt="bilinear",
           scale=None, bias=None, cache=None):
    """The tight destination planes of one frame of ``size`` = (width, height).  ``cache``: a dict the caller keeps per
    set of source planes; the filtered planes are stored there and shared by the formats that need the same ones."""
    mono = len(planes) == 1
    Y = planes[0]
    h, w = Y.shape
    l, r, t, b = crop
    nw, nh = w - l - r, h - t - b
    mw, mh = size
    dt = X.sample_dtype(sample, B)
    yw = Y[t:h - b, l:w - r]
    cw = [] if mono else [c[t // 2:(h - b) // 2, l // 2:(w - r) // 2] for c in planes[1:]]

    def plane(k, win, cp, cg):
        key = (k, tuple(crop), cp, cg, filt, mw, mh)
        if cache is None:
            return resize_plane(win, nw, nh, cp, cg, filt, mw, mh)
        if key not in cache:
            cache[key] = resize_plane(win, nw, nh, cp, cg, filt, mw, mh)
        return cache[key]

    y = plane(0, yw, False, False)
    if fmt in ("planar", "semiplanar"):
        sh = 16 - B if sample == "msb16" else 0
        out = [(y << sh).astype(dt)]
        if mono:
            if fmt == "semiplanar":
                out.append(np.full((mh // 2, mw // 2, 2), (1 << (B - 1)) << sh, dt))
            return out
        cb, cr = [(plane(1 + k, c, True, True) << sh).astype(dt) for k, c in enumerate(cw)]
        return out + ([cb, cr] if fmt == "planar" else [np.stack([cb, cr], axis=-1)])
    D = 8 if sample == "u8" else B
    co = X.coefficients(matrix, full_range, B, D)
    if mono:
        cb = cr = np.full((mh, mw), 1 << (B - 1), np.int64)
    else:
        cb, cr = [plane(1 + k, c, True, False) for k, c in enumerate(cw)]
    rgb = X.rgb_int(y, cb, cr, co)
    if sample in ("f16", "f32"):
        sc = [1 / (2 ** B - 1)] * 3 if scale is None and bias is None else ([1.0] * 3 if scale is None else scale)
        bi = [0.0] * 3 if bias is None else bias
        rgb = [float_out(c, sc[k], bi[k], dt) for k, c in enumerate(rgb)]
    else:
        rgb = [c.astype(dt) for c in rgb]
    return list(rgb) if fmt == "rgb_planar" else [np.stack(rgb, axis=-1)]
