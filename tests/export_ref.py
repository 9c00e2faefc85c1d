"""numpy restatement of the device-side output arithmetic (include/p265r.h), written from
the specification and not from the kernel: whole-plane numpy, Python's own ``round`` for the coefficients.

Inputs are the decoded, uncropped planes [Y, Cb, Cr] (what ``ReconContext.download`` returns); outputs are
the tight destination planes an export writes, as a list of arrays:

    planar      [Y (H, W), Cb (H/2, W/2), Cr (H/2, W/2)]
    semiplanar  [Y (H, W), CbCr (H/2, W/2, 2)]
    rgb_planar  [R, G, B] each (H, W)
    rgb_packed  [RGB (H, W, 3)]
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MATRICES = ("bt601", "bt709", "bt2020")


def coefficients(matrix, full_range, B, D):
    """{cy, crr, cgb, cgr, cbb, yoff, 1 << (B - 1), D} as p265r_export_coefficients returns them."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if full_range:
        my = mc = (2 ** D - 1) / (2 ** B - 1)
        yoff = 0
    else:
        my = (2 ** D - 1) / (219 * 2 ** (B - 8))
        mc = (2 ** D - 1) / (224 * 2 ** (B - 8))
        yoff = 16 << (B - 8)
    return [round(my * 2 ** 14), round(2 * (1 - kr) * mc * 2 ** 14), round(2 * kb * (1 - kb) / kg * mc * 2 ** 14),
            round(2 * kr * (1 - kr) / kg * mc * 2 ** 14), round(2 * (1 - kb) * mc * 2 ** 14), yoff, 1 << (B - 1), D]


def rgb_int(Y, Cb, Cr, co):
    """Integer R, G, B (int32 arrays, as specified: the largest sum stays under 2^28) of luma / chroma sample
    arrays of one shape (or broadcastable ones)."""
    cy, crr, cgb, cgr, cbb, yoff, half, D = (np.int32(v) for v in co)
    y = np.asarray(Y).astype(np.int32) - yoff
    cb = np.asarray(Cb).astype(np.int32) - half
    cr = np.asarray(Cr).astype(np.int32) - half
    top = 2 ** D - 1
    r = np.clip((cy * y + crr * cr + 8192) >> 14, 0, top)
    g = np.clip((cy * y - cgb * cb - cgr * cr + 8192) >> 14, 0, top)
    b = np.clip((cy * y + cbb * cb + 8192) >> 14, 0, top)
    return r, g, b


def rgb_exact(Y, Cb, Cr, matrix, full_range, B, D):
    """The float64 conversion the integers approximate, before rounding and clipping."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if full_range:
        my = mc = (2 ** D - 1) / (2 ** B - 1)
        yoff = 0
    else:
        my = (2 ** D - 1) / (219 * 2 ** (B - 8))
        mc = (2 ** D - 1) / (224 * 2 ** (B - 8))
        yoff = 16 << (B - 8)
    y = (np.asarray(Y, np.float64) - yoff) * my
    cb = (np.asarray(Cb, np.float64) - (1 << (B - 1))) * mc
    cr = (np.asarray(Cr, np.float64) - (1 << (B - 1))) * mc
    return (y + 2 * (1 - kr) * cr, y - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr, y + 2 * (1 - kb) * cb)


def upsample(C, upsample_mode):
    """A chroma plane (h/2, w/2) at every luma position of the decoded picture -> (h, w) int64."""
    C = np.asarray(C, np.int64)
    ch, cw = C.shape
    ys, xs = np.arange(2 * ch), np.arange(2 * cw)
    if upsample_mode == "nearest":
        return C[(ys >> 1)[:, None], (xs >> 1)[None, :]]
    j = ys >> 1
    up, dn = np.clip(j - 1, 0, ch - 1), np.clip(j + 1, 0, ch - 1)
    even_y = (ys & 1) == 0
    v = np.where(even_y[:, None], C[up] + 3 * C[j], 3 * C[j] + C[dn])          # (h, cw), scale 4
    i = xs >> 1
    nx = np.clip(i + 1, 0, cw - 1)
    even_x = (xs & 1) == 0
    return np.where(even_x[None, :], (v[:, i] + 2) >> 2, (v[:, i] + v[:, nx] + 4) >> 3)


def sample_dtype(sample, B):
    return {"native": np.uint16 if B > 8 else np.uint8, "msb16": np.uint16, "u8": np.uint8, "f16": np.float16,
            "f32": np.float32}[sample]


def export(planes, B, fmt, sample="native", matrix="bt709", full_range=False, upsample_mode="nearest", crop=(0, 0, 0, 0)):
    """The tight destination planes of one picture."""
    Y, Cb, Cr = planes
    h, w = Y.shape
    l, r, t, b = crop
    dt = sample_dtype(sample, B)
    if fmt in ("planar", "semiplanar"):
        sh = 16 - B if sample == "msb16" else 0
        y = (Y[t:h - b, l:w - r].astype(np.uint32) << sh).astype(dt)
        cb = (Cb[t // 2:(h - b) // 2, l // 2:(w - r) // 2].astype(np.uint32) << sh).astype(dt)
        cr = (Cr[t // 2:(h - b) // 2, l // 2:(w - r) // 2].astype(np.uint32) << sh).astype(dt)
        return [y, cb, cr] if fmt == "planar" else [y, np.stack([cb, cr], axis=-1)]
    D = 8 if sample == "u8" else B
    co = coefficients(matrix, full_range, B, D)
    ucb = upsample(Cb, upsample_mode)[t:h - b, l:w - r]         # clamped to the decoded picture, then cropped
    ucr = upsample(Cr, upsample_mode)[t:h - b, l:w - r]
    rgb = rgb_int(Y[t:h - b, l:w - r], ucb, ucr, co)
    if sample in ("f16", "f32"):
        k = np.float32(1 / (2 ** B - 1))
        rgb = [(c.astype(np.float32) * k).astype(dt) for c in rgb]
    else:
        rgb = [c.astype(dt) for c in rgb]
    return list(rgb) if fmt == "rgb_planar" else [np.stack(rgb, axis=-1)]
