"""numpy restatement of the scaled grid export (include/p265r.h, "scaled grid export"), written from the header's
words and not from the kernel:

    canvas   grid_ref.canvas(tiles, rows, cols)
    window   [crop_left, out_width - crop_right) x [crop_top, out_height - crop_bottom) of the canvas
    R        resize_ref.resize(canvas, crop = the window, size = (pw, ph)); (pw, ph) = (ow, oh), k odd: (oh, ow)
    slot     grid_ref.orient(R, orientation) of every plane: ow x oh whatever the frame

``frame`` is one slot; ``expected_plan`` restates the constants the host planner hands the kernels.
"""
import numpy as np

import grid_ref as G
import resize_ref as RZ


def pre_turn(size, orientation):
    ow, oh = size
    return (oh, ow) if orientation & 1 else (ow, oh)


def frame(tiles, rows, cols, out_size, B, fmt, size, sample="native", matrix="bt709", full_range=False, crop=(0, 0, 0, 0),
          orientation=0, filt="bilinear", scale=None, bias=None):
    """The tight destination planes of one slot of ``size`` = (ow, oh)."""
    cv = G.canvas(tiles, rows, cols)
    h, w = cv[0].shape
    l, r, t, b = crop
    win = (l, w - out_size[0] + r, t, h - out_size[1] + b)          # the window as a crop of the canvas
    R = RZ.resize(cv, B, fmt, sample, matrix, full_range, crop=win, size=pre_turn(size, orientation), filt=filt,
                  scale=scale, bias=bias)
    return [np.ascontiguousarray(G.orient(p, orientation)) for p in R]


def expected_plan(frames, size):
    """Per frame (rows, cols, out_w, out_h, crop, orientation): what p265r_grid_resize_plan must report.  The flips are
    derived here from numpy itself: R is marked with its own indices, turned and mirrored, and read back."""
    out, tile0, stage = [], 0, 0
    for rows, cols, ow_, oh_, crop, o in frames:
        l, r, t, b = crop
        pw, ph = pre_turn(size, o)
        idx = np.arange(ph * pw).reshape(ph, pw)
        d = G.orient(idx, o)
        tr = int(o & 1)
        u = d.T if tr else d                                        # R reversed, before the transpose
        fx, fy = int(u[0, 0] % pw != 0), int(u[0, 0] // pw != 0)
        want = idx[::-1 if fy else 1, ::-1 if fx else 1]
        assert np.array_equal(u, want)
        out.append({"tile0": tile0, "cols": cols, "window": (l, t, ow_ - l - r, oh_ - t - b), "pre_turn": (pw, ph), "fx": fx,
                    "fy": fy, "transpose": tr, "stage": stage if tr else -1})
        tile0 += rows * cols
        stage += tr
    return out
