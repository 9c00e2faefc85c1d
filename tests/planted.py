"""Planted-TB pictures: one ordinary intra CU with a chosen mode, size, placement and neighbour values
in a picture whose every other CU is PCM (plain Python, no GPU).

synth.make_picture draws modes, sizes and neighbours at random, so whether a (component, size, mode,
neighbour-availability) cell is decoded at all is luck.  Here every cell is built on purpose:

  * picture: CTB 64, SAO off, no deblocking, at most 128 x 128;
  * target CU of size S in {8, 16, 32}: one luma TB of size S (NxN at S = 8: four 4x4 luma TBs) and one
    Cb and one Cr TB of size S / 2 (4x4 at S = 8); luma and chroma modes are free (0..34 each);
  * every other CU is a PCM CU of 32x32 or smaller, emitted in z-order like a coded quadtree; its samples
    are seeded random except on the target's reference lines (row above, column to the left, 2N + 1 each
    way), which carry the requested neighbour values, independently per component;
  * PLACEMENTS puts the target where z-scan order, the picture edge, a slice start or a tile boundary
    give one availability pattern over (bottom-left, left, corner, top, top-right), the same for the luma
    TB of size S and the chroma TBs (tests/test_planted.py asserts the table from the oracle's 6.4.1).

planted_set(bit_depth) is the fixed set the CPU and GPU tests decode: every placement x {8 NxN, 8, 16,
32} x 35 pictures, picture i with luma mode i and chroma mode (i + 17) % 35; at ``interior`` once per
neighbour style (NEIGHBOUR_STYLES), the styles rotating over the other placements; the residual styles
(RESIDUAL_STYLES) rotate everywhere.
"""
import os

import numpy as np

from oracle import recon_oracle as O
from p265_amd import frontend, synth
from p265_amd import records as R

# name -> (picture (w, h), target (x, y)) as functions of S, slice start at CTU 3, tile columns,
# availability of (bottom-left, left, corner, top, top-right)
PLACEMENTS = {
    "interior":     (lambda s: (128, 128),    lambda s: (64, 64),         False, 1, (1, 1, 1, 1, 1)),
    "bl_missing":   (lambda s: (128, 128),    lambda s: (64, 128 - s),    False, 1, (0, 1, 1, 1, 1)),
    "both_missing": (lambda s: (128, 128),    lambda s: (64 + s, 64 + s), False, 1, (0, 1, 1, 1, 0)),
    "left_edge":    (lambda s: (128, 128),    lambda s: (0, 64),          False, 1, (0, 0, 0, 1, 1)),
    "origin":       (lambda s: (128, 128),    lambda s: (0, 0),           False, 1, (0, 0, 0, 0, 0)),
    "tr_missing":   (lambda s: (64 + s, 128), lambda s: (64, 64),         False, 1, (1, 1, 1, 1, 0)),
    "top_edge":     (lambda s: (128, 128),    lambda s: (64, 0),          False, 1, (1, 1, 0, 0, 0)),
    "new_slice":    (lambda s: (128, 128),    lambda s: (64, 64),         True,  1, (0, 0, 0, 0, 0)),
    "tile_col":     (lambda s: (128, 128),    lambda s: (64, 64),         False, 2, (0, 0, 0, 1, 1)),
}
SIZES = ((8, True), (8, False), (16, False), (32, False))          # (S, NxN)
NEIGHBOUR_STYLES = ("uniform", "extremes", "flat", "ramp_up", "ramp_down")
RESIDUAL_STYLES = ("none", "coef", "saturate")
MAX_W, MAX_H = 128, 128


def segments(n):
    """Slices of the linear reference order (oracle/recon_oracle.py ref_positions) for
    (bottom-left, left, corner, top, top-right)."""
    return (slice(0, n), slice(n, 2 * n), slice(2 * n, 2 * n + 1), slice(2 * n + 1, 3 * n + 1),
            slice(3 * n + 1, 4 * n + 1))


def pattern_avail(n, pattern):
    a = np.zeros(4 * n + 1, bool)
    for seg, on in zip(segments(n), pattern):
        a[seg] = bool(on)
    return a


def neighbour_values(rng, style, n, c_idx, bit_depth, variant=0):
    """Linear reference values (4n + 1) of one component for a style.

    uniform    over the whole sample range;
    extremes   every value 0 or max (the caller complements Cb into Cr);
    flat       mid-range +-2; at luma 32x32 the two strong-filter differences |corner + end - 2 * middle|
               are ``thr - 1`` or ``thr`` (thr = 1 << (BitDepth - 5)), bit 0 / bit 1 of ``variant`` choosing
               which for the top / left side and bit 2 the sign;
    ramp_up    corner 0, both sides rising steeply from 3/4 of the range: the mode 10 / 26 edge filter
               p[0] + ((p[k] - corner) >> 1) passes max;
    ramp_down  corner max, both sides falling from 1/4 of the range: the edge filter passes below 0.
    """
    mx = (1 << bit_depth) - 1
    m = 4 * n + 1
    if style == "uniform":
        return rng.integers(0, mx + 1, m)
    if style == "extremes":
        return rng.integers(0, 2, m) * mx
    if style == "flat":
        v = (1 << (bit_depth - 1)) + rng.integers(-2, 3, m)
        if n == 32 and c_idx == 0:
            thr = 1 << (bit_depth - 5)
            sgn = -1 if variant & 4 else 1
            d_top, d_left = thr - 1 + (variant & 1), thr - 1 + ((variant >> 1) & 1)
            v[4 * n] = 2 * v[3 * n] - v[2 * n] + sgn * d_top           # corner + tr - 2 * p[N-1][-1]
            v[0] = 2 * v[n] - v[2 * n] - sgn * d_left                  # corner + bl - 2 * p[-1][N-1]
        return v
    if style in ("ramp_up", "ramp_down"):
        k = np.abs(np.arange(m) - 2 * n)                               # distance from the corner, 1..2n
        step = max(1, (mx // 4) // (2 * n))
        if style == "ramp_up":
            v = (3 * (mx + 1)) // 4 + (k - 1) * step + rng.integers(0, 2, m)
            v[2 * n] = 0
        else:
            v = (mx + 1) // 4 - (k - 1) * step - rng.integers(0, 2, m)
            v[2 * n] = mx
        return np.clip(v, 0, mx)
    raise KeyError(style)


def styled_neighbours(rng, style, s, bit_depth, variant=0):
    """[luma (4S + 1), Cb (2S + 1), Cr (2S + 1)] for a style; at ``extremes`` Cr is the complement of Cb, so
    one half of a packed Cb | Cr << 16 word saturates while the other is empty."""
    nc = max(s // 2, 4)
    out = [neighbour_values(rng, style, s, 0, bit_depth, variant),
           neighbour_values(rng, style, nc, 1, bit_depth, variant),
           neighbour_values(rng, style, nc, 2, bit_depth, variant)]
    if style == "extremes":
        out[2] = ((1 << bit_depth) - 1) - out[1]
    return out


def _residual(rng, style, log2, sign):
    if style == "none":
        return None
    if style == "coef":
        return synth._coef_block(rng, log2, 0.2)
    co = np.zeros((1 << log2, 1 << log2), np.int16)                    # saturate: the clip of 8.6.7 fires
    co[0, 0] = 2000 * sign
    return co


def build(s, placement, luma_modes, chroma_mode, bit_depth, neighbours=None, nxn=False, residual="none",
          seed=0, sign=1, meta=None):
    """-> (params, records.Picture) of one planted picture.

    ``luma_modes``: one mode, or four for an NxN CU (S = 8 only).  ``neighbours``: [luma, Cb, Cr] linear
    reference arrays (4N + 1 each, N = S for luma and S / 2 for chroma, or 4 for the first luma block of an
    NxN CU; ref_positions order) for the reference lines, each or all None for seeded random ones.
    ``residual``: RESIDUAL_STYLES; ``sign``: sign of the saturating DC level of luma and Cr (Cb takes the
    opposite one).
    """
    size_of, at_of, new_slice, tile_cols, _ = PLACEMENTS[placement]
    (w, h), (x0, y0) = size_of(s), at_of(s)
    if nxn and s != 8:
        raise ValueError("NxN only at the minimum CU size 8")
    modes = [int(m) for m in (luma_modes if np.ndim(luma_modes) else [luma_modes] * 4)]
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=6, sample_adaptive_offset=0,
                           bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth)
    rng = np.random.default_rng([seed, s, bit_depth])
    mx = (1 << bit_depth) - 1
    planes = [rng.integers(0, mx + 1, (h >> (c > 0), w >> (c > 0))) for c in range(3)]
    if neighbours is not None:
        for c in range(3):
            if neighbours[c] is None:
                continue
            n = (len(neighbours[c]) - 1) // 4              # 4 at an NxN CU's first luma block
            xs, ys = (x0 >> (c > 0)) + O.ref_positions(n)[0], (y0 >> (c > 0)) + O.ref_positions(n)[1]
            ph, pw = planes[c].shape
            ok = (xs >= 0) & (ys >= 0) & (xs < pw) & (ys < ph)
            planes[c][ys[ok], xs[ok]] = np.asarray(neighbours[c])[ok]
    offy, offc = R.qp_bd_offset(params, 0), R.qp_bd_offset(params, 1)
    qcb, qcr = frontend.chroma_qp(30, 0, 0, offc)
    qps = (30 + offy, qcb + offc, qcr + offc)
    b = frontend.PictureBuilder(params)

    def target():
        if nxn:
            tus = []
            for i in range(4):
                co = [_residual(rng, residual, 2, sign if i % 2 == 0 else -sign), None, None]
                if i == 3:
                    co[1], co[2] = _residual(rng, residual, 2, -sign), _residual(rng, residual, 2, sign)
                tus.append(dict(x=x0 + 4 * (i % 2), y=y0 + 4 * (i // 2), log2=2, blk=i,
                                cbf=[int(v is not None) for v in co], tskip=[0, 0, 0], coef=co))
            b.add_cu(x0, y0, 3, 1, modes, int(chroma_mode), *qps, tus)
            return
        lg = s.bit_length() - 1
        co = [_residual(rng, residual, lg, sign), _residual(rng, residual, max(lg - 1, 2), -sign),
              _residual(rng, residual, max(lg - 1, 2), sign)]
        tu = dict(x=x0, y=y0, log2=lg, blk=0, cbf=[int(v is not None) for v in co], tskip=[0, 0, 0], coef=co)
        b.add_cu(x0, y0, lg, 0, modes, int(chroma_mode), *qps, [tu])

    def node(x, y, log2):
        n = 1 << log2
        if x >= w or y >= h:
            return
        if (x, y, n) == (x0, y0, s):
            target()
            return
        holds = x <= x0 < x + n and y <= y0 < y + n
        if log2 > 5 or holds or x + n > w or y + n > h:
            for i in range(4):
                node(x + (n >> 1) * (i % 2), y + (n >> 1) * (i // 2), log2 - 1)
            return
        smp = [planes[c][y >> (c > 0):(y + n) >> (c > 0), x >> (c > 0):(x + n) >> (c > 0)].astype(np.int16)
               for c in range(3)]
        b.add_cu(x, y, log2, 0, [0] * 4, 0, *qps, [], pcm=True, pcm_samples=smp)

    wc, hc = R.ctb_grid(params)
    for rs in range(wc * hc):
        node((rs % wc) << 6, (rs // wc) << 6, 6)
        b.add_ctu(rs, slice_addr=3 if (new_slice and rs == 3) else 0,
                  tile_id=(rs % wc) * tile_cols // wc if tile_cols > 1 else 0)
    m = dict(placement=placement, s=s, nxn=bool(nxn), target=(x0, y0), modes=modes, chroma_mode=int(chroma_mode),
             residual=residual, bit_depth=bit_depth)
    m.update(meta or {})
    pic = b.finish(meta=m)
    pic.size = (w, h)
    return params, pic


def target_region(pic, c_idx):
    """(y slice, x slice) of the target CU in plane ``c_idx``."""
    x0, y0 = pic.meta["target"]
    s, sub = pic.meta["s"], int(c_idx > 0)
    return slice(y0 >> sub, (y0 + s) >> sub), slice(x0 >> sub, (x0 + s) >> sub)


def set_params(bit_depth):
    """The parameter set a context decodes the whole planted set with (pictures carry their own size)."""
    return R.make_params(pic_width=MAX_W, pic_height=MAX_H, ctb_log2_size=6, sample_adaptive_offset=0,
                         bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth)


def plan():
    """The fixed set as [(placement, S, NxN, i, neighbour style, variant, residual style, sign)], the same at
    every bit depth: at ``interior`` every neighbour style for every (size, i); elsewhere one style per
    picture, rotating with i, the size and the placement, so every style meets every placement."""
    out = []
    for p_idx, placement in enumerate(PLACEMENTS):
        for s_idx, (s, nxn) in enumerate(SIZES):
            for i in range(35):
                styles = range(len(NEIGHBOUR_STYLES)) if placement == "interior" else [(i + s_idx + p_idx) % 5]
                for st in styles:
                    k = i + s_idx + p_idx + st
                    res = RESIDUAL_STYLES[k % 3]
                    if res == "saturate" and NEIGHBOUR_STYLES[st].startswith("ramp"):
                        res = "none"            # a saturating residual would hide the edge filter's clip
                    out.append((placement, s, nxn, i, NEIGHBOUR_STYLES[st], k // 5, res, 1 if (k // 3) % 2 == 0 else -1))
    return out


_SETS = {}


def planted_set(bit_depth):
    """[(params, Picture)] of the fixed set at one bit depth (built once per process)."""
    if bit_depth not in _SETS:
        pics = []
        for k, (placement, s, nxn, i, style, variant, res, sign) in enumerate(plan()):
            rng = np.random.default_rng([7, k, bit_depth])
            nb = styled_neighbours(rng, style, s, bit_depth, variant)
            modes = [(i + 9 * j) % 35 for j in range(4)] if nxn else i
            pics.append(build(s, placement, modes, (i + 17) % 35, bit_depth, nb, nxn=nxn, residual=res, seed=k,
                              sign=sign, meta=dict(style=style, i=i, variant=variant)))
        _SETS[bit_depth] = pics
    return _SETS[bit_depth]


# ---------------------------------------------------------------------------------
# pictures planted from the reference's chain vectors (tests/golden/ref_chain*.npz)
# ---------------------------------------------------------------------------------

CHAIN_PLACEMENTS = ("interior", "bl_missing", "both_missing", "left_edge", "origin")   # chain_pattern index
# a 4x4 luma block only exists in an NxN CU, whose first block shares its left and its top CU with the
# block below / beside it: "bottom-left missing, left present" and "top present, top-right missing" cannot
# be had from PCM neighbours alone, so at n = 4 only these patterns are planted
CHAIN_PLACEMENTS_4 = ("interior", "left_edge", "origin")


def load_chain(bit_depth):
    """The chain vectors as a list of dicts (n, mode, pattern, vals, avail, out [y][x])."""
    f = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                     "ref_chain%s.npz" % ("" if bit_depth == 8 else "_bd%d" % bit_depth))
    z = np.load(f)
    out, kv, ko = [], 0, 0
    for n, mode, pat in zip(z["chain_n"], z["chain_mode"], z["chain_pattern"]):
        n, m = int(n), 4 * int(n) + 1
        out.append(dict(n=n, mode=int(mode), pattern=int(pat), vals=z["chain_vals"][kv:kv + m].astype(np.int64),
                        avail=z["chain_avail"][kv:kv + m].astype(bool),
                        out=z["chain_out"][ko:ko + n * n].astype(np.int64).reshape(n, n)))
        kv, ko = kv + m, ko + n * n
    assert kv == len(z["chain_vals"]) and ko == len(z["chain_out"])
    return out


_CHAIN_SETS = {}


def chain_set(bit_depth):
    """[(params, Picture, expected)]: one planted picture per chain vector that can be planted (every one at
    n >= 8; CHAIN_PLACEMENTS_4 at n = 4), no residual; ``expected`` is the reference's n x n prediction, which
    the picture's luma plane must hold at the target's top-left n x n."""
    if bit_depth not in _CHAIN_SETS:
        res = []
        for k, v in enumerate(load_chain(bit_depth)):
            placement = CHAIN_PLACEMENTS[v["pattern"]]
            assert np.array_equal(v["avail"], pattern_avail(v["n"], PLACEMENTS[placement][4]))
            if v["n"] == 4 and placement not in CHAIN_PLACEMENTS_4:
                continue
            nxn = v["n"] == 4
            modes = [v["mode"]] + [(v["mode"] + 9 * j) % 35 for j in (1, 2, 3)] if nxn else v["mode"]
            params, pic = build(max(v["n"], 8), placement, modes, (v["mode"] + 17) % 35, bit_depth,
                                [v["vals"], None, None], nxn=nxn, seed=100000 + k, meta=dict(chain=k, n=v["n"]))
            res.append((params, pic, v["out"]))
        _CHAIN_SETS[bit_depth] = res
    return _CHAIN_SETS[bit_depth]


def chain_region(pic):
    x0, y0 = pic.meta["target"]
    n = pic.meta["n"]
    return slice(y0, y0 + n), slice(x0, x0 + n)
