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

residual_set(bit_depth), further down, is the planted residual set: the same builder at ``interior`` on a constant
prediction, with chosen coefficients, qP and flags.
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
          seed=0, sign=1, meta=None, qp_y=30, coefs=None, tskip=(0, 0, 0), bypass=False, chroma_qp_offsets=(0, 0)):
    """-> (params, records.Picture) of one planted picture.

    ``luma_modes``: one mode, or four for an NxN CU (S = 8 only).  ``neighbours``: [luma, Cb, Cr] linear
    reference arrays (4N + 1 each, N = S for luma and S / 2 for chroma, or 4 for the first luma block of an
    NxN CU; ref_positions order) for the reference lines, each or all None for seeded random ones.
    ``residual``: RESIDUAL_STYLES; ``sign``: sign of the saturating DC level of luma and Cr (Cb takes the
    opposite one).  ``qp_y``: QpY of every CU (-QpBdOffsetY..51); the chroma qP follow from it and
    ``chroma_qp_offsets`` (Cb, Cr) through frontend.chroma_qp.  ``coefs``: [luma, Cb, Cr] TransCoeffLevel arrays
    [y][x] of the target's TBs instead of a residual style, each None for an uncoded TB; at an NxN CU the luma
    array is the first 4x4 block's (the three others, which do not predict from the planted reference lines,
    stay uncoded).  ``tskip``: transform_skip_flag per component; ``bypass``: cu_transquant_bypass_flag.
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
    qcb, qcr = frontend.chroma_qp(qp_y, chroma_qp_offsets[0], chroma_qp_offsets[1], offc)
    qps = (qp_y + offy, qcb + offc, qcr + offc)
    b = frontend.PictureBuilder(params)

    def target():
        if nxn:
            tus = []
            for i in range(4):
                if coefs is not None:
                    co = [coefs[0] if i == 0 else None, coefs[1] if i == 3 else None, coefs[2] if i == 3 else None]
                else:
                    co = [_residual(rng, residual, 2, sign if i % 2 == 0 else -sign), None, None]
                    if i == 3:
                        co[1], co[2] = _residual(rng, residual, 2, -sign), _residual(rng, residual, 2, sign)
                tus.append(dict(x=x0 + 4 * (i % 2), y=y0 + 4 * (i // 2), log2=2, blk=i,
                                cbf=[int(v is not None) for v in co], tskip=[int(v) for v in tskip], coef=co))
            b.add_cu(x0, y0, 3, 1, modes, int(chroma_mode), *qps, tus, bypass=bypass)
            return
        lg = s.bit_length() - 1
        if coefs is not None:
            co = list(coefs)
        else:
            co = [_residual(rng, residual, lg, sign), _residual(rng, residual, max(lg - 1, 2), -sign),
                  _residual(rng, residual, max(lg - 1, 2), sign)]
        tu = dict(x=x0, y=y0, log2=lg, blk=0, cbf=[int(v is not None) for v in co], tskip=[int(v) for v in tskip],
                  coef=co)
        b.add_cu(x0, y0, lg, 0, modes, int(chroma_mode), *qps, [tu], bypass=bypass)

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


def set_params(bit_depth, scaling=False):
    """The parameter set a context decodes the whole planted set with (pictures carry their own size);
    ``scaling``: with scaling_list_enabled (the context is then given a ScalingFactor table)."""
    return R.make_params(pic_width=MAX_W, pic_height=MAX_H, ctb_log2_size=6, sample_adaptive_offset=0,
                         bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth, scaling_list_enabled=int(scaling))


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


# ---------------------------------------------------------------------------------
# the planted residual set: chosen coefficients, qP and flags on a constant prediction
# ---------------------------------------------------------------------------------
# Every picture is the ``interior`` placement with every reference sample of the target set to one value v,
# so every mode predicts the constant v and the target holds clip(v + r): a residual r is observed in full
# where v + r stays inside the sample range, and by its sign where it does not (which tells a clamp from a
# wrap).  residual_set(bit_depth) is the fixed set:
#
#   impulse   one non-zero level at every (ky, kx) of luma 32x32 / 16x16 / 8x8 / 4x4 (DST, NxN CU), the Cb and
#             Cr TBs of the same picture carrying impulses at positions of their own, so that every (ky, kx) of
#             chroma 16x16 / 8x8 / 4x4 occurs too; qP'Y = 30 + QpBdOffset, v = mid, the level the largest whose
#             response at the TB's qP' stays strictly inside the sample range (impulse_level);
#   sweep     a seeded synth._coef_block per TB at every qP'Y = 0 .. 51 + QpBdOffset for each size; Cb at the
#             chroma qP of cb_qp_offset 0 and Cr at that of +12, which together take every qP'C as well;
#   extreme   EXTREME_PATTERNS at qP' in {0, 29, max} and v in {0, max};
#   tskip     4x4 transform skip, luma and chroma, levels -32768, 32767, 1, -1 at qP' 0 and max (of all three);
#   bypass    transform-quant bypass at every size, levels -32768, 32767, max sample value and its negative;
#   count     8x8 CUs that code chroma 4x4 TBs alone (Cb and Cr, or Cb only), for job_count_batches.
#
# The pictures with ``scaled`` in their meta (sweep and extreme) are decoded once more in contexts with scaling
# lists (scaling_tables).

RES_CLASSES = ("dst4", "dct4", "dct8", "dct16", "dct32")             # the residual kernels' job classes
RES_TPB = {"dst4": 256, "dct4": 256, "dct8": 32, "dct16": 16, "dct32": 8}   # TBs per 256-thread block
EXTREME_PATTERNS = ("pos", "neg", "checker", "colsign", "colsign_neg")
V_NAMES = ("zero", "mid", "max")


def res_class(log2, c_idx):
    return "dst4" if (log2 == 2 and c_idx == 0) else "dct%d" % (1 << log2)


def _v_of(name, bit_depth):
    return {"zero": 0, "mid": 1 << (bit_depth - 1), "max": (1 << bit_depth) - 1}[name]


def _impulse(n, ky, kx, level):
    co = np.zeros((n, n), np.int16)
    co[ky, kx] = level
    return co


def _impulse_inside(level, log2, c_idx, bit_depth, qp, positions):
    n, mid = 1 << log2, 1 << (bit_depth - 1)
    for ky, kx in positions:
        for sg in (1, -1):
            r = O.residual_block(_impulse(n, ky, kx, sg * level), log2, c_idx, qp, R.TB_CBF, bit_depth)
            if r.min() <= -mid or r.max() >= mid - 1:              # 0 < mid + r < max
                return False
    return True


_LEVELS = {}


def impulse_level(log2, c_idx, bit_depth, qp):
    """The largest level whose response in the Python oracle at qP' ``qp``, at any (ky, kx) and with either
    sign, stays strictly inside the sample range around v = mid (bisected on the lowest four frequencies each
    way, which hold the largest matrix entries, then stepped down until every position passes)."""
    key = (log2, c_idx, bit_depth, qp)
    if key not in _LEVELS:
        n = 1 << log2
        low = [(a, b) for a in range(4) for b in range(4)]
        lo, hi = 1, 32767                                           # inside at lo, not known inside at hi + 1
        while lo < hi:
            m = (lo + hi + 1) // 2
            lo, hi = (m, hi) if _impulse_inside(m, log2, c_idx, bit_depth, qp, low) else (lo, m - 1)
        every = [(a, b) for a in range(n) for b in range(n)]
        while not _impulse_inside(lo, log2, c_idx, bit_depth, qp, every):
            lo -= 1
        assert lo >= 1
        _LEVELS[key] = lo
    return _LEVELS[key]


def extreme_block(pattern, log2, c_idx):
    """EXTREME_PATTERNS: all +32767; all -32768; a +-32767 checkerboard; every column 32767 * sign(M[:, 0]) (M
    the TB's transform matrix: the first output of stage 1 is the largest sum there is, in every column) and
    its negative."""
    n = 1 << log2
    if pattern == "pos":
        return np.full((n, n), 32767, np.int16)
    if pattern == "neg":
        return np.full((n, n), -32768, np.int16)
    if pattern == "checker":
        ys, xs = np.mgrid[0:n, 0:n]
        return np.where((ys + xs) % 2 == 0, 32767, -32767).astype(np.int16)
    m = O.transform_matrix(log2, 1 if (log2 == 2 and c_idx == 0) else 0)
    col = np.where(m[:, 0] >= 0, 32767, -32767)
    blk = np.repeat(col[:, None], n, axis=1)
    return (blk if pattern == "colsign" else -blk).astype(np.int16)


def _cycle_block(n, values):
    return np.resize(np.asarray(values, np.int64), n * n).reshape(n, n).astype(np.int16)


def chroma_qps(qp_prime, bit_depth):
    """(qP'Cb, qP'Cr) of the residual set's pictures at luma qP' ``qp_prime``: cb_qp_offset 0, cr_qp_offset 12."""
    off = 6 * (bit_depth - 8)
    qcb, qcr = frontend.chroma_qp(qp_prime - off, 0, 12, off)
    return qcb + off, qcr + off


def residual_build(k, s, nxn, bit_depth, v_name, qp_prime, coefs, kind, tskip=(0, 0, 0), bypass=False, scaled=False,
                   meta=None, chroma_qp_offsets=(0, 12)):
    """One picture of the residual set: target CU of size ``s`` at ``interior`` on the constant ``v_name``,
    luma qP' ``qp_prime``, Cb at cb_qp_offset 0 and Cr at +12 unless given; the modes rotate with ``k``."""
    v = _v_of(v_name, bit_depth)
    nc = max(s // 2, 4)
    nb = [np.full(4 * s + 1, v), np.full(4 * nc + 1, v), np.full(4 * nc + 1, v)]
    m = dict(kind=kind, v=v, scaled=bool(scaled), qp_prime=int(qp_prime))
    m.update(meta or {})
    modes = [(k + 9 * j) % 35 for j in range(4)] if nxn else k % 35
    return build(s, "interior", modes, (k + 17) % 35, bit_depth, nb, nxn=nxn, seed=200000 + k, meta=m,
                 qp_y=qp_prime - 6 * (bit_depth - 8), coefs=coefs, tskip=tskip, bypass=bypass,
                 chroma_qp_offsets=chroma_qp_offsets)


_RES_SETS = {}


def residual_set(bit_depth):
    """[(params, Picture)] of the fixed residual set at one bit depth (built once per process)."""
    if bit_depth in _RES_SETS:
        return _RES_SETS[bit_depth]
    bd, pics = bit_depth, []
    qp_max = 51 + 6 * (bd - 8)
    mx = (1 << bd) - 1

    def add(*a, **kw):
        pics.append(residual_build(len(pics), *a, **kw))

    for s, nxn in SIZES:                                                # impulses
        lg = 2 if nxn else s.bit_length() - 1
        lgc = max(s.bit_length() - 2, 2)
        n, nc = 1 << lg, 1 << lgc
        qp = 30 + 6 * (bd - 8)
        lv, (lvb, lvr) = impulse_level(lg, 0, bd, qp), (impulse_level(lgc, c + 1, bd, q) for c, q in enumerate(chroma_qps(qp, bd)))
        for k in range(n * n):
            ky, kx = k // n, k % n
            pb, pr = k % (nc * nc), (k + nc * nc // 2 + 1) % (nc * nc)
            sb = 1 if ((k // (nc * nc)) + pb) % 2 == 0 else -1
            co = [_impulse(n, ky, kx, lv if (ky + kx) % 2 == 0 else -lv), _impulse(nc, pb // nc, pb % nc, sb * lvb),
                  _impulse(nc, pr // nc, pr % nc, -sb * lvr)]
            add(s, nxn, bd, "mid", qp, co, "impulse")
    for s_idx, (s, nxn) in enumerate(SIZES):                            # qP sweep
        lg = 2 if nxn else s.bit_length() - 1
        lgc = max(s.bit_length() - 2, 2)
        rng = np.random.default_rng([11, s_idx])
        co = [synth._coef_block(rng, lg, 0.2), synth._coef_block(rng, lgc, 0.2), synth._coef_block(rng, lgc, 0.2)]
        for qp in range(qp_max + 1):
            add(s, nxn, bd, V_NAMES[(qp + s_idx) % 3], qp, co, "sweep", scaled=True)
    for s, nxn in SIZES:                                                # extremes
        lg = 2 if nxn else s.bit_length() - 1
        lgc = max(s.bit_length() - 2, 2)
        for i, pat in enumerate(EXTREME_PATTERNS):
            pat_r = EXTREME_PATTERNS[(i + 1) % len(EXTREME_PATTERNS)]
            co = [extreme_block(pat, lg, 0), extreme_block(pat, lgc, 1), extreme_block(pat_r, lgc, 2)]
            for qp in (0, 29, qp_max):
                for v_name in ("zero", "max"):
                    add(s, nxn, bd, v_name, qp, co, "extreme", scaled=True, meta=dict(patterns=(pat, pat, pat_r)))
    ts = _cycle_block(4, [-32768, 32767, 1, -1])                        # transform skip (4x4 only)
    for qp in (0, qp_max):
        for v_name in V_NAMES:
            # (chroma offsets 0 at the bottom and 12 at the top: Cb and Cr are at qP' 0 and max with luma)
            add(8, True, bd, v_name, qp, [ts, ts.T.copy(), ts[::-1].copy()], "tskip", tskip=(1, 1, 1),
                chroma_qp_offsets=(12, 12) if qp else (0, 0))
    for s, nxn in SIZES:                                                # transform-quant bypass
        lg = 2 if nxn else s.bit_length() - 1
        lgc = max(s.bit_length() - 2, 2)
        for v_name in V_NAMES:
            co = [_cycle_block(1 << lg, [-32768, 32767, mx, -mx]), _cycle_block(1 << lgc, [32767, -mx, -32768, mx]),
                  _cycle_block(1 << lgc, [mx, -32768, -mx, 32767])]
            add(s, nxn, bd, v_name, 30 + 6 * (bd - 8), co, "bypass", bypass=True)
    rng = np.random.default_rng([11, 99])                               # chroma 4x4 alone, two TBs or one
    cb, cr = synth._coef_block(rng, 2, 0.3), synth._coef_block(rng, 2, 0.3)
    add(8, False, bd, "mid", 27 + 6 * (bd - 8), [None, cb, cr], "count", meta=dict(n_dct4=2))
    add(8, False, bd, "mid", 33 + 6 * (bd - 8), [None, cr, None], "count", meta=dict(n_dct4=1))
    _RES_SETS[bit_depth] = pics
    return pics


def planted_tbs(pic):
    """The TB records of a residual-set picture that sit on the constant prediction and carry a residual: the
    coded TBs that are not PCM."""
    f = pic.tbs["flags"]
    return pic.tbs[((f & R.TB_PCM) == 0) & ((f & R.TB_CBF) != 0)]


def class_counts(pics):
    """TBs per residual job class over a batch (transform-skip TBs are a class of their own, bypass TBs have
    no residual job)."""
    out = dict.fromkeys(RES_CLASSES, 0)
    for pic in pics:
        for t in planted_tbs(pic):
            if not int(t["flags"]) & (R.TB_TSKIP | R.TB_BYPASS):
                out[res_class(int(t["log2_size"]), int(t["c_idx"]))] += 1
    return out


def job_count_batches(bit_depth):
    """[(class, n, indices into residual_set)]: sub-batches whose TB count in one residual job class is exactly
    n, for n = 1, TPB - 1, TPB, TPB + 1 (the last block of residualN_kernel then has TPB - 1 inactive TBs, one,
    none, and again TPB - 1; residual4_kernel's last block a tail).  The pictures are the sweep's of the size
    whose luma TB is of the class (cycled when n exceeds their number), for chroma 4x4 the ``count`` ones."""
    pics = residual_set(bit_depth)
    pool = {}
    for i, (_, pic) in enumerate(pics):
        if pic.meta["kind"] == "sweep":
            pool.setdefault("dst4" if pic.meta["nxn"] else "dct%d" % pic.meta["s"], []).append(i)
        if pic.meta["kind"] == "count":
            pool[("dct4", pic.meta["n_dct4"])] = i
    out = []
    for cls in RES_CLASSES:
        for n in (1, RES_TPB[cls] - 1, RES_TPB[cls], RES_TPB[cls] + 1):
            if cls == "dct4":
                idx = [pool[("dct4", 2)]] * (n // 2) + [pool[("dct4", 1)]] * (n % 2)
            else:
                idx = [pool[cls][j % len(pool[cls])] for j in range(n)]
            out.append((cls, n, idx))
    return out


def scaling_tables():
    """ScalingFactor tables (the 2032-byte ABI array) the scaled pictures are decoded with: random factors
    1..255; 1 everywhere but 255 at DC and at (N - 1, N - 1); 255 everywhere."""
    rng = np.random.default_rng(12)
    rand, corners, full = {}, {}, {}
    for key in O.SF_OFFSETS:
        n = 4 << key[0]
        rand[key] = rng.integers(1, 256, (n, n))
        corners[key] = np.ones((n, n), np.int64)
        corners[key][0, 0] = corners[key][n - 1, n - 1] = 255
        full[key] = np.full((n, n), 255, np.int64)
    return {"random": O.scaling_factor_bytes(rand), "corners": O.scaling_factor_bytes(corners),
            "all255": O.scaling_factor_bytes(full)}
