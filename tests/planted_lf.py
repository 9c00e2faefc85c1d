"""Planted deblocking pictures: 128 x 128 pictures made of PCM CUs whose samples, QpY and CTU attributes are
chosen, so the deblocking input is exactly the planted planes (plain Python, no GPU).

synth.make_picture reaches the strong filter, the clips and the table ends by luck.  Here a picture is a grid of
PCM CUs of one size (8, 16 or 32; pcm_loop_filter_disabled is off, so they are filtered; a PCM CU with
cu_transquant_bypass is a no-filter side) and every 4-line edge segment is given a *recipe*: eight samples
across the edge on four lines, computed from the segment's own beta and tC so that one decision of 8.7.2.5
sits at its threshold or one clip fires.

Where the cells live.  Vertical edges are filtered first, on the planted planes, so every segment of every
vertical edge on the 8-sample grid holds a recipe (columns e - 4 .. e + 3).  Horizontal edges are filtered on the
vertically filtered picture, which differs from the planted one in the three columns either side of a vertical
CU edge; a horizontal segment (four columns) that keeps clear of those is filtered on planted samples.  With
16 x 16 CUs those are the columns 4..11 of every CU, with 32 x 32 CUs 4..27, with 8 x 8 CUs none: the horizontal
recipes sit there (rows e - 4 .. e + 3) and overwrite the vertical recipes of edges inside a CU, which are not
edges.  Chroma likewise: columns 2..5 of every 8 chroma samples.  Only lines 0 and 3 of a segment enter the
decisions, so lines 1 and 2 carry what a decision would forbid: the steps that drive the clips.

lf_set(bit_depth, ctb_log2, variant) is the fixed set of one context (VARIANTS: the pps chroma QP offsets and
loop_filter_across_tiles): ``cells`` pictures (16 x 16 CUs, recipes both ways, QpY cycling over its whole range,
CTU offsets cycling over -6..6, bypass CUs), ``grid8`` (8 x 8 CUs: luma edges at 8 mod 16, which chroma does
not filter), ``grid32`` (32 x 32 CUs: no edge inside a CU), ``rules`` (block-constant planes with a small step
at every 8 x 8 block border, which any filtering changes, under seeded slice, tile, deblocking-off and offset
layouts) and ``nxn`` (ordinary 8 x 8 NxN CUs: 4 x 4 TBs, no edge at 4-sample offsets).
"""
import numpy as np

from oracle import recon_oracle as O
from p265_amd import frontend
from p265_amd import records as R

W = H = 128
VARIANTS = {"a": dict(cb=0, cr=0, lf_tiles=1), "b": dict(cb=-12, cr=12, lf_tiles=0), "c": dict(cb=12, cr=-12, lf_tiles=1)}
CTB_LOG2 = (4, 5, 6)
OFFSETS = ((0, 0), (-6, -6), (6, 6), (-6, 6), (6, -6), (2, -3), (-1, 4), (0, -1))     # (beta, tc) _offset_div2


def params_of(bit_depth, ctb_log2, variant, sao=False, w=W, h=H):
    v = VARIANTS[variant]
    return R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, sample_adaptive_offset=int(sao),
                         bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth, loop_filter_across_tiles=v["lf_tiles"],
                         pps_cb_qp_offset=v["cb"], pps_cr_qp_offset=v["cr"])


class Spec:
    """What a picture is built from: the CU size, QpY and the bypass flag per CU ([cy][cx]), and per CTU
    (raster) slice id, tile id, slice_loop_filter_across_slices, deblocking on, (beta, tc) offsets.  The
    picture is 128 x 128 unless ``w`` and ``h`` say otherwise (multiples of 8; CTBs and CUs at the right and
    bottom may be partial).  ``nf_pcm``: PCM CUs under pcm_loop_filter_disabled (a no-filter CU without
    bypass); ``sao``: per CTU the SAO arguments of PictureBuilder.add_ctu, or None."""

    def __init__(self, bit_depth, ctb_log2, cu, w=W, h=H):
        self.bd, self.ctb_log2, self.cu = bit_depth, ctb_log2, cu
        self.w, self.h = w, h
        self.ctb = 1 << ctb_log2
        self.wc, self.hc = -(-w >> ctb_log2), -(-h >> ctb_log2)
        n, nc = (-(-h // cu), -(-w // cu)), self.wc * self.hc
        self.qp = np.full(n, 30, np.int64)
        self.nf = np.zeros(n, bool)
        self.nf_pcm = np.zeros(n, bool)
        self.sao = None
        self.slice = np.zeros(nc, np.int64)
        self.tile = np.zeros(nc, np.int64)
        self.lf_across = np.ones(nc, bool)
        self.dbk = np.ones(nc, bool)
        self.off = [(0, 0)] * nc

    def ctu_of(self, x, y):
        return (y >> self.ctb_log2) * self.wc + (x >> self.ctb_log2)

    def qp_at(self, x, y):
        return int(self.qp[y // self.cu, x // self.cu])

    def beta_tc(self, xp, yp, xq, yq):
        """(beta, tC) of the luma edge between the samples p0 and q0 (8.7.2.5.3, bS = 2)."""
        qpl = (self.qp_at(xq, yq) + self.qp_at(xp, yp) + 1) >> 1
        bo, to = self.off[self.ctu_of(xq, yq)]
        sc = 1 << (self.bd - 8)
        return (O.BETA_TABLE[min(max(qpl + 2 * bo, 0), 51)] * sc, O.TC_TABLE[min(max(qpl + 2 + 2 * to, 0), 53)] * sc)

    def chroma_tc(self, xp, yp, xq, yq, c_off):
        _, to = self.off[self.ctu_of(xq, yq)]
        return O.chroma_tc(self.qp_at(xp, yp), self.qp_at(xq, yq), c_off, to, self.bd)


# ---------------------------------------------------------------------------------
# recipes: lines [k][p3 p2 p1 p0 q0 q1 q2 q3] of one luma segment, or None when beta / tC / the range forbid
# ---------------------------------------------------------------------------------

def _flat(a, b):
    return np.array([[a] * 4 + [b] * 4] * 4, np.int64)


def _tight(thr, parity2):
    """(largest value below thr, smallest value at or above it) a left side can take: any integer, or an even
    one (2 * dpq)."""
    if not parity2:
        return thr - 1, thr
    return (thr - 1) - ((thr - 1) % 2), thr + (thr % 2)


def luma_recipe(name, beta, tc, mx):
    mid = (mx + 1) // 2
    thr_a, thr_b, thr_c, thr_e = beta >> 2, beta >> 3, (5 * tc + 1) >> 1, (beta + (beta >> 1)) >> 3
    far = thr_b + 5                                   # |p3 - p0| that rules the strong filter out
    L = None
    if name == "flat":                                # d = 0; strong if beta >= 8 and tC >= 1
        L = _flat(mid, mid + min(2, max(thr_c - 1, 0)))
    elif name in ("d_below", "d_at") and beta >= 1:
        L = _flat(mid, mid + 3)
        L[0, 1] += beta - (name == "d_below")
    elif name in ("a_below", "a_at") and thr_a >= 2 and thr_b >= 1 and thr_c >= 2:
        lo, hi = _tight(thr_a, True)
        L = _flat(mid, mid + 1)
        L[0, 1] += (lo if name == "a_below" else hi) // 2
        L[3, 1] += (lo if name == "a_below" else hi) // 2
    elif name in ("b_below", "b_at") and thr_a >= 1 and thr_b >= 1 and thr_c >= 2:
        L = _flat(mid, mid + 1)
        L[0, 0] += thr_b - (name == "b_below")
        L[3, 0] += thr_b - (name == "b_below")
    elif name in ("c_below", "c_at") and thr_a >= 1 and thr_b >= 1 and thr_c >= 1:
        L = _flat(mid, mid + thr_c - (name == "c_below"))
    elif name in ("strong_l0_only", "strong_l3_only") and thr_a >= 1 and thr_b >= 1 and thr_c >= 2:
        L = _flat(mid, mid + 1)
        L[3 if name == "strong_l0_only" else 0, 0] += thr_b
    elif name == "strong_clips" and thr_a >= 1 and thr_b >= 1 and thr_c >= 2 and tc >= 1:
        big = 16 * tc + 16                            # big / 8 > 2 tC: p2 and q2 clip as well
        L = _flat(mid, mid + 1)
        L[1, 4:] = mid + big
        L[2, 4:] = mid - big
    elif name == "delta_10tc" and tc >= 1 and beta >= 1:
        L = _flat(0, 0)
        L[:, 0] = far
        L[1, 4:] = -(-(16 * (10 * tc - 1) - 8) // 6)  # delta = 10 tC - 1: filtered
        L[2, 4:] = -(-(16 * (10 * tc) - 8) // 6)      # delta = 10 tC: left alone
    elif name == "delta_clip" and tc >= 2 and beta >= 1:
        L = _flat(mid, mid)
        L[:, 0] += far
        L[1, 4:] = mid + -(-(16 * (2 * tc) - 8) // 6)               # delta = 2 tC -> + tC
        L[2, 4:] = mid + -(-(16 * (tc - 1) - 8) // 6)               # delta = tC - 1: unclipped
        L[0, 4:] = mid - 1
    elif name.startswith("de_") and thr_e >= 1 and 2 * thr_e < beta and tc >= 1:     # de_<p><q>, 1 = on
        L = _flat(mid, mid + 3)
        L[0, 0] += far
        L[0, 1] += thr_e - (name[3] == "1")
        L[0, 6] += thr_e - (name[4] == "1")
    elif name == "dp_clip" and thr_e >= 1 and tc >= 2:
        L = _flat(mid, mid + 1)
        L[:, 0] += far
        L[1, 1] = mid + 4 * tc + 8                    # (p2 - p1) / 4 > tC >> 1
        L[2, 1] = mid - 4 * tc - 8
    elif name == "clip1" and thr_e >= 1 and tc >= 2 and beta >= 1:
        L = _flat(mx, mx)
        L[:, 0] -= far
        L[1, 5:] = mx - (-(-(16 * tc - 8) // 3))      # delta = tC with p0 = p1 = p2 = q0 = max
        L[2, 5:] = mx - (-(-(16 * tc - 8) // 3))
    if L is None or L.min() < 0 or L.max() > mx:
        return None
    return L


LUMA_RECIPES = ("flat", "d_below", "d_at", "a_below", "a_at", "b_below", "b_at", "c_below", "c_at", "strong_l0_only",
                "strong_l3_only", "strong_clips", "delta_10tc", "delta_clip", "de_11", "de_10", "de_01", "de_00",
                "dp_clip", "clip1")


def luma_lines(k, beta, tc, mx):
    """The k-th segment's lines: recipe k (the next one that beta, tC and the range allow), mirrored (p <-> q)
    and / or complemented (v -> max - v) in turn, so every recipe meets both sides and both signs."""
    n = len(LUMA_RECIPES)
    for j in range(n):
        L = luma_recipe(LUMA_RECIPES[(k + j) % n], beta, tc, mx)
        if L is not None:
            break
    else:
        L = _flat(mx // 2, mx // 2 + 1)
    v = k // n
    if v & 1:
        L = L[:, ::-1]
    if v & 2:
        L = mx - L
    return L


def chroma_line(k, tc, mx):
    """[p1 p0 q0 q1] of one chroma line: delta unclipped, clipped at + tC, Clip1 at max; mirrored and
    complemented in turn (- tC, Clip1 at 0)."""
    mid = (mx + 1) // 2
    kind = k % 3
    if kind == 0:
        L = np.array([mid, mid, mid + 2, mid + 2])                    # delta = 1
    elif kind == 1:
        s = -(-(8 * (tc + 1) - 4) // 3)                               # delta = tC + 1
        L = np.array([mid, mid, mid + s, mid + s])
    else:
        L = np.array([mx - 12, mx, mx, mx])                           # delta = 2 with q0 = max
        L = L[::-1]
    v = k // 3
    if v & 1:
        L = L[::-1]
    if v & 2:
        L = mx - L
    return np.clip(L, 0, mx)


def _free_starts(cu):
    """Starts s0 (multiples of 4) within a CU of the luma segments that the vertical pass leaves alone
    (columns 4 .. cu - 5)."""
    return [s for s in range(4, cu - 7, 4)]


def plant_cells(spec, variant, seed):
    """Planes of a ``cells`` / ``grid`` picture: random samples, a recipe in every vertical segment on the
    8-sample grid and in every horizontal segment that stays clear of the vertical pass."""
    rng = np.random.default_rng([21, seed])
    mx = (1 << spec.bd) - 1
    planes = [rng.integers(0, mx + 1, (H >> (c > 0), W >> (c > 0))) for c in range(3)]
    Y, k = planes[0], seed * 7
    for e in range(8, W, 8):                                          # vertical edges (also the ones inside a CU)
        for s0 in range(0, H, 4):
            beta, tc = spec.beta_tc(e - 1, s0, e, s0)
            Y[s0:s0 + 4, e - 4:e + 4] = luma_lines(k, beta, tc, mx)
            k += 1
    free = _free_starts(spec.cu)
    for e in range(spec.cu, H, spec.cu):                              # horizontal CU edges
        for c0 in range(0, W, spec.cu):
            for s in free:
                beta, tc = spec.beta_tc(c0 + s, e - 1, c0 + s, e)
                Y[e - 4:e + 4, c0 + s:c0 + s + 4] = luma_lines(k, beta, tc, mx).T
                k += 1
    cqp = (VARIANTS[variant]["cb"], VARIANTS[variant]["cr"])
    for c in (1, 2):
        C = planes[c]
        for e in range(8, W // 2, 8):
            for r in range(H // 2):
                tc = spec.chroma_tc(2 * e - 1, 2 * r, 2 * e, 2 * r, cqp[c - 1])
                C[r, e - 2:e + 2] = chroma_line(k, tc, mx)
                k += 1
        for e in range(8, H // 2, 8):
            for c0 in range(0, W // 2, 8):
                for x in range(c0 + 2, c0 + 6):
                    tc = spec.chroma_tc(2 * x, 2 * e - 1, 2 * x, 2 * e, cqp[c - 1])
                    C[e - 2:e + 2, x] = chroma_line(k, tc, mx)
                    k += 1
    return planes


def plant_blocks(spec, seed):
    """Block-constant planes: every 8 x 8 luma block (4 x 4 chroma) one value, neighbours 5..7 apart, so a
    filtered edge always moves p0 or q0 (tC >= 1 at the QpY these pictures use) and an unfiltered one stays."""
    rng = np.random.default_rng([22, seed])
    mx = (1 << spec.bd) - 1
    out = []
    for c in range(3):
        n = W // 8
        ys, xs = np.mgrid[0:n, 0:n]
        v = (mx + 1) // 2 + 3 * (((xs + ys) % 2) * 2 - 1) + rng.integers(0, 2, (n, n))
        b = 8 >> (c > 0)
        out.append(np.repeat(np.repeat(v, b, axis=0), b, axis=1))
    return out


# ---------------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------------

def _sao_args(bit_depth, rs):
    a = (1 << (min(bit_depth, 10) - 5)) - 1                          # the largest sao_offset_abs
    return dict(sao_type=(2, 2, 2), sao_abs=[[a] * 4] * 3, sao_eo=(rs % 4, (rs + 1) % 4, (rs + 1) % 4))


def build(spec, planes, variant, sao=False, meta=None, nxn_modes=None, params=None):
    """-> records.Picture of PCM CUs carrying ``planes`` (``nxn_modes``: ordinary 8 x 8 NxN CUs without a
    DC residual instead, which predict their own samples).  ``sao``: the SAO twin's arguments for every CTU,
    unless spec.sao gives each CTU its own; ``params``: instead of params_of(variant)."""
    if params is None:
        params = params_of(spec.bd, spec.ctb_log2, variant, sao, spec.w, spec.h)
    offy, offc = R.qp_bd_offset(params, 0), R.qp_bd_offset(params, 1)
    b = frontend.PictureBuilder(params)
    cu_log2 = spec.cu.bit_length() - 1
    nxn_rng = np.random.default_rng(24)

    def node(x, y, log2):
        n = 1 << log2
        if x >= spec.w or y >= spec.h:
            return
        if log2 > cu_log2:
            for i in range(4):
                node(x + (n >> 1) * (i % 2), y + (n >> 1) * (i // 2), log2 - 1)
            return
        qy = spec.qp_at(x, y)
        qcb, qcr = frontend.chroma_qp(qy, 0, 0, offc)
        qps = (qy + offy, qcb + offc, qcr + offc)
        if nxn_modes is not None:
            dc = lambda: np.array([[int(nxn_rng.integers(-60, 61))] + [0] * 15], np.int16).reshape(4, 4)
            tus = [dict(x=x + 4 * (i % 2), y=y + 4 * (i // 2), log2=2, blk=i, cbf=[1, int(i == 3), int(i == 3)],
                        tskip=[0, 0, 0], coef=[dc(), dc(), dc()]) for i in range(4)]
            m = nxn_modes[(x // 8 + 3 * (y // 8)) % len(nxn_modes)]
            b.add_cu(x, y, 3, 1, [m, (m + 9) % 35, (m + 18) % 35, (m + 27) % 35], (m + 5) % 35, *qps, tus)
            return
        smp = [planes[c][y >> (c > 0):(y + n) >> (c > 0), x >> (c > 0):(x + n) >> (c > 0)].astype(np.int16)
               for c in range(3)]
        b.pcm_lf_disabled = bool(spec.nf_pcm[y // n, x // n])
        b.add_cu(x, y, log2, 0, [0] * 4, 0, *qps, [], pcm=True, pcm_samples=smp, bypass=bool(spec.nf[y // n, x // n]))

    first = {}
    order = np.lexsort((np.arange(len(spec.tile)), spec.tile))        # tile scan: a slice's address is its first CTU
    for rs in order:
        first.setdefault((int(spec.tile[rs]), int(spec.slice[rs])), int(rs))
    for rs in range(spec.wc * spec.hc):
        node((rs % spec.wc) << spec.ctb_log2, (rs // spec.wc) << spec.ctb_log2, spec.ctb_log2)
        bo, to = spec.off[rs]
        b.add_ctu(rs, slice_addr=first[(int(spec.tile[rs]), int(spec.slice[rs]))], tile_id=int(spec.tile[rs]),
                  lf_across_slices=bool(spec.lf_across[rs]), deblocking=bool(spec.dbk[rs]), beta_offset_div2=bo,
                  tc_offset_div2=to, **(spec.sao[rs] if spec.sao is not None else _sao_args(spec.bd, rs) if sao else {}))
    m = dict(bit_depth=spec.bd, ctb_log2=spec.ctb_log2, cu=spec.cu, variant=variant, sao=bool(sao))
    m.update(meta or {})
    pic = b.finish(meta=m)
    pic.spec, pic.planes = spec, planes
    return pic


def _cells_spec(bd, ctb_log2, cu, j):
    """QpY cycling over -QpBdOffsetY..51 (neighbours 7 and 11 apart: odd sums, QpP != QpQ), CTU offsets cycling over
    OFFSETS, every 13th CU a bypass CU."""
    s = Spec(bd, ctb_log2, cu)
    n, lo = W // cu, -6 * (bd - 8)
    ys, xs = np.mgrid[0:n, 0:n]
    s.qp = lo + (xs * 7 + ys * 11 + j * 5) % (52 - lo)
    if j % 2:                                        # every other picture: the upper QpY, where beta and tC are large
        s.qp = 26 + (xs * 7 + ys * 11 + j * 5) % 26
    s.nf = (xs + 5 * ys + j) % 13 == 0
    s.off = [OFFSETS[(rs + j) % len(OFFSETS)] for rs in range(s.wc * s.wc)]
    return s


def _rules_spec(bd, ctb_log2, cu, j):
    """Seeded slice / tile / deblocking-off / offset layouts: slices are runs of CTUs in tile-scan order, every
    slice with its own slice_loop_filter_across_slices, deblocking flag and offsets; QpY 30..45."""
    rng = np.random.default_rng([23, ctb_log2, j])
    s = Spec(bd, ctb_log2, cu)
    n, nc = W // cu, s.wc * s.wc
    s.qp = rng.integers(30, 46, (n, n))
    if j % 3:                                                         # two tile columns / rows / 2 x 2
        cols, rows = ((2, 1), (1, 2), (2, 2))[(j // 3) % 3]
        for rs in range(nc):
            s.tile[rs] = ((rs // s.wc) * rows // s.wc) * cols + (rs % s.wc) * cols // s.wc
    order = np.lexsort((np.arange(nc), s.tile))
    n_slices = int(rng.integers(1, min(nc, 6) + 1))
    cuts = set(rng.choice(np.arange(1, nc), n_slices - 1, replace=False).tolist()) if n_slices > 1 else set()
    sid, attrs = 0, {}
    for ts, rs in enumerate(order):
        sid += ts in cuts
        if sid not in attrs:
            attrs[sid] = (bool(rng.integers(0, 2)), bool(rng.random() < 0.7), (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))))
        s.slice[rs], (s.lf_across[rs], s.dbk[rs], off) = sid, attrs[sid]
        s.off[rs] = off
    s.nf = rng.random((n, n)) < 0.08
    return s


_SETS = {}
N_CELLS = 4
N_RULES = 6


def lf_set(bit_depth, ctb_log2, variant, sao=False):
    """[Picture] of the fixed set of one context (built once per process)."""
    key = (bit_depth, ctb_log2, variant, bool(sao))
    if key in _SETS:
        return _SETS[key]
    vi = "abc".index(variant)
    pics = []
    for j in range(N_CELLS):
        spec = _cells_spec(bit_depth, ctb_log2, 16, N_CELLS * vi + j)
        pics.append(build(spec, plant_cells(spec, variant, 100 * vi + j), variant, sao, dict(kind="cells", j=j)))
    spec = _cells_spec(bit_depth, ctb_log2, 8, 3 * vi + 1)
    pics.append(build(spec, plant_cells(spec, variant, 100 * vi + 50), variant, sao, dict(kind="grid8")))
    if ctb_log2 >= 5:
        spec = _cells_spec(bit_depth, ctb_log2, 32, 3 * vi + 1)
        pics.append(build(spec, plant_cells(spec, variant, 100 * vi + 60), variant, sao, dict(kind="grid32")))
    for j in range(N_RULES):
        spec = _rules_spec(bit_depth, ctb_log2, 8 if j % 2 else 16, N_RULES * vi + j)
        pics.append(build(spec, plant_blocks(spec, 100 * vi + j), variant, sao, dict(kind="rules", j=j)))
    if variant == "a":
        spec = _cells_spec(bit_depth, ctb_log2, 8, 1)
        spec.nf[:] = False
        pics.append(build(spec, None, variant, sao, dict(kind="nxn"), nxn_modes=(0, 1, 10, 26, 34, 2, 18)))
    _SETS[key] = pics
    return pics
