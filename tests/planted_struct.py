"""Planted structure pictures: the bookkeeping around the blocks (plain Python, no GPU).

tests/planted.py plants what one block computes.  This set plants the structure the blocks sit in: how a
CTU is tiled with TBs, in which order its records come, how many jobs job preparation makes of them
(p265_amd/csrc/intra_prep.h: Cb / Cr pairing, compaction into [chroma][luma] lists, 4x4 quad merging) and the
two indices the row kernel synchronises on (`tr`, the first job that reads the top-right CTU; `br`, one past
the last job of the bottom-left quadrant).

  * a picture is 3 x 2 CTBs (the ``edges`` family: 2 CTBs and a part), no in-loop filter, qP' 30 + QpBdOffset;
    every CU is an ordinary intra CU and every TB carries a seeded synth._coef_block residual unless a cell
    needs it uncoded, so every block depends on its neighbours' reconstruction and on decode order;
  * a CTU is described by a tree: a leaf 8 / 16 / 32 (CUs of that size with one TB), "nxn" (8x8 NxN CUs: four
    4x4 luma TBs with a mode each), "s4" (the largest CU of at most 32 split down to 4x4 with one mode), or a
    list of four subtrees (the quadrants in z-order);
  * FLOWS: one luma mode everywhere (34: top and top-right only; 2: left and bottom-left; 18: corner; 26, 10,
    1, 0; 17 and 20, under which the chroma TBs predict with 34 and 2) or ``cycle`` (all 35 modes in turn per
    TB); chroma mode (luma + 17) % 35;
  * records come from frontend.PictureBuilder; component_major() is the [all Y, all Cb, all Cr] twin.

struct_set(bit_depth, ctb_log2) is the fixed set; expected_jobs() is the host model of job preparation;
direction_cells() / direction_cells_wanted() are the coverage helpers tests/test_planted_struct.py asserts with
(the other cells are read from expected_jobs()).
"""
import numpy as np

from oracle import recon_oracle as O
from p265_amd import frontend, synth
from p265_amd import records as R

FLOWS = (34, 2, 18, 26, 10, 1, 0, "cycle", 17, 20)     # (luma 17 / 20 / 1: chroma 34 / 2 / 18)
RC_DST4, RC_DCT4, RC_DCT8, RC_DCT16, RC_DCT32, RC_TSKIP, RC_RAW = range(7)     # batch_types.h ResClass


# ---------------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------------

def _z4(x, y, s):
    """4x4 positions of an s x s region in z-order with blkIdx inside the parent 8x8."""
    if s == 4:
        return [(x, y)]
    h = s >> 1
    return [p for i in range(4) for p in _z4(x + h * (i % 2), y + h * (i // 2), h)]


_POOL, _POOLS = 2048, {}


def _coef_pool(log2):
    """2048 seeded synth._coef_block residuals of one size, drawn once per process; a picture's TBs take them
    from a seeded start in steps of 7919 (drawing one per TB costs more than everything else the builder does).
    Four to ten levels per TB whatever its size, clipped to +-32 - a dense large block or one of _coef_block's large
    levels (one in fifty, up to 2000) saturates the whole TB, and a saturated sample hides what it was predicted
    from - and a DC level of 3..6 either way, so that negating a TB's levels moves every one of its samples."""
    if log2 not in _POOLS:
        rng = np.random.default_rng([77, log2])
        pool = []
        for _ in range(_POOL):
            co = np.clip(synth._coef_block(rng, log2, {2: 0.25, 3: 0.08, 4: 0.03, 5: 0.01}[log2]), -32, 32).astype(np.int16)
            if abs(int(co[0, 0])) < 3:
                co[0, 0] = int(rng.integers(3, 7)) * (1 if rng.integers(0, 2) else -1)
            pool.append(co)
        _POOLS[log2] = pool
    return _POOLS[log2]


class _Build:
    def __init__(self, bit_depth, ctb_log2, size, flow, seed):
        self.w, self.h = size
        self.params = R.make_params(pic_width=self.w, pic_height=self.h, ctb_log2_size=ctb_log2,
                                    sample_adaptive_offset=0, bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth)
        self.b = frontend.PictureBuilder(self.params)
        self.rng = np.random.default_rng([seed, bit_depth, ctb_log2])
        self.flow, self.k = flow, 0
        self.c0, self.kc = int(self.rng.integers(0, _POOL)), 0
        off = 6 * (bit_depth - 8)
        qcb, qcr = frontend.chroma_qp(30, 0, 0, off)
        self.qps = (30 + off, qcb + off, qcr + off)

    def modes(self, n):
        if self.flow != "cycle":
            return [int(self.flow)] * n
        m = [(self.k + i) % 35 for i in range(n)]
        self.k += n
        return m

    def coef(self, log2):
        self.kc += 1
        return _coef_pool(log2)[(self.c0 + 7919 * self.kc) % _POOL]

    def cu(self, x, y, size, leaf, opt):
        """One CU at (x, y).  ``opt``: luma (coded flag per TU in z-order), chroma ((Cb, Cr) coded flags per
        chroma pair in z-order), tskip (TU indices with luma transform skip), bypass."""
        lg = size.bit_length() - 1
        tb = size if isinstance(leaf, int) else 4
        pos = [(x, y)] if tb == size else _z4(x, y, size)
        nxn = leaf == "nxn"
        modes = self.modes(4) if nxn else self.modes(1) * 4
        luma = opt.get("luma", [1] * len(pos))
        chroma = opt.get("chroma")
        tskip = opt.get("tskip", ())
        tus, kc = [], 0
        for i, (tx, ty) in enumerate(pos):
            tl = tb.bit_length() - 1
            blk = i % 4 if tb == 4 else 0
            has_c = tb > 4 or blk == 3
            cb, cr = (chroma[kc] if chroma is not None else (1, 1)) if has_c else (0, 0)
            kc += int(has_c)
            co = [self.coef(tl) if luma[i] else None, self.coef(max(tl - 1, 2)) if cb else None,
                  self.coef(max(tl - 1, 2)) if cr else None]
            tus.append(dict(x=tx, y=ty, log2=tl, blk=blk, cbf=[int(v is not None) for v in co],
                            tskip=[int(i in tskip), 0, 0], coef=co))
        self.b.add_cu(x, y, lg, 1 if nxn else 0, modes, (modes[0] + 17) % 35, *self.qps, tus,
                      bypass=bool(opt.get("bypass", False)))

    def node(self, x, y, size, tree, opts):
        if x >= self.w or y >= self.h:
            return
        h = size >> 1
        if isinstance(tree, list):
            for i in range(4):
                self.node(x + h * (i % 2), y + h * (i // 2), h, tree[i], opts)
            return
        cu = tree if isinstance(tree, int) else (8 if tree == "nxn" else min(32, size))
        if cu > size:
            raise ValueError("a %r leaf does not fit a region of %d" % (tree, size))
        if cu < size or x + size > self.w or y + size > self.h:
            # (a CU that would cross the picture edge splits further: 8 at the least, widths are multiples of 8)
            sub = tree if cu < size or not isinstance(tree, int) else max(tree >> 1, 8)
            for i in range(4):
                self.node(x + h * (i % 2), y + h * (i // 2), h, sub, opts)
            return
        self.cu(x, y, size, tree, opts.get((x, y), {}))


def build(bit_depth, ctb_log2, trees, flow, size=None, slices=None, tiles=None, seed=0, opts=None, meta=None):
    """-> records.Picture.  ``trees``: {CTU raster address: tree} (8 elsewhere); ``slices`` / ``tiles``:
    slice_addr / tile_id per CTU; ``opts``: {CU origin: options of _Build.cu}."""
    ctb = 1 << ctb_log2
    size = size or (3 * ctb, 2 * ctb)
    bld = _Build(bit_depth, ctb_log2, size, flow, seed)
    wc, hc = R.ctb_grid(bld.params)
    for rs in range(wc * hc):
        bld.node((rs % wc) * ctb, (rs // wc) * ctb, ctb, trees.get(rs, 8), opts or {})
        bld.b.add_ctu(rs, slice_addr=int(slices[rs]) if slices else 0, tile_id=int(tiles[rs]) if tiles else 0)
    m = dict(flow=flow, order="tu", bit_depth=bit_depth, ctb=ctb, seed=seed)
    m.update(meta or {})
    pic = bld.b.finish(meta=m)
    pic.size = size
    return pic


def component_major(pic):
    """The picture with each CTU's TBs reordered to [all Y, all Cb, all Cr] (the reorder of
    test_gpu_parity._component_major): the order inside a component is unchanged, the output identical, no
    Cb is followed by its Cr."""
    tbs = pic.tbs.copy()
    for ctu in pic.ctus:
        b, n = int(ctu["tb_begin"]), int(ctu["tb_count"])
        seg = pic.tbs[b:b + n]
        tbs[b:b + n] = seg[np.argsort(seg["c_idx"], kind="stable")]
    m = dict(pic.meta)
    m["order"] = "cm"
    return R.Picture(ctus=pic.ctus, tbs=tbs, coef=pic.coef, nofilter=pic.nofilter, meta=m, size=pic.size)


def set_params(bit_depth, ctb_log2, edges=False):
    """The context a set decodes in: 3 x 2 CTBs; the ``edges`` pictures in one of 3 x 3 CTBs, where each is
    smaller than the context (a ragged batch)."""
    ctb = 1 << ctb_log2
    return R.make_params(pic_width=3 * ctb, pic_height=(3 if edges else 2) * ctb, ctb_log2_size=ctb_log2,
                         sample_adaptive_offset=0, bit_depth_luma=bit_depth, bit_depth_chroma=bit_depth)


# ---------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------

def _gf4_mul(a, b):
    """GF(4) = {0, 1, w, w + 1} as 0..3 (addition is xor)."""
    if a == 0 or b == 0:
        return 0
    return ((a - 1 + b - 1) % 3) + 1


def orthogonal_tuples(levels):
    """4-tuples over range(levels) in which every ordered pair occurs in every pair of columns (a strength-2
    orthogonal array): (a, b, a + b, a + 2b) over GF(3) (9 rows), (a, b, a + b, a + w b) over GF(4) (16 rows),
    every tuple at two levels."""
    if levels == 2:
        return [(a, b, c, d) for a in range(2) for b in range(2) for c in range(2) for d in range(2)]
    if levels == 3:
        return [(a, b, (a + b) % 3, (a + 2 * b) % 3) for a in range(3) for b in range(3)]
    if levels == 4:
        return [(a, b, a ^ b, a ^ _gf4_mul(2, b)) for a in range(4) for b in range(4)]
    raise ValueError(levels)


def _leaves(fit):
    """Leaves that tile a region of ``fit`` samples, smallest TB first."""
    return ["nxn"] + [n for n in (8, 16, 32) if n <= fit]


def _tiling(ctb_log2, bd):
    ctb = 1 << ctb_log2
    kinds = [8] + ([16] if ctb >= 16 else []) + ([32] if ctb == 64 else []) + ["nxn", "s4"]
    out = []
    for kind in kinds:
        for fi, flow in enumerate(FLOWS):
            p = build(bd, ctb_log2, {rs: kind for rs in range(6)}, flow, seed=1000 + fi,
                      meta=dict(family="tiling", cell="%s/%s" % (kind, flow), kind=kind))
            out += [p, component_major(p)]
    return out


def _quadrants(ctb_log2, bd):
    ctb = 1 << ctb_log2
    out = []
    lv = _leaves(ctb >> 1)
    tup = orthogonal_tuples(len(lv))
    # one level up: whole CTUs of one leaf each, rows [a, b, a] / [b, b, a].  Over all ordered (a, b) every
    # ordered pair of leaves meets as (target, neighbour CTU) to the left (row 0), above (column 0), above left
    # (a above left of b at column 1, b of a at column 2), above right (b / a above right of b at columns 0 / 1)
    # and below left (row 1 column 0 / 1 below left of b / a)
    lv0 = _leaves(ctb)
    flows = ("cycle", 34, 2, 17, 20) if bd == 8 else ("cycle",)     # (the 10 / 12-bit repeats are thinned: CPU time)
    for fi, flow in enumerate(flows):
        for a in lv0:
            for b in lv0:
                out.append(build(bd, ctb_log2, dict(enumerate([a, b, a, b, b, a])), flow, seed=1900 + fi,
                                 meta=dict(family="quadrants", cell="CTUs %s %s/%s" % (a, b, flow))))
    for fi, flow in enumerate(flows):
        for k in range(len(tup)):
            # CTU rs takes tuple k + rs, so a picture also holds six different CTU tilings side by side
            trees = {rs: [lv[i] for i in tup[(k + rs) % len(tup)]] for rs in range(6)}
            out.append(build(bd, ctb_log2, trees, flow, seed=2000 + 100 * fi + k,
                             meta=dict(family="quadrants", cell="L0 tuple %d/%s" % (k, flow))))
    if ctb >= 32:                                        # one level down, inside one quadrant (rotating)
        lv2 = _leaves(ctb >> 2)
        tup2 = orthogonal_tuples(len(lv2))
        for fi, flow in enumerate(flows):
            for k in range(len(tup2)):
                trees = {}
                for rs in range(6):
                    t = [lv[i] for i in tup[(k + rs) % len(tup)]]
                    t[(k + rs) % 4] = [lv2[i] for i in tup2[(k + rs) % len(tup2)]]
                    trees[rs] = t
                out.append(build(bd, ctb_log2, trees, flow, seed=2500 + 100 * fi + k,
                                 meta=dict(family="quadrants", cell="L1 tuple %d/%s" % (k, flow))))
    return out


def _regions8(ctb):
    """The 8x8 regions of a CTB in z-order (CTB-relative origins)."""
    def z(x, y, s):
        if s == 8:
            return [(x, y)]
        h = s >> 1
        return [p for i in range(4) for p in z(x + h * (i % 2), y + h * (i // 2), h)]
    return z(0, 0, ctb)


def _tree_of_regions(ctb, kinds):
    """Tree of a CTB from the kind of each 8x8 region in z-order: 8, "nxn", or 16 for all four regions of an
    aligned 16x16."""
    def t(i, s):
        n = (s >> 3) ** 2
        if s == 8:
            return kinds[i]
        if s == 16 and kinds[i] == 16:
            assert kinds[i:i + 4] == [16] * 4
            return 16
        return [t(i + q * (n >> 2), s >> 1) for q in range(4)]
    return t(0, ctb)


def counts_plan(ctb):
    """[(name, kinds per 8x8 region in z-order, 8x8 regions whose first sub-TB is transform skip)] of the
    ``counts`` CTUs.  With a 8x8 TBs, b 4x4 regions and c 16x16 TBs, a + b + 4c = R regions (R = 64 at CTB 64):
    the luma list holds a + 4b + c = R + 3 (b - c) entries before merging, so its reachable lengths are those
    = R mod 3: 61, 64, 67 / 127, 130 / 190, 193 / 256 sit either side of the window edges.  p 8x8 TBs ahead of a
    run of 4x4 regions put the quad heads at slots p, p + 4, ...: p = 0..3 gives slots 60 and 0 (= 64), 61, 62,
    63 of each edge the run reaches.  A region whose first sub-TB is transform skip (another residual class,
    another slab) stays four jobs: k of them in an all-4x4 CTU leave R + 3k jobs after merging."""
    r = (ctb >> 3) ** 2
    out = []

    def add(name, kinds, ts=()):
        assert len(kinds) == r
        out.append((name, kinds, tuple(ts)))

    for b, c in ((0, 1), (0, 0), (1, 0)) + (((21, 0), (22, 0), (42, 0), (43, 0)) if ctb == 64 else ((15, 0),)):
        add("len%d" % (r + 3 * (b - c)), [16] * (4 * c) + [8] * (r - 4 * c - b) + ["nxn"] * b)
    for p in range(4):                                   # heads at slots = p mod 4, up to the last window edge
        add("head%d" % p, [8] * p + ["nxn"] * (r - p))
    if ctb == 64:
        for k in (1, 21, 22):
            add("merged%d" % (r + 3 * k), ["nxn"] * r, ts=range(k))
        # chroma list of the component-major twin: 2 (64 - 3c) unpaired entries
        for c in (15, 14, 8, 7):                         # 3 (64 - 3c) records: 57, 66 / 120, 129
            add("rec%d" % (3 * (r - 3 * c)), [16] * (4 * c) + [8] * (r - 4 * c))
        add("chroma62", [16] * 44 + [8] * 20)
        add("chroma68", [16] * 40 + [8] * 24)
    return out


def _counts(ctb_log2, bd):
    ctb = 1 << ctb_log2
    if ctb < 32:
        return []
    out = []
    reg = _regions8(ctb)
    for i, (name, kinds, ts) in enumerate(counts_plan(ctb)):
        trees, opts = {}, {}
        for rs in range(6):
            trees[rs] = _tree_of_regions(ctb, kinds)
            for k in ts:
                opts[((rs % 3) * ctb + reg[k][0], (rs // 3) * ctb + reg[k][1])] = dict(tskip=(0,))
        p = build(bd, ctb_log2, trees, "cycle", seed=3000 + i, opts=opts,
                  meta=dict(family="counts", cell=name))
        out += [p, component_major(p)]
    return out


CHROMA_QUAD_PATTERNS = [0, 255] + [1 << i for i in range(8)] + [int(v) for v in
                                                                np.random.default_rng(44).permutation(254)[:16] + 1]


def _quads(ctb_log2, bd):
    """One 4x4 region per CTU at the CTU's region 3 (8, 8) among 8x8 TBs; chroma: the four 8x8 CUs of the 16x16
    at the CTU's origin (four consecutive Cb+Cr 4x4 pairs)."""
    ctb = 1 << ctb_log2
    cells = [("luma%d" % m, "nxn", dict(luma=[(m >> i) & 1 for i in range(4)])) for m in range(16)]
    cells += [("tskip%d" % i, "nxn", dict(tskip=(i,))) for i in range(4)]
    cells += [("bypass", "nxn", dict(bypass=True)), ("bypass_s4", "s4", dict(bypass=True)), ("s4", "s4", {})]
    cells += [("tskip_uncoded", "nxn", dict(tskip=(1,), luma=[1, 1, 0, 1]))]
    out = []
    origin = lambda rs: ((rs % 3) * ctb, (rs // 3) * ctb)
    for k in range(0, len(cells), 6):
        trees, opts, names = {}, {}, []
        for rs, (name, leaf, opt) in enumerate(cells[k:k + 6]):
            x0, y0 = origin(rs)
            kinds = [8] * ((ctb >> 3) ** 2)
            kinds[3] = leaf
            trees[rs] = _tree_of_regions(ctb, kinds)
            opts[(x0 + 8, y0 + 8)] = opt
            names.append(name)
        out.append(build(bd, ctb_log2, trees, "cycle", seed=4000 + k, opts=opts,
                         meta=dict(family="quads", cell="+".join(names), cells=names)))
    for k in range(0, len(CHROMA_QUAD_PATTERNS), 6):
        opts, names = {}, []
        for rs, m in enumerate(CHROMA_QUAD_PATTERNS[k:k + 6]):
            x0, y0 = origin(rs)
            for q in range(4):
                opts[(x0 + 8 * (q % 2), y0 + 8 * (q // 2))] = dict(chroma=[((m >> (2 * q)) & 1, (m >> (2 * q + 1)) & 1)])
            names.append("chroma%d" % m)
        out.append(build(bd, ctb_log2, {}, "cycle", seed=4100 + k, opts=opts,
                         meta=dict(family="quads", cell="+".join(names), cells=names)))
    # a bypass CU among the four 8x8 CUs of a chroma region (its Cb / Cr are in the raw slab: no common base), one
    # per CTU at each position; the next 16x16 of 8x8 CUs follows sub-pairs 1, 2, 3 of the unmerged one
    if ctb >= 16:
        opts = {(origin(rs)[0] + 8 * (rs % 2), origin(rs)[1] + 8 * ((rs // 2) % 2)): dict(bypass=True) for rs in range(6)}
        out.append(build(bd, ctb_log2, {}, "cycle", seed=4150, opts=opts,
                         meta=dict(family="quads", cell="chroma bypass", cells=["chroma_bypass"])))
    # four consecutive luma 4x4 TBs that are not one region: sub-TBs 1, 2, 3 of a region that does not merge (its
    # first sub-TB is transform skip) and sub-TB 0 of the next, at every CTU's first and third region
    opts = {(origin(rs)[0] + 8 * k, origin(rs)[1] + 8 * k): dict(tskip=(0,)) for rs in range(6) for k in range(2 if ctb > 16 else 1)}
    out.append(build(bd, ctb_log2, {rs: "nxn" for rs in range(6)}, "cycle", seed=4160, opts=opts,
                     meta=dict(family="quads", cell="1, 2, 3 + 0 of the next", cells=["unaligned"])))
    # a region whose first sub-TB has no reference at all: the picture origin and the first CTU of a slice
    kinds = [8] * ((ctb >> 3) ** 2)
    kinds[0] = "nxn"
    t = _tree_of_regions(ctb, kinds)
    out.append(build(bd, ctb_log2, {0: t, 4: t}, "cycle", slices=[0, 0, 0, 0, 4, 4], seed=4200,
                     meta=dict(family="quads", cell="noref", cells=["noref"])))
    return out


def _nonfast(ctb_log2, bd):
    """Target at the origin of CTU 4 (column 1, row 1).  ``above``: the slice starts at the CTU above, so left
    and top are available and the corner is not; ``aboveright``: it starts at the CTU above right, so left and
    top-right are available and corner and top are not.  Neither is one run of available units.

    No tile layout gives such a pattern: tiles are the cells of a column x row grid, so if two of the left, top
    and top-right CTUs are in the target's tile, the CTUs between them along the row above are too, and the
    top-left CTU with the left and the top one.  Inside one tile the CTUs follow in raster order, which is the
    slice case built here; the ``tile`` pictures add a tile column boundary left of the target CTU under the
    same slice start (left, bottom-left and corner missing, top and top-right available: one run)."""
    ctb = 1 << ctb_log2
    out = []
    r = (ctb >> 3) ** 2
    for li, leaf in enumerate(["nxn", 8] + ([16] if ctb >= 16 else [])):
        kinds = [8] * r
        if leaf == 16 and ctb > 16:
            kinds[0:4] = [16] * 4
        elif leaf != 16:
            kinds[0] = leaf
        t = 16 if (leaf == 16 and ctb == 16) else _tree_of_regions(ctb, kinds)
        for name, start, tiles in (("above", 1, None), ("aboveright", 2, None), ("tile", 1, [0, 1, 1] * 2)):
            for flow in ("cycle", 18):
                out.append(build(bd, ctb_log2, {4: t}, flow, slices=[0] * start + [start] * (6 - start), tiles=tiles,
                                 seed=5000 + 10 * li, meta=dict(family="nonfast", cell="%s/%s/%s" % (leaf, name, flow))))
    return out


def _path_tree(ctb, n, pre, rest=8):
    """Tree of a CTB whose block at (ctb - n, 0) is a TB of n ("nxn" region at n = 4): quadrant 1 down to the
    block; the quadrants decoded before it are tiled with ``pre``, the ones after it with ``rest``."""
    s = max(n, 8)

    def t(size):
        if size == s:
            return "nxn" if n == 4 else n
        fit = lambda leaf: leaf if (isinstance(leaf, str) or leaf <= size >> 1) else size >> 1
        return [fit(pre), t(size >> 1), fit(rest), fit(rest)]
    return t(ctb)


TR_VARIANTS = ("same", "slice", "tile", "absent", "first_row")


def _topright(ctb_log2, bd):
    ctb = 1 << ctb_log2
    out = []
    sizes = [n for n in (4, 8, 16, 32) if n <= ctb]
    for n in sizes:
        for pi, pre in enumerate((32, 8, "nxn")):       # `tr` a small, a middle and a large index
            if n == ctb:
                if pi:
                    continue
                t = n
            else:
                t = _path_tree(ctb, n, pre)
            for flow in (34, 17):                       # (luma 17: chroma mode 34)
                p = build(bd, ctb_log2, {4: t, 1: t}, flow, seed=6000 + 10 * n + pi,
                          meta=dict(family="topright", cell="n%d/pre%s/%d" % (n, pre, flow), variant="same", n=n))
                out += [p, component_major(p)]
    # the top-right CTU of the target: same slice and tile, another slice, another tile, absent, first CTU row
    t = _path_tree(ctb, 8, 8) if ctb > 8 else 8
    for vi, var in enumerate(TR_VARIANTS):
        kw = dict(slices=[0, 0, 0, 3, 3, 3]) if var == "slice" else dict(tiles=[0, 0, 1] * 2) if var == "tile" else {}
        target = {"absent": 5, "first_row": 1}.get(var, 4)
        for flow in (34, "cycle"):
            trees = {0: "nxn", 1: 16 if ctb >= 16 else 8, 2: "nxn"}
            trees[target] = t
            out.append(build(bd, ctb_log2, trees, flow, seed=6500 + vi, meta=dict(family="topright", cell="variant %s/%s" % (var, flow),
                                                       variant=var, target=target), **kw))
    if ctb <= 32:             # whole-CTB TBs in a tile two CTBs wide: the CTB above right is the job just before
        for flow in (34, 17):
            out.append(build(bd, ctb_log2, {rs: ctb for rs in range(6)}, flow, tiles=[0, 1, 1] * 2, seed=6700,
                             meta=dict(family="topright", cell="whole CTBs, tile of 2/%d" % flow, variant="tile2")))
    if ctb == 64:                                        # the top-right CTU's bottom-left quadrant, five ways
        mix = [16, 8, "nxn", [8, 8, 8, "nxn"]]
        for bi, (name, bl) in enumerate((("32", 32), ("16", 16), ("8", 8), ("nxn", "nxn"), ("mix", mix))):
            # (the target CTU's 32x32 at x = 32 reads the first 32 samples of that CTU's bottom row, its Cb+Cr 16)
            for flow in (34, 17):
                p = build(bd, ctb_log2, {2: [8, 16, bl, "nxn"], 4: _path_tree(ctb, 32, "nxn")}, flow, seed=6800 + bi,
                          meta=dict(family="topright", cell="bl %s/%d" % (name, flow), variant="same", bl=name))
                out += [p, component_major(p)]
    return out


def _edges(ctb_log2, bd):
    ctb = 1 << ctb_log2
    out = []
    for off in (8, 24, 40, 56):
        if off >= ctb:
            continue
        for flow in (34, 2):
            for k, size in enumerate(((2 * ctb + off, 2 * ctb), (2 * ctb, 2 * ctb + off), (2 * ctb + off, 2 * ctb + off))):
                lv = _leaves(ctb >> 1)
                trees = {rs: [lv[(rs + q + k) % len(lv)] for q in range(4)] for rs in range(9)}
                out.append(build(bd, ctb_log2, trees, flow, size=size, seed=7000 + off + k,
                                 meta=dict(family="edges", cell="%dx%d/%s" % (size[0], size[1], flow))))
    return out


def _adjacent(ctb_log2, bd):
    """Pictures for "the neighbour is the job just before the target" where the tilings above do not give it
    (direction_cells_wanted):

      column  every column of CTBs a tile of its own, so the CTB above is the previous one in tile scan: its last TB
              lies above (and above right of) the first TB of the CTB below; leaves [a, b, a] / [b, b, a] over all
              ordered (a, b), whole-CTB TBs included;
      tile2   a tile two CTBs wide, whole-CTB TBs below, every leaf in the CTB above right;
      col8    a last CTB column of 8 samples, 8x8 TBs and 4x4 regions alternating down it: the job before a TB is
              the one above it."""
    ctb = 1 << ctb_log2
    out = []
    lv0 = _leaves(ctb)
    flows = ("cycle", 34, 2, 17, 20) if bd == 8 else ("cycle",)
    for fi, flow in enumerate(flows):
        for a in lv0:
            for b in lv0:
                out.append(build(bd, ctb_log2, dict(enumerate([a, b, a, b, b, a])), flow, tiles=[0, 1, 2] * 2, seed=8000 + fi,
                                 meta=dict(family="adjacent", cell="column %s %s/%s" % (a, b, flow))))
            if ctb <= 32:
                trees = {rs: ctb for rs in range(6)}
                trees[2] = a
                out.append(build(bd, ctb_log2, trees, flow, tiles=[0, 1, 1] * 2, seed=8100 + fi,
                                 meta=dict(family="adjacent", cell="tile2 %s/%s" % (a, flow))))
        r8 = _regions8(ctb)
        for k in range(2):
            kinds = [8 if ((y >> 3) + k) % 2 == 0 else "nxn" for _, y in r8]
            t = _tree_of_regions(ctb, kinds)
            out.append(build(bd, ctb_log2, {2: t, 5: t}, flow, size=(2 * ctb + 8, 2 * ctb), seed=8200 + fi,
                             meta=dict(family="adjacent", cell="col8 %d/%s" % (k, flow))))
    return out


FAMILIES = dict(tiling=_tiling, quadrants=_quadrants, counts=_counts, quads=_quads, nonfast=_nonfast,
                topright=_topright, adjacent=_adjacent, edges=_edges)
_SETS = {}


def struct_set(bit_depth, ctb_log2, family=None):
    """The fixed set of one (bit depth, CTB size) as a list of pictures (built once per process); the ``edges``
    pictures last (they decode in set_params(edges=True))."""
    key = (bit_depth, ctb_log2)
    if key not in _SETS:
        _SETS[key] = [p for name, f in FAMILIES.items() for p in f(ctb_log2, bit_depth)]
    return [p for p in _SETS[key] if family is None or p.meta["family"] == family]


# ---------------------------------------------------------------------------------
# host model of job preparation (intra_prep.h)
# ---------------------------------------------------------------------------------

def tb_class(t):
    """batch_types.h tb_class (lines 89-98)."""
    f, lg = int(t["flags"]), int(t["log2_size"])
    if f & (R.TB_BYPASS | R.TB_PCM):
        return RC_RAW
    if f & R.TB_TSKIP:
        return RC_TSKIP
    return {2: RC_DST4 if int(t["c_idx"]) == 0 else RC_DCT4, 3: RC_DCT8, 4: RC_DCT16}.get(lg, RC_DCT32)


def pool_offsets(pics):
    """Residual offset of every TB of a batch as intra_prep_kernel sees it (its ``roff``), per picture, and the
    zero block's offset.  Restates upload_host.cpp: plan_upload's ``pool_base`` / ``pool_at`` (one slab per
    class in ResClass order, the raw slab last, each the sum over the batch's pictures of N * N of their coded
    TBs; the loops at lines 158-181) and pack_picture's fill (lines 313-337: every TB of the picture's array in
    array order takes the next N * N of its class's slab); raw TBs are addressed relative to the residual pool
    at ``pool_rel`` = -(o_res - o_pool) / 2 with o_res - o_pool = align_up(2 * pool_total + 256, 256) (lines 212,
    346); an uncoded TB reads the zero block at ``pool_total`` (line 347)."""
    coded = [(p.tbs["flags"] & (R.TB_CBF | R.TB_PCM)) != 0 for p in pics]
    cls = [np.array([tb_class(t) for t in p.tbs], np.int64) for p in pics]
    nn = [1 << (2 * p.tbs["log2_size"].astype(np.int64)) for p in pics]
    sz = np.array([[int(nn[i][coded[i] & (cls[i] == c)].sum()) for c in range(7)] for i in range(len(pics))]).reshape(-1, 7)
    base = np.concatenate([[0], np.cumsum(sz.sum(axis=0))])
    total = int(base[7])
    pool_rel = -(((2 * total + 256 + 255) // 256 * 256) // 2)
    at = base[:7] + np.concatenate([np.zeros((1, 7), np.int64), np.cumsum(sz, axis=0)[:-1]])
    out = []
    for i, p in enumerate(pics):
        fill = [int(v) for v in at[i]]
        off = np.full(len(p.tbs), total, np.int64)
        for t in range(len(p.tbs)):
            if coded[i][t]:
                c = int(cls[i][t])
                off[t] = fill[c] + (pool_rel if c == RC_RAW else 0)
                fill[c] += int(nn[i][t])
        out.append(off)
    return out, total


def _same_tu(cb, cr):
    """intra_prep.h tb_same_tu_chroma."""
    return (int(cb["c_idx"]) == 1 and int(cr["c_idx"]) == 2 and cb["x"] == cr["x"] and cb["y"] == cr["y"]
            and cb["log2_size"] == cr["log2_size"] and cb["pred_mode"] == cr["pred_mode"]
            and not (int(cb["flags"]) ^ int(cr["flags"])) & R.TB_PCM)


def unit_avail(geo, t):
    """Availability of the reference units of a TB (4 luma samples each) in the linear order of 8.4.4.2.2, from
    the oracle's 6.4.1 (Geometry.available) at each unit's first sample."""
    sub = 1 if int(t["c_idx"]) else 0
    n, x0, y0 = 1 << int(t["log2_size"]), int(t["x"]), int(t["y"])
    us = 4 >> sub
    dx, dy = O.ref_positions(n)
    ks = list(range(0, 2 * n, us)) + [2 * n] + list(range(2 * n + 1, 4 * n + 1, us))
    return [bool(geo.available(x0 << sub, y0 << sub, (x0 + int(dx[k])) << sub, (y0 + int(dy[k])) << sub)) for k in ks]


def _one_run(av):
    on = [i for i, a in enumerate(av) if a]
    return not on or on[-1] - on[0] + 1 == len(on)


def _codes_ok(offs, zero):
    """intra_prep.h quad_codes: the coded offsets are base + 16 * code with code <= 14."""
    c = [o for o in offs if o != zero]
    return all((o - min(c)) % 16 == 0 and o - min(c) <= 14 * 16 for o in c)


def _merge(entries, chroma, on, zero):
    """Quad heads over a staged list (quad_jobs / cquad_jobs and the absorbed mask) -> emitted jobs as
    (entry index, is quad), refusal reasons of the region heads that did not merge."""
    n = len(entries)
    row = 32 if chroma else 64
    heads, why = set(), {}
    for s in range(n):
        e = entries[s]
        if e["lg"] != 2 or e["xr"] % 8 or e["yr"] % 8 or (chroma and e["cm"] != 3):
            # not the first block of an aligned region; four consecutive fast 4x4 entries that are not one
            # region (sub-TBs 1, 2, 3 of one and 0 of the next) are noted for the coverage test
            if on and s + 3 < n and all(q["lg"] == 2 and q["fast"] and (q["cm"] == 3 or not chroma) for q in entries[s:s + 4]):
                why[s] = "unaligned"
            continue
        reason = None
        if not on:
            reason = "off"
        elif s + 3 >= n:
            reason = "short"
        else:
            j = entries[s:s + 4]
            if any(q["lg"] != 2 or (chroma and q["cm"] != 3) or
                   (q["xr"], q["yr"]) != (e["xr"] + 4 * (i % 2), e["yr"] + 4 * (i // 2)) for i, q in enumerate(j)):
                reason = "position"
            elif not all(q["fast"] for q in j):
                reason = "notfast"
            elif any(q["none"] for q in j[1:]):
                reason = "none123"
            elif not _codes_ok([o for q in j for o in q["offs"]], zero):
                reason = "codes"
        if reason is None:
            heads.add(s)
        else:
            why[s] = reason
    # (sub-TBs 1..3 of a region that merged are absorbed, not a window of their own)
    why = {s: r for s, r in why.items() if r != "unaligned" or not any(h in heads for h in (s - 1, s - 2, s - 3))}
    jobs = [(s, s in heads) for s in range(n) if not any(h in heads for h in (s - 1, s - 2, s - 3))]
    return jobs, heads, why


def expected_jobs(params, pic, quad_bits, offsets=None):
    """The host model of intra_prep_kernel: per CTU (raster order) a dict with the job counts after merging
    (``luma``, ``chroma``), each list's ``tr`` (index of the first job that reads the top-right CTU, the count
    when none does) and ``br`` (one past the last job in the bottom-left quadrant, the count when none is), and
    what the coverage tests read: the staged list lengths, the head slots and the refusal reasons.

    ``quad_bits``: P265R_QUAD (bit 0 luma quads, bit 1 chroma quads, bit 2: Cb+Cr 8x8 pairs off the fast path).
    ``offsets``: (per-TB offsets of this picture, zero offset) from pool_offsets of the batch it is uploaded in
    (by default the picture alone).  The rules, as the header comment of intra_prep.h states them:

      pairing  a Cb TB followed by the Cr TB of the same TU (position, size, mode, PCM flag) is one job;
      fast     luma 4..16, Cb+Cr pairs 4 and 8 (4 alone under bit 2), not PCM, whose available units are one
               run or none (availability: the oracle's 6.4.1);
      quad     four consecutive fast 4x4 entries at an aligned region's (0, 0), (4, 0), (0, 4), (4, 4), sub-TBs
               1..3 not reference-less, the coded residuals at base + 16 * code, code <= 14 (pool_offsets);
      reach    a job in the CTB's first row reads the top-right CTU when x + 2n (a quad: x + 12) passes the CTB
               and that CTU is usable; a job is in the bottom-left quadrant by its origin."""
    ctb, staged = _staged(params, pic)
    offs, zero = offsets if offsets is not None else (lambda o: (o[0][0], o[1]))(pool_offsets([pic]))
    out = []
    for cnt, tr_ok, base in staged:
        lists = ([], [])
        for b in base:
            t, c, cm = b["t"], b["c"], b["cm"]
            fast_size = (c == 0 and b["lg"] <= 4) or (cm == 3 and b["lg"] <= (2 if quad_bits & 4 else 3))
            e = dict(b, fast=fast_size and not b["pcm"] and b["run"],
                     offs=[int(offs[t])] + ([int(offs[t + 1])] if cm == 3 else [zero] if c else []))
            lists[1 if c else 0].append(e)
        res = dict(records=cnt)
        for name, entries, chroma, bit in (("luma", lists[0], False, 1), ("chroma", lists[1], True, 2)):
            jobs, heads, why = _merge(entries, chroma, bool(quad_bits & bit), zero)
            cs = ctb >> 1 if chroma else ctb
            tr, br = len(jobs), len(jobs)
            last_bl = -1
            for k, (s, quad) in enumerate(jobs):
                e = entries[s]
                reach = e["xr"] + 12 if quad else e["xr"] + (2 << e["lg"])
                if tr == len(jobs) and e["yr"] == 0 and reach > cs and tr_ok:
                    tr = k
                if e["xr"] < cs // 2 and e["yr"] >= cs // 2:
                    last_bl = k
            if last_bl >= 0:
                br = last_bl + 1
            res[name] = len(jobs)
            res[name + "_staged"] = len(entries)
            res[name + "_tr"], res[name + "_br"] = tr, br
            res[name + "_heads"], res[name + "_refused"] = sorted(heads), why
            res[name + "_unpaired"] = sum(1 for e in entries if chroma and e["cm"] != 3)
            res[name + "_entries"], res[name + "_jobs"], res["zero"] = entries, jobs, zero
        out.append(res)
    return out


def structure_key(pic):
    """What the geometry and the model see of a picture: positions, sizes, components and flags of the records in
    their order, the CTUs' slices, tiles and record ranges, the picture size (not modes, qP or coefficients)."""
    return (np.stack([pic.tbs[f].astype(np.int64) for f in ("x", "y", "log2_size", "c_idx", "flags")]).tobytes(),
            np.stack([pic.ctus[f].astype(np.int64) for f in ("slice_addr", "tile_id", "tb_begin", "tb_count")]).tobytes(),
            tuple(pic.size))


_STAGED = {}


def _staged(params, pic):
    """(CTB size, per CTU (record count, top-right CTU usable, entries after pairing)): the part of the model that
    depends on the structure alone, kept per structure_key (the flows of a tiling share it)."""
    pp = R.pic_params(params, pic)
    key = (structure_key(pic), int(pp["ctb_log2_size"]))
    if key in _STAGED:
        return _STAGED[key]
    geo = O.Geometry(R.params_dict(pp), pic.ctus)
    ctb = geo.ctb
    out = []
    for rs, ctu in enumerate(pic.ctus):
        x0, y0 = (rs % geo.wc) * ctb, (rs // geo.wc) * ctb
        b, cnt = int(ctu["tb_begin"]), int(ctu["tb_count"])
        tr_ok = bool(geo.available(x0, y0, x0 + ctb, y0 - 1))    # flags bit 3: same slice and tile, in the picture
        base = []
        for t in range(b, b + cnt):
            rec = pic.tbs[t]
            c = int(rec["c_idx"])
            if t > b and _same_tu(pic.tbs[t - 1], rec):
                continue                                          # the Cr of a pair: taken by its Cb
            pair = t + 1 < b + cnt and _same_tu(rec, pic.tbs[t + 1])
            sub = 1 if c else 0
            av = unit_avail(geo, rec)
            base.append(dict(t=t, c=c, lg=int(rec["log2_size"]), cm=0 if c == 0 else (3 if pair else c),
                             xr=int(rec["x"]) - (x0 >> sub), yr=int(rec["y"]) - (y0 >> sub), none=not any(av),
                             run=_one_run(av), pcm=bool(int(rec["flags"]) & R.TB_PCM)))
        out.append((cnt, tr_ok, base))
    _STAGED[key] = (ctb, out)
    return _STAGED[key]


def job_sums(params, pics, quad_bits):
    """(luma, chroma) job counts of a batch, the sums p265r_batch_job_count reports."""
    offs, zero = pool_offsets(pics)
    lu = ch = 0
    for p, o in zip(pics, offs):
        for r in expected_jobs(params, p, quad_bits, (o, zero)):
            lu, ch = lu + r["luma"], ch + r["chroma"]
    return lu, ch


# ---------------------------------------------------------------------------------
# coverage helpers
# ---------------------------------------------------------------------------------

DIRECTIONS = ("left", "top", "corner", "tr_avail", "tr_later", "bl_avail", "bl_later")


def owner_maps(pic, params):
    """Per component, the index of the TB record that owns each sample (-1: none)."""
    pp = R.pic_params(params, pic)
    w, h = int(pp["pic_width"]), int(pp["pic_height"])
    maps = [np.full((h >> (c > 0), w >> (c > 0)), -1, np.int64) for c in range(3)]
    for t, rec in enumerate(pic.tbs):
        n, x, y = 1 << int(rec["log2_size"]), int(rec["x"]), int(rec["y"])
        maps[int(rec["c_idx"])][y:y + n, x:x + n] = t
    return maps


def decode_rank(pic, params):
    """Rank of every TB record in its component's decode order over the picture (CTUs in tile scan)."""
    geo = O.Geometry(R.params_dict(R.pic_params(params, pic)), pic.ctus)
    rank = np.zeros(len(pic.tbs), np.int64)
    k = [0, 0, 0]
    for rs in geo.ts_order:
        b, n = int(pic.ctus[rs]["tb_begin"]), int(pic.ctus[rs]["tb_count"])
        for t in range(b, b + n):
            c = int(pic.tbs[t]["c_idx"])
            rank[t] = k[c]
            k[c] += 1
    return rank


def direction_cells(pic, params):
    """{(component 0 luma / 1 chroma, target size, neighbour size, direction, neighbour is the job just before
    the target in its component's decode order): [(target record, neighbour record, offset of the unit's first
    sample in its segment)]} of one picture.  A
    neighbour is the TB that owns the first sample of a reference unit of the target: the left, top, top-right
    or bottom-left segment (8.4.4.2.2) or the corner.  left / top / corner / *_avail: the unit is available
    (6.4.1); *_later: it is inside the picture, slice and tile but later in z-order."""
    pp = R.pic_params(params, pic)
    geo = O.Geometry(R.params_dict(pp), pic.ctus)
    maps, rank = owner_maps(pic, params), decode_rank(pic, params)
    out = {}
    for t, rec in enumerate(pic.tbs):
        c = int(rec["c_idx"])
        sub = 1 if c else 0
        n, x0, y0 = 1 << int(rec["log2_size"]), int(rec["x"]), int(rec["y"])
        us = 4 >> sub
        h, w = maps[c].shape
        dx, dy = O.ref_positions(n)
        for k in list(range(0, 2 * n, us)) + [2 * n] + list(range(2 * n + 1, 4 * n + 1, us)):
            xn, yn = x0 + int(dx[k]), y0 + int(dy[k])
            if xn < 0 or yn < 0 or xn >= w or yn >= h:
                continue
            nb = int(maps[c][yn, xn])
            seg = "bl" if k < n else "left" if k < 2 * n else "corner" if k == 2 * n else "top" if k <= 3 * n else "tr"
            av = geo.available(x0 << sub, y0 << sub, xn << sub, yn << sub)
            if seg in ("bl", "tr"):
                a, b = geo.ctb_of(x0 << sub, y0 << sub), geo.ctb_of(xn << sub, yn << sub)
                if not av and (geo.slice_addr[a] != geo.slice_addr[b] or geo.tile[a] != geo.tile[b]):
                    continue
                d = seg + ("_avail" if av else "_later")
            elif av:
                d = seg
            else:
                continue
            key = (min(c, 1), n, 1 << int(pic.tbs[nb]["log2_size"]), d, bool(rank[nb] == rank[t] - 1))
            j = {"bl": n - 1 - k, "left": 2 * n - 1 - k, "corner": 0, "top": k - 2 * n - 1, "tr": k - 3 * n - 1}[seg]
            out.setdefault(key, []).append((t, nb, j))
    return out


def mode_reads(mode, n, direction, j):
    """Does intra mode ``mode`` of an n x n TB read the reference sample at offset ``j`` of a segment (8.4.4.2.4-6;
    left / bottom-left offsets run downwards, top / top-right ones rightwards)?  Conservative: False where it
    depends on more than this."""
    # planar and DC read the whole left column and top row; so do the angular modes 3..17 / 19..33: the block's
    # first column / row reads ref[y + idx + 1] with idx = 0 (positive angles below 32) or -1 (negative ones, with
    # a non-zero fraction), i.e. the sample beside it; modes 2 / 34 (angle 32, idx = 1) start one sample further
    if direction == "left":
        return mode in (0, 1) or 3 <= mode <= 17 or (mode == 2 and j >= 1)
    if direction == "top":
        return mode in (0, 1) or 19 <= mode <= 33 or (mode == 34 and j >= 1)
    if direction == "corner":
        return 11 <= mode <= 25                         # negative angles: ref[0] at the block's first sample
    if direction.startswith("tr"):
        return mode == 34 or (mode == 0 and j == 0)     # 34: ref[x + y + 2] up to 2n; planar: p[n][-1]
    return mode == 2 or (mode == 0 and j == 0)


def is_ragged(pic):
    """Smaller than the 3 x 2 CTB context of its set (``edges`` and the ``col8`` pictures of ``adjacent``): decoded
    in set_params(edges=True)."""
    return tuple(pic.size) != (3 * pic.meta["ctb"], 2 * pic.meta["ctb"])


def direction_cells_wanted(ctb):
    """Every (component, target size n, neighbour size m, direction, adjacency) cell asserted per CTB size.
    Adjacency True: the neighbour N is the job just before the target T in its component's decode order.

    Sizes: luma 4..min(32, CTB); chroma 4..min(16, CTB / 2) (chroma 4 under luma 8 and under a 4x4 region).  S is
    the component's CTB size.  A CTB's TBs are decoded in z-order and CTBs in tile scan, so the job before T is

      (a) inside a CTB: with R the smallest aligned region holding both, N the last TB of a quadrant of R (at its
          bottom right) and T the first TB of the next one (at its top left).  Quadrant 0 -> 1 and 2 -> 3: N lies
          left of T, its rows ending where the quadrant ends; 1 -> 2: N lies above right, its columns ending at R's
          right edge, at x_T + s/2 or beyond (s the size of R; n, m <= s/2);
      (b) across CTBs: N is the last TB of the previous CTB in tile scan, at that CTB's bottom right, and T the
          first TB of its CTB.  The previous CTB is the one to the left, or the last of the tile's row above: the
          one above in a tile one CTB wide, the one above right in a tile two CTBs wide, never the one above left;
      (c) at the picture's right edge, where a region's right half is outside the picture: quadrant 0 -> 2, N above
          T.  With the widths of the set (2 CTB + 8, 24, 40, 56) the present part of such a region is 8 wide (a
          present part of 24, 40 or 56 has a present, narrower quadrant 1), so n, m <= 8 there.  A cut at the
          bottom edge gives 0 -> 1, as (a).

    Not adjacent (False), every (n, m, direction) is wanted but for:

      * bottom-left available at n = S: the samples below left lie in the CTB row below, decoded later;
      * top-right later at n = S or m = S: a whole-CTB target's top-right samples lie in the CTB row above, a
        whole-CTB neighbour above right is the CTB above right; either is earlier in tile scan or in another
        slice or tile, never later;
      * bottom-left available at n = S / 2 with m >= S / 2: in quadrant 1 the samples below left belong to
        quadrant 2 (later), in quadrants 2 and 3 to the CTB row below, so T is quadrant 0 and N lies in the left
        CTB at y0 + S / 2: its quadrant 3 or all of it, which is its last TB - (b).  Wanted adjacent instead;
      * left at n = m = S: the left CTB is the previous one in tile scan whenever it is in T's tile.  Wanted
        adjacent instead.

    Adjacent (True):

      * left: every (n, m) - (a) 0 -> 1 with N the last TB of quadrant 0, (b) for whole CTBs;
      * bottom-left available: every n < S.  (a) 0 -> 1 with s/2 = max(2n, m): N's rows [s/2 - m, s/2) meet T's
        bottom-left rows [n, 2n); that needs n <= S / 4 and m <= S / 2.  (b): N's rows [S - m, S) meet [n, 2n) for
        n = S / 2 with any m, and for m = S with any n < S;
      * corner: none.  N would hold (x_T - 1, y_T - 1): in (a) N lies left of T with rows below y_T, or above
        right; in (b) the previous CTB is never above left, and the last TB of the one to the left or above does
        not reach the corner sample; in (c) N is above T within T's columns;
      * top: (b) with the CTB above, N's columns [S - m, S) meet T's [0, n): n + m > S, so n = S or m = S (CTB <= 32,
        where S is a TB size); (c): luma (4, 8), (8, 4), (8, 8) - an 8x8 TB above or below a 4x4 region's first
        block, or two 8x8 TBs; not (4, 4): the last 4x4 of the region above is at columns 4..7 - and chroma (4, 4).
        (a) never: 1 -> 2 puts N's columns at x_T + s/2 or beyond, T's top row ends before x_T + n <= x_T + s/2;
      * top-right available: (a) 1 -> 2 with m <= n < S (n = s/2: N's columns [s - m, s) lie in T's top-right
        [n, 2n)); m > n never in (a): T's top-right columns end before x_T + 2n <= x_T + s/2 unless n = s/2, and
        then m <= s/2 = n.  (b) with the CTB above right (a tile two CTBs wide): N's columns [2S - m, 2S) meet
        [n, 2n) for n = S only, any m; with the CTB above (a tile one CTB wide): [S - m, S) meets [n, 2n) for
        2n + m > S, n <= S / 2.  (c): luma (4, 8), the 8x8 TB above a 4x4 region's first block.
    """
    want = set()
    for c, s in ((0, ctb), (1, ctb >> 1)):
        sizes = [n for n in (4, 8, 16, 32 >> c) if n <= s]
        for n in sizes:
            for m in sizes:
                for d in DIRECTIONS:
                    if (d == "bl_avail" and n == s) or (d == "tr_later" and s in (n, m)):
                        continue
                    adjacent_only = (d == "bl_avail" and 2 * n == s and 2 * m >= s) or (d == "left" and n == m == s)
                    want.add((c, n, m, d, adjacent_only))
                want.add((c, n, m, "left", True))
                if n < s:
                    want.add((c, n, m, "bl_avail", True))
                if n + m > s or (c == 0 and (n, m) in ((4, 8), (8, 4), (8, 8))) or (c == 1 and n == m == 4):
                    want.add((c, n, m, "top", True))
                if m <= n < s or n == s or (2 * n + m > s and 2 * n <= s) or (c == 0 and (n, m) == (4, 8)):
                    want.add((c, n, m, "tr_avail", True))
    return want
