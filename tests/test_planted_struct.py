"""The planted structure set (tests/planted_struct.py) on the CPU.

  * the host model of job preparation on three hand-worked CTUs, and against an independent restatement of the
    half-CTU publish rule (no job at or after `br` covers the bottom row's left half) on the whole set;
  * coverage, from the records and the model: every (component, target size, neighbour size, direction) meeting,
    the limits validate_picture admits, every ``counts`` cell, every quad pattern and refusal reason, every `tr`
    and `br` cell, the partial widths and heights;
  * the dependence is real: negating the neighbour's coefficients changes the target (C twin);
  * the C twin equals the Python oracle;
  * defects planted into the Python oracle's availability or into the record order are noticed.
"""
import numpy as np
import pytest

import planted_struct as S
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import records as R

DEPTHS = (8, 10, 12)
CTBS = (4, 5, 6)
_REF, _MODEL, _CELLS = {}, {}, {}


def _ref(bd, lg):
    """The C twin's reconstruction of the set, computed once."""
    if (bd, lg) not in _REF:
        pics = S.struct_set(bd, lg)
        ref = c_oracle.decode(S.set_params(bd, lg, edges=True), pics, threads=8)
        for rec, out in ref:                       # no in-loop filter: the output is the reconstruction
            assert all(np.array_equal(rec[c], out[c]) for c in range(3))
        _REF[(bd, lg)] = [r[0] for r in ref]
    return _REF[(bd, lg)]


def _prm(pic, bd=8):
    return S.set_params(bd, pic.meta["ctb"].bit_length() - 1, edges=S.is_ragged(pic))


_structure = S.structure_key


def _distinct(pics):
    """Pictures that differ in structure (modes, coefficients and qP aside): what the model and the geometry see."""
    seen, out = set(), []
    for i, p in enumerate(pics):
        k = _structure(p)
        if k not in seen:
            seen.add(k)
            out.append((i, p))
    return out


def _model(lg, quad):
    if (lg, quad) not in _MODEL:
        _MODEL[(lg, quad)] = [(p, S.expected_jobs(_prm(p), p, quad)) for _, p in _distinct(S.struct_set(8, lg))]
    return _MODEL[(lg, quad)]


def _cells(lg):
    if lg not in _CELLS:
        cells = {}
        for i, p in _distinct(S.struct_set(8, lg)):
            for k, v in S.direction_cells(p, _prm(p)).items():
                cells.setdefault(k, []).extend((i, t, nb, j) for t, nb, j in v[:16])
        _CELLS[lg] = cells
    return _CELLS[lg]


# ---------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------

def _pic(lg, family, cell, order="tu", bd=8):
    return next(p for p in S.struct_set(bd, lg, family) if p.meta["cell"] == cell and p.meta["order"] == order)


def test_model_hand_worked_ctus():
    """CTU 4 (column 1, row 1: every neighbour CTU present) of three CTB 64 pictures, worked by hand.  The z-order
    index of the 8x8 region at (x, y) interleaves the bits of x / 8 and y / 8: (56, 0) -> binary 010101 = 21, the
    16x16 at (48, 0) is the 5th of its size, the bottom-left quadrant holds the 8x8 regions 32..47 and the 16x16
    regions 8..11."""
    get = lambda pic, quad: S.expected_jobs(S.set_params(8, 6), pic, quad)[4]
    # all 8x8: 64 luma jobs; 64 Cb+Cr 4x4 pairs, four per 16x16 merge: 16 chroma quads.  The first luma job whose
    # x + 16 passes 64 is the one at x = 56 (21); a chroma quad reaches x + 12, past 32 from x = 24 (luma 48: 5)
    r = get(_pic(6, "tiling", "8/cycle"), 3)
    assert (r["records"], r["luma_staged"], r["chroma_staged"]) == (192, 64, 64)
    assert (r["luma"], r["chroma"], r["luma_tr"], r["chroma_tr"], r["luma_br"], r["chroma_br"]) == (64, 16, 21, 5, 48, 12)
    r = get(_pic(6, "tiling", "8/cycle"), 1)                   # no chroma quads: the pair at chroma x = 28 (21)
    assert (r["luma"], r["chroma"], r["chroma_tr"], r["chroma_br"]) == (64, 64, 21, 48)
    r = get(_pic(6, "tiling", "8/cycle", "cm"), 3)             # component-major: 128 unpaired chroma jobs, no quads;
    assert (r["luma"], r["chroma"], r["chroma_unpaired"]) == (64, 128, 128)     # Cb job 21 reaches first, the last
    assert (r["chroma_tr"], r["chroma_br"]) == (21, 64 + 48)                    # bottom-left job is Cr's 47th
    # all 4x4 NxN: 384 records, 256 luma entries -> 64 quads; a quad at x = 56 reaches 56 + 12 (x = 48: 60, not)
    p = _pic(6, "tiling", "nxn/cycle")
    r = get(p, 3)
    assert (r["records"], r["luma_staged"], r["chroma_staged"]) == (384, 256, 64)
    assert (r["luma"], r["chroma"], r["luma_tr"], r["chroma_tr"], r["luma_br"], r["chroma_br"]) == (64, 16, 21, 5, 48, 12)
    assert r["luma_heads"] == list(range(0, 256, 4))
    r = get(p, 4)          # no quads: 256 luma jobs; the 4x4 at x = 60 (region 21's sub-TB 1: 85) reaches 68, x = 56: 64
    assert (r["luma"], r["chroma"], r["luma_tr"], r["luma_br"]) == (256, 64, 85, 192)
    # ``counts`` head2: two 8x8 TBs then 62 4x4 regions: 250 entries, heads at 2, 6, ..., so at slot 62 of each window
    r = get(_pic(6, "counts", "head2"), 3)
    assert (r["luma_staged"], r["luma"]) == (250, 64) and r["luma_heads"] == list(range(2, 250, 4))
    assert {62, 126, 190} <= set(r["luma_heads"])
    assert (r["luma_tr"], r["luma_br"]) == (21, 48)


@pytest.mark.parametrize("lg", CTBS)
@pytest.mark.parametrize("quad", (3, 1, 4))
def test_model_br_covers_every_bottom_left_writer(lg, quad):
    """`br` by origin (the model, as intra_prep.h in_bl) against the extents (touches_bl_row): no job at or after
    `br` covers a sample of the bottom row of the CTB's left half; and `tr` <= count."""
    ctb = 1 << lg
    for p, res in _model(lg, quad):
        for r in res:
            for name, cs in (("luma", ctb), ("chroma", ctb >> 1)):
                jobs = r[name + "_jobs"]
                assert len(jobs) == r[name]
                for k, (s, q) in enumerate(jobs):
                    e = r[name + "_entries"][s]
                    ext = 8 if q else 1 << e["lg"]
                    if e["xr"] < cs // 2 and e["yr"] + ext >= cs:
                        assert k < r[name + "_br"], (p.meta, name, k)
                assert 0 <= r[name + "_tr"] <= r[name] and 0 <= r[name + "_br"] <= r[name]


# ---------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------

@pytest.mark.parametrize("lg", CTBS)
def test_direction_cells(lg):
    """Every (component, target size, neighbour size, direction, adjacency) cell of direction_cells_wanted occurs."""
    missing = S.direction_cells_wanted(1 << lg) - set(_cells(lg))
    assert not missing, sorted(missing)


@pytest.mark.parametrize("bd", (10, 12))
@pytest.mark.parametrize("lg", CTBS)
def test_structure_is_the_same_at_every_bit_depth(bd, lg):
    """The 10 / 12-bit sets hold every structure of the 8-bit one (they repeat fewer flows of ``quadrants``), so the
    coverage asserted from the 8-bit records holds per bit depth."""
    assert {_structure(p) for p in S.struct_set(bd, lg)} == {_structure(p) for p in S.struct_set(8, lg)}
    assert all(p.meta["bit_depth"] == bd and int(p.tbs["qp"][p.tbs["c_idx"] == 0].min()) == 30 + 6 * (bd - 8) for p in S.struct_set(bd, lg))


@pytest.mark.parametrize("lg", CTBS)
def test_limits(lg):
    """The all-4x4 pictures reach what validate_picture admits per CTU: 3 (CTB / 4)^2 / 2 records, (CTB / 4)^2 luma
    TBs, 2 (CTB / 8)^2 chroma TBs (unpaired in the component-major twin, half as many pairs in TU order)."""
    ctb = 1 << lg
    top = (3 * (ctb // 4) ** 2 // 2, (ctb // 4) ** 2, 2 * (ctb // 8) ** 2)
    for kind in ("nxn", "s4"):
        for order in ("tu", "cm"):
            p = _pic(lg, "tiling", "%s/cycle" % kind, order)
            for r in S.expected_jobs(S.set_params(8, lg), p, 4):
                assert (r["records"], r["luma_staged"]) == top[:2]
                assert r["chroma_staged"] == (top[2] if order == "cm" else top[2] // 2)
                assert r["chroma_unpaired"] == (top[2] if order == "cm" else 0)
                assert r["luma"] == top[1]
    assert top == {4: (24, 16, 8), 5: (96, 64, 32), 6: (384, 256, 128)}[lg]


def test_counts_cells():
    """Every cell of the ``counts`` family, from the records and the model."""
    staged, heads, merged, unpaired, paired, cb_at, records = set(), set(), set(), set(), set(), set(), set()
    for lg in (5, 6):
        for p in S.struct_set(8, lg, "counts"):
            for r, ctu in zip(S.expected_jobs(S.set_params(8, lg), p, 3), p.ctus):
                staged.add((lg, r["luma_staged"]))
                heads |= {(lg, h) for h in r["luma_heads"]}
                merged.add((lg, r["luma"]))
                unpaired.add((lg, r["chroma_unpaired"]))
                paired.add((lg, r["chroma_staged"] - r["chroma_unpaired"]))
                records.add((lg, r["records"]))
                seg = p.tbs[int(ctu["tb_begin"]):int(ctu["tb_begin"]) + int(ctu["tb_count"])]
                pair = [k for k in range(len(seg) - 1) if S._same_tu(seg[k], seg[k + 1])]
                # in the builder's TU order every CU appends a multiple of three records and its Cb is the second
                # of a (Y, Cb, Cr) triple or the fifth of (Y, Y, Y, Y, Cb, Cr): a Cb record's index is 1 mod 3.  A pair
                # split over a chunk edge has its Cb at 64 m - 1 = 63, 127, 191, 255, 319 = 0, 1, 2, 0, 1 mod 3: only
                # 127 | 128 and 319 | 320 can split (the component-major order has no pairs)
                assert all(k % 3 == 1 for k in pair)
                cb_at |= {(lg, k) for k in pair if k % 64 == 63}
    assert {(6, n) for n in (61, 64, 67, 127, 130, 190, 193, 256)} | {(5, 61), (5, 64)} <= staged
    assert {(6, w + s) for w in (0, 64, 128) for s in (60, 61, 62, 63, 64)} | {(5, 60)} <= heads
    assert {(6, 127), (6, 319)} == cb_at
    for edge in (64, 128, 192, 256, 320):                     # the record count crosses each chunk edge
        assert any(lg == 6 and n <= edge for lg, n in records) and any(lg == 6 and n > edge for lg, n in records)
    assert any(lg == 5 and n <= 64 for lg, n in records) and any(lg == 5 and n > 64 for lg, n in records)
    assert (6, 64) in paired and {(6, 62), (6, 68), (6, 128)} <= unpaired
    assert {(6, 64), (6, 67), (6, 127), (6, 130)} <= merged
    noquad = {r["luma"] for p in S.struct_set(8, 6, "counts") for r in S.expected_jobs(S.set_params(8, 6), p, 4)}
    assert 256 in noquad


@pytest.mark.parametrize("lg", CTBS)
def test_quad_cells(lg):
    """Every coded pattern of a luma quad and the planted ones of a chroma quad merge; every refusal reason occurs."""
    luma_pat, chroma_pat, why_l, why_c, noref = set(), set(), set(), set(), 0
    for p, res in _model(lg, 3):
        for r in res:
            zero = r["zero"]
            for h in r["luma_heads"]:
                e = r["luma_entries"][h:h + 4]
                luma_pat.add(tuple(int(q["offs"][0] != zero) for q in e))
                noref += e[0]["none"]
            for h in r["chroma_heads"]:
                e = r["chroma_entries"][h:h + 4]
                chroma_pat.add(sum(int(o != zero) << i for i, o in enumerate(o for q in e for o in q["offs"])))
            why_l |= set(r["luma_refused"].values())
            why_c |= set(r["chroma_refused"].values())
    assert luma_pat == {tuple((m >> i) & 1 for i in range(4)) for m in range(16)}
    assert set(S.CHROMA_QUAD_PATTERNS) <= chroma_pat and len(S.CHROMA_QUAD_PATTERNS) == 26
    assert noref >= 2                                          # picture origin and the first CTU of a slice
    # a transform-skip sub-TB (another slab: codes), a sub-TB off the fast path, sub-TBs 1, 2, 3 + 0 of the next
    # region.  "none123" (a reference-less sub-TB 1..3) cannot occur: sub-TB 0 is always available to them
    # "position" and "short" (the three entries after a region's first block are not its other blocks, or are not
    # there) cannot occur in the luma list: both record orders keep a region's four luma TBs together
    assert why_l == {"codes", "notfast", "unaligned"}
    # chroma: a bypass CU among the four (codes), a pair off the fast path, pairs 1, 2, 3 of an unmerged region and 0 of
    # the next, a region cut by the picture's right edge whose two pairs end the list (short) or are followed by the
    # next region's (position).  At CTB 16 a CTU holds one chroma region, at most four pairs: nothing follows it, so
    # neither "unaligned" nor "position" can occur there
    assert why_c == {"codes", "notfast", "short"} | ({"position", "unaligned"} if lg > 4 else set())
    off = {v for p, res in _model(lg, 4) for r in res for v in r["luma_refused"].values()}
    assert off == {"off"}


@pytest.mark.parametrize("lg", CTBS)
def test_tr_cells(lg):
    """`tr`: first / middle / last job and none; per size and offset reaching and exactly not reaching; a quad at
    CTB - 8 (reach x + 12) and at CTB - 16; every top-right CTU variant."""
    ctb = 1 << lg
    where, reach, variants = {"luma": set(), "chroma": set()}, set(), {}
    for quad, (p, res) in [(q, pr) for q in (3, 4) for pr in _model(lg, q)]:     # (4: the 4x4 jobs unmerged)
        geo = O.Geometry(R.params_dict(R.pic_params(_prm(p), p)), p.ctus)
        for rs, r in enumerate(res):
            x0, y0 = (rs % geo.wc) * ctb, (rs // geo.wc) * ctb
            usable = bool(geo.available(x0, y0, x0 + ctb, y0 - 1))
            for name, cs, bit in (("luma", ctb, 1), ("chroma", ctb >> 1, 2)):
                tr, n = r[name + "_tr"], r[name]
                where[name].add("none" if tr == n else "first" if tr == 0 else "last" if tr == n - 1 else "middle")
                if tr == 0 and n == 1:
                    where[name].add("last")
                if not usable:
                    assert tr == n
                    continue
                jobs = r[name + "_jobs"]
                for k, (s, q) in enumerate(jobs):
                    e = r[name + "_entries"][s]
                    if e["yr"] == 0:
                        end = e["xr"] + (12 if q else 2 << e["lg"])
                        if end >= cs:
                            reach.add((name, "quad" if q else 1 << e["lg"], e["xr"], end > cs))
                            assert (k >= tr) if end > cs else True
    for p in S.struct_set(8, lg, "topright"):
        if "target" in p.meta:
            rs = p.meta["target"]
            geo = O.Geometry(R.params_dict(_prm(p)), p.ctus)
            r = S.expected_jobs(_prm(p), p, 3)[rs]
            variants[p.meta["variant"]] = (bool(geo.available((rs % 3) * ctb, (rs // 3) * ctb, (rs % 3 + 1) * ctb, (rs // 3) * ctb - 1)),
                                           r["luma_tr"] < r["luma"], r["chroma_tr"] < r["chroma"])
    for name, cs in (("luma", ctb), ("chroma", ctb >> 1)):
        # `tr` = 0 needs a job at x = 0 that reads past the CTB: 2n > S, a whole-CTB TB; luma TBs end at 32
        want = {"none", "middle", "last"} | ({"first"} if cs <= (32 if name == "luma" else 16) else set())
        assert want <= where[name], (name, where[name])
        for n in (4, 8, 16, 32):
            if n <= min(cs, 32 if name == "luma" else 16):
                assert (name, n, cs - n, True) in reach, (name, n)
                if 2 * n <= cs:
                    assert (name, n, cs - 2 * n, False) in reach, (name, n)
        assert (name, "quad", cs - 8, True) in reach
        if cs >= 16:
            assert all(not past for nm, n, x, past in reach if nm == name and n == "quad" and x == cs - 16)
    assert variants == {"same": (True, True, True), "slice": (False,) * 3, "tile": (False,) * 3, "absent": (False,) * 3,
                        "first_row": (False,) * 3}


def test_br_cells():
    """CTB 64: every tiling of the top-right CTU's bottom-left quadrant in both record orders, with the last
    bottom-left job what the tiling says (a quad for ``nxn`` and ``mix``)."""
    seen, flows = {}, set()
    for p in S.struct_set(8, 6, "topright"):
        if "bl" in p.meta:
            r = S.expected_jobs(S.set_params(8, 6), p, 3)[2]
            s, quad = r["luma_jobs"][r["luma_br"] - 1]
            seen[(p.meta["bl"], p.meta["order"])] = (1 << r["luma_entries"][s]["lg"], quad)
            flows.add(p.meta["flow"])
            assert r["luma_br"] < r["luma"] and r["chroma_br"] < r["chroma"]
            if p.meta["order"] == "cm":                       # every Cb job precedes the Cr jobs: `br` is in Cr's part
                assert r["chroma_br"] > r["chroma"] // 2
    want = {"32": (32, False), "16": (16, False), "8": (8, False), "nxn": (4, True), "mix": (4, True)}
    assert seen == {(k, o): v for k, v in want.items() for o in ("tu", "cm")} and flows == {34, 17}


@pytest.mark.parametrize("lg", CTBS)
def test_partial_widths_and_heights(lg):
    ctb = 1 << lg
    offs = [o for o in (8, 24, 40, 56) if o < ctb]
    sizes = {tuple(p.size) for p in S.struct_set(8, lg, "edges")}
    assert {(2 * ctb + o, 2 * ctb) for o in offs} | {(2 * ctb, 2 * ctb + o) for o in offs} <= sizes
    assert {p.meta["flow"] for p in S.struct_set(8, lg, "edges")} == {34, 2}
    assert all(S.is_ragged(p) for p in S.struct_set(8, lg, "edges"))


# ---------------------------------------------------------------------------------
# the dependence is real
# ---------------------------------------------------------------------------------

def _negated(pic, t):
    rec = pic.tbs[t]
    off, nn = int(rec["coef_off"]), 1 << (2 * int(rec["log2_size"]))
    coef = pic.coef.copy()
    coef[off:off + nn] = -coef[off:off + nn]
    return R.Picture(ctus=pic.ctus, tbs=pic.tbs, coef=coef, nofilter=pic.nofilter, meta=pic.meta, size=pic.size)


def _region(planes, rec):
    n, x, y = 1 << int(rec["log2_size"]), int(rec["x"]), int(rec["y"])
    return planes[int(rec["c_idx"])][y:y + n, x:x + n]


@pytest.mark.parametrize("lg", CTBS)
def test_direction_cells_depend_on_the_neighbour(lg):
    """For every available-direction cell: negate the neighbour TB's coefficients, decode again with the C twin;
    a sample of the target TB changes.  A cell's examples are tried in a fixed order, those whose target mode
    reads the unit by rule (mode_reads) first, over the pictures of the same structure under every flow; the
    cell holds when one of its first 12 examples shows the dependence."""
    pics, ref = S.struct_set(8, lg), _ref(8, lg)
    same = {}
    for i, p in enumerate(pics):
        same.setdefault(_structure(p), []).append(i)
    todo = []
    for key in sorted(S.direction_cells_wanted(1 << lg)):
        d = key[3]
        if d.endswith("later"):
            continue                                 # an unavailable neighbour is not read
        cand = []
        for i0, t, nb, j in _cells(lg)[key]:
            for i in same[_structure(pics[i0])]:
                p = pics[i]
                if int(p.tbs[nb]["flags"]) & R.TB_CBF and not int(p.tbs[nb]["flags"]) & R.TB_BYPASS:
                    rule = S.mode_reads(int(p.tbs[t]["pred_mode"]), 1 << int(p.tbs[t]["log2_size"]), d, j)
                    cand.append((not rule, len(cand), key, i, t, nb))
        assert cand, key
        todo += sorted(cand)[:12]
    out = c_oracle.decode(S.set_params(8, lg, edges=True), [_negated(pics[i], nb) for *_, i, t, nb in todo], threads=8)
    shown = set()
    for (_, _, key, i, t, nb), (rec, _) in zip(todo, out):
        if not np.array_equal(_region(rec, pics[i].tbs[t]), _region(ref[i], pics[i].tbs[t])):
            shown.add(key)
    missing = {k for _, _, k, *_ in todo} - shown
    assert not missing, sorted(missing)


def _topright_targets(pic, params):
    """[(target record, record owning its first top-right sample)] of a ``topright`` picture: per component the
    job the model names as `tr` of the target CTU."""
    r = S.expected_jobs(params, pic, 4)[pic.meta.get("target", 4)]
    maps = S.owner_maps(pic, params)
    out = []
    for name in ("luma", "chroma"):
        if r[name + "_tr"] < r[name]:
            t = r[name + "_entries"][r[name + "_tr"]]["t"]
            rec = pic.tbs[t]
            out.append((t, int(maps[int(rec["c_idx"])][int(rec["y"]) - 1, int(rec["x"]) + (1 << int(rec["log2_size"]))])))
    return out


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("lg", CTBS)
def test_topright_pictures_depend_on_the_top_right_ctu(bd, lg):
    """Every ``topright`` picture of flow 34 whose target reads the top-right CTU: negating the TB that owns the
    top-right samples changes the target."""
    params = S.set_params(bd, lg)
    pics, ref = S.struct_set(bd, lg), _ref(bd, lg)
    # (luma mode 34 under flow 34; chroma mode (17 + 17) % 35 = 34 under flow 17)
    todo = [(i, t, nb) for i, p in enumerate(pics) if p.meta["family"] == "topright" and p.meta["flow"] in (34, 17)
            for t, nb in _topright_targets(p, params) if (p.meta["flow"] == 34) == (int(p.tbs[t]["c_idx"]) == 0)]
    assert len({i for i, _, _ in todo}) >= sum(p.meta["family"] == "topright" and p.meta["variant"] == "same" and
                                               p.meta["flow"] in (34, 17) for p in pics)
    out = c_oracle.decode(params, [_negated(pics[i], nb) for i, _, nb in todo], threads=8)
    for (i, t, nb), (rec, _) in zip(todo, out):
        assert not np.array_equal(_region(rec, pics[i].tbs[t]), _region(ref[i], pics[i].tbs[t])), pics[i].meta


# ---------------------------------------------------------------------------------
# the oracles agree
# ---------------------------------------------------------------------------------

def _python_planes(bd, pic):
    pd = R.params_dict(R.pic_params(_prm(pic, bd), pic))
    return O.reconstruct_picture(pd, pic.as_oracle_dict())


def _compare_oracles(bd, lg, idx):
    pics, ref = S.struct_set(bd, lg), _ref(bd, lg)
    for i in idx:
        got = _python_planes(bd, pics[i])
        for c in range(3):
            np.testing.assert_array_equal(got[c], ref[i][c], err_msg="c%d %r" % (c, pics[i].meta))


@pytest.mark.parametrize("family", sorted(S.FAMILIES))
@pytest.mark.parametrize("lg", CTBS)
def test_c_twin_equals_python_oracle_8_bits(lg, family):
    """The whole 8-bit set, one test per family (half a second per CTB 64 picture in Python)."""
    _compare_oracles(8, lg, [i for i, p in enumerate(S.struct_set(8, lg)) if p.meta["family"] == family])


@pytest.mark.parametrize("bd", (10, 12))
@pytest.mark.parametrize("lg", CTBS)
def test_c_twin_equals_python_oracle_10_12_bits(bd, lg):
    """The ``tiling`` limits and ``topright``."""
    _compare_oracles(bd, lg, [i for i, p in enumerate(S.struct_set(bd, lg)) if p.meta["family"] == "topright" or (
        p.meta["family"] == "tiling" and p.meta["kind"] in ("nxn", "s4") and p.meta["flow"] == "cycle")])


# ---------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------

def _noticed_by_oracle(lg, families):
    """Does the (patched) Python oracle differ from the C twin's planes on a picture of the set?"""
    pics, ref = S.struct_set(8, lg), _ref(8, lg)
    for i, p in enumerate(pics):
        if p.meta["family"] in families and p.meta["flow"] in (34, 2, "cycle"):
            got = _python_planes(8, p)
            if any(not np.array_equal(got[c], ref[i][c]) for c in range(3)):
                return p.meta
    return None


def _patched_available(rule):
    real = O.Geometry.available

    def available(self, xc, yc, xn, yn):
        v = rule(self, xc, yc, xn, yn)
        return real(self, xc, yc, xn, yn) if v is None else v
    return available


def _same_ctb(g, xc, yc, xn, yn):
    return 0 <= xn < g.w and 0 <= yn < g.h and g.ctb_of(xc, yc) == g.ctb_of(xn, yn)


AVAILABILITY_DEFECTS = {
    # top-right by raster order of the 4x4 units inside the CTB instead of z-scan: a block above is always earlier
    "tr_raster": lambda g, xc, yc, xn, yn: True if (yn < yc and xn > xc and _same_ctb(g, xc, yc, xn, yn)) else None,
    # top-right cut at the own CTU
    "tr_cut": lambda g, xc, yc, xn, yn: False if (yn < yc and (xn >> g.ctb_log2) > (xc >> g.ctb_log2)) else None,
    # bottom-left ignoring z-order
    "bl_any": lambda g, xc, yc, xn, yn: True if (xn < xc and yn > yc and _same_ctb(g, xc, yc, xn, yn)) else None,
}


def test_comparison_notices_chroma_pair_with_sub_tb_0_rules(monkeypatch):
    """The shared Cb / Cr 4x4 pair of a 4x4 region judged by the position rules of the region's sub-TB 0: its
    reference samples looked up at the luma distances of a 4x4 luma block at the region's origin (x + 4 .. x + 7 for
    the top-right ones, inside the region itself and later in z-order) instead of the chroma block's own (x + 8 ..
    x + 15).  The all-4x4 tilings, NxN and split, notice it."""
    real_tb, real_av = O._recon_tb, O.Geometry.available
    state = {}

    def recon_tb(geo, planes, t, *a, **kw):
        state["on"] = int(t["c_idx"]) > 0 and int(t["log2_size"]) == 2
        return real_tb(geo, planes, t, *a, **kw)

    def available(self, xc, yc, xn, yn):
        if state.get("on") and 0 <= xn < self.w and 0 <= yn < self.h:      # (outside the picture stays outside)
            xn, yn = xc + (xn - xc) // 2, yc + (yn - yc) // 2
        return real_av(self, xc, yc, xn, yn)
    monkeypatch.setattr(O, "_recon_tb", recon_tb)
    monkeypatch.setattr(O.Geometry, "available", available)
    pics, ref = S.struct_set(8, 4), _ref(8, 4)
    for kind in ("nxn", "s4"):
        noticed = False
        for i, p in enumerate(pics):
            if p.meta["family"] == "tiling" and p.meta["kind"] == kind and not noticed:
                got = _python_planes(8, p)
                assert np.array_equal(got[0], ref[i][0])          # (luma is untouched)
                noticed = any(not np.array_equal(got[c], ref[i][c]) for c in (1, 2))
        assert noticed, kind


@pytest.mark.parametrize("name", sorted(AVAILABILITY_DEFECTS))
def test_comparison_notices_availability_defects(monkeypatch, name):
    assert _noticed_by_oracle(4, ("tiling", "quadrants", "topright")) is None
    monkeypatch.setattr(O.Geometry, "available", _patched_available(AVAILABILITY_DEFECTS[name]))
    assert _noticed_by_oracle(4, ("tiling", "quadrants", "topright")) is not None


def _reordered(pic, order_of):
    """The picture with every CTU's records permuted by ``order_of(records of the CTU) -> indices``."""
    tbs = pic.tbs.copy()
    for ctu in pic.ctus:
        b, n = int(ctu["tb_begin"]), int(ctu["tb_count"])
        tbs[b:b + n] = pic.tbs[b:b + n][order_of(pic.tbs[b:b + n])]
    return R.Picture(ctus=pic.ctus, tbs=tbs, coef=pic.coef, nofilter=pic.nofilter, meta=pic.meta, size=pic.size)


def _raster(seg):
    return np.lexsort((seg["x"], seg["y"]))


def _swap_12(seg):
    """Sub-TBs 1 and 2 of every 4x4 luma region swapped."""
    idx = np.arange(len(seg))
    for k in range(len(seg) - 3):
        q = seg[k:k + 4]
        if (q["c_idx"] == 0).all() and (q["log2_size"] == 2).all() and q["x"][0] % 8 == 0 and q["y"][0] % 8 == 0 \
                and q["x"][1] == q["x"][0] + 4 and q["y"][2] == q["y"][0] + 4:
            idx[k + 1], idx[k + 2] = k + 2, k + 1
    return idx


@pytest.mark.parametrize("lg", CTBS)
@pytest.mark.parametrize("order_of", (_raster, _swap_12), ids=("raster", "swap12"))
def test_comparison_notices_record_order_defects(lg, order_of):
    """A CTU's TBs decoded in raster order of position, or sub-TBs 1 and 2 of a 4x4 region swapped: the C twin's
    planes differ on the ``tiling`` pictures."""
    pics = [(i, p) for i, p in enumerate(S.struct_set(8, lg)) if p.meta["family"] == "tiling" and p.meta["flow"] == "cycle"]
    out = c_oracle.decode(S.set_params(8, lg), [_reordered(p, order_of) for _, p in pics], threads=8)
    ref = _ref(8, lg)
    differs = [p.meta["cell"] for (i, p), (rec, _) in zip(pics, out)
               if any(not np.array_equal(rec[c], ref[i][c]) for c in range(3))]
    assert any(c.startswith("nxn") for c in differs), differs
    if order_of is _raster and lg > 4:                  # (two by two 8x8 TBs: raster order is z-order)
        assert any(c.startswith("8/") for c in differs), differs


def test_comparison_notices_an_early_half_ctu_publish():
    """The top-right CTU's bottom row read before its bottom-left quadrant's last job is applied: the target CTU (4)
    is decoded with the left half of CTU 2's bottom row as it was just before the last bottom-left job of each
    list ran.  It differs from the C twin's for every bottom-left tiling, in both record orders."""
    params = S.set_params(8, 6)
    pd = R.params_dict(params)
    pics, ref = S.struct_set(8, 6), _ref(8, 6)
    n = 0
    for i, p in enumerate(pics):
        if p.meta["family"] != "topright" or "bl" not in p.meta:
            continue
        r = S.expected_jobs(params, p, 3)[2]
        first_late = {}
        for c, name in ((0, "luma"), (1, "chroma")):
            s, _ = r[name + "_jobs"][r[name + "_br"] - 1]
            e = r[name + "_entries"][s]                    # (component-major: the last bottom-left job is a Cr one)
            first_late[e["t"]] = [0] if c == 0 else [1, 2] if e["cm"] == 3 else [e["cm"]]
        geo = O.Geometry(pd, p.ctus)
        planes = [np.zeros(s, np.int64) for s in O._plane_shapes(pd)]
        span = lambda rs: range(int(p.ctus[rs]["tb_begin"]), int(p.ctus[rs]["tb_begin"]) + int(p.ctus[rs]["tb_count"]))
        row = lambda c: (planes[c][63 >> (c > 0)], slice(128 >> (c > 0), 160 >> (c > 0)))   # CTU 2's bottom row, left half
        stale = {}
        for rs in (0, 1, 2, 3, 4):
            if rs == 4:
                for c in stale:
                    row(c)[0][row(c)[1]] = stale[c]
            for t in span(rs):
                if rs == 2 and t in first_late:
                    for c in first_late[t]:
                        stale[c] = row(c)[0][row(c)[1]].copy()
                O._recon_tb(geo, planes, p.tbs[t], p.coef, [8, 8, 8], True)
        # (flow 34: the luma TBs predict with mode 34; flow 17: the chroma TBs)
        differs = [not np.array_equal(planes[k][64 >> (k > 0):128 >> (k > 0), 64 >> (k > 0):128 >> (k > 0)],
                                      ref[i][k][64 >> (k > 0):128 >> (k > 0), 64 >> (k > 0):128 >> (k > 0)]) for k in range(3)]
        assert differs[0] if p.meta["flow"] == 34 else (differs[1] or differs[2]), p.meta
        assert all(np.array_equal(planes[k][:, :64 >> (k > 0)], ref[i][k][:, :64 >> (k > 0)]) for k in range(3))  # CTUs 0, 3
        n += 1
    assert n == 20
