"""The planted SAO set (tests/planted_sao.py) on the CPU.

  * scalar_sao below restates 8.7.3.1 / 8.7.3.2 one sample at a time in plain Python integers, sharing nothing
    with the vectorised oracle; it equals the Python oracle on the ``edge``, ``band``, ``mix``, ``wide`` and
    ``nofilter`` pictures of every context, on the ``borders`` pictures at 8 bits (every CTB size) and at 10 and
    12 bits (one CTB size each), and on one ``strips`` picture per strip kernel;
  * the C twin equals the Python oracle on every picture of every set, and its reconstruction is the planted
    planes; with deblocking on at QpY 0 nothing changes (sao_set asserts it with the C twin, the Python oracle
    is asked here);
  * coverage, from a recorder inside scalar_sao and from the outputs: see the test docstrings;
  * sensitivity: the Python oracle with one defect planted no longer equals the C twin on the set.
"""
import inspect

import numpy as np
import pytest

import planted_sao as S
from oracle import recon_oracle as O
from p265_amd import frontend
from p265_amd import records as R

CONTEXTS = [(bd, lg) for bd in S.DEPTHS for lg in S.CTB_LOG2]
H_POS = ((-1, 1), (0, 0), (-1, 1), (1, -1))          # Table 8-12: hPos[k], vPos[k] of SaoEoClass 0..3
V_POS = ((0, 0), (-1, 1), (-1, 1), (-1, 1))


class Recorder:
    def __init__(self):
        self.pairs, self.rows, self.eidx, self.clips, self.bands = set(), set(), set(), set(), set()


def scalar_sao(params, pic, planes, rec=None):
    """8.7.3 sample by sample -> [Y, Cb, Cr] as lists of rows."""
    w, h, log2 = int(params["pic_width"]), int(params["pic_height"]), int(params["ctb_log2_size"])
    wc = (w + (1 << log2) - 1) >> log2
    across_tiles = int(params["loop_filter_across_tiles"]) != 0
    ctus = pic.ctus
    n_ctb = len(ctus)
    tile = [int(v) for v in ctus["tile_id"]]
    slice_addr = [int(v) for v in ctus["slice_addr"]]
    across_slices = [(int(v) & R.CTU_LF_ACROSS_SLICES) != 0 for v in ctus["flags"]]
    rs_to_ts = [0] * n_ctb                                    # 6.5.1: tiles in raster order, CTBs in raster order inside
    for ts, rs in enumerate(sorted(range(n_ctb), key=lambda a: (tile[a], a))):
        rs_to_ts[rs] = ts
    sao_type = ctus["sao_type"].tolist()
    sao_class = ctus["sao_class"].tolist()
    sao_off = ctus["sao_offset"].tolist()
    nf = None if pic.nofilter is None else pic.nofilter.tolist()
    nf_w = (w + 7) >> 3
    result = []
    for c_idx in range(3):
        sub = 1 if c_idx else 0
        bit_depth = int(params["bit_depth_chroma" if c_idx else "bit_depth_luma"])
        max_v, band_shift = (1 << bit_depth) - 1, bit_depth - 5
        src = np.asarray(planes[c_idx]).tolist()
        dst = [row[:] for row in src]
        pw, ph = w >> sub, h >> sub
        ctb_mask = (1 << (log2 - sub)) - 1
        for y in range(ph):
            row, yl = src[y], y << sub
            for x in range(pw):
                xl = x << sub
                rs = (yl >> log2) * wc + (xl >> log2)
                typ = sao_type[rs][c_idx]
                if typ == 0:
                    continue
                if nf is not None and nf[(yl >> 3) * nf_w + (xl >> 3)]:
                    continue                                  # pcm_loop_filter_disabled / cu_transquant_bypass
                v = row[x]
                offsets = sao_off[rs][c_idx]
                if typ == 2:
                    cls = sao_class[rs][c_idx]
                    edge_idx, signs = 2, []
                    for k in (0, 1):
                        xs, ys = x + H_POS[cls][k], y + V_POS[cls][k]
                        if xs < 0 or ys < 0 or xs >= pw or ys >= ph:
                            edge_idx = -1
                            break
                        rn = ((ys << sub) >> log2) * wc + ((xs << sub) >> log2)
                        if rn != rs:
                            if slice_addr[rn] != slice_addr[rs]:
                                if rs_to_ts[rn] < rs_to_ts[rs]:
                                    if not across_slices[rs]:
                                        edge_idx = -1
                                elif not across_slices[rn]:
                                    edge_idx = -1
                            if tile[rn] != tile[rs] and not across_tiles:
                                edge_idx = -1
                            if edge_idx < 0:
                                break
                        n = src[ys][xs]
                        signs.append(1 if v > n else -1 if v < n else 0)
                    if edge_idx < 0:
                        continue                              # edgeIdx = 0
                    edge_idx = 2 + signs[0] + signs[1]
                    if edge_idx in (0, 1, 2):
                        edge_idx = 0 if edge_idx == 2 else edge_idx + 1
                    off = offsets[edge_idx - 1] if edge_idx else 0
                    if rec is not None:
                        yc = (y & ctb_mask)
                        kind = "first" if yc == 0 else "last" if yc == ctb_mask else "inner"
                        rec.pairs.add((c_idx, cls, signs[0], signs[1], x & 15))
                        rec.rows.add((c_idx, cls, signs[0], signs[1], kind))
                        rec.eidx.add((c_idx, edge_idx))
                else:
                    band_table = [0] * 32
                    for k in range(4):
                        band_table[(k + sao_class[rs][c_idx]) & 31] = k + 1
                    band_idx = band_table[v >> band_shift]
                    off = offsets[band_idx - 1] if band_idx else 0
                    if rec is not None:
                        rec.bands.add((c_idx, sao_class[rs][c_idx], v >> band_shift))
                s = v + off
                if rec is not None and off:
                    tag = "clip0" if s < 0 else "clipmax" if s > max_v else "exact0" if s == 0 else "exactmax" if s == max_v else None
                    if tag:
                        rec.clips.add((c_idx, typ, tag))
                dst[y][x] = 0 if s < 0 else max_v if s > max_v else s
        result.append(dst)
    return result


_REF = {}


def _ref(bd, lg, lf):
    key = (bd, lg, lf)
    if key not in _REF:
        _REF[key] = S.c_decode(bd, lg, lf, S.sao_set(bd, lg, lf))
    return _REF[key]


def _check_scalar(bd, lg, lf, pic, rec=None):
    prm = S.params_of(bd, lg, lf, *pic.size)
    got, want = scalar_sao(prm, pic, pic.planes, rec), S.py_sao(bd, lg, lf, pic)
    for c in range(3):
        np.testing.assert_array_equal(np.array(got[c]), want[c], err_msg="scalar c%d %r" % (c, pic.meta))


# ---------------------------------------------------------------------------------
# the scalar restatement against the oracle, and what its recorder saw
# ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,lg", CONTEXTS)
def test_scalar_equals_oracle_and_cells(bd, lg):
    """Per bit depth, CTB size and component, on the edge / band / mix / wide / nofilter pictures: every one of the
    36 (class, sign pair) occurs at every x residue modulo 16 and on the first, an inner and the last row of a
    CTB; edgeIdx 0..4 occur; edge offset and band offset clip at 0 and at max and land on 0 and on max exactly;
    every band position meets samples of all 32 bands.  No cell is narrowed: at CTB 16 a chroma CTB is 8
    samples wide, but its neighbours along the row carry the other classes in turn (they rotate over the four
    ``edge`` pictures), so every class still meets all sixteen residues of the plane's x."""
    rec = Recorder()
    pics = [p for p in S.sao_set(bd, lg, 1) if p.meta["kind"] in ("edge", "band", "mix", "wide", "nofilter")]
    assert len(pics) == S.N_EDGE + S.n_band_pictures(lg) + 1 + S.N_WIDE + S.N_NOFILTER
    for pic in pics:
        _check_scalar(bd, lg, 1, pic, rec)
    pairs = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    for c in range(3):
        miss = [(k, p, r) for k in range(4) for p in pairs for r in range(16) if (c, k) + p + (r,) not in rec.pairs]
        assert not miss, "c%d (class, pair, residue): %s" % (c, miss[:12])
        miss = [(k, p, r) for k in range(4) for p in pairs for r in ("first", "inner", "last") if (c, k) + p + (r,) not in rec.rows]
        assert not miss, "c%d (class, pair, row): %s" % (c, miss[:12])
        assert {e for cc, e in rec.eidx if cc == c} == {0, 1, 2, 3, 4}
        miss = [(t, g) for t in (1, 2) for g in ("clip0", "clipmax", "exact0", "exactmax") if (c, t, g) not in rec.clips]
        assert not miss, "c%d clips: %s" % (c, miss)
        miss = [(p, b) for p in range(32) for b in range(32) if (c, p, b) not in rec.bands]
        assert not miss, "c%d (band position, band): %s" % (c, miss[:12])


SCALAR_BORDERS = [(8, 4), (8, 5), (8, 6), (10, 5), (12, 4)]


@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("bd,lg", SCALAR_BORDERS)
def test_scalar_equals_oracle_borders(bd, lg, lf):
    for pic in S.sao_set(bd, lg, lf):
        if pic.meta["kind"] == "borders":
            _check_scalar(bd, lg, lf, pic)


@pytest.mark.parametrize("bd,lg", [(8, 4), (8, 5), (10, 4)])
def test_scalar_equals_oracle_strips(bd, lg):
    """One ``strips`` picture per strip kernel: 520 x 40 (sao_rows_kernel), 2008 x 72 (sao_strip16_kernel),
    1000 x 40 (sao16_strip_kernel)."""
    pic = [p for p in S.sao_set(bd, lg, 0) if p.meta["kind"] == "strips"][0]
    assert tuple(pic.size) == S.strip_size(bd, lg)[:2]
    _check_scalar(bd, lg, 0, pic)


# ---------------------------------------------------------------------------------
# C twin == Python oracle on every picture; coverage read from the outputs
# ---------------------------------------------------------------------------------

def _rule(pic, wc, hc, rs, d, lf):
    """(allowed, labels) of CTB rs using its neighbour CTB in direction d (for the bookkeeping only: the samples
    come from the oracles)."""
    nx, ny = rs % wc + d[0], rs // wc + d[1]
    if nx < 0 or ny < 0 or nx >= wc or ny >= hc:
        return False, ["outside"]
    o, ctus = ny * wc + nx, pic.ctus
    if ctus["slice_addr"][o] == ctus["slice_addr"][rs]:
        return True, ["same"]
    to, tm = int(ctus["tile_id"][o]), int(ctus["tile_id"][rs])
    labels = []
    if to != tm:
        if not lf:
            return False, ["tile_lf0"]
        labels.append("tile_lf1")
        if (to > tm) != (o > rs):
            labels.append("order_disagree")
    earlier = (to, o) < (tm, rs)
    flag = int(ctus["flags"][rs if earlier else o]) & R.CTU_LF_ACROSS_SLICES != 0
    if flag == (int(ctus["flags"][o if earlier else rs]) & R.CTU_LF_ACROSS_SLICES != 0):
        return flag, labels                          # a slice cell counts where reading the other slice's flag flips it
    return flag, labels + ["%s_f%d" % ("earlier" if earlier else "later", flag)]


def _probes(cls, cs):
    """[(x, y, direction)] inside a CTB of class cls: samples with one neighbour in the CTB at ``direction`` and
    the other inside their own CTB."""
    m, e = cs // 2, cs - 1
    return {0: [(0, m, (-1, 0)), (e, m, (1, 0))],
            1: [(m, 0, (0, -1)), (m, e, (0, 1))],
            2: [(0, 0, (-1, -1)), (m, 0, (0, -1)), (0, m, (-1, 0)), (e, e, (1, 1)), (m, e, (0, 1)), (e, m, (1, 0))],
            3: [(e, 0, (1, -1)), (m, 0, (0, -1)), (e, m, (1, 0)), (0, e, (-1, 1)), (m, e, (0, 1)), (0, m, (-1, 0))]}[cls]


def _border_cells(pic, out, lg, lf, seen):
    """On a ``borders`` picture every sample changes iff it is filtered: each probe's sample changed iff the rule
    allows its CTB the neighbour; the (component, direction, case) cells that occurred go into ``seen``."""
    for rs in range(9):
        for c in range(3):
            cs = (1 << lg) >> (c > 0)
            x0, y0 = (rs % 3) * cs, (rs // 3) * cs
            for x, y, d in _probes(int(pic.ctus["sao_class"][rs][c]), cs):
                ok, labels = _rule(pic, 3, 3, rs, d, lf)
                assert (out[c][y0 + y, x0 + x] != pic.planes[c][y0 + y, x0 + x]) == ok, (pic.meta, rs, c, d, labels)
                seen |= {(c, d, lab) for lab in labels}
                if d[0] and d[1]:
                    orth = [_rule(pic, 3, 3, rs, dd, lf)[0] for dd in ((d[0], 0), (0, d[1]))]
                    if not ok and labels != ["outside"] and all(orth):
                        seen.add((c, d, "diag_forbidden_orth_allowed"))
                    if ok and not all(orth):
                        seen.add((c, d, "diag_allowed_orth_forbidden"))


def border_cells_wanted():
    """Every (direction, case).  Narrowed, with the proof: CTBs are ordered by (tile id, raster address) and tiles
    are numbered in raster order of a grid, so a CTB to the left, above or above-left lies in the same tile or in
    one with a lower id and is always earlier: (left / up / up-left, later) cannot exist, nor can (right / down /
    down-right, earlier).  Up-right later and down-left earlier exist only across a tile-column boundary: that
    is the ``order_disagree`` cell (tile id higher, raster address lower), asked for on those two directions.
    Up-left allowed beside a forbidden up or left cannot exist either: all three CTBs precede the current one
    in tile scan, up and left between up-left and it, so the slice rule reads the current slice's flag for each,
    and a slice, a run in tile scan, that holds up-left and the current CTB holds the two between them; without
    loop_filter_across_tiles, a tile, a rectangle, that holds up-left and the current CTB holds up and left."""
    want = set()
    for d in S.DIRS:
        want |= {(d, "same"), (d, "outside"), (d, "tile_lf0"), (d, "tile_lf1")}
        if d not in ((1, 0), (0, 1), (1, 1)):
            want |= {(d, "earlier_f0"), (d, "earlier_f1")}
        if d not in ((-1, 0), (0, -1), (-1, -1)):
            want |= {(d, "later_f0"), (d, "later_f1")}
        if d[0] and d[1]:
            want |= {(d, "diag_forbidden_orth_allowed")} | ({(d, "diag_allowed_orth_forbidden")} if d != (-1, -1) else set())
    return want | {((1, -1), "order_disagree"), ((-1, 1), "order_disagree")}


LANE = {248: 4, 992: 16, 496: 8}                      # samples per lane of the strip kernel, by its strip


def _strip_cells(pics, outs):
    """Samples change in every component in the two columns either side of every strip boundary and in every
    column of the partial last lane, the last column among them (in one ``strips`` picture of the set or the
    other: beside a tile boundary only the vertical class and band offset reach the last column)."""
    strip, pic = pics[0].meta["strip"], pics[0]
    for c in range(3):
        diff = np.any([o[c] != p.planes[c] for p, o in zip(pics, outs)], axis=0)
        pw = diff.shape[1]
        bounds = list(range(strip, pw, strip))
        assert bounds, pic.meta
        for b in bounds:
            assert diff[:, b - 2:b].any(axis=0).all() and diff[:, b:b + 2].any(axis=0).all(), (pic.meta, c, b)
        # a partial last lane: 2008 % 16 = 8 and 1004 % 16 = 12 (sao_strip16_kernel), 500 % 8 = 4 (sao16_strip_kernel's
        # chroma); 520, 260 and 1000 are whole lanes
        assert (pw % LANE[strip] != 0) == (strip == 992 or (strip == 496 and c > 0)), (pic.meta, c)
        assert diff[:, pw - max(pw % LANE[strip], 1):].any(axis=0).all(), (pic.meta, c)


@pytest.mark.parametrize("bd,lg", CONTEXTS)
def test_c_twin_equals_python_and_layout_cells(bd, lg):
    """Both loop_filter_across_tiles sets of the context: the C twin's reconstruction is the planted planes and
    its output the Python oracle's SAO of them, on every picture.  Read from the outputs: every cell of
    border_cells_wanted per component; in the ``nofilter`` pictures no-filter blocks of either kind (bypass, PCM
    under pcm_loop_filter_disabled) at every (column, row) parity would change and do not; the ``strips``
    cells."""
    seen, parity = set(), set()
    for lf in (0, 1):
        pics, ref = S.sao_set(bd, lg, lf), _ref(bd, lg, lf)
        kinds, strips = [p.meta["kind"] for p in pics], []
        assert kinds.count("borders") == len(S.BORDER_PICTURES) and kinds.count("strips") == S.N_STRIPS
        for k, pic in enumerate(pics):
            assert (pic.tbs["flags"] & R.TB_PCM != 0).all()
            out = S.py_sao(bd, lg, lf, pic)
            for c in range(3):
                np.testing.assert_array_equal(ref[k][0][c], pic.planes[c], err_msg="recon c%d %r" % (c, pic.meta))
                np.testing.assert_array_equal(ref[k][1][c], out[c], err_msg="out c%d %r" % (c, pic.meta))
            if pic.meta["kind"] == "borders":
                _border_cells(pic, out, lg, lf, seen)
            elif pic.meta["kind"] == "strips":
                strips.append((pic, out))
            elif pic.meta["kind"] == "nofilter" and lf:
                free = S.py_sao(bd, lg, lf, R.Picture(ctus=pic.ctus, tbs=pic.tbs, coef=pic.coef, size=pic.size), pic.planes)
                for name, grid in (("bypass", pic.spec.nf), ("pcm", pic.spec.nf_pcm)):
                    for by, bx in zip(*np.nonzero(grid)):
                        for c in range(3):
                            n = 8 >> (c > 0)
                            blk = (slice(by * n, by * n + n), slice(bx * n, bx * n + n))
                            # (all of them but those on the picture's edge, whose neighbour is outside)
                            assert (free[c][blk] != pic.planes[c][blk]).sum() * 2 > n * n and (out[c][blk] == pic.planes[c][blk]).all()
                            parity.add((c, name, bx % 2, by % 2))
                        assert pic.nofilter[by * 17 + bx]
                beside = [(free[c] == out[c]) & (out[c] != pic.planes[c]) for c in range(3)]
                assert all(b.sum() > 1000 for b in beside)
        _strip_cells(*zip(*strips))
    for c in range(3):
        miss = sorted(w for w in border_cells_wanted() if (c,) + w not in seen)
        assert not miss, "bd%d ctb%d c%d borders: %s" % (bd, 1 << lg, c, miss)
        assert {p[1:] for p in parity if p[0] == c} == {(n, i, j) for n in ("bypass", "pcm") for i in (0, 1) for j in (0, 1)}


def test_set_shapes_and_floor():
    """What the set is made of, and that the filters change a great many samples of every component."""
    for bd, lg in ((8, 6), (10, 4)):
        pics = S.sao_set(bd, lg, 0)
        assert all(p.meta["kind"] and tuple(p.size) == (p.spec.w, p.spec.h) for p in pics)
        sizes = set(S.by_size(pics))
        assert sizes == {(128, 128), (136, 128), (3 << lg, 3 << lg), S.strip_size(bd, lg)[:2]}
        wide = [p for p in pics if p.meta["kind"] == "wide"]
        for c in range(3):
            for slot in range(4):
                assert set(S.WIDE) == {int(p.ctus["sao_offset"][rs, c, slot]) for p in wide for rs in range(len(p.ctus))}
        edge_signs = {tuple(np.sign(p.ctus["sao_offset"][rs, 0]).tolist()) for p in wide for rs in range(len(p.ctus))
                      if p.ctus["sao_type"][rs, 0] == 2}
        assert len(edge_signs - {(1, 1, -1, -1)}) >= 3
        mix = [p for p in pics if p.meta["kind"] in ("mix", "strips")]
        assert all({0, 1, 2} == set(p.ctus["sao_type"][:, c].tolist()) for p in mix for c in (0, 1))
        assert all(n > 20000 for n in S.changed_floor(bd, lg, 0))


@pytest.mark.parametrize("bd", S.DEPTHS)
def test_deblocking_at_qp0_changes_nothing(bd):
    """The Python oracle on deblocking-on twins (sao_set(dbk=True) asserts it for all with the C twin): recon,
    the deblocked planes and the planted planes are identical, and the output is the SAO-only output."""
    pics = S.sao_set(bd, 4, 1, dbk=True)
    for pic in [p for p in pics if p.meta["kind"] in ("edge", "nofilter")][::3] + [p for p in pics if p.meta["kind"] == "borders"][:2]:
        assert (pic.ctus["flags"] & R.CTU_DEBLOCK).all()
        prm = R.params_dict(S.params_of(bd, 4, 1, *pic.size))
        rec = O.reconstruct_picture(prm, pic.as_oracle_dict())
        dbk = O.deblock_picture(prm, pic.as_oracle_dict(), rec)
        for c in range(3):
            np.testing.assert_array_equal(rec[c], pic.planes[c])
            np.testing.assert_array_equal(dbk[c], pic.planes[c])


def test_lf_set_unchanged():
    """planted_lf.build gained the picture size, per-CTU SAO arguments and PCM no-filter CUs: lf_set's records
    are what they were."""
    import hashlib
    import planted_lf as L
    want = {(8, 5, "b", True): "b0db92a847be7015a658735c6a08ab32dd74cf1ad1852b63a040c6a7fb29dcdd",
            (10, 4, "a", False): "347310df52b0f459e2e1b619b8b4f12b78a64e2a353f305776d8a9866fcc87af"}
    for key, digest in want.items():
        h = hashlib.sha256()
        for p in L.lf_set(*key):
            for a in (p.ctus, p.tbs, p.coef, p.nofilter):
                h.update(b"-" if a is None else a.tobytes())
        assert h.hexdigest() == digest, key


# ---------------------------------------------------------------------------------
# sensitivity: the comparison fails an oracle with a planted defect
# ---------------------------------------------------------------------------------

def _patched(fn, subs, ns):
    src = inspect.getsource(fn)
    for old, new in subs:
        assert src.count(old) >= 1, old
        src = src.replace(old, new)
    ns = dict(ns)
    exec(compile(src, "<defect>", "exec"), ns)
    return ns[fn.__name__]


_CLIP_B = "np.clip(blk + np.asarray(offs)[idx], 0, (1 << bd) - 1)"
_CLIP_E = "np.clip(blk + np.asarray(offs)[edge], 0, (1 << bd) - 1)"
_SLICE = ('bad = not (int(ctus[rs]["flags"]) & CTU_LF_ACROSS_SLICES)', 'bad = not (int(ctus[other]["flags"]) & CTU_LF_ACROSS_SLICES)')
_NRS = "nrs = ((yn_c << sub) >> geo.ctb_log2) * geo.wc + ((xn_c << sub) >> geo.ctb_log2)"
_NB = "nb.append(rec[yn_c, xn_c])"

# name -> (substitutions in sao_picture, bit depth, loop_filter_across_tiles of the set that must notice)
DEFECTS = {
    "none": ([("shift = bd - 5", "shift = bd - 4 - 1")], 8, 0),
    "band_table_without_wrap": ([("table = np.zeros(32, np.int64)", "table = np.zeros(64, np.int64)"),
                                 ("table[(k + band) & 31]", "table[k + band]")], 8, 0),
    "band_shift_3_above_8_bits": ([("shift = bd - 5", "shift = 3"), ("table[blk >> shift]", "table[np.minimum(blk >> shift, 31)]")], 10, 0),
    "band_no_clip_at_0": ([(_CLIP_B, "np.minimum(blk + np.asarray(offs)[idx], (1 << bd) - 1)")], 8, 0),
    "band_no_clip_at_max": ([(_CLIP_B, "np.maximum(blk + np.asarray(offs)[idx], 0)")], 8, 0),
    "edge_no_clip_at_0": ([(_CLIP_E, "np.minimum(blk + np.asarray(offs)[edge], (1 << bd) - 1)")], 8, 0),
    "edge_no_clip_at_max": ([(_CLIP_E, "np.maximum(blk + np.asarray(offs)[edge], 0)")], 8, 0),
    "ge_in_first_sign": ([("np.sign(blk - nb[0])", "np.where(blk >= nb[0], 1, -1)")], 8, 0),
    "ge_in_second_sign": ([("np.sign(blk - nb[1])", "np.where(blk >= nb[1], 1, -1)")], 8, 0),
    "edge_idx_without_swap": ([("edge = np.where(edge == 2, 0, np.where(edge < 2, edge + 1, edge))", "edge = edge + 0")], 8, 0),
    "class_2_and_3_swapped": ([('_EO_POS[int(c["sao_class"][c_idx])]', '_EO_POS[(0, 1, 3, 2)[int(c["sao_class"][c_idx])]]')], 8, 0),
    "earlier_samples_slice_flag": ([(_SLICE[0], "bad = None"), (_SLICE[1], _SLICE[0]), ("bad = None", _SLICE[1])], 8, 1),
    "raster_order_for_tile_scan": ([("geo.rs2ts[other] < geo.rs2ts[rs]", "other < rs")], 8, 1),
    "diagonal_judged_by_orthogonal_ctb": ([(_NRS, "nrs = np.where((((xn_c << sub) >> geo.ctb_log2) != rx) & (((yn_c << sub) >> geo.ctb_log2) != ry), "
                                            "ry * geo.wc + ((xn_c << sub) >> geo.ctb_log2), " + _NRS[6:] + ")")], 8, 1),
    "tile_boundary_ignored": ([("if not lf_tiles and geo.tile[other] != geo.tile[rs]:", "if False:")], 8, 0),
    "tile_boundary_always_enforced": ([("if not lf_tiles and geo.tile[other] != geo.tile[rs]:", "if geo.tile[other] != geo.tile[rs]:")], 8, 1),
    "picture_edge_clamped_neighbour": ([("ok &= inside", "ok &= True")], 8, 0),
    "nofilter_samples_filtered": ([("if nofilter is not None:", "if False:")], 8, 0),
    "nofilter_neighbour_unavailable": ([(_NB, _NB + "\n                    if nofilter is not None:\n                        ok &= np.asarray(nofilter)"
                                         "[((yn_c << sub) >> 3) * ((geo.w + 7) >> 3) + ((xn_c << sub) >> 3)] == 0")], 8, 0),
    "cr_with_cb_band_position": ([('band = int(c["sao_class"][c_idx])', 'band = int(c["sao_class"][min(c_idx, 1)])')], 8, 0),
    "cr_with_cb_offsets": ([('c["sao_offset"][c_idx]', 'c["sao_offset"][min(c_idx, 1)]')], 8, 0),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_sao_comparison_notices_defects(monkeypatch, defect):
    """Each defect planted into the Python oracle's SAO breaks its equality with the C twin on a set at CTB 32;
    the recompiled function without a defect does not."""
    subs, bd, lf = DEFECTS[defect]
    monkeypatch.setattr(O, "sao_picture", _patched(O.sao_picture, subs, O.__dict__))
    pics, ref = S.sao_set(bd, 5, lf), _ref(bd, 5, lf)
    bad = [pic.meta for k, pic in enumerate(pics)
           if any(not np.array_equal(o, r) for o, r in zip(S.py_sao(bd, 5, lf, pic), ref[k][1]))]
    assert (not bad) if defect == "none" else bad, defect


def test_set_notices_unscaled_offsets_at_12_bits(monkeypatch):
    """SaoOffsetVal = offset << (BitDepth - 10) above 10 bits (7.4.9.3.2) is the front-end's: without it the
    ``edge`` and ``band`` pictures' records, and the oracle's output of them, differ."""
    want = [S.py_sao(12, 5, 1, p) for p in (S.edge_picture(12, 5, 0), S.band_picture(12, 5, 0))]
    monkeypatch.setattr(frontend, "sao_offset_val", _patched(frontend.sao_offset_val, [("shift = bit_depth - min(bit_depth, 10)", "shift = 0")],
                                                             frontend.__dict__))
    for w, pic in zip(want, (S.edge_picture(12, 5, 0), S.band_picture(12, 5, 0))):
        assert np.abs(pic.ctus["sao_offset"]).max() == 31
        assert all((o != r).any() for o, r in zip(S.py_sao(12, 5, 1, pic), w))
