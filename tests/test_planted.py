"""Directed intra tests on the CPU: the new reference pins, and the planted-TB set (tests/planted.py).

  * the oracle against tests/golden/ref_pins*.npz (vertical angular family and luma mode 10, pinned to the
    reference by transposition) and ref_chain*.npz (neighbour substitution -> filtering -> prediction chains);
  * pictures planted from the chain inputs reconstruct to the reference's output in both oracles;
  * the C twin equals the Python oracle on whole planes of the planted set at 8, 10 and 12 bits;
  * the set covers every (component, size, mode, placement) and (component, size, mode, style) cell;
  * the set notices the reference's known defects and a packed-arithmetic slip planted into the oracle.
"""
import os

import numpy as np
import pytest

import planted as P
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import records as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEPTHS = (8, 10, 12)


def _pins(bd):
    return np.load(os.path.join(GOLDEN, "ref_pins%s.npz" % ("" if bd == 8 else "_bd%d" % bd)))


# ---------------------------------------------------------------------------------
# reference pins
# ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", DEPTHS)
def test_vertical_family_matches_reference_by_transposition(bd):
    """Modes 19..25 and 27..34: O.predict equals the reference's horizontal branch run on the transposed
    neighbours (8.4.4.2.6 is symmetric under transposition), luma and chroma, every size."""
    F = _pins(bd)
    assert len(F["vert_n"]) >= 400
    seen = set()
    kl = ko = 0
    for n, mode, c in zip(F["vert_n"], F["vert_mode"], F["vert_c"]):
        n, mode, c = int(n), int(mode), int(c)
        L = F["vert_L"][kl:kl + 4 * n + 1].astype(np.int64)
        want = F["vert_out"][ko:ko + n * n].reshape(n, n)
        kl, ko = kl + 4 * n + 1, ko + n * n
        np.testing.assert_array_equal(O.predict(L, n, mode, c, bd), want, err_msg="n=%d mode=%d c=%d" % (n, mode, c))
        seen.add((n, mode, c))
    assert seen == {(n, m, c) for n in (4, 8, 16, 32) for m in list(range(19, 26)) + list(range(27, 35)) for c in (0, 1)}
    assert F["vert_L"].max() == (1 << bd) - 1 and F["vert_L"].min() == 0


@pytest.mark.parametrize("bd", DEPTHS)
def test_luma_mode10_matches_reference_mode26(bd):
    """Luma mode 10 below 32x32 (edge filter with its clip) equals the transposed output of the reference's
    mode 26; the clip fires in many of the vectors."""
    F = _pins(bd)
    kl = ko = clipped = 0
    for n in F["m10_n"]:
        n = int(n)
        L = F["m10_L"][kl:kl + 4 * n + 1].astype(np.int64)
        want = F["m10_out"][ko:ko + n * n].reshape(n, n)
        kl, ko = kl + 4 * n + 1, ko + n * n
        np.testing.assert_array_equal(O.predict(L, n, 10, 0, bd), want, err_msg="n=%d" % n)
        raw = L[2 * n - 1] + ((L[2 * n + 1: 3 * n + 1] - L[2 * n]) >> 1)
        clipped += int(((raw < 0) | (raw > (1 << bd) - 1)).any())
    assert len(F["m10_n"]) >= 60 and clipped >= 10


@pytest.mark.parametrize("bd", DEPTHS)
def test_oracle_chain_matches_reference(bd):
    """substitute -> filter_refs -> predict on planted values and availability equals decode_neighbor + the
    reference's prediction: every reference-correct availability pattern x luma size x mode."""
    vs = P.load_chain(bd)
    for v in vs:
        n, mode = v["n"], v["mode"]
        p = O.substitute(np.where(v["avail"], v["vals"], 0), v["avail"], bd)
        p = O.filter_refs(p, n, mode, 0, True, bd)
        np.testing.assert_array_equal(O.predict(p, n, mode, 0, bd), v["out"],
                                      err_msg="pattern %d n=%d mode=%d" % (v["pattern"], n, mode))
    assert {(v["pattern"], v["n"], v["mode"]) for v in vs} == {(p, n, m) for p in range(5) for n in (4, 8, 16, 32)
                                                               for m in range(35)}


def _decode_c(bd, pics):
    return c_oracle.decode(P.set_params(bd), pics, threads=4)


def _decode_py(pic):
    pp = R.pic_params(P.set_params(pic.meta["bit_depth"]), pic)
    return O.reconstruct_picture(R.params_dict(pp), pic.as_oracle_dict())


@pytest.mark.parametrize("bd", DEPTHS)
def test_chain_pictures_reconstruct_to_reference_output(bd):
    """Pictures planted from the chain inputs: both oracles' luma plane holds the reference's prediction in the
    target block (no oracle function stands between the planted samples and the expected block)."""
    cs = P.chain_set(bd)
    assert len(cs) == 5 * 3 * 35 + len(P.CHAIN_PLACEMENTS_4) * 35
    ref = _decode_c(bd, [pic for _, pic, _ in cs])
    for k, (_, pic, want) in enumerate(cs):
        ys, xs = P.chain_region(pic)
        np.testing.assert_array_equal(ref[k][0][0][ys, xs], want, err_msg="C twin, %r" % pic.meta)
        np.testing.assert_array_equal(_decode_py(pic)[0][ys, xs], want, err_msg="Python oracle, %r" % pic.meta)


# ---------------------------------------------------------------------------------
# the planted set
# ---------------------------------------------------------------------------------

def python_subset(bd):
    """Indices of the planted set the Python oracle decodes (the full set takes it 20 s per bit depth): the
    pictures with (i + bd) % 5 == 0 at ``interior`` (seven of each size and style) and five consecutive i, starting
    at bd, elsewhere (the styles rotate with i, period 5): one picture or more per (placement, size, style), other
    modes at each bit depth.  The C twin always runs the full set; the Python oracle's modes are pinned by the
    chain vectors."""
    return [k for k, (placement, _, _, i, *_rest) in enumerate(P.plan())
            if ((i + bd) % 5 == 0 if placement == "interior" else bd <= i < bd + 5)]


@pytest.mark.parametrize("bd", DEPTHS)
def test_c_twin_equals_python_oracle_on_planted_set(bd):
    pics = [pic for _, pic in P.planted_set(bd)]
    ref = _decode_c(bd, pics)
    sub = python_subset(bd)
    cells = {(P.plan()[k][0], P.plan()[k][1], P.plan()[k][2], P.plan()[k][4]) for k in sub}
    want_cells = {(p, s, nxn, st) for (p, s, nxn, _, st, *_r) in P.plan()}
    assert cells == want_cells
    for k in sub:
        rec = _decode_py(pics[k])
        for c in range(3):
            np.testing.assert_array_equal(ref[k][0][c], rec[c], err_msg="c%d %r" % (c, pics[k].meta))
            np.testing.assert_array_equal(ref[k][1][c], rec[c], err_msg="out c%d %r" % (c, pics[k].meta))


def test_placements_give_their_availability():
    """PLACEMENTS' (bottom-left, left, corner, top, top-right) table, from the oracle's 6.4.1 availability, for
    the luma TB and the chroma TBs at S = 8, 16, 32."""
    for placement, (_, _, _, _, pattern) in P.PLACEMENTS.items():
        for s in (8, 16, 32):
            params, pic = P.build(s, placement, 3, 5, 8)
            geo = O.Geometry(R.params_dict(params), pic.ctus)
            x0, y0 = pic.meta["target"]
            for sub, n in ((0, s), (1, s // 2)):
                dx, dy = O.ref_positions(n)
                got = np.array([geo.available(x0, y0, ((x0 >> sub) + a) << sub, ((y0 >> sub) + b) << sub)
                                for a, b in zip(dx, dy)])
                np.testing.assert_array_equal(got, P.pattern_avail(n, pattern), err_msg="%s S=%d sub=%d" % (placement, s, sub))


@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_set_coverage(bd):
    """Computed from the records: every (component, size, mode, placement) cell occurs, every (component, size,
    mode, neighbour style) and (component, size, mode, residual style) cell occurs at ``interior``, and no
    picture exceeds 128 x 128 or holds anything but PCM CUs around its target."""
    by_place, by_style, by_res = set(), set(), set()
    for params, pic in P.planted_set(bd):
        assert int(params["pic_width"]) <= 128 and int(params["pic_height"]) <= 128 and int(params["bit_depth_luma"]) == bd
        t = pic.tbs[(pic.tbs["flags"] & R.TB_PCM) == 0]
        assert len(t) == (6 if pic.meta["nxn"] else 3)
        for r in t:
            cell = (min(int(r["c_idx"]), 1), 1 << int(r["log2_size"]), int(r["pred_mode"]))
            by_place.add(cell + (pic.meta["placement"],))
            if pic.meta["placement"] == "interior":
                by_style.add(cell + (pic.meta["style"],))
                by_res.add(cell + (pic.meta["residual"],))
    cells = [(c, n, m) for c, sizes in ((0, (4, 8, 16, 32)), (1, (4, 8, 16))) for n in sizes for m in range(35)]
    assert by_place == {x + (p,) for x in cells for p in P.PLACEMENTS}
    assert by_style == {x + (s,) for x in cells for s in P.NEIGHBOUR_STYLES}
    assert by_res == {x + (s,) for x in cells for s in P.RESIDUAL_STYLES}
    assert len(P.planted_set(bd)) == len(P.plan()) == 5 * 140 + 8 * 140


@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_set_reaches_the_value_edges(bd):
    """The edges the styles are there for really occur in the C twin's decode of the set: the reconstruction
    clip fires at 0 and at max in every component, the mode 10 / 26 edge filter clips at both ends, the
    strong-filter differences sit at thr - 1 and thr on either side, and Cb is at max beside Cr at 0."""
    mx, thr = (1 << bd) - 1, 1 << (bd - 5)
    items = P.planted_set(bd)
    ref = _decode_c(bd, [pic for _, pic in items])
    sat, edge, strong, packed = set(), set(), set(), False
    for k, (_, pic) in enumerate(items):
        m = pic.meta
        if m["placement"] != "interior":
            continue
        if m["residual"] == "saturate" and not m["nxn"]:
            for c in range(3):
                blk = ref[k][0][c][P.target_region(pic, c)]
                sat |= {(c, v) for v in (0, mx) if (blk == v).all()}
        x0, y0 = m["target"]
        Y = ref[k][0][0].astype(np.int64)
        if m["residual"] != "saturate" and not m["nxn"] and m["s"] < 32 and m["modes"][0] in (10, 26):
            s = m["s"]
            if m["modes"][0] == 26:
                raw = Y[y0 - 1, x0] + ((Y[y0:y0 + s, x0 - 1] - Y[y0 - 1, x0 - 1]) >> 1)
            else:
                raw = Y[y0, x0 - 1] + ((Y[y0 - 1, x0:x0 + s] - Y[y0 - 1, x0 - 1]) >> 1)
            edge |= {(m["modes"][0], "low")} if (raw < 0).any() else set()
            edge |= {(m["modes"][0], "high")} if (raw > mx).any() else set()
        if m["style"] == "flat" and m["s"] == 32:
            d_top = abs(Y[y0 - 1, x0 - 1] + Y[y0 - 1, x0 + 63] - 2 * Y[y0 - 1, x0 + 31])
            d_left = abs(Y[y0 - 1, x0 - 1] + Y[y0 + 63, x0 - 1] - 2 * Y[y0 + 31, x0 - 1])
            strong.add((int(d_top) - thr, int(d_left) - thr))
        if m["style"] == "extremes":
            cb, cr = ref[k][0][1].astype(np.int64), ref[k][0][2].astype(np.int64)
            row = (slice(y0 // 2 - 1, y0 // 2), slice(x0 // 2 - 1, x0 // 2 + m["s"]))
            packed |= bool(((cb[row] == mx) & (cr[row] == 0)).any() and ((cb[row] == 0) & (cr[row] == mx)).any())
    assert sat == {(c, v) for c in range(3) for v in (0, mx)}
    assert edge == {(md, e) for md in (10, 26) for e in ("low", "high")}
    assert strong == {(a, b) for a in (-1, 0) for b in (-1, 0)}
    assert packed


# ---------------------------------------------------------------------------------
# sensitivity: the set fails an oracle with a planted defect
# ---------------------------------------------------------------------------------

def _angular(p, n, mode, bd, fact_inverted=False, no_round=False, carry_from=None):
    """8.4.4.2.6 without the edge filter, as O.predict computes it, with optional defects: the reference's
    inverted iFact test in the vertical family (intra.py:155-158), its inverse-angle projection without
    + 128 (intra.py:146), and ``carry_from`` (Cb's reference array while predicting Cr): the packed sum
    Cb | Cr << 16 without the split, so bit 16 of Cb's weighted sum is added to Cr's."""
    angle = O.INTRA_PRED_ANGLE[mode - 2]
    vertical = mode >= 18

    def refs(p):
        main = (lambda x: p[2 * n + 1 + x]) if vertical else (lambda y: p[2 * n - 1 - y])
        side = (lambda y: p[2 * n - 1 - y]) if vertical else (lambda x: p[2 * n + 1 + x])
        ref = {x: main(x - 1) for x in range(0, 2 * n + 1)}
        if angle < 0 and (n * angle) >> 5 < -1:
            inv = O.INV_ANGLE[mode - 11]
            for x in range((n * angle) >> 5, 0):
                ref[x] = side(-1 + ((x * inv + (0 if no_round else 128)) >> 8))
        return ref

    ref = refs(np.asarray(p, np.int64))
    ref_cb = refs(np.asarray(carry_from, np.int64)) if carry_from is not None else None
    pred = np.empty((n, n), np.int64)
    for a in range(n):
        idx, fact = ((a + 1) * angle) >> 5, ((a + 1) * angle) & 31
        interpolate = (fact == 0) if (fact_inverted and vertical) else (fact != 0)
        for b in range(n):
            if interpolate:
                s = (32 - fact) * ref[b + idx + 1] + fact * ref[b + idx + 2] + 16
                if ref_cb is not None:
                    s += ((32 - fact) * ref_cb[b + idx + 1] + fact * ref_cb[b + idx + 2] + 16) >> 16
                v = s >> 5
            else:
                v = ref[b + idx + 1]
            pred[(a, b) if vertical else (b, a)] = v
    return pred


def _mutants(monkeypatch):
    real_predict, real_substitute = O.predict, O.substitute
    state = {}

    def angular_mutant(**kw):
        def predict(p, n, mode, c_idx, bd):
            if mode < 2 or (c_idx == 0 and n < 32 and mode in (10, 26)):
                return real_predict(p, n, mode, c_idx, bd)
            if "carry" in kw:
                if c_idx == 1:
                    state["cb"] = np.asarray(p, np.int64)
                return _angular(p, n, mode, bd, carry_from=state["cb"] if c_idx == 2 else None)
            return _angular(p, n, mode, bd, **kw)
        return lambda: monkeypatch.setattr(O, "predict", predict)

    def chroma_edge_filter():
        monkeypatch.setattr(O, "predict", lambda p, n, mode, c_idx, bd: real_predict(p, n, mode, 0 if mode in (10, 26) else c_idx, bd))

    def no_substitution_when_bl_present():
        def substitute(vals, avail, bd):
            if np.asarray(avail, bool)[0]:                     # intra.py:243: nothing is substituted then
                return np.asarray(vals, np.int64).copy()
            return real_substitute(vals, avail, bd)
        monkeypatch.setattr(O, "substitute", substitute)

    return {"none": angular_mutant(), "fact_inverted": angular_mutant(fact_inverted=True),
            "no_128_in_projection": angular_mutant(no_round=True), "edge_filter_on_chroma": chroma_edge_filter,
            "no_substitution_when_bl_present": no_substitution_when_bl_present, "cb_carry_into_cr": angular_mutant(carry=True)}


# Cb's weighted sum reaches bit 16 only above 10 bits (32 * 1023 + 16 < 65536): that defect is looked for at 12
@pytest.mark.parametrize("defect,bd", [("none", 8), ("none", 12), ("fact_inverted", 8), ("no_128_in_projection", 8),
                                       ("edge_filter_on_chroma", 8), ("no_substitution_when_bl_present", 8),
                                       ("cb_carry_into_cr", 12)])
def test_planted_comparison_notices_defects(monkeypatch, defect, bd):
    """The Python oracle with one defect planted (the reference's four, and Cb's carry leaking into Cr in a packed
    chroma sum) no longer equals the C twin on the planted set; the defect-free rewrite of the angular
    prediction used for the planting does.  Stands in for 'would fail if a kernel were subtly wrong'."""
    pics = [pic for _, pic in P.planted_set(bd)]
    ref = _decode_c(bd, pics)
    _mutants(monkeypatch)[defect]()
    # the cells a defect can show in, so the search stays short: interior and the two placements with the
    # bottom-left present and something else missing
    order = [k for k, pl in enumerate(P.plan()) if pl[0] in ("tr_missing", "top_edge")][::3] + \
            [k for k, pl in enumerate(P.plan()) if pl[0] == "interior"]
    bad = []
    for k in order:
        rec = _decode_py(pics[k])
        if any(not np.array_equal(rec[c], ref[k][0][c]) for c in range(3)):
            bad.append(pics[k].meta)
            if defect != "none":
                break
    if defect == "none":
        assert not bad, bad[:3]
    else:
        assert bad, "the planted set does not notice %s" % defect
