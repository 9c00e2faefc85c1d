"""The planted residual set (tests/planted.py residual_set) on the CPU.

  * for every planted TB the C twin's target block equals clip(v + O.residual_block(...)): the Python oracle's
    residual is called directly on the TB's levels, so the whole set is checked without whole-picture Python
    decodes (a handful of whole pictures are decoded too: the constant prediction really holds, and nothing
    else in the picture moves);
  * coverage, from the records: every (class, ky, kx) impulse, every (class, qP'), every extreme pattern, the
    transform-skip and bypass levels, the job-count sub-batches;
  * reach, from the oracle's stages: both clamps fire at both ends, residuals pass int16 at 10 and 12 bits,
    every shift of the GPU's folded dequantisation occurs;
  * sensitivity: the Python oracle with one defect planted no longer equals the C twin on the set.
"""
import numpy as np
import pytest

import planted as P
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import records as R

DEPTHS = (8, 10, 12)
_REF = {}


def _pics(bd, table=None):
    return [pic for _, pic in P.residual_set(bd) if table is None or pic.meta["scaled"]]


def _ref(bd, table=None):
    """The C twin's reconstruction planes of the set (flat), or of its scaled pictures under a table."""
    if (bd, table) not in _REF:
        sf = None if table is None else P.scaling_tables()[table]
        ref = c_oracle.decode(P.set_params(bd, table is not None), _pics(bd, table), threads=8, scaling=sf)
        _REF[(bd, table)] = [r[0] for r in ref]
    return _REF[(bd, table)]


def _levels(pic, t):
    n = 1 << int(t["log2_size"])
    off = int(t["coef_off"])
    return np.asarray(pic.coef[off:off + n * n], np.int64).reshape(n, n)


def _mismatches(bd, table=None, only=None, first=False):
    """[(picture meta, c_idx)] of the planted TBs whose block in the C twin is not clip(v + O.residual_block)."""
    sf = None if table is None else P.scaling_tables()[table]
    ref, bad = _ref(bd, table), []
    for k, pic in enumerate(_pics(bd, table)):
        if only is not None and not only(pic):
            continue
        for t in P.planted_tbs(pic):
            lg, c = int(t["log2_size"]), int(t["c_idx"])
            n, x, y = 1 << lg, int(t["x"]), int(t["y"])
            m = None if sf is None else O.factor_of(sf, lg, c)
            r = O.residual_block(_levels(pic, t), lg, c, int(t["qp"]), int(t["flags"]), bd, m)
            want = np.clip(pic.meta["v"] + r, 0, (1 << bd) - 1)
            if not np.array_equal(ref[k][c][y:y + n, x:x + n], want):
                bad.append((pic.meta, c))
                if first:
                    return bad
    return bad


@pytest.mark.parametrize("bd", DEPTHS)
def test_c_twin_equals_constant_plus_residual(bd):
    assert not _mismatches(bd)
    for table in P.scaling_tables():
        assert not _mismatches(bd, table), table


@pytest.mark.parametrize("bd", DEPTHS)
def test_whole_pictures_in_python_oracle(bd):
    """One picture of every kind and size decoded whole by the Python oracle equals the C twin: every mode
    predicts the constant from the planted reference lines and the PCM surround is left alone."""
    seen = set()
    ref = _ref(bd)
    for k, pic in enumerate(_pics(bd)):
        key = (pic.meta["kind"], pic.meta["s"], pic.meta["nxn"])
        if key in seen:
            continue
        seen.add(key)
        rec = O.reconstruct_picture(R.params_dict(P.set_params(bd)), pic.as_oracle_dict())
        for c in range(3):
            np.testing.assert_array_equal(ref[k][c], rec[c], err_msg="c%d %r" % (c, pic.meta))
    assert len(seen) == 4 * 4 + 2                   # impulse, sweep, extreme, bypass x 4 sizes; tskip; count


@pytest.mark.parametrize("bd", DEPTHS)
def test_residual_set_coverage(bd):
    qp_max = 51 + 6 * (bd - 8)
    mx = (1 << bd) - 1
    impulses, signs, sweep, extreme, tskip, bypass = set(), set(), set(), set(), set(), set()
    for params, pic in P.residual_set(bd):
        m = pic.meta
        assert m["placement"] == "interior" and int(params["bit_depth_luma"]) == bd
        tbs = P.planted_tbs(pic)
        assert len(tbs) == (m["n_dct4"] if m["kind"] == "count" else 3)
        assert all(int(t["qp"]) <= qp_max for t in pic.tbs)
        for t in tbs:
            lg, c, f = int(t["log2_size"]), int(t["c_idx"]), int(t["flags"])
            cls, lv = P.res_class(lg, c), _levels(pic, t)
            if m["kind"] == "impulse":
                assert np.count_nonzero(lv) == 1
                ky, kx = (int(a[0]) for a in np.nonzero(lv))
                assert abs(int(lv[ky, kx])) == P.impulse_level(lg, c, bd, int(t["qp"]))
                assert int(t["qp"]) == (30 + 6 * (bd - 8), *P.chroma_qps(30 + 6 * (bd - 8), bd))[c]
                r = O.residual_block(lv, lg, c, int(t["qp"]), f, bd)
                assert 0 < m["v"] + r.min() and m["v"] + r.max() < mx and r.any()       # observed in full
                impulses.add((cls, c > 0, ky, kx))
                signs.add((cls, c > 0, int(np.sign(lv[ky, kx]))))
            elif m["kind"] == "sweep":
                assert lv.any()
                sweep.add((cls, int(t["qp"])))
            elif m["kind"] == "extreme":
                assert np.array_equal(lv, P.extreme_block(m["patterns"][c], lg, c))
                extreme.add((cls, m["patterns"][c], m["qp_prime"] if c == 0 else None, m["v"]))
            elif m["kind"] == "tskip":
                assert f & R.TB_TSKIP and lg == 2 and {-32768, 32767, 1, -1} == set(lv.ravel().tolist())
                tskip.add((c, int(t["qp"]), m["v"]))
            elif m["kind"] == "bypass":
                assert f & R.TB_BYPASS and {-32768, 32767, mx, -mx} == set(lv.ravel().tolist())
                bypass.add((cls, m["v"]))
    sizes = {"dst4": 4, "dct4": 4, "dct8": 8, "dct16": 16, "dct32": 32}
    luma, chroma = ("dst4", "dct8", "dct16", "dct32"), ("dct4", "dct8", "dct16")
    want = {(cls, ch, ky, kx) for ch, group in ((False, luma), (True, chroma)) for cls in group
            for ky in range(sizes[cls]) for kx in range(sizes[cls])}
    assert impulses == want
    assert signs == {(cls, ch, sg) for ch, group in ((False, luma), (True, chroma)) for cls in group for sg in (1, -1)}
    assert sweep >= {(cls, qp) for cls in P.RES_CLASSES for qp in range(qp_max + 1)}
    v_ext = (0, mx)
    assert {e for e in extreme if e[2] is not None} == {(cls, pat, qp, v) for cls in luma for pat in P.EXTREME_PATTERNS
                                                        for qp in (0, 29, qp_max) for v in v_ext}
    assert {(e[0], e[1], e[3]) for e in extreme if e[2] is None} == {(cls, pat, v) for cls in chroma
                                                                     for pat in P.EXTREME_PATTERNS for v in v_ext}
    vs = (0, 1 << (bd - 1), mx)
    assert tskip == {(c, qp, v) for c in range(3) for qp in (0, qp_max) for v in vs}
    assert bypass == {(cls, v) for cls in P.RES_CLASSES for v in vs}


@pytest.mark.parametrize("bd", DEPTHS)
def test_job_count_batches(bd):
    """The sub-batches hold exactly 1, TPB - 1, TPB and TPB + 1 TBs of their class."""
    pics = [pic for _, pic in P.residual_set(bd)]
    got = set()
    for cls, n, idx in P.job_count_batches(bd):
        assert P.class_counts([pics[i] for i in idx])[cls] == n
        got.add((cls, n - P.RES_TPB[cls] if n > 1 else "one"))
    assert got == {(cls, d) for cls in P.RES_CLASSES for d in ("one", -1, 0, 1)}


def _stages(lv, lg, c, qp, bd, m=None):
    """(dequantised value before its clamp, stage-1 output before its clamp, residual) of a transformed TB,
    from the oracle's tables and functions."""
    bds = bd + lg - 5
    mm = 16 if m is None else np.asarray(m, np.int64)
    pre_d = (((lv * mm * O.LEVEL_SCALE[qp % 6]) << (qp // 6)) + (1 << (bds - 1))) >> bds
    d = O.dequantize(lv, qp, lg, bd, m)
    assert np.array_equal(d, np.clip(pre_d, -32768, 32767))
    t = O.transform_matrix(lg, 1 if (lg == 2 and c == 0) else 0)
    pre_g = (t.T @ d + 64) >> 7
    return pre_d, pre_g, O.residual_block(lv, lg, c, qp, R.TB_CBF, bd, m)


@pytest.mark.parametrize("bd", DEPTHS)
def test_residual_set_reach(bd):
    """What the set is there for really happens in the oracle: the dequantisation clamp and the stage-1 clamp
    fire at both ends, in every job class; a residual leaves int16 in both directions at 10 and 12 bits (the GPU
    keeps residuals as int16: clamped, which the reconstruction clip hides, where a wrap would flip the block)
    and stays inside at 8; Dequant (residual.h) takes every left shift 0..3 and every right shift 1..BitDepth;
    with the ScalingFactor tables the clamps fire too."""
    clamps, beyond, left, right = set(), set(), set(), set()
    tables = P.scaling_tables()
    for _, pic in P.residual_set(bd):
        for t in P.planted_tbs(pic):
            lg, c, f, qp = int(t["log2_size"]), int(t["c_idx"]), int(t["flags"]), int(t["qp"])
            if f & R.TB_BYPASS:
                continue
            per, bds = qp // 6, bd + lg - 5
            left |= {per - bds} if per >= bds else set()
            right |= {bds - per} if per < bds else set()
            if f & R.TB_TSKIP or pic.meta["kind"] != "extreme":
                continue
            cls = P.res_class(lg, c)
            for name in [None] + (list(tables) if pic.meta["scaled"] else []):
                m = None if name is None else O.factor_of(tables[name], lg, c)
                pre_d, pre_g, r = _stages(_levels(pic, t), lg, c, qp, bd, m)
                sl = name is not None
                clamps |= {("dequant", cls, sl, "low")} if pre_d.min() < -32768 else set()
                clamps |= {("dequant", cls, sl, "high")} if pre_d.max() > 32767 else set()
                clamps |= {("stage1", cls, sl, "low")} if pre_g.min() < -32768 else set()
                clamps |= {("stage1", cls, sl, "high")} if pre_g.max() > 32767 else set()
                beyond |= {"low"} if r.min() < -32768 else set()
                beyond |= {"high"} if r.max() > 32767 else set()
    assert clamps == {(st, cls, sl, e) for st in ("dequant", "stage1") for cls in P.RES_CLASSES for sl in (False, True)
                      for e in ("low", "high")}
    assert beyond == (set() if bd == 8 else {"low", "high"})
    assert left == {0, 1, 2, 3} and right == set(range(1, bd + 1))


# ---------------------------------------------------------------------------------
# sensitivity: the comparison fails an oracle with a planted defect
# ---------------------------------------------------------------------------------

def _entries(n):
    """Five (k, n) of an N x N transform matrix: the corners (the last row included) and one inside."""
    return [(0, 0), (1, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, n // 2 - 1)]


ENTRY_CASES = [(lg, tr, k, col, d) for lg, tr in ((2, 1), (2, 0), (3, 0), (4, 0), (5, 0))
               for i, (k, col) in enumerate(_entries(1 << lg)) for d in ((1,) if i % 2 else (-1,))]


def _residual_with(round_div=1, wrap=False, bd_final=None):
    def residual_block(level, log2, c_idx, qp, flags, bit_depth, m=None):
        level = np.asarray(level, np.int64)
        if flags & (O.TB_BYPASS | O.TB_PCM):
            return level.copy()
        d = O.dequantize(level, qp, log2, bit_depth, m)
        if flags & O.TB_TSKIP:
            r = d << (5 + log2)
        else:
            r = O.inverse_transform(d, log2, 1 if (log2 == 2 and c_idx == 0) else 0)
        sh = 20 - (bit_depth if bd_final is None else bd_final)
        r = (r + (1 << (sh - 1)) // round_div) >> sh
        return ((r + 32768) & 0xffff) - 32768 if wrap else r
    return residual_block


def _plant(monkeypatch, defect):
    real_tm, real_dq = O.transform_matrix, O.dequantize
    if defect == "none":
        monkeypatch.setattr(O, "residual_block", _residual_with())
    elif defect == "transposed":
        monkeypatch.setattr(O, "transform_matrix", lambda lg, tr: np.ascontiguousarray(real_tm(lg, tr).T))
    elif defect == "no_stage1_clamp":
        def inverse_transform(d, log2, tr_type):
            t = real_tm(log2, tr_type)
            return ((t.T @ np.asarray(d, np.int64) + 64) >> 7) @ t
        monkeypatch.setattr(O, "inverse_transform", inverse_transform)
    elif defect == "no_dequant_clamp":
        def dequantize(level, qp, log2, bit_depth, m=None):
            bds = bit_depth + log2 - 5
            mm = 16 if m is None else np.asarray(m, np.int64)
            return (((np.asarray(level, np.int64) * mm * O.LEVEL_SCALE[qp % 6]) << (qp // 6)) + (1 << (bds - 1))) >> bds
        monkeypatch.setattr(O, "dequantize", dequantize)
        assert real_dq is not O.dequantize
    elif defect == "stage2_rounding_halved":
        monkeypatch.setattr(O, "residual_block", _residual_with(round_div=2))
    elif defect == "level_scale_5_is_71":
        monkeypatch.setattr(O, "LEVEL_SCALE", [40, 45, 51, 57, 64, 71])
    elif defect == "residual_wrapped_to_int16":
        monkeypatch.setattr(O, "residual_block", _residual_with(wrap=True))
    elif defect == "bdshift_of_8_bits":
        monkeypatch.setattr(O, "residual_block", _residual_with(bd_final=8))
    else:
        raise KeyError(defect)


# a residual passes int16 only above 8 bits, and the final bdShift is that of 8 bits at 8 bits
@pytest.mark.parametrize("defect,bd", [("none", 8), ("none", 12), ("transposed", 8), ("no_stage1_clamp", 8),
                                       ("no_dequant_clamp", 8), ("stage2_rounding_halved", 8),
                                       ("level_scale_5_is_71", 8), ("residual_wrapped_to_int16", 10),
                                       ("residual_wrapped_to_int16", 12), ("bdshift_of_8_bits", 12)])
def test_residual_comparison_notices_defects(monkeypatch, defect, bd):
    """Each defect planted into the Python oracle breaks its equality with the C twin on the set (the
    transposed matrix is the reference's own defect); the restated residual_block without a defect does not."""
    _ref(bd)
    _plant(monkeypatch, defect)
    bad = _mismatches(bd, first=defect != "none")
    assert (not bad) if defect == "none" else bad, defect


@pytest.mark.parametrize("lg,tr,k,col,delta", ENTRY_CASES)
def test_residual_comparison_notices_a_matrix_entry(monkeypatch, lg, tr, k, col, delta):
    """One entry of one size's transform matrix off by one (five entries per size, row 31 of the 32 x 32
    matrix and the DST among them) shows in the impulse pictures of that size."""
    real_tm = O.transform_matrix
    _ref(8)

    def transform_matrix(log2, tr_type):
        t = np.array(real_tm(log2, tr_type))
        if (log2, tr_type) == (lg, tr):
            t[k, col] += delta
        return t

    monkeypatch.setattr(O, "transform_matrix", transform_matrix)
    assert _mismatches(8, only=lambda pic: pic.meta["kind"] == "impulse", first=True)
