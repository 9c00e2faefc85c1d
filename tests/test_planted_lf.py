"""The planted deblocking set (tests/planted_lf.py) on the CPU.

  * the deblocking input of the PCM pictures is exactly the planted planes;
  * the C twin equals the Python oracle on the whole set (every bit depth, CTB size and variant), and with the
    SAO twin of the pictures at one of them;
  * coverage: O.deblock_luma_segment, O.deblock_chroma_line and O.chroma_tc are wrapped by a recorder that
    classifies every call's arguments into cells and calls the real function; every cell of LUMA_CELLS occurs
    per direction, CTB size and bit depth, and so do every chroma cell, every QpY and every qPi cell;
  * the edge rules (8.7.2.3), from the records against the oracle's output on block-constant pictures, which any
    filtering changes;
  * sensitivity: the Python oracle with one defect planted no longer equals the C twin on the set.
"""
import inspect

import numpy as np
import pytest

import planted_lf as L
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import records as R

DEPTHS = (8, 10, 12)

STRONG_CLIPS = ["strong_%s_%s" % (s, e) for s in ("p0", "p2", "q0", "q2") for e in ("hi", "lo")]
CLIP1 = ["clip1_%s_%s" % (s, e) for s in ("p0", "q0", "p1", "q1") for e in ("0", "max")]
LUMA_CELLS = (["d_below", "d_at", "beta0", "tc0", "a_below", "a_at", "a_eq", "b_below", "b_at", "c_below", "c_at",
               "strong_l0_only", "strong_l3_only", "strong_unclipped", "delta_10tc_m1", "delta_10tc", "delta_clip_hi",
               "delta_clip_lo", "de_11", "de_10", "de_01", "de_00", "dp_clip_hi", "dp_clip_lo", "dq_clip_hi",
               "dq_clip_lo", "qp_odd_sum", "beta_idx_lo", "beta_idx_hi", "tc_idx_lo", "tc_idx_hi", "nf_p", "nf_q",
               "nf_both"] + STRONG_CLIPS + CLIP1)
QPI_CELLS = ["neg", "lt30", "ge43"] + list(range(30, 43))
CHROMA_CELLS = ["tc0", "delta_unclipped", "delta_clip_hi", "delta_clip_lo", "clip1_0", "clip1_max", "nf_p", "nf_q",
                "nf_both"]


def _c3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def classify_luma(p, q, qp_p, qp_q, boff, toff, no_p, no_q, bd, moved=(True, True)):
    """The cells one call of deblock_luma_segment sits in (8.7.2.5.3 / .6 / .7 restated for the bookkeeping only:
    the samples come from the real function).

    a / b / c are the three conditions of the strong decision: 2 * dpq < beta >> 2, |p3 - p0| + |q0 - q3| <
    beta >> 3, |p0 - q0| < (5 tC + 1) >> 1.  ``x_below``: the other two hold on lines 0 and 3 and x's left
    side, at its larger line, is the largest value below the threshold it can take; ``x_at``: the smallest at or
    above it.  For b and c those are threshold - 1 and threshold.  a's left side 2 * dpq is even: where beta >> 2
    is odd they are threshold - 1 and threshold + 1, where it is even threshold - 2 and threshold.  ``a_m1`` and
    ``a_eq`` are the exact cases 2 * dpq == threshold - 1 and == threshold (the other two conditions holding),
    the first asked for at 8 and 10 bits only: above 10 bits beta is a multiple of 16, beta >> 2 a multiple of
    four, and an even 2 * dpq cannot be threshold - 1.

    ``moved``: whether the filter without the no-filter flags moves a sample on the (P, Q) side; a no-filter
    cell counts only where its flag keeps a sample from moving."""
    cells = set()
    p = [[int(v) for v in r] for r in p]
    q = [[int(v) for v in r] for r in q]
    sc, mx = 1 << (bd - 8), (1 << bd) - 1
    qpl = (qp_q + qp_p + 1) >> 1
    ib, it = qpl + 2 * boff, qpl + 2 + 2 * toff
    cells |= {"beta_idx_lo"} if ib < 0 else set()
    cells |= {"beta_idx_hi"} if ib > 51 else set()
    cells |= {"tc_idx_lo"} if it < 0 else set()
    cells |= {"tc_idx_hi"} if it > 53 else set()
    beta, tc = O.BETA_TABLE[_c3(0, 51, ib)] * sc, O.TC_TABLE[_c3(0, 53, it)] * sc
    cells |= {("qp", int(qp_p)), ("qp", int(qp_q))}
    if qp_p != qp_q and (qp_p + qp_q) & 1:
        cells.add("qp_odd_sum")
    dpk = {k: abs(p[2][k] - 2 * p[1][k] + p[0][k]) for k in (0, 3)}
    dqk = {k: abs(q[2][k] - 2 * q[1][k] + q[0][k]) for k in (0, 3)}
    d = dpk[0] + dpk[3] + dqk[0] + dqk[3]
    if beta == 0:
        return cells | {"beta0"}
    cells |= {"d_below"} if d == beta - 1 else set()
    cells |= {"d_at"} if d == beta else set()
    if d >= beta:
        return cells
    if tc == 0:
        return cells | {"tc0"}
    if no_p and no_q:
        cells |= {"nf_both"} if (moved[0] and moved[1]) else set()
    elif no_p or no_q:
        cells |= {"nf_p" if no_p else "nf_q"} if moved[0 if no_p else 1] else set()
    lhs = {"a": [2 * (dpk[k] + dqk[k]) for k in (0, 3)],
           "b": [abs(p[3][k] - p[0][k]) + abs(q[0][k] - q[3][k]) for k in (0, 3)],
           "c": [abs(p[0][k] - q[0][k]) for k in (0, 3)]}
    thr = {"a": beta >> 2, "b": beta >> 3, "c": (5 * tc + 1) >> 1}
    holds = {x: [v < thr[x] for v in lhs[x]] for x in lhs}
    for x in lhs:
        if all(all(holds[o]) for o in lhs if o != x):
            lo, hi = L._tight(thr[x], x == "a")
            cells |= {x + "_below"} if max(lhs[x]) == lo and lo >= 0 else set()
            cells |= {x + "_at"} if max(lhs[x]) == hi else set()
            if x == "a":
                cells |= {"a_m1"} if max(lhs[x]) == thr[x] - 1 else set()
                cells |= {"a_eq"} if max(lhs[x]) == thr[x] else set()
    s0, s3 = all(holds[x][0] for x in lhs), all(holds[x][1] for x in lhs)
    cells |= {"strong_l0_only"} if s0 and not s3 else set()
    cells |= {"strong_l3_only"} if s3 and not s0 else set()
    side = (beta + (beta >> 1)) >> 3
    dp, dq = dpk[0] + dpk[3], dqk[0] + dqk[3]
    dep, deq = dp < side, dq < side
    if not (s0 and s3) and dp in (side - 1, side) and dq in (side - 1, side):
        cells.add("de_%d%d" % (dep, deq))
    for k in range(4):
        p0, p1, p2, p3 = (p[i][k] for i in range(4))
        q0, q1, q2, q3 = (q[i][k] for i in range(4))
        if s0 and s3:
            raw = {"p0": (p0, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3), "p1": (p1, (p2 + p1 + p0 + q0 + 2) >> 2),
                   "p2": (p2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3),
                   "q0": (q0, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3), "q1": (q1, (p0 + q0 + q1 + q2 + 2) >> 2),
                   "q2": (q2, (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3)}
            for name, (old, new) in raw.items():
                if new > old + 2 * tc:
                    cells.add("strong_%s_hi" % name)
                elif new < old - 2 * tc:
                    cells.add("strong_%s_lo" % name)
                elif new != old:
                    cells.add("strong_unclipped")
            continue
        delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
        cells |= {"delta_10tc_m1"} if abs(delta) == 10 * tc - 1 else set()
        cells |= {"delta_10tc"} if abs(delta) == 10 * tc else set()
        if abs(delta) >= 10 * tc:
            continue
        cells |= {"delta_clip_hi"} if delta > tc else set()
        cells |= {"delta_clip_lo"} if delta < -tc else set()
        delta = _c3(-tc, tc, delta)
        for name, v in (("p0", p0 + delta), ("q0", q0 - delta)):
            cells |= {"clip1_%s_max" % name} if v > mx else set()
            cells |= {"clip1_%s_0" % name} if v < 0 else set()
        for name, on, a2, a1, a0, dl in (("p", dep, p2, p1, p0, delta), ("q", deq, q2, q1, q0, -delta)):
            if on:
                r = (((a2 + a0 + 1) >> 1) - a1 + dl) >> 1
                cells |= {"d%s_clip_hi" % name} if r > (tc >> 1) else set()
                cells |= {"d%s_clip_lo" % name} if r < -(tc >> 1) else set()
                v = a1 + _c3(-(tc >> 1), tc >> 1, r)
                cells |= {"clip1_%s1_max" % name} if v > mx else set()
                cells |= {"clip1_%s1_0" % name} if v < 0 else set()
    return cells


class Recorder:
    """Wraps the oracle's three deblocking functions: classifies the arguments, then calls the real function.
    The direction comes from deblock_picture itself, recompiled with one line added that notes which pass its
    loop is in."""

    def __init__(self, monkeypatch):
        self.luma, self.chroma, self.qpi = set(), set(), set()
        self.real = (O.deblock_luma_segment, O.deblock_chroma_line, O.chroma_tc)
        monkeypatch.setattr(O, "deblock_luma_segment", self._luma)
        monkeypatch.setattr(O, "deblock_chroma_line", self._line)
        monkeypatch.setattr(O, "chroma_tc", self._tc)
        loop = "    for vertical in (True, False):\n"
        src = inspect.getsource(O.deblock_picture)
        assert src.count(loop) == 1
        ns = dict(O.__dict__, _note_pass=self._pass)             # (the wrappers above included)
        exec(compile(src.replace(loop, loop + "        _note_pass(vertical)\n"), "<recorder>", "exec"), ns)
        monkeypatch.setattr(O, "deblock_picture", ns["deblock_picture"])
        self.dir, self.c_off = None, 0

    def _pass(self, vertical):
        self.dir = "v" if vertical else "h"

    def _luma(self, p, q, qp_p, qp_q, boff, toff, no_p, no_q, bit_depth=8, bs=2):
        moved = (True, True)
        if no_p or no_q:
            fp, fq = self.real[0](p, q, qp_p, qp_q, boff, toff, False, False, bit_depth, bs)
            moved = ([list(map(int, r)) for r in p] != fp, [list(map(int, r)) for r in q] != fq)
        self.luma |= {(self.dir, c) for c in classify_luma(p, q, qp_p, qp_q, boff, toff, no_p, no_q, bit_depth, moved)}
        return self.real[0](p, q, qp_p, qp_q, boff, toff, no_p, no_q, bit_depth, bs)

    def _tc(self, qp_p, qp_q, c_off, tc_off, bit_depth=8):
        self.c_off = c_off
        qpi = ((qp_q + qp_p + 1) >> 1) + c_off
        self.qpi.add((self.dir, "neg" if qpi < 0 else "lt30" if qpi < 30 else "ge43" if qpi >= 43 else qpi))
        tc = self.real[2](qp_p, qp_q, c_off, tc_off, bit_depth)
        if tc == 0:
            self.chroma.add((self.dir, c_off, "tc0"))
        return tc

    def _line(self, p0, p1, q0, q1, tc, no_p, no_q, bit_depth=8):
        mx, key = (1 << bit_depth) - 1, (self.dir, self.c_off)
        raw = ((((int(q0) - int(p0)) << 2) + int(p1) - int(q1) + 4) >> 3)
        if tc > 0:
            self.chroma.add(key + ("delta_clip_hi" if raw > tc else "delta_clip_lo" if raw < -tc else
                                   "delta_unclipped" if raw else "delta_zero",))
            dl = _c3(-tc, tc, raw)
            if not no_p and not no_q:
                if p0 + dl > mx or q0 - dl > mx:
                    self.chroma.add(key + ("clip1_max",))
                if p0 + dl < 0 or q0 - dl < 0:
                    self.chroma.add(key + ("clip1_0",))
            if (no_p or no_q) and dl:
                self.chroma.add(key + ("nf_both" if (no_p and no_q) else "nf_p" if no_p else "nf_q",))
        return self.real[1](p0, p1, q0, q1, tc, no_p, no_q, bit_depth)


_REF = {}


def _ref(bd, ctb_log2, variant, sao=False):
    """The C twin's (recon, out) planes of one set."""
    key = (bd, ctb_log2, variant, sao)
    if key not in _REF:
        _REF[key] = c_oracle.decode(L.params_of(bd, ctb_log2, variant, sao), L.lf_set(bd, ctb_log2, variant, sao), threads=8)
    return _REF[key]


def _py(bd, ctb_log2, variant, pic, sao=False):
    return O.decode_picture(R.params_dict(L.params_of(bd, ctb_log2, variant, sao)), pic.as_oracle_dict())


@pytest.mark.parametrize("ctb_log2", L.CTB_LOG2)
@pytest.mark.parametrize("bd", DEPTHS)
def test_lf_set_oracles_and_coverage(monkeypatch, bd, ctb_log2):
    """One Python decode of every picture of the three variants' sets, under the recorder: the deblocking input is
    the planted planes, the C twin's output equals the Python oracle's, and every cell occurs."""
    rec = Recorder(monkeypatch)
    for variant in L.VARIANTS:
        pics, ref = L.lf_set(bd, ctb_log2, variant), _ref(bd, ctb_log2, variant)
        kinds = [p.meta["kind"] for p in pics]
        assert kinds.count("cells") == L.N_CELLS and kinds.count("rules") == L.N_RULES and kinds.count("grid8") == 1
        assert kinds.count("grid32") == (ctb_log2 >= 5) and kinds.count("nxn") == (variant == "a")
        for k, pic in enumerate(pics):
            assert (pic.tbs["flags"] & R.TB_PCM != 0).all() == (pic.meta["kind"] != "nxn")
            recon, out = _py(bd, ctb_log2, variant, pic)
            for c in range(3):
                if pic.planes is not None:
                    np.testing.assert_array_equal(recon[c], pic.planes[c], err_msg="planted c%d %r" % (c, pic.meta))
                np.testing.assert_array_equal(ref[k][0][c], recon[c], err_msg="recon c%d %r" % (c, pic.meta))
                np.testing.assert_array_equal(ref[k][1][c], out[c], err_msg="out c%d %r" % (c, pic.meta))
    for direction in ("v", "h"):
        missing = [c for c in LUMA_CELLS if (direction, c) not in rec.luma]
        assert not missing, "luma %s bd%d ctb%d: %s" % (direction, bd, 1 << ctb_log2, missing)
        for c_off in (-12, 0, 12):
            missing = [c for c in CHROMA_CELLS if (direction, c_off, c) not in rec.chroma]
            assert not missing, "chroma %s offset %d bd%d ctb%d: %s" % (direction, c_off, bd, 1 << ctb_log2, missing)
        if bd <= 10:
            assert (direction, "a_m1") in rec.luma, "luma %s bd%d ctb%d: a_m1" % (direction, bd, 1 << ctb_log2)
        missing = [c for c in QPI_CELLS if (direction, c) not in rec.qpi]
        assert not missing, "qPi %s bd%d ctb%d: %s" % (direction, bd, 1 << ctb_log2, missing)
        qps = {c[1] for d, c in rec.luma if d == direction and isinstance(c, tuple)}
        assert qps == set(range(-6 * (bd - 8), 52)), (direction, sorted(set(range(-6 * (bd - 8), 52)) - qps))


def test_lf_set_with_sao_twin():
    """The SAO twin of a set (edge offset, classes rotating per CTU, the largest offsets): C twin == Python."""
    for bd, ctb_log2, variant in ((8, 5, "b"), (10, 4, "a")):
        pics, ref = L.lf_set(bd, ctb_log2, variant, sao=True), _ref(bd, ctb_log2, variant, True)
        base = _ref(bd, ctb_log2, variant)
        changed = 0
        for k, pic in enumerate(pics):
            assert (pic.ctus["sao_type"] == 2).all() and set(pic.ctus["sao_class"][:, 0].tolist()) == {0, 1, 2, 3}
            _, out = _py(bd, ctb_log2, variant, pic, sao=True)
            for c in range(3):
                np.testing.assert_array_equal(ref[k][1][c], out[c], err_msg="out c%d %r" % (c, pic.meta))
                changed += int((ref[k][1][c] != base[k][1][c]).sum())
        assert changed > 1000


# ---------------------------------------------------------------------------------
# edge rules, from the records against the oracle's output
# ---------------------------------------------------------------------------------

def _edge_rule(spec, lf_tiles, xp, yp, xq, yq):
    """(filtered?, the rules that say so) of the luma edge between p0 and q0 by 8.7.2.3, from the picture's spec
    (Q is the CTU holding q0, the current one; ``border``: P lies in another CTU)."""
    vertical = yp == yq
    if (xq if vertical else yq) % spec.cu:
        return False, {"inside_cu"}
    a, b = spec.ctu_of(xq, yq), spec.ctu_of(xp, yp)
    where = "border" if a != b else "inside"
    if not spec.dbk[a]:
        return False, {"dbk_off_q_" + where} | ({"dbk_off_q_on_p"} if spec.dbk[b] else set())
    if spec.nf[yp // spec.cu, xp // spec.cu] and spec.nf[yq // spec.cu, xq // spec.cu]:
        return False, {"nf_both"}
    tags = {"plain_" + where}
    if a != b:
        tags |= {"dbk_on_q_off_p"} if not spec.dbk[b] else set()
        tags |= {"offsets_differ"} if spec.off[a] != spec.off[b] and spec.dbk[b] else set()
        if spec.tile[a] != spec.tile[b]:
            if not lf_tiles:
                return False, {"tile_off"}
            tags.add("tile_on")
        if (spec.tile[a], spec.slice[a]) != (spec.tile[b], spec.slice[b]):
            if not spec.lf_across[a]:
                return False, {"slice_off"}
            tags.add("slice_on")
    return True, tags


RULES = ("inside_cu", "plain_border", "plain_inside", "slice_on", "slice_off", "tile_on", "tile_off", "dbk_off_q_border",
         "dbk_off_q_inside", "dbk_off_q_on_p", "dbk_on_q_off_p", "offsets_differ", "nf_both")


@pytest.mark.parametrize("ctb_log2", L.CTB_LOG2)
@pytest.mark.parametrize("bd", DEPTHS)
def test_edge_rules(bd, ctb_log2):
    """On the block-constant ``rules`` pictures every filtered edge moves p0 or q0 and nothing else moves them:
    the oracle's output says which edges it filtered, in a row (column) the other pass leaves alone.  They are
    the edges 8.7.2.3 names: none inside a CU, none on the picture boundary, at a slice boundary by the
    slice_loop_filter_across_slices of Q's slice, at a tile boundary by loop_filter_across_tiles, none where
    Q's slice has deblocking off (whatever P's has) and all where only P's has, at a CTB border and inside a
    CTB.  Every rule occurs in either direction at every CTB size and bit depth (the 8-bit and the 16-bit
    loop-filter and edge-map kernels)."""
    seen = set()
    for variant in L.VARIANTS:
        lf_tiles = L.VARIANTS[variant]["lf_tiles"]
        ref = _ref(bd, ctb_log2, variant)
        for k, pic in enumerate(L.lf_set(bd, ctb_log2, variant)):
            if pic.meta["kind"] != "rules":
                continue
            spec, Y, out = pic.spec, pic.planes[0], ref[k][1][0].astype(np.int64)
            assert np.array_equal(out[3::8, [0, L.W - 1]], Y[3::8, [0, L.W - 1]])          # picture boundary
            assert np.array_equal(out[[0, L.H - 1], 3::8], Y[[0, L.H - 1], 3::8])
            for e in range(8, L.W, 8):
                for r in range(3, L.H, 8):
                    for direction, (xp, yp, xq, yq) in (("v", (e - 1, r, e, r)), ("h", (r, e - 1, r, e))):
                        want, tags = _edge_rule(spec, lf_tiles, xp, yp, xq, yq)
                        got = out[yp, xp] != Y[yp, xp] or out[yq, xq] != Y[yq, xq]
                        assert got == want, (pic.meta, direction, e, r, tags)
                        seen |= {(direction, t) for t in tags}
    want = {(d, r) for d in ("v", "h") for r in RULES}
    assert seen >= want, sorted(want - seen)


@pytest.mark.parametrize("bd", DEPTHS)
def test_inside_cu_and_chroma_grid(bd):
    """No edge inside a 16 x 16 or 32 x 32 PCM CU although the planted samples there would be filtered (the
    vertical recipes sit on every 8-sample line), no edge at the 4-sample offsets of NxN CUs' TBs although edges
    at the 8-sample ones move samples, and chroma is filtered at luma 0 mod 16 only although luma is at 8 mod 16."""
    for ctb_log2 in L.CTB_LOG2:
        ref = _ref(bd, ctb_log2, "a")
        for k, pic in enumerate(L.lf_set(bd, ctb_log2, "a")):
            rec, out = [[p.astype(np.int64) for p in ref[k][j]] for j in (0, 1)]
            cu, kind = pic.meta["cu"], pic.meta["kind"]
            diff = [out[c] != rec[c] for c in range(3)]
            if kind in ("cells", "grid32"):
                inside = [x for e in range(8, L.W, 8) if e % cu for x in range(e - 3, e + 3)]
                rows = [r for r in range(L.H) if 3 <= r % cu < cu - 3]       # clear of the horizontal pass
                assert not diff[0][np.ix_(rows, inside)].any(), pic.meta
                assert diff[0][rows].any()
            if kind == "nxn":
                off4 = [x for x in range(L.W) if x % 8 in (3, 4)]
                assert not diff[0][np.ix_(off4, off4)].any() and diff[0].any()
            if kind == "grid8":
                rows = [r for r in range(L.H // 2) if 1 <= r % 8 <= 6]
                at8 = [x for x in range(L.W // 2) if x % 8 in (3, 4)]
                for c in (1, 2):
                    assert not diff[c][np.ix_(rows, at8)].any() and diff[c][rows].any(), pic.meta
                assert diff[0][3::8, 8::16].any()


# ---------------------------------------------------------------------------------
# sensitivity: the comparison fails an oracle with a planted defect
# ---------------------------------------------------------------------------------

def _patched(fn, *subs):
    """``fn`` recompiled from its source with text replaced (each ``old`` must occur)."""
    src = inspect.getsource(fn)
    for old, new in subs:
        assert old in src, old
        src = src.replace(old, new)
    ns = dict(O.__dict__)
    exec(compile(src, "<defect>", "exec"), ns)
    return ns[fn.__name__]


DEFECTS = {
    "none": ("deblock_luma_segment", [("if d >= beta:", "if not d < beta:")], 8),
    "d_le_beta": ("deblock_luma_segment", [("if d >= beta:", "if d > beta:")], 8),
    "no_bit_depth_scale": ("deblock_luma_segment", [("* (1 << (bit_depth - 8))", "* 1")], 10),
    "de_threshold_without_half_beta": ("deblock_luma_segment", [("(beta + (beta >> 1)) >> 3", "beta >> 3")], 8),
    "strong_clip_tc": ("deblock_luma_segment", [("2 * tc", "tc")], 8),
    "no_clip1": ("deblock_luma_segment", [("_clip3(0, maxv, ", "(lambda lo, hi, v: v)(0, maxv, ")], 8),
    "qpl_without_plus_one": ("deblock_luma_segment", [("qpl = (qp_q + qp_p + 1) >> 1", "qpl = (qp_q + qp_p) >> 1")], 8),
    "offsets_from_p": ("deblock_picture", [('_unpack_offsets(ctus[geo.ctb_of(xq, yq)]["deblock_offsets"])',
                                            '_unpack_offsets(ctus[geo.ctb_of(xp, yp)]["deblock_offsets"])'),
                                           ('_unpack_offsets(ctus[geo.ctb_of(*lq)]["deblock_offsets"])',
                                            '_unpack_offsets(ctus[geo.ctb_of(*lp)]["deblock_offsets"])')], 8),
    "chroma_tc_without_table": ("chroma_tc", [("qpc_from_qpi(", "(lambda v: v)(")], 8),
    "chroma_edge_at_8_mod_16": ("deblock_picture", [("for e in range(8, e_max, 8):\n                for s0 in range(0, s_max, 4):\n                    xq, yq = ((e, s0)",
                                                     "for e in range(4, e_max, 4):\n                for s0 in range(0, s_max, 4):\n                    xq, yq = ((e, s0)")], 8),
    "horizontal_before_vertical": ("deblock_picture", [("for vertical in (True, False):", "for vertical in (False, True):")], 8),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_lf_comparison_notices_defects(monkeypatch, defect):
    """Each defect planted into the Python oracle breaks its equality with the C twin on the set at CTB 32
    (the bit-depth scaling at 10 bits); the recompiled function without a defect does not."""
    name, subs, bd = DEFECTS[defect]
    monkeypatch.setattr(O, name, _patched(getattr(O, name), *subs))
    bad = []
    for variant in L.VARIANTS:
        ref = _ref(bd, 5, variant)
        for k, pic in enumerate(L.lf_set(bd, 5, variant)):
            _, out = _py(bd, 5, variant, pic)
            if any(not np.array_equal(out[c], ref[k][1][c]) for c in range(3)):
                bad.append(pic.meta)
                break
        if bad or defect == "none" and variant == "a":
            break
    assert (not bad) if defect == "none" else bad, defect
