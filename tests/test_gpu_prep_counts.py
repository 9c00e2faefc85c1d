"""Directed cases for the counts job preparation branches on (p265_amd/csrc/intra_prep.h): how many TB records a CTU
has, how many it keeps once the Cr of every Cb+Cr pair is folded into its Cb, and where pairs, unpaired chroma TBs
and 4x4 quads sit relative to the 64-record chunks and the 64-slot emission windows.

A CTU of CTB 64 is tiled from 8x8 regions: ``a`` 8x8 CUs, ``b`` NxN CUs (four 4x4 luma TBs) and ``c`` 16x16 CUs (four
regions each).  Every CU lists its luma TBs, then Cb, then Cr, so with m = a + c a CTU has 3 m + 6 b records and keeps
2 m + 5 b (m + 4 b luma, m + b chroma pairs).  With R = a + b + 4 c regions the kept count is 2 R mod 3, so the counts
next to 64, 128 and 192 need CTUs of R = 0, 1 and 2 mod 3: whole CTUs (R = 64: 65, 128, 191) and the last CTU column
of pictures 128 + 48 and 128 + 56 samples wide (R = 48: 63, 129, 192; R = 56: 64, 127, 193).  The record counts of these
CTUs (93 .. 255) cross 64, 128 and 192 at other places than the kept counts do.

Record groups are multiples of three, so a Cb sits at index 1 mod 3: the all-8x8 CTU has the Cb | Cr of its CU 42 at
records 127 | 128.  For 63 | 64 the luma TB of CU 21 is moved behind its Cb and Cr (``rot``: the order inside each
component is unchanged, as in planted_struct.component_major, so the output is the same).  ``split`` moves the luma TB of
the first s CUs between their Cb and Cr: two unpaired chroma TBs instead of one pair, 64 + s chroma entries, and the
chroma quad of the CTU's last 16x16 at slots 60 + s .. 63 + s.  ``lhead`` puts p 8x8 CUs ahead of the NxN ones: luma
quads at slots p, p + 4, ...  The component-major twins have no pairs at all: unpaired Cb and Cr runs that end and
begin at records 64, 128 (all 8x8: the chroma list at its 128-entry cap), and kept = records.  One picture is decoded
without its chroma records (no chroma job), the all-8x8 CTUs have no luma quad.

The full-width pictures put a luma-quad straddle, kept counts 65 and 128 and the 127 | 128 pair at CTU 4, the one CTU
of a 3 x 2 picture whose four neighbour CTUs are usable and which is clear of the picture's edges (prep_avail_clear);
every other CTU takes the generic availability arithmetic.

Asserted: the model's counts of the cases themselves (no GPU); on the GPU the job counts against
planted_struct.expected_jobs under P265R_QUAD 3, 1 and 4 with the planes bit-equal to the C oracle, and the same planes
on the cross-group layout with P265R_TR_CHECK=1 (`tr` and `br`).
"""
import os
import subprocess

import numpy as np
import pytest

import mono as M
import planted_struct as S
from oracle import c_oracle
from p265_amd import records as R
from test_gpu_parity import ROW_VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD_BITS = {"rows": 3, "rows_quad1": 1, "rows_noquad": 4}

# case -> (present width of the CTU, 16x16 CUs, NxN CUs, reorder, kept records, records)
CASES = {
    "k65": (64, 11, 1, None, 65, 96),
    "all8": (64, 0, 0, None, 128, 192),
    "k191": (64, 0, 21, None, 191, 255),
    "rot63": (64, 0, 0, ("rot", 21), 128, 192),
    "csplit1": (64, 0, 0, ("split", 1), 129, 192),
    "csplit2": (64, 0, 0, ("split", 2), 130, 192),
    "csplit3": (64, 0, 0, ("split", 3), 131, 192),
    "lhead61": (64, 0, 3, None, 137, 201),
    "lhead62": (64, 0, 2, None, 134, 198),
    "lhead63": (64, 0, 1, None, 131, 195),
    "p48_63": (48, 6, 1, None, 63, 93),
    "p48_129": (48, 2, 15, None, 129, 171),
    "p48_192": (48, 0, 32, None, 192, 240),
    "p56_64": (56, 8, 0, None, 64, 96),
    "p56_127": (56, 0, 5, None, 127, 183),
    "p56_193": (56, 0, 27, None, 193, 249),
}
# (name, picture width, case per CTU in raster order; the third column is the partial one)
PICTURES = [
    ("A", 176, ["k65", "all8", "p48_63", "k191", "rot63", "p48_129"]),
    ("B", 176, ["csplit1", "csplit2", "p48_192", "csplit3", "lhead61", "p48_63"]),
    ("C", 184, ["lhead62", "lhead63", "p56_64", "k65", "all8", "p56_127"]),
    ("D", 184, ["all8", "k191", "p56_193", "rot63", "k65", "p56_64"]),
    ("E", 192, ["csplit1", "k191", "csplit2", "all8", "lhead61", "rot63"]),
    ("F", 192, ["lhead63", "csplit3", "k191", "lhead62", "k65", "all8"]),
    ("G", 192, ["k65", "rot63", "lhead62", "k191", "all8", "lhead63"]),
]
# CTB 32 (16 regions): 11 NxN + 5 8x8 keep 65 of 81; 10 + 6 keep 62 of 78; all NxN keeps 80 of 96
CASES32 = {"k65": (11, 65, 81), "k62": (10, 62, 78), "nxn": (16, 80, 96), "all8": (0, 32, 48)}
PICTURE32 = ["k65", "k62", "nxn", "all8", "nxn", "k65"]


def _params(bd, lg, size):
    return R.make_params(pic_width=size[0], pic_height=size[1], ctb_log2_size=lg, sample_adaptive_offset=0,
                         bit_depth_luma=bd, bit_depth_chroma=bd)


def _kinds(ctb, present_w, n16, nnxn):
    """Kind of each 8x8 region in z-order: ``n16`` 16x16 CUs in the first aligned blocks that are wholly present,
    ``nnxn`` NxN CUs in the last present regions, 8x8 CUs elsewhere."""
    reg = S._regions8(ctb)
    present = [x < present_w for x, _ in reg]
    kinds = [8] * len(reg)
    for q in range(0, len(reg), 4):
        if n16 and all(present[q:q + 4]):
            kinds[q:q + 4] = [16] * 4
            n16 -= 1
    assert n16 == 0
    free = [k for k in range(len(reg)) if present[k] and kinds[k] == 8]
    for k in (free[-nnxn:] if nnxn else []):
        kinds[k] = "nxn"
    return kinds


def _reorder(pic, rs, op):
    """``rot``: [Y, Cb, Cr] of CU k of an all-8x8 CTU -> [Cb, Cr, Y]; ``split``: the first s CUs -> [Cb, Y, Cr]."""
    b, n = int(pic.ctus[rs]["tb_begin"]), int(pic.ctus[rs]["tb_count"])
    perm = list(range(n))
    kind, k = op
    if kind == "rot":
        perm[3 * k:3 * k + 3] = [3 * k + 1, 3 * k + 2, 3 * k]
    else:
        for i in range(k):
            perm[3 * i:3 * i + 3] = [3 * i + 1, 3 * i, 3 * i + 2]
    seg = pic.tbs[b:b + n].copy()
    assert [int(c) for c in seg["c_idx"][:3]] == [0, 1, 2]
    pic.tbs[b:b + n] = seg[perm]


def _picture(bd, name, width, cases):
    trees = {rs: S._tree_of_regions(64, _kinds(64, *CASES[c][:3])) for rs, c in enumerate(cases)}
    pic = S.build(bd, 6, trees, "cycle", size=(width, 128), seed=9000 + ord(name),
                  meta=dict(family="prep", cell="%s: %s" % (name, " ".join(cases)), cases=cases))
    pic = R.Picture(ctus=pic.ctus, tbs=pic.tbs.copy(), coef=pic.coef, nofilter=pic.nofilter, meta=pic.meta, size=pic.size)
    for rs, c in enumerate(cases):
        if CASES[c][3]:
            _reorder(pic, rs, CASES[c][3])
    return pic


class _Set:
    """The pictures, grouped by the context they decode in, and the C oracle's planes (computed once)."""

    def __init__(self):
        self.groups = []                                           # (label, params, pictures, reference planes)
        by_width = {}
        for name, width, cases in PICTURES:
            p = _picture(8, name, width, cases)
            by_width.setdefault(width, []).extend([p, S.component_major(p)])
        for width, pics in sorted(by_width.items()):
            self.groups.append(("ctb64 w%d" % width, _params(8, 6, (width, 128)), pics))
        trees = {rs: S._tree_of_regions(32, _kinds(32, 32, 0, CASES32[c][0])) for rs, c in enumerate(PICTURE32)}
        p32 = S.build(8, 5, trees, "cycle", seed=9100, meta=dict(family="prep", cell="ctb32", cases=PICTURE32))
        self.groups.append(("ctb32", _params(8, 5, (96, 64)), [p32, S.component_major(p32)]))
        p10 = _picture(10, *PICTURES[4])
        self.groups.append(("10 bits", _params(10, 6, (192, 128)), [p10, S.component_major(p10)]))
        self.groups = [(label, prm, pics, [rec for rec, _ in c_oracle.decode(prm, pics, threads=8)])
                       for label, prm, pics in self.groups]
        # without its chroma records: no CTU has a chroma job (expected: the luma plane of the 4:2:0 picture)
        label, prm, pics, ref = self.groups[2]                     # (the full-width CTB 64 group, picture E)
        self.mono = (M.mono_params(prm), M.to_mono(pics[0]), ref[0][0])


_SET = []


def _set():
    if not _SET:
        _SET.append(_Set())
    return _SET[0]


def test_cases_have_the_counts_they_are_named_for():
    """The model's record, kept, list and head counts of every case (no GPU): the cases are what the GPU tests
    take them for."""
    s = _set()
    seen = set()
    for label, prm, pics, _ in s.groups[:3]:
        for pic in pics:
            exp = S.expected_jobs(prm, pic, 3)
            for rs, case in enumerate(pic.meta["cases"]):
                e, (_, _, _, op, kept, records) = exp[rs], CASES[case]
                assert e["records"] == records, (label, pic.meta["cell"], case)
                if pic.meta["order"] == "cm":
                    assert e["luma_staged"] + e["chroma_staged"] == records and e["chroma_unpaired"] == e["chroma_staged"]
                    if case == "all8":
                        assert e["chroma_staged"] == 128 and e["luma_heads"] == [] and e["chroma_heads"] == []
                    continue
                assert e["luma_staged"] + e["chroma_staged"] == kept, (label, pic.meta["cell"], case)
                seen.add(kept)
                b = int(pic.ctus[rs]["tb_begin"])
                c_at = lambda i: int(pic.tbs[b + i]["c_idx"])
                if case == "all8":
                    assert (c_at(127), c_at(128)) == (1, 2) and e["luma_heads"] == [] and e["chroma_unpaired"] == 0
                    assert e["chroma_heads"] == list(range(0, 64, 4))
                if case == "rot63":
                    assert (c_at(63), c_at(64), c_at(65)) == (1, 2, 0) and e["chroma_unpaired"] == 0
                if op and op[0] == "split":
                    assert e["chroma_unpaired"] == 2 * op[1] and e["chroma_staged"] == 64 + op[1]
                    assert e["chroma_heads"][-1] == 60 + op[1] and len(e["chroma_heads"]) == 15
                if case.startswith("lhead"):
                    assert e["luma_heads"][0] == int(case[5:]) and e["luma_heads"][0] + 3 >= 64
    assert seen >= {63, 64, 65, 127, 128, 129, 191, 192, 193}
    label, prm, pics, _ = s.groups[3]
    for pic in pics[:1]:
        exp = S.expected_jobs(prm, pic, 3)
        for rs, case in enumerate(pic.meta["cases"]):
            assert (exp[rs]["luma_staged"] + exp[rs]["chroma_staged"], exp[rs]["records"]) == CASES32[case][1:]
    mprm, mpic, _ = s.mono
    assert all(e["chroma"] == 0 and e["luma"] > 0 for e in S.expected_jobs(mprm, mpic, 3))


def test_prep_short_cuts_match_the_generic_arithmetic(tmp_path):
    """intra_prep.h: prep_avail_clear == ref_avail_mask32 and the generic run bounds for every TB place of a clear
    CTU, prep_filter_min_lg == the rule of 8.4.4.2.3 (`make prep-check`: tools/prep_check.hip, compiled with hipcc, run on the CPU)."""
    r = subprocess.run(["make", "-s", "-C", ROOT, "prep-check", "PREP_CHECK=" + str(tmp_path / "prep_check")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _set_schedule(monkeypatch, schedule):
    monkeypatch.setenv("P265R_SCHEDULE", "rows")
    for k, v in ROW_VARIANTS[schedule].items():
        monkeypatch.setenv(k, v)


def _check(pics, ref, outs, recs, label):
    for p, want, out, rec in zip(pics, ref, outs, recs):
        for c in range(len(out)):
            for name, got in (("recon", rec), ("out", out)):
                np.testing.assert_array_equal(got[c], want[c], err_msg="%s %s c%d %s (%s order)" % (
                    label, name, c, p.meta["cell"], p.meta["order"]))


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", sorted(QUAD_BITS))
def test_prep_job_counts_and_planes(recon_mod, monkeypatch, schedule):
    """One batch per picture: the job counts equal the model's, the planes the C oracle's."""
    s = _set()
    quad = QUAD_BITS[schedule]
    _set_schedule(monkeypatch, schedule)
    todo = [(label, prm, [p], [r]) for label, prm, pics, ref in s.groups for p, r in zip(pics, ref)]
    todo.append(("mono", s.mono[0], [s.mono[1]], [[s.mono[2]]]))
    ctx, ctx_prm = None, None
    try:
        for label, prm, pics, ref in todo:
            if ctx_prm is not prm:
                if ctx is not None:
                    ctx.close()
                ctx, ctx_prm = recon_mod.ReconContext(prm), prm
            b = ctx.upload(pics)
            try:
                ctx.run(b)
                outs, recs = ctx.download(b, with_recon=True)
                got = ctx.job_count(b)
            finally:
                b.free()
            what = "P265R_QUAD=%d %s %s (%s order)" % (quad, label, pics[0].meta["cell"], pics[0].meta["order"])
            assert got == S.job_sums(prm, pics, quad), what
            _check(pics, ref, outs, recs, what)
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.gpu
def test_prep_cross_group_layout_with_tr_check(recon_mod, monkeypatch):
    """The pictures on the cross-group layout with P265R_TR_CHECK=1: a wrong `tr` or `br` fails parity on every run."""
    s = _set()
    _set_schedule(monkeypatch, "rows_xgchk")
    for label, prm, pics, ref in s.groups:
        with recon_mod.ReconContext(prm) as ctx:
            d = ctx.describe()
            assert d["xg"] > 0
            n = int(d["num_cus"]) // (2 * int(d["xg"]))
            idx = [i % len(pics) for i in range(n)]               # (a full batch: a shorter one may take another layout)
            batch = [pics[i] for i in idx]
            b = ctx.upload(batch)
            try:
                ctx.run(b)
                outs, recs = ctx.download(b, with_recon=True)
                got = ctx.job_count(b)
            finally:
                b.free()
            d = ctx.describe()
        # (16-bit samples have no cross-group kernel, launch_rows: there the run still makes prep check its `br`)
        assert bool(d["last_launch_xg"]) == (d["bit_depth"] == 8), label
        assert got == S.job_sums(prm, batch, 3), label
        _check(batch, [ref[i] for i in idx], outs, recs, "xg tr_check " + label)
