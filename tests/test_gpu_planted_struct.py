"""The planted structure set (tests/planted_struct.py) on the GPU through the C ABI, bit-exact against the C oracle,
and the job counts of intra_prep_kernel against the host model (planted_struct.expected_jobs).

  parity   8 / 10 / 12 bits x CTB 16 / 32 / 64 under the schedules that select other kernels or job paths: the set
           as one batch (whole pictures per workgroup, the bench's layout), the ``edges`` pictures as a ragged batch;
  latency  8 bits: batches of num_cus / 2 pictures (component split, W = 16 by run) and of num_cus / (2 xg) (the
           cross-group kernel, with P265R_TR_CHECK=1 in three variants: a wrong `tr` or `br` then fails parity on
           every run, not by timing);
  counts   ctx.job_count(batch) equals the model's sums under P265R_QUAD 3 / 1 / 4, one batch per family and one
           per picture for ``counts`` and ``quads``, the pictures cut by the picture edge in contexts of their own size;
  sparse   the all-4x4 CTB 64 pictures and ``counts`` through the sparse upload.

The C oracle's planes are computed once per (bit depth, CTB size).
"""
import numpy as np
import pytest

import planted_struct as S
from oracle import c_oracle
from p265_amd import records as R
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
CTBS = (4, 5, 6)
SCHEDULES = ("steps", "rows", "rows12", "rows_nosplit", "rows_quad1", "rows_noquad", "rows_lead0")
QUAD_BITS = {"rows": 3, "rows_quad1": 1, "rows_noquad": 4}


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


class _Expect:
    """The set of one (bit depth, CTB size): the 3 x 2 CTB pictures, the ``edges`` pictures (ragged, in a 3 x 3 CTB
    context) and the C oracle's planes."""

    def __init__(self, bd, lg):
        pics = S.struct_set(bd, lg)
        self.main = [p for p in pics if not S.is_ragged(p)]
        self.edges = [p for p in pics if S.is_ragged(p)]          # ``edges`` and the 8-wide columns of ``adjacent``
        self.params, self.eparams = S.set_params(bd, lg), S.set_params(bd, lg, edges=True)
        self.ref = {}
        for group, prm in ((self.main, self.params), (self.edges, self.eparams)):
            for p, (rec, out) in zip(group, c_oracle.decode(prm, group, threads=8)):
                assert all(np.array_equal(rec[c], out[c]) for c in range(3))   # no in-loop filter is on
                self.ref[id(p)] = rec
        self.stack = [np.stack([self.ref[id(p)][c] for p in self.main]) for c in range(3)]
        self.index = {id(p): i for i, p in enumerate(self.main)}

    def check(self, pics, outs, recs, label):
        """Reconstruction and output of ``pics`` (any of the set) against the C oracle; the message names the
        picture's family and cell."""
        for name, got in (("recon", recs), ("out", outs)):
            if got is None:
                continue
            if all(id(p) in self.index for p in pics):
                idx = [self.index[id(p)] for p in pics]
                for c in range(3):
                    g, want = np.stack([x[c] for x in got]), self.stack[c][idx]
                    if not np.array_equal(g, want):
                        i = int(np.nonzero((g != want).reshape(len(idx), -1).any(axis=1))[0][0])
                        np.testing.assert_array_equal(g[i], want[i], err_msg="%s %s c%d %s: %s (%s order)" % (
                            label, name, c, pics[i].meta["family"], pics[i].meta["cell"], pics[i].meta["order"]))
            else:
                for p, x in zip(pics, got):
                    for c in range(3):
                        np.testing.assert_array_equal(x[c], self.ref[id(p)][c], err_msg="%s %s c%d %s: %s" % (
                            label, name, c, p.meta["family"], p.meta["cell"]))


_EXPECT = {}


def _expect(bd, lg):
    if (bd, lg) not in _EXPECT:
        _EXPECT[(bd, lg)] = _Expect(bd, lg)
    return _EXPECT[(bd, lg)]


def _set_schedule(monkeypatch, schedule):
    if schedule == "steps":
        monkeypatch.setenv("P265R_SCHEDULE", "steps")
    else:
        monkeypatch.setenv("P265R_SCHEDULE", "rows")
        for k, v in ROW_VARIANTS[schedule].items():
            monkeypatch.setenv(k, v)


def _run(ctx, groups):
    """Decode the batches in one context -> (outs, recs, layout of every batch's row launch)."""
    outs, recs, layouts = [], [], []
    before = ctx.describe()["row_launches"]
    for g in groups:
        o, r = ctx.decode(g, with_recon=True)
        outs += o
        recs += r
        d = ctx.describe()
        kind = [k for k in d["row_launches"] if d["row_launches"][k] != before[k]]
        before = d["row_launches"]
        layouts.append(("xg" if d["last_launch_xg"] else "split" if d["last_launch_split"] else "whole", tuple(kind)))
    return outs, recs, layouts


def _chunks(pics, n):
    return [pics[i:i + n] for i in range(0, len(pics), n)]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("lg", CTBS)
@pytest.mark.parametrize("bd", DEPTHS)
def test_struct_parity(recon_mod, monkeypatch, bd, lg, schedule):
    """The set as one batch (whole pictures per workgroup, not ragged), then the ``edges`` pictures as a ragged
    batch in the wider context."""
    e = _expect(bd, lg)
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        # launch_rows_w splits a batch by component while 2 n_pics <= workgroups per CU x num_cus; a CU holds at
        # most four W = 8 workgroups, so the set is repeated until it passes 2 num_cus pictures
        batch = e.main * (2 * int(ctx.describe()["num_cus"]) // len(e.main) + 1)
        outs, recs, layouts = _run(ctx, [batch])
        d = ctx.describe()
    assert d["schedule"] == ("steps" if schedule == "steps" else "rows") and d["bit_depth"] == bd
    if schedule == "steps":
        assert not any(d["row_launches"].values())
    else:
        assert len(batch) > 2 * d["num_cus"]
        assert layouts[0][0] == "whole" and len(layouts[0][1]) == 1, layouts
    e.check(batch, outs, recs, "bd%d ctb%d %s" % (bd, 1 << lg, schedule))
    with recon_mod.ReconContext(e.eparams) as ctx:
        outs, recs, elay = _run(ctx, [e.edges])
        d = ctx.describe()
    if schedule == "steps":
        assert not any(d["row_launches"].values())
    else:               # a few pictures: a workgroup per component, unless P265R_SPLIT=0 keeps whole pictures
        assert 2 * len(e.edges) <= d["num_cus"]
        assert elay[0][0] == ("whole" if ROW_VARIANTS[schedule].get("P265R_SPLIT") == "0" else "split"), elay
        assert len(elay[0][1]) == 1, elay
    e.check(e.edges, outs, recs, "bd%d ctb%d %s ragged" % (bd, 1 << lg, schedule))
    print("struct bd%d ctb%d %s: %d + %d pictures, layouts %s %s" % (bd, 1 << lg, schedule, len(e.main), len(e.edges), layouts, elay))


LATENCY = {"split": ("rows_auto", 1), "rows_w16": ("rows_w16", 1), "rows_auto": ("rows_auto", 0),
           "rows_xgchk": ("rows_xgchk", 0), "rows_xg2": ("rows_xg2", 0), "rows_xg8": ("rows_xg8", 0)}


@pytest.mark.parametrize("variant", sorted(LATENCY))
@pytest.mark.parametrize("lg", CTBS)
def test_struct_latency_layouts(recon_mod, monkeypatch, lg, variant):
    """8 bits, the whole set in small batches: num_cus / 2 pictures (component split; the W = 16 kernel by run and
    under P265R_XG=0) and num_cus / (2 xg) (cross-group chains; xgchk / xg2 / xg8 with P265R_TR_CHECK=1)."""
    e = _expect(8, lg)
    schedule, split = LATENCY[variant]
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        d = ctx.describe()
        if split:
            n = int(d["num_cus"]) // 2
        else:
            assert d["xg"] > 0
            n = int(d["num_cus"]) // (2 * int(d["xg"]))
        groups = _chunks(e.main, n)
        outs, recs, layouts = _run(ctx, groups)
        d = ctx.describe()
    full = [l for l, g in zip(layouts, groups) if len(g) == n]      # (a shorter last batch may take another layout)
    assert full
    if split:
        assert {k for k, _ in full} == {"split"}, sorted(set(layouts))
        assert {k for _, k in full} == {("w16_split",)}, sorted(set(layouts))       # (8 bits: the W = 16 kernel)
    else:
        assert set(layouts) == {("xg", ("xg",))}, sorted(set(layouts))
        assert d["row_launches"]["xg"] == len(groups)
    print("struct ctb%d %s: %d batches of %d, layouts %s" % (1 << lg, variant, len(groups), n, sorted(set(layouts))))
    e.check(e.main, outs, recs, "ctb%d %s" % (1 << lg, variant))


@pytest.mark.parametrize("schedule", sorted(QUAD_BITS))
@pytest.mark.parametrize("lg", CTBS)
def test_struct_job_counts(recon_mod, monkeypatch, lg, schedule):
    """(luma, chroma) jobs after preparation equal the model's, exactly: one batch per family, one per picture
    for ``counts`` and ``quads`` (a mismatch names the case).  p265r_batch_job_count sums the context's CTU slots, of
    which a smaller picture fills only the front, so the pictures cut by the picture edge (``edges`` and the 8-wide
    columns of ``adjacent``) are counted in a context of their own size, one batch per size."""
    e = _expect(8, lg)
    quad = QUAD_BITS[schedule]
    _set_schedule(monkeypatch, schedule)
    batches = []
    for fam in S.FAMILIES:
        pics = [p for p in e.main if p.meta["family"] == fam]
        if fam in ("counts", "quads"):
            seen = set()
            for p in pics:                                   # (one per structure: the model sees no more)
                if S.structure_key(p) not in seen:
                    seen.add(S.structure_key(p))
                    batches.append(("%s: %s (%s order)" % (fam, p.meta["cell"], p.meta["order"]), [p]))
        elif pics:
            batches.append((fam, pics))
    by_size = {}
    for p in e.edges:
        by_size.setdefault(tuple(p.size), []).append(p)
    groups = [(e.params, batches)] + [(R.pic_params(e.eparams, pics[0]), [("%s %dx%d" % ((pics[0].meta["family"],) + size), pics)])
                                      for size, pics in sorted(by_size.items())]
    for params, todo in groups:
        with recon_mod.ReconContext(params) as ctx:
            assert ctx.describe()["schedule"] == "rows"
            for label, pics in todo:
                b = ctx.upload(pics)
                try:
                    ctx.run(b)
                    got = ctx.job_count(b)
                finally:
                    b.free()
                assert got == S.job_sums(params, pics, quad), "ctb%d P265R_QUAD=%d %s" % (1 << lg, quad, label)


@pytest.mark.parametrize("schedule", ("rows", "rows_noquad"))
def test_struct_sparse_upload(recon_mod, monkeypatch, schedule):
    """The all-4x4 CTB 64 pictures and ``counts`` through the sparse upload (the quad codes depend on its packing):
    parity and job counts."""
    e = _expect(8, 6)
    pics = [p for p in e.main if p.meta["family"] == "counts" or
            (p.meta["family"] == "tiling" and p.meta["kind"] in ("nxn", "s4"))]
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        b = ctx.upload(pics, sparse=True)
        try:
            ctx.run(b)
            outs, recs = ctx.download(b, with_recon=True)
            got = ctx.job_count(b)
        finally:
            b.free()
    e.check(pics, outs, recs, "sparse %s" % schedule)
    assert got == S.job_sums(e.params, pics, QUAD_BITS[schedule])
