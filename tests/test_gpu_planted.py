"""The planted-TB set (tests/planted.py) on the GPU through the C ABI, bit-exact against the C oracle.

Every (component, size, mode, neighbour pattern) cell and the value edges of tests/test_planted.py, at 8, 10 and
12 bits (the uint8_t, uint16_t and int16_t instances of the row kernel), under the schedules that select
different kernels or job paths, and in the three row layouts launch_rows (p265_amd/csrc/p265r.hip) chooses by
batch size against the CU count:

  large  one batch of the whole set (far more pictures than workgroups fit: the bench's layout, no split);
  mid    batches of num_cus / 2 pictures: a picture's luma and chroma chains on two workgroups (component
         split; at 8 bits with the row build chosen by run, the W = 16 kernel);
  small  batches of num_cus / (2 xg) pictures: every chain on xg workgroups (cross-group kernel).  It exists at
         8 bits only and only while the row build is chosen by run (launch_rows), so it runs under rows_auto.

The pictures planted from the reference's chain vectors ride along; their target blocks are also compared with
the committed reference output directly, with no oracle in between.  The C oracle's planes are computed once per
bit depth.
"""
import numpy as np
import pytest

import planted as P
from oracle import c_oracle
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
SCHEDULES = ("steps", "rows", "rows12", "rows_auto", "rows_nosplit", "rows_quad1", "rows_noquad")


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


class _Expect:
    """The set of one bit depth: pictures (full-size ones first, then the narrower ``tr_missing`` ones, which
    make a batch ragged), the C oracle's planes, stacked per plane for the full-size pictures, and the chain
    pictures' reference blocks."""

    def __init__(self, bd):
        chain = P.chain_set(bd)
        pics = [pic for _, pic in P.planted_set(bd)] + [pic for _, pic, _ in chain]
        want = {id(pic): out for _, pic, out in chain}
        full = [p for p in pics if tuple(p.size) == (P.MAX_W, P.MAX_H)]
        self.n_full = len(full)
        self.pics = full + [p for p in pics if tuple(p.size) != (P.MAX_W, P.MAX_H)]
        self.params = P.set_params(bd)
        ref = c_oracle.decode(self.params, self.pics, threads=8)
        self.stack = [np.stack([ref[i][0][c] for i in range(self.n_full)]) for c in range(3)]
        for c in range(3):                  # no in-loop filter is on: the output is the reconstruction
            assert all(np.array_equal(ref[i][1][c], ref[i][0][c]) for i in range(len(self.pics)))
        self.rest = [ref[i][0] for i in range(self.n_full, len(self.pics))]
        self.chain = [(i, P.chain_region(p), want[id(p)]) for i, p in enumerate(self.pics) if id(p) in want]
        assert len(self.chain) == len(chain)

    def check(self, outs, recs, label):
        for name, got in (("recon", recs), ("out", outs)):
            for c in range(3):
                g = np.stack([got[i][c] for i in range(self.n_full)])
                if not np.array_equal(g, self.stack[c]):
                    i = int(np.nonzero((g != self.stack[c]).reshape(self.n_full, -1).any(axis=1))[0][0])
                    np.testing.assert_array_equal(g[i], self.stack[c][i],
                                                  err_msg="%s %s c%d %r" % (label, name, c, self.pics[i].meta))
                for k, ref in enumerate(self.rest):
                    np.testing.assert_array_equal(got[self.n_full + k][c], ref[c], err_msg="%s %s c%d %r" % (
                        label, name, c, self.pics[self.n_full + k].meta))
        for i, (ys, xs), want in self.chain:
            np.testing.assert_array_equal(recs[i][0][ys, xs], want, err_msg="%s reference block %r" % (label, self.pics[i].meta))


_EXPECT = {}


def _expect(bd):
    if bd not in _EXPECT:
        _EXPECT[bd] = _Expect(bd)
    return _EXPECT[bd]


def _set_schedule(monkeypatch, schedule):
    if schedule == "steps":
        monkeypatch.setenv("P265R_SCHEDULE", "steps")
    else:
        monkeypatch.setenv("P265R_SCHEDULE", "rows")
        for k, v in ROW_VARIANTS[schedule].items():
            monkeypatch.setenv(k, v)


def _run(recon_mod, e, groups):
    """Decode the set as the given batches in one context -> (outs, recs, layout of every batch's row launch)."""
    outs, recs, layouts = [], [], []
    with recon_mod.ReconContext(e.params) as ctx:
        before = ctx.describe()["row_launches"]
        for g in groups:
            o, r = ctx.decode(g, with_recon=True)
            outs += o
            recs += r
            d = ctx.describe()
            kind = [k for k in d["row_launches"] if d["row_launches"][k] != before[k]]
            before = d["row_launches"]
            layouts.append(("xg" if d["last_launch_xg"] else "split" if d["last_launch_split"] else "whole", tuple(kind)))
        d = ctx.describe()
    return outs, recs, layouts, d


def _chunks(pics, n):
    return [pics[i:i + n] for i in range(0, len(pics), n)]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_large_batch(recon_mod, monkeypatch, bd, schedule):
    """The full-size pictures as one batch (the bench's layout: whole pictures per workgroup, not ragged), the
    narrower ones as a ragged batch of their own."""
    e = _expect(bd)
    _set_schedule(monkeypatch, schedule)
    outs, recs, layouts, d = _run(recon_mod, e, [e.pics[:e.n_full], e.pics[e.n_full:]])
    assert d["schedule"] == ("steps" if schedule == "steps" else "rows") and d["bit_depth"] == bd
    if schedule == "steps":
        assert not any(d["row_launches"].values())
    else:
        assert layouts[0][0] == "whole" and len(layouts[0][1]) == 1, layouts
        assert e.n_full > 2 * d["num_cus"]
    print("planted large bd%d %s: %d + %d pictures, layouts %s" % (bd, schedule, e.n_full, len(e.pics) - e.n_full, layouts))
    e.check(outs, recs, "large bd%d %s" % (bd, schedule))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_component_split_batches(recon_mod, monkeypatch, bd, schedule):
    """Batches of num_cus / 2 pictures: 2 * n_pics <= num_cus, the component-split threshold of launch_rows_w
    (one workgroup per CU suffices) and of the W = 16 kernel.  rows_nosplit (P265R_SPLIT=0) keeps whole
    pictures per workgroup at this batch size; the per-diagonal schedule has no row launch."""
    e = _expect(bd)
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        n = int(ctx.describe()["num_cus"]) // 2
    groups = _chunks(e.pics, n)
    outs, recs, layouts, d = _run(recon_mod, e, groups)
    first = layouts[0]
    if schedule == "steps":
        assert not any(d["row_launches"].values())
    elif schedule == "rows_nosplit":
        assert first[0] == "whole", layouts
    else:
        assert first[0] == "split", layouts
        if bd == 8 and schedule == "rows_auto":
            assert first[1] == ("w16_split",), layouts
    print("planted mid bd%d %s: %d batches of %d, layouts %s" % (bd, schedule, len(groups), n, sorted(set(layouts))))
    e.check(outs, recs, "mid bd%d %s" % (bd, schedule))


def test_planted_cross_group_batches(recon_mod, monkeypatch):
    """Batches of num_cus / (2 xg) pictures at 8 bits with the row build chosen by run: every batch runs the
    cross-group kernel (2 * n_pics * xg <= num_cus)."""
    e = _expect(8)
    _set_schedule(monkeypatch, "rows_auto")
    with recon_mod.ReconContext(e.params) as ctx:
        d = ctx.describe()
    assert d["xg"] > 0
    n = int(d["num_cus"]) // (2 * int(d["xg"]))
    groups = _chunks(e.pics, n)
    outs, recs, layouts, d = _run(recon_mod, e, groups)
    assert set(layouts) == {("xg", ("xg",))}, sorted(set(layouts))
    assert d["row_launches"]["xg"] == len(groups)
    print("planted small bd8 rows_auto: %d batches of %d, layouts %s" % (len(groups), n, sorted(set(layouts))))
    e.check(outs, recs, "small bd8 rows_auto")
