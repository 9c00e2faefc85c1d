"""The planted residual set (tests/planted.py residual_set) on the GPU through the C ABI, bit-exact against the
C oracle: every (class, ky, kx) impulse, every qP', the saturating extremes, transform skip and bypass, at 8, 10
and 12 bits, through the dense and the sparse coefficient upload, under the per-diagonal and the row schedule,
in sub-batches whose TB count per residual job class sits around the kernels' TBs-per-block, and in contexts
with scaling lists.  tests/test_planted_residual.py pins the C oracle's planes to the Python oracle's residual
on the CPU; they are computed once per bit depth and table here.
"""
import numpy as np
import pytest

import planted as P
from oracle import c_oracle
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
SCHEDULES = ("steps", "rows")


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


class _Expect:
    """The set of one bit depth (``table``: its scaled pictures under a ScalingFactor table) and the C oracle's
    reconstruction planes, stacked per plane (every picture is 128 x 128)."""

    def __init__(self, bd, table):
        self.sf = None if table is None else P.scaling_tables()[table]
        self.params = P.set_params(bd, table is not None)
        self.pics = [pic for _, pic in P.residual_set(bd) if table is None or pic.meta["scaled"]]
        assert all(tuple(p.size) == (P.MAX_W, P.MAX_H) for p in self.pics)
        ref = c_oracle.decode(self.params, self.pics, threads=8, scaling=self.sf)
        self.stack = [np.stack([r[0][c] for r in ref]) for c in range(3)]
        for c in range(3):                  # no in-loop filter is on: the output is the reconstruction
            assert all(np.array_equal(r[1][c], r[0][c]) for r in ref)

    def check(self, outs, recs, label, idx=None):
        idx = list(range(len(self.pics))) if idx is None else idx
        for name, got in (("recon", recs), ("out", outs)):
            for c in range(3):
                g, want = np.stack([p[c] for p in got]), self.stack[c][idx]
                if not np.array_equal(g, want):
                    i = int(np.nonzero((g != want).reshape(len(idx), -1).any(axis=1))[0][0])
                    np.testing.assert_array_equal(g[i], want[i], err_msg="%s %s c%d picture %d of the batch %r" % (
                        label, name, c, i, self.pics[idx[i]].meta))


_EXPECT = {}


def _expect(bd, table=None):
    if (bd, table) not in _EXPECT:
        _EXPECT[(bd, table)] = _Expect(bd, table)
    return _EXPECT[(bd, table)]


def _set_schedule(monkeypatch, schedule):
    monkeypatch.setenv("P265R_SCHEDULE", "steps" if schedule == "steps" else "rows")
    if schedule != "steps":
        for k, v in ROW_VARIANTS[schedule].items():
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_residual_set(recon_mod, monkeypatch, bd, schedule, sparse):
    """The whole set as one batch."""
    e = _expect(bd)
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        outs, recs = ctx.decode(e.pics, with_recon=True, sparse=sparse)
        d = ctx.describe()
    assert d["schedule"] == schedule and d["bit_depth"] == bd
    e.check(outs, recs, "bd%d %s sparse=%r" % (bd, schedule, sparse))


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("table", ["random", "corners", "all255"])
@pytest.mark.parametrize("bd", DEPTHS)
def test_residual_set_scaling_lists(recon_mod, monkeypatch, bd, table, schedule, sparse):
    """The qP sweep and the extremes in a context with scaling lists: random factors, 1 with 255 at DC and
    at (N - 1, N - 1), and 255 everywhere."""
    e = _expect(bd, table)
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params, scaling=e.sf) as ctx:
        outs, recs = ctx.decode(e.pics, with_recon=True, sparse=sparse)
    e.check(outs, recs, "bd%d %s %s sparse=%r" % (bd, table, schedule, sparse))


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_residual_job_count_batches(recon_mod, monkeypatch, bd, schedule, sparse):
    """Sub-batches with 1, TPB - 1, TPB and TPB + 1 TBs of one residual job class (TPB = 256 / N TBs per block,
    256 at 4x4): residualN_kernel's inactive TBs and residual4_kernel's tail."""
    e = _expect(bd)
    _set_schedule(monkeypatch, schedule)
    with recon_mod.ReconContext(e.params) as ctx:
        for cls, n, idx in P.job_count_batches(bd):
            outs, recs = ctx.decode([e.pics[i] for i in idx], with_recon=True, sparse=sparse)
            e.check(outs, recs, "bd%d %s sparse=%r: %d TBs of %s" % (bd, schedule, sparse, n, cls), idx)
