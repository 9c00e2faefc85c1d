"""The planted SAO set (tests/planted_sao.py) on the GPU through the C ABI, bit-exact against the C oracle, on every
kernel that filters SAO:

  sao_rows_kernel                8 bits, SAO only: the default at CTB 16, P265R_SAO_ROWS=2 at CTB 32 and 64
  sao_strip16_kernel<5>, <6>     8 bits, SAO only: the default at CTB 32 and 64
  loopfilter_kernel<L, false>    8 bits, SAO only, P265R_SAO_ROWS=0
  loopfilter_kernel<L, true>     8 bits, deblocking on at QpY 0 (it changes nothing)
  sao16_strip_kernel             10 and 12 bits, SAO only
  loopfilter16_kernel<L, true>   10 and 12 bits, deblocking on at QpY 0

at CTB 16, 32 and 64 and both values of loop_filter_across_tiles; the window kernels under the per-diagonal and
the row schedule.  A set is decoded as one batch per picture size.  The pre-filter reconstruction must be the
planted planes and the output the C oracle's; the oracle's output differs from the reconstruction in as many
samples of every component as planted_sao.changed_floor counts with the Python oracle, so a comparison of
untouched planes cannot pass.
"""
import numpy as np
import pytest

import planted_sao as S
from p265_amd import records as R
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _ref(bd, lg, lf, dbk):
    key = (bd, lg, lf, dbk)
    if key not in _REF:
        _REF[key] = S.c_decode(bd, lg, lf, S.sao_set(bd, lg, lf, dbk))
    return _REF[key]


def _set_schedule(monkeypatch, schedule):
    monkeypatch.setenv("P265R_SCHEDULE", schedule)
    if schedule == "rows":
        for k, v in ROW_VARIANTS["rows"].items():
            monkeypatch.setenv(k, v)


def _check(recon_mod, bd, lg, lf, dbk, sao_rows=None, schedule=None, keep=None, sparse=False, context=None):
    """Decode the set (the pictures ``keep`` selects) and compare.  ``context``: one ragged batch in a context of
    that size instead of one batch per picture size."""
    pics, ref = S.sao_set(bd, lg, lf, dbk), _ref(bd, lg, lf, dbk)
    idx = [i for i, p in enumerate(pics) if keep is None or keep(p)]
    groups = {context: idx} if context else {size: [i for i in g if i in idx] for size, g in S.by_size(pics).items()}
    changed = [0, 0, 0]
    for (w, h), g in groups.items():
        if not g:
            continue
        with recon_mod.ReconContext(S.params_of(bd, lg, lf, w, h)) as ctx:
            outs, recs = ctx.decode([pics[i] for i in g], with_recon=True, sparse=sparse)
            d = ctx.describe()
        assert sao_rows is None or d["sao_rows"] == sao_rows
        assert schedule is None or d["schedule"] == schedule
        for k, i in enumerate(g):
            for c in range(3):
                label = "bd%d ctb%d lf_tiles=%d dbk=%r c%d %r" % (bd, 1 << lg, lf, dbk, c, pics[i].meta)
                assert outs[k][c].shape == pics[i].planes[c].shape, label
                np.testing.assert_array_equal(recs[k][c], pics[i].planes[c], err_msg="planted " + label)
                np.testing.assert_array_equal(recs[k][c], ref[i][0][c], err_msg="recon " + label)
                np.testing.assert_array_equal(outs[k][c], ref[i][1][c], err_msg="out " + label)
                changed[c] += int((ref[i][1][c] != ref[i][0][c]).sum())
    floor = S.changed_floor(bd, lg, lf, [pics[i] for i in idx])
    assert all(n >= f > 1000 for n, f in zip(changed, floor)), (changed, floor)


@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("lg", S.CTB_LOG2)
def test_sao_rows_kernel(recon_mod, monkeypatch, lg, lf):
    if lg > 4:
        monkeypatch.setenv("P265R_SAO_ROWS", "2")
    _check(recon_mod, 8, lg, lf, False, sao_rows=2 if lg > 4 else 1)


@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("lg", [5, 6])
def test_sao_strip16_kernel(recon_mod, lg, lf):
    _check(recon_mod, 8, lg, lf, False, sao_rows=1)


@pytest.mark.parametrize("schedule", ["steps", "rows"])
@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("lg", S.CTB_LOG2)
def test_window_kernel_sao_only(recon_mod, monkeypatch, lg, lf, schedule):
    _set_schedule(monkeypatch, schedule)
    monkeypatch.setenv("P265R_SAO_ROWS", "0")
    _check(recon_mod, 8, lg, lf, False, sao_rows=0, schedule=schedule)


@pytest.mark.parametrize("schedule", ["steps", "rows"])
@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("lg", S.CTB_LOG2)
@pytest.mark.parametrize("bd", S.DEPTHS)
def test_window_kernels_with_deblocking(recon_mod, monkeypatch, bd, lg, lf, schedule):
    _set_schedule(monkeypatch, schedule)
    _check(recon_mod, bd, lg, lf, True, schedule=schedule)


@pytest.mark.parametrize("lf", [0, 1])
@pytest.mark.parametrize("lg", S.CTB_LOG2)
@pytest.mark.parametrize("bd", [10, 12])
def test_sao16_strip_kernel(recon_mod, bd, lg, lf):
    _check(recon_mod, bd, lg, lf, False)


@pytest.mark.parametrize("bd,lg", [(8, 5), (10, 4), (12, 6)])
def test_ragged_batch(recon_mod, bd, lg):
    """The whole set (the 3 x 3-CTB ``borders`` pictures, the 128 x 128 and 136 x 128 ones, the ``strips``) as one
    batch of a context as wide as the strips and as high as the highest picture: every picture is filtered at
    its own size (pic_geo in strip_pos)."""
    w, h, _ = S.strip_size(bd, lg)
    _check(recon_mod, bd, lg, 0, False, context=(w, max(h, 128, 3 << lg)))


@pytest.mark.parametrize("bd", [8, 10])
def test_sparse_upload(recon_mod, bd):
    """The SAO inputs do not depend on the upload path: the ``edge`` and ``band`` pictures through
    upload(sparse=True)."""
    _check(recon_mod, bd, 5, 1, False, keep=lambda p: p.meta["kind"] in ("edge", "band", "mix"), sparse=True)


def test_height_must_be_a_multiple_of_8(recon_mod):
    """launch_loop_filters sends a height that is no multiple of 8 to sao_rows_kernel, but no context has one:
    the set has no such picture because none can exist."""
    from p265_amd import _lib
    with pytest.raises((_lib.P265RError, R.RecordError, ValueError)):
        recon_mod.ReconContext(S.params_of(8, 5, 1, 2008, 68))
