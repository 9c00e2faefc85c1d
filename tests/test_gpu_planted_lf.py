"""The planted deblocking set (tests/planted_lf.py) on the GPU through the C ABI, bit-exact against the C oracle:
every decision threshold, clip, table end, QpY and edge rule of tests/test_planted_lf.py, in the 8-bit and the
16-bit loop-filter kernels (8, 10 and 12 bits), at CTB 16, 32 and 64, with SAO off and with the SAO twin of the
pictures (edge offset, classes rotating per CTU, the largest offsets: the fused kernels' SAO then reads deblocked
samples across CTB borders), under the per-diagonal and the row schedule.  Every set (one context: bit depth,
CTB size, pps chroma QP offsets, loop_filter_across_tiles) is decoded as one batch.
"""
import numpy as np
import pytest

import planted_lf as L
from oracle import c_oracle
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
_REF = {}


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _ref(bd, ctb_log2, variant, sao):
    key = (bd, ctb_log2, variant, sao)
    if key not in _REF:
        _REF[key] = c_oracle.decode(L.params_of(bd, ctb_log2, variant, sao), L.lf_set(bd, ctb_log2, variant, sao), threads=8)
    return _REF[key]


@pytest.mark.parametrize("schedule", ["steps", "rows"])
@pytest.mark.parametrize("sao", [False, True], ids=["nosao", "sao"])
@pytest.mark.parametrize("ctb_log2", L.CTB_LOG2)
@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_deblocking(recon_mod, monkeypatch, bd, ctb_log2, sao, schedule):
    monkeypatch.setenv("P265R_SCHEDULE", schedule)
    if schedule == "rows":
        for k, v in ROW_VARIANTS["rows"].items():
            monkeypatch.setenv(k, v)
    for variant in L.VARIANTS:
        pics, ref = L.lf_set(bd, ctb_log2, variant, sao), _ref(bd, ctb_log2, variant, sao)
        with recon_mod.ReconContext(L.params_of(bd, ctb_log2, variant, sao)) as ctx:
            outs, recs = ctx.decode(pics, with_recon=True)
            assert ctx.describe()["schedule"] == schedule
        changed = 0
        for k, pic in enumerate(pics):
            for c in range(3):
                label = "bd%d ctb%d %s sao=%r %s c%d %r" % (bd, 1 << ctb_log2, variant, sao, schedule, c, pic.meta)
                np.testing.assert_array_equal(recs[k][c], ref[k][0][c], err_msg="recon " + label)
                np.testing.assert_array_equal(outs[k][c], ref[k][1][c], err_msg="out " + label)
                changed += int((ref[k][1][c] != ref[k][0][c]).sum())
        assert changed > 10000                      # the filters did run
