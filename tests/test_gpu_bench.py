"""bench.py on the GPU box: a plain run (set up, warm up, timed steps, the line) and --dump-outputs.

One small run in a child process: the line carries the headline fields and none of the --full legs, and the
dumped planes -- what the last timed step left in its batch -- equal the C oracle's decode of the same seeded
pictures."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_prints_the_headline_and_dumps_the_last_steps_planes(tmp_path):
    steps, frames = 3, 6
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--frames", str(frames), "--unique", "2"]
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE") and not k.startswith("P265R_")}
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "CTU/s" and d["higher_is_better"] is True and d["dtype"].startswith("u8")
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - frames * 510 * steps / (d["ms_per_step"] * steps * 1e-3)) <= 2e-3 * d["value"]
    for leg in ("verified", "roofline", "phases_ms_per_step", "cpu_baseline", "cpu_baseline_c", "pcie", "end_to_end"):
        assert leg not in d, leg
    # the dump: every picture of the small batch, float32, equal to the oracle's decode of the same records
    b = _bench()
    (params, pics), = b.build_workload(b.parse(args), 0, 1)[0]
    idx = b.pictures_to_dump([1920 * 1080 * 3 // 2] * frames)      # six 1080p pictures exceed the budget: a sample
    assert len(idx) == 4 and idx[0] == 0 and idx[-1] == frames - 1
    assert d["dumped_outputs"]["pictures"] == [idx] and d["dumped_outputs"]["files"] == 3 * len(idx)
    assert d["dumped_outputs"]["batch_slot"] == (steps - 1) % 2
    assert d["dumped_outputs"]["bytes"] == 4 * len(idx) * 1920 * 1080 * 3 // 2 <= 64 << 20
    uniq = pics[:2]
    ref = [r[1] for r in c_oracle.decode(params, uniq, with_recon=False)]
    assert len(os.listdir(tmp_path)) == 3 * len(idx)
    for i in idx:
        for c, name in enumerate(("y", "cb", "cr")):
            got = np.load(tmp_path / ("ctx0_pic%05d_%s.npy" % (i, name)))
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, ref[i % 2][c].astype(np.float32), err_msg="picture %d %s" % (i, name))
