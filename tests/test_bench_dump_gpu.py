"""A plain ``bench.py`` run with ``--dump-outputs``: the result line is the headline alone (the legs
that take runs of their own appear only with ``--full``) and the last timed step's outputs are
written as float32 ``.npy`` files.  One tiny run (UNet at 64x64, batch 4): the benchmark's command
line is what this test is about."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "2", "--size", "64",
           "--batch", "4", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["execution"] == "native_plan"
    for leg in ("no_step_sync", "roofline", "doubleconv", "kernels_census_step", "dice_vs_ref", "cpu_baseline"):
        assert leg not in d, leg
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["logits", "loss", "params_sample"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    assert got["logits"].shape == (4, 2, 64, 64) and got["logits"].std() > 0
    assert got["loss"].shape == (1,) and abs(float(got["loss"][0]) - d["last_loss"]) <= 1e-5
    assert got["params_sample"].shape == (1 << 20,) and got["params_sample"].std() > 0
