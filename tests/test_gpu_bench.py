"""A plain `bench.py --gpus 1 --steps K --warmup W` run (MI355X): the result line carries the
headline figure and only what the timed region itself measured, --steps sets the number of
timed steps, and --dump-outputs writes the last timed step's outputs.  What takes work outside
the timed steps (`cpu_baseline`, `mfma`, the figures read from the committed profiles) is
`--full`'s, off by default."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["metric"].startswith("train samples/sec")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["roofline"]["launches"] == 3   # one pair launch per timed step
    assert out["ms_per_step"] > 0 and out["dtype"].startswith("bf16 MFMA")
    assert math.isclose(out["value"], 256 / (out["ms_per_step"] * 1e-3), rel_tol=1e-3)
    for k in ("cpu_baseline", "mfma", "hbm_kernels", "lstm"):
        assert k not in out, k
    assert out["roofline"]["traffic"] is None
    man = json.load(open(dump / "manifest.json"))
    got = {k: np.load(dump / (k + ".npy")) for k in man}
    assert sum(os.path.getsize(dump / (k + ".npy")) for k in man) <= 64_000_000
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    for k, v in out["elbo"].items():           # the dumped losses are the last timed step's
        assert got[k].shape == () and math.isclose(float(got[k]), v, rel_tol=0, abs_tol=1e-6), k
    assert man["params"]["sampled"] and man["params"]["shape"][0] > got["params"].size == 4 << 20
    assert np.abs(got["params"]).max() > 0
