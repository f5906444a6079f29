"""bench.py's plain command line: one headline JSON line for exactly --steps timed steps, and --dump-outputs writing what the last
timed step computed (rendered views and gradient rows) within its 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_are_fixed_and_within_budget(tmp_path):
    """CPU: an array above its share of the budget is written as the same seeded sample every time; a small one whole."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = {"big": torch.rand(20_000_000, generator=g), "small": torch.rand(1000, 3, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"].numpy())
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.ndim == 1 and big.size == bench.DUMP_BUDGET_BYTES // 4 // 2
    assert np.isin(big, arrays["big"].numpy()).all()                     # a sample of the array's own elements
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64_000_000


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "C1",
           "--dump-outputs", str(dump_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_headline_and_dumps_last_step(gpu_device, tmp_path):
    rec = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "views/s" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] > 0 and len(rec["step_ms_p10_p50_p90"]) == 3
    assert abs(rec["value"] - rec["config"]["views_per_step"] * 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"]
    assert not rec["full"] and "roofline" not in rec and "cpu_baseline" not in rec       # side measurements are --full only
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(["rgb", "grad_pos", "grad_scale", "grad_rot", "grad_opacity", "grad_sh0", "grad_shN", "grad_absgrad2d"])
    rgb = np.load(tmp_path / "a" / "rgb.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (8, 3, 256, 256) and np.isfinite(rgb).all() and rgb.max() > 0
    gpos = np.load(tmp_path / "a" / "grad_pos.npy")
    assert gpos.shape == (10_000, 3) and np.isfinite(gpos).all() and np.abs(gpos).max() > 0
    # same arguments, same inputs: a second run renders the same views
    _plain_run(tmp_path / "b")
    assert np.allclose(np.load(tmp_path / "b" / "rgb.npy"), rgb, rtol=1e-5, atol=1e-6)
