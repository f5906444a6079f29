"""The importance prune through the product: `gaussian_train` on a synthetic spec of 2000 splats, 64x48, 4 cameras, 30 iterations, with
--refineStopIter 10 --pruneEvery 20 so that exactly one prune occasion (iteration 20) falls inside, and --importancePrune 30.
The log carries `importance prune @20: a -> b` with b = a - a * 30 / 100, the saved PLY holds b finite splats and training runs to the
end; the same command without the flag prints no such line and keeps its count. Two runs with the flag at 16x12 (one tile: the size at
which tests/test_gpu_render_views.py relies on run-to-run repeatability) save byte-identical PLYs, and the two replicas of a two-rank
run (TCP test backend, DVS_SAVE_ALL_RANKS=1, the pattern of tests/test_gpu_multirank.py) are identical after the step that pruned."""
import os
import re
import subprocess
import numpy as np
import pytest
from test_gpu_multirank import DRIVER, _plugin_run, _read_ply_rows

pytestmark = pytest.mark.gpu
STEPS = 30
LINE = r"importance prune @(\d+): (\d+) -> (\d+) splats, (\d+) views, (\d+) never taken, score [\d.]+ ms, select\+compact [\d.]+ ms"


def args(w, h, *extra):
    return ["--inputPath", f"synthetic:N=2000,W={w},H={h},cams=4,sh=1,seed=5", "--maxIteration", str(STEPS), "--densifyStrategy", "0",
            "--refineStopIter", "10", "--pruneEvery", "20"] + list(extra)


def run(tmp, tag, argv):
    out = os.path.join(str(tmp), tag, "it")
    env = {k: v for k, v in os.environ.items() if k != "DVS_IMPORTANCE_PRUNE"}
    p = subprocess.run([DRIVER] + argv + ["--outputPath", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return out, p.stdout, p.stderr


def test_one_prune_occasion_removes_thirty_percent(gpu_device, tmp_path):
    out, so, log = run(tmp_path, "on", args(64, 48, "--importancePrune", "30"))
    found = re.findall(LINE, log)
    assert len(found) == 1, log[-3000:]
    it, a, b, views, never = (int(v) for v in found[0])
    assert it == 20 and views == 4 and 0 < a <= 2000 and b == a - a * 30 // 100 and 0 <= never <= a
    assert re.search(r"config: importancePrune 30: ", log)
    rows = _read_ply_rows(out + f"_{STEPS}.ply")
    assert rows.shape == (b, 59) and np.isfinite(rows).all()
    assert "Train Done" in so

    out0, so0, log0 = run(tmp_path, "off", args(64, 48))
    assert "importance prune" not in log0 and "importancePrune" not in log0
    light = re.findall(r"light prune @20: (\d+) -> (\d+) splats", log0)
    assert _read_ply_rows(out0 + f"_{STEPS}.ply").shape[0] == (int(light[0][1]) if light else 2000)


def test_the_environment_variable_overrides_and_clamps(gpu_device, tmp_path):
    out = os.path.join(str(tmp_path), "env", "it")
    p = subprocess.run([DRIVER] + args(16, 12, "--importancePrune", "10") + ["--outputPath", out], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DVS_IMPORTANCE_PRUNE="95"))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    assert "config: importancePrune 95 clamped to 90" in p.stderr
    it, a, b = (int(v) for v in re.findall(LINE, p.stderr)[0][:3])
    assert b == a - a * 90 // 100 and _read_ply_rows(out + f"_{STEPS}.ply").shape[0] == b


def test_two_runs_at_one_tile_save_identical_models(gpu_device, tmp_path):
    files = []
    for tag in ("a", "b"):
        out, _, log = run(tmp_path, tag, args(16, 12, "--importancePrune", "30"))
        assert len(re.findall(LINE, log)) == 1
        files.append(open(out + f"_{STEPS}.ply", "rb").read())
    assert files[0] == files[1] and len(files[0]) > 1000


def test_two_ranks_stay_identical_through_a_prune(gpu_device, tmp_path):
    out, res = _plugin_run(tmp_path, "w2", args(64, 48, "--importancePrune", "30"), 2, timeout=300)
    found = re.findall(LINE, res[0][2])
    assert len(found) == 1 and int(found[0][0]) == 20, res[0][2][-3000:]
    assert "importance prune" not in res[1][2]                       # rank 0 alone logs
    a, b = open(out + f"_{STEPS}.ply", "rb").read(), open(out + f"_{STEPS}.ply.rank1", "rb").read()
    assert a == b, "the two replicas differ"
    assert _read_ply_rows(out + f"_{STEPS}.ply").shape[0] == int(found[0][2])
