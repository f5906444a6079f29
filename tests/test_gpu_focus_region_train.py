"""The focus region through the product: `gaussian_train --enableFocusRegion 1` on the synthetic scene N=2000, W=64, H=48, cams=4, sh=1.

Region runs (one per densification strategy, 30 steps with --warmupLength 10 --refineEvery 20: one refinement at step 20): the box is
turned by --focusRotation 0,0,0.3 and cut at the median local x of the generating centres, so that tests/region_ref.py finds between
30 % and 70 % of them inside. Every centre of the saved PLY is inside the box in float64 (centres within 1e-5 (hi - lo) of a face are
not judged), the count is above 0 and below 2000, a `region prune @` line and the `config: focusRegion` line are logged, enableFocusRegion
is absent from the IGNORED line, the run exits 0. The ADC run also holds out camera 0 (--eval) and writes a mesh (--meshResolution 32):
the mesh's logged bounds are the world bounds of the region's eight corners and every vertex lies inside them plus one voxel.
Evaluation: the renders the evaluation scores are not retrievable (the written renders are JPEG files), so the weaker of the two checks
is made: the logged PSNR of the region run differs from that of the same run without the flag.
A box around everything: the same scene at one tile (W=16, H=12 in the spec — a synthetic scene is not resized by --maxImageWidth 16,
which is passed all the same), the size at which tests/test_gpu_render_views.py already relies on run-to-run repeatability, with a box
far larger than the scene and all cameras inside: the saved PLY is byte-identical to the run without the flag."""
import os
import re
import subprocess
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import region
import region_ref as RR
import mesh_ref as MR
from test_gpu_multirank import DRIVER, _read_ply_rows

pytestmark = pytest.mark.gpu
N, STEPS, ROT = 2000, 30, (0.0, 0.0, 0.3)
SCENE = "synthetic:N=2000,W=64,H=48,cams=4,sh=1,seed=5"
SMALL = "synthetic:N=2000,W=16,H=12,cams=4,sh=1,seed=5"
SCHEDULE = ["--warmupLength", "10", "--refineEvery", "20"]


def box():
    """(lo, hi) as the strings' float32 values: local bounds of the generating centres under ROT, widened by 1, cut at the median local x"""
    P = dv.synth_splats(dv.make_spec(N, 64, 48, sh_degree=1, n_cams=4, seed=5))["pos"]
    w2b, _ = RR.from_trs((0, 0, 0), ROT, (1, 1, 1))
    c = RR.local(P, w2b)
    lo, hi = c.min(0) - 1.0, c.max(0) + 1.0
    hi[0] = np.median(c[:, 0])
    text = ",".join(f"{v:.6f}" for v in list(lo) + list(hi))
    v = np.array([float(t) for t in text.split(",")], np.float32)
    return text, v[:3], v[3:], P


def run(scene, out, *extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DVS_FOCUS_", "DVS_MESH_"))}
    p = subprocess.run([DRIVER, "--inputPath", scene, "--maxIteration", str(STEPS), "--outputPath", out] + SCHEDULE + list(extra), capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return p.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("focus"))
    text, lo, hi, P = box()
    flags = ["--enableFocusRegion", "1", "--focusRegion", text, "--focusRotation", ",".join(str(v) for v in ROT)]
    out = {k: os.path.join(tmp, k, "it") for k in ("adc", "mcmc", "plain")}
    logs = dict(adc=run(SCENE, out["adc"], "--densifyStrategy", "0", "--eval", "--meshResolution", "32", *flags),
                mcmc=run(SCENE, out["mcmc"], "--densifyStrategy", "1", *flags),
                plain=run(SCENE, out["plain"], "--densifyStrategy", "0", "--eval"))
    return dict(out=out, logs=logs, lo=lo, hi=hi, P=P)


def test_the_box_holds_about_half_of_the_initial_centres(runs):
    reg, _ = region.region_from_trs((0, 0, 0), ROT, (1, 1, 1), runs["lo"], runs["hi"])
    _, _, count, _ = RR.plan(runs["P"], list(reg.w2b), runs["lo"], runs["hi"])
    assert 0.3 * N <= count <= 0.7 * N, count


@pytest.mark.parametrize("strategy", ["adc", "mcmc"])
def test_region_run_saves_only_inside_splats(runs, strategy):
    log = runs["logs"][strategy]
    assert re.search(r"region prune @\d+: \d+ -> \d+ splats", log), log[-3000:]
    assert re.search(r"region prune @0: 2000 -> \d+ splats", log), log[-3000:]           # right after load
    assert "config: focusRegion box " in log
    assert all("enableFocusRegion" not in line for line in re.findall(r"config: IGNORED by this build:(.*)", log))
    assert re.search(r"(densify|mcmc) @20: \d+ -> \d+ splats", log), log[-3000:]          # the refinement ran
    rows = _read_ply_rows(runs["out"][strategy] + f"_{STEPS}.ply")
    assert 0 < len(rows) < N
    reg, _ = region.region_from_trs((0, 0, 0), ROT, (1, 1, 1), runs["lo"], runs["hi"])
    action, _, count, near = RR.plan(rows[:, :3], list(reg.w2b), runs["lo"], runs["hi"], 1e-5)
    print(f"{strategy}: {len(rows)} splats saved, {int(near.sum())} within the band of a face")
    assert (action[~near] == RR.KEEP).all(), int((action[~near] != RR.KEEP).sum())


def test_evaluation_sees_the_region(runs):
    def psnr(log):
        m = re.search(rf"eval @{STEPS}: 1 views, PSNR ([-\d.e+]+) dB", log)
        assert m, log[-3000:]
        return float(m.group(1))
    a, b = psnr(runs["logs"]["adc"]), psnr(runs["logs"]["plain"])
    print(f"held-out PSNR {a:.4f} dB with the region, {b:.4f} dB without")
    assert np.isfinite(a) and a != b
    assert os.path.exists(runs["out"]["adc"] + f"_{STEPS}_eval.json")


def test_mesh_takes_the_region_bounds(runs):
    log = runs["logs"]["adc"]
    xyz, _, tri = MR.parse_mesh_ply(runs["out"]["adc"] + f"_{STEPS}_mesh.ply")
    m = re.findall(rf"mesh @{STEPS}: (\d+) vertices, (\d+) triangles, grid \d+x\d+x\d+, voxel (\S+), bounds ([^ ]+)[ ,]", log)
    assert m, log[-3000:]
    voxel = float(m[-1][2].rstrip(","))
    logged = np.array([float(v) for v in m[-1][3].rstrip(",").split(",")])
    _, F = RR.from_trs((0, 0, 0), ROT, (1, 1, 1))
    corners = np.array([[(runs["lo"], runs["hi"])[(c >> k) & 1][k] for k in range(3)] for c in range(8)], np.float64)
    world = corners @ F[:3, :3].T + F[:3, 3]
    want = np.concatenate([world.min(0), world.max(0)])
    tol = 1e-5 * np.abs(want).max()                             # (the log's upper corner is the grid's last voxel centre: at most one voxel past the box)
    assert np.abs(logged[:3] - want[:3]).max() <= tol and (logged[3:] >= want[3:] - tol).all() and (logged[3:] <= want[3:] + voxel + tol).all(), (logged, want)
    print(f"mesh: {len(xyz)} vertices, {len(tri)} triangles, voxel {voxel}")
    if len(xyz):
        assert (xyz >= want[:3] - voxel - 1e-5).all() and (xyz <= want[3:] + voxel + 1e-5).all()


def test_a_box_around_everything_changes_nothing(tmp_path):
    on, off = str(tmp_path / "on" / "it"), str(tmp_path / "off" / "it")
    log_on = run(SMALL, on, "--maxImageWidth", "16", "--enableFocusRegion", "1", "--focusRegion", "-1000,-1000,-1000,1000,1000,1000")
    log_off = run(SMALL, off, "--maxImageWidth", "16")
    assert "config: focusRegion box " in log_on and "focusRegion" not in log_off and "region prune" not in log_on
    a, b = open(on + f"_{STEPS}.ply", "rb").read(), open(off + f"_{STEPS}.ply", "rb").read()
    assert len(a) > 1000 and a == b
