"""The export frame through the plugin, end to end: gaussian_train on a small synthetic scene (2000 splats, 20x12, 8 cameras, SH 2, 20
iterations: the size at which the trainer repeats run to run) with --exportTransform and every export format, the same run without it,
and an --exportOrient +y run. The resume PLY stays in the training frame, .transformed.ply equals the restatement applied to it bit for
bit, the compact files are written and their decoded models scored with finite numbers, and without a flag nothing new is logged."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest
import transform_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
SCENE = ["--inputPath", "synthetic:N=2000,W=20,H=12,cams=8,sh=2", "--maxIteration", "20"]
FORMATS = ["--exportFormat", "compressed,splat,reduced", "--exportSpz", "--eval"]
TRS = "0.5,-1,2,0.3,-0.7,1.1,2.5"


def _run(args):
    e = dict(os.environ)
    for k in ("DVS_EXPORT_FORMATS", "DVS_EXPORT_TRANSFORM", "DVS_EXPORT_ORIENT"):
        e.pop(k, None)
    p = subprocess.run([DRIVER] + SCENE + args, capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("frame")
    on, off, orient = (str(base / t / "iteration") for t in ("on", "off", "orient"))
    p_on = _run(["--outputPath", on, "--exportTransform", TRS, "--exportFormat", "compressed,splat,reduced,transformed", "--exportSpz", "--eval"])
    p_off = _run(["--outputPath", off] + FORMATS)
    p_orient = _run(["--outputPath", orient, "--exportOrient", "+y"])
    return on, p_on, off, p_off, orient, p_orient


def test_resume_ply_is_untouched_and_transformed_ply_is_the_restatement(gpu_device, runs):
    from divshot_amd import transform as X
    from divshot_amd._lib import read_ply
    on, p_on, off = runs[0], runs[1], runs[2]
    assert open(on + "_20.ply", "rb").read() == open(off + "_20.ply", "rb").read()
    model, moved = read_ply(on + "_20.ply"), read_ply(on + "_20.transformed.ply")
    v = [float(x) for x in TRS.split(",")]
    sim = X.similarity_from_trs(v[0:3], v[3:6], v[6])
    want = T.transform_splats(sim.R, sim.t, sim.s, X.sh_rotation(sim.R), model["pos"], model["shN"], model["scale"], model["rot"], 2)
    for k in ("pos", "shN", "scale", "rot"):
        assert np.array_equal(moved[k].view(np.uint32), want[k].reshape(moved[k].shape).view(np.uint32)), k
    for k in ("sh0", "opacity"):
        assert np.array_equal(moved[k].view(np.uint32), model[k].view(np.uint32)), k
    assert np.array_equal(moved["shN"][:, 24:].view(np.uint32), model["shN"][:, 24:].view(np.uint32))      # band 3 of a degree-2 model: copied
    assert not np.array_equal(moved["pos"], model["pos"]) and not np.array_equal(moved["rot"], model["rot"])


def test_files_and_log_lines(gpu_device, runs):
    on, p_on = runs[0], runs[1]
    for suffix in (".compressed.ply", ".splat", ".spz", ".reduced.ply"):
        assert os.path.getsize(on + "_20" + suffix) > 0, suffix
    err = p_on.stderr
    for name in ("spz", "reduced"):
        m = re.search(rf"export @20: {name} decoded model: PSNR (\S+) dB \(full model (\S+) dB\)", err)
        assert m, err[-3000:]
        assert math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2)))
        print(f"{name}: decoded {float(m.group(1)):.3f} dB, full {float(m.group(2)):.3f} dB")
    assert re.search(r"config: exportTransform p' = s R p \+ t with R = \[.*\], t = \(0\.5, -1, 2\), s = 2\.5, from DVS_EXPORT_TRANSFORM=", err)
    assert re.search(r"export @20: transform 2000 splats, [\d.]+ ms", err)
    assert re.search(r"export @20: transformed\.ply 2000 splats, \d+ bytes", err)


def test_scores_are_taken_in_the_cameras_frame(gpu_device, runs):
    """The evaluation cameras and the training arrays stay as they are: the full model's score in the transformed run is the untransformed
    run's, digit for digit (the two resume PLYs are byte-identical). The decoded models are taken back by the inverse before they are
    scored, so each decoded PSNR must agree with the untransformed run's within 1 dB. Why 1 dB and not less: the two payloads quantise
    DIFFERENT numbers of the same model (log scales shifted by ln 2.5 = 14.66 steps of the .spz byte, so every rounding falls elsewhere;
    positions 2.5 x finer against the 1/4096 grid; other quaternions), so each carries its own quantisation loss, which for these formats
    on a model of about 30 dB is a few tenths of a dB either way; a payload scored in the wrong frame (moved by |t| = 2.3 units and
    enlarged 2.5 x in a scene a few units across) shares no pixel with the targets and loses more than 10 dB. 1 dB lies a factor of
    several from both."""
    p_on, p_off = runs[1], runs[3]
    pat = r"eval @20: 1 views, PSNR (\S+) dB"
    assert re.search(pat, p_on.stderr) and re.search(pat, p_on.stderr).group(1) == re.search(pat, p_off.stderr).group(1)
    for name in ("spz", "reduced"):
        a, b = (float(re.search(rf"export @20: {name} decoded model: PSNR (\S+) dB", p.stderr).group(1)) for p in (p_on, p_off))
        print(f"{name}: decoded PSNR {a:.3f} dB with the transform (scored after the inverse), {b:.3f} dB without")
        assert abs(a - b) <= 1.0


def test_orient_run_turns_the_mean_camera_up_onto_y(gpu_device, runs):
    """--exportOrient +y alone implies the transformed PLY; R and t recovered from the two files (least squares over the positions) take
    the scene's mean camera-up, recomputed here from the synthetic cameras, onto +y within 1e-5 and the camera centroid to the origin"""
    import divshot_amd as dv
    from divshot_amd._lib import read_ply
    orient, p = runs[4], runs[5]
    assert sorted(os.listdir(os.path.dirname(orient))) == ["iteration_20.ply", "iteration_20.transformed.ply"]
    assert "config: exportTransform" in p.stderr and "DVS_EXPORT_ORIENT +y" in p.stderr
    spec = dv.make_spec(2000, 20, 12, sh_degree=2, n_cams=8)
    cams = [dv.synth_camera(spec, i) for i in range(8)]
    up = -np.array([[c.view[1], c.view[5], c.view[9]] for c in cams], np.float64).mean(axis=0)
    up /= np.linalg.norm(up)
    centroid = np.array([list(c.campos) for c in cams], np.float64).mean(axis=0)
    a, b = read_ply(orient + "_20.ply")["pos"].astype(np.float64), read_ply(orient + "_20.transformed.ply")["pos"].astype(np.float64)
    A = np.concatenate([a, np.ones((len(a), 1))], axis=1)
    M = np.linalg.lstsq(A, b, rcond=None)[0]                                     # b = a R^T + t
    R, t = M[:3].T, M[3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5
    assert np.abs(R @ up - np.array([0.0, 1.0, 0.0])).max() <= 1e-5
    assert np.abs(R @ centroid + t).max() <= 1e-4


def test_without_a_flag_nothing_new_is_logged(gpu_device, runs):
    off, p_off = runs[2], runs[3]
    assert "exportTransform" not in p_off.stderr and ": transform " not in p_off.stderr and "transformed" not in p_off.stderr
    assert not os.path.exists(off + "_20.transformed.ply")
