"""Rendered views as JPEG files, end to end on the GPU. A pinhole capture of 8 cameras at 64x48 with smooth synthetic pictures as PPM
targets (written by tests/colmap_ref.py, so the test holds the targets) and 300 sparse points goes through `gaussian_train` for 20
steps with --eval: camera 0 is the held-out one.

The metric check. `--renderViews test --renderQuality 100 --renderSampling 444` writes <out>_20_renders/view_000.jpg; the project's own
decoder (gstrain_jpeg_open + jpeg_ref.reconstruct) turns it back into 64x48 pixels d. The evaluator scored the same render r (clamped
to [0, 1]) against the same target t: sqrt(mse) = rms(r - t). By the triangle inequality |rms(d / 255 - t) - rms(r - t)| <= rms(d / 255 - r).
With b the bytes of r, |d - b| <= e = 4 levels per pixel, the largest round-trip error of the restatement at Q 100 / 4:4:4 over the
images of tests/test_jpeg_write_format.py (measured there on the CPU and asserted), and |b - 255 r| <= 0.5 level, so
the strict bound is (e + 0.5) / 255. The test asserts the tighter e / 255 it was specified with; the difference seen is 6e-5.

Flag variants: --renderViews all writes one file per camera, the default sampling gives a 2x2 file, --renderViews bogus is a command-line
error. Off: the same run without the flag leaves no _renders directory and no `render @` / `config: render` line, and its `eval @20`
line equals the flagged run's — compared at 16x12 (--maxImageWidth 16: one tile), where the trainer repeats from run to run
(tests/test_gpu_dataset_jpeg.py explains why a view of at most two tiles does). renderCameraToJpeg through a host that links the class
(tests/hosts/render_one.cpp): a valid file for camera 1, false for camera -1.

The pass boundary: with --evalHoldout 3 the evaluation context renders 3 views per pass; renders of all 8 cameras, the mesh export and the
importance prune over the 5 training cameras and the scored .spz export then all end in a partial pass, and two runs write the same bytes."""
import json
import os
import re
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import jpeg_ref as J
from test_jpeg_write_format import ROUND_TRIP_ERROR_Q100_444

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
W, H, CAMS, STEPS = 64, 48, 8, 20


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """-> (directory, {name: uint8 [H][W][3]})"""
    root = str(tmp_path_factory.mktemp("capture"))
    r = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W]
    cameras, images, pixels = [], [], {}
    for k in range(CAMS):
        name = f"view_{k:03d}.ppm"
        px = np.stack([127 + 100 * np.sin((x + 3 * k) / 9.0), 127 + 100 * np.cos((y - 2 * k) / 7.0), 40 + 2 * x + y], -1)
        pixels[name] = np.clip(px + r.normal(0, 6, px.shape), 0, 255).astype(np.uint8)
        cameras.append(dict(id=k + 1, model="PINHOLE", width=W, height=H, params=[58.0, 58.0, W / 2.0, H / 2.0]))
        images.append(dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.15 * (k - 3.5), 0.04 * (k % 3), 0.0]), camera_id=k + 1, name=name))
    points = [dict(id=k + 1, xyz=np.array([r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), r.uniform(2.5, 4.0)]), rgb=r.integers(0, 256, 3)) for k in range(300)]
    CR.write_dataset(root, cameras, images, points, pixels)
    return root, pixels


@pytest.fixture(scope="module")
def run(capture, tmp_path_factory):
    """run(extra args) -> (output prefix, stderr), each distinct run made once"""
    cache = {}

    def go(*extra):
        if extra not in cache:
            out = str(tmp_path_factory.mktemp("out") / "iteration")
            env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_RENDER_")}
            p = subprocess.run([DRIVER, "--inputPath", capture[0], "--maxIteration", str(STEPS), "--eval", "--outputPath", out] + list(extra),
                               capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
            cache[extra] = (out, p.stderr)
        return cache[extra]
    return go


def decode_file(path):
    """-> uint8 [3][H][W] through the project's C entropy decoder and the restated reconstruction; and the frame"""
    from divshot_amd import _lib
    desc, coef = _lib.jpeg_decode_coefficients(path)
    f = J.Frame()
    f.width, f.height, f.ncomp = desc.width, desc.height, desc.components
    f.hs, f.vs = [desc.hs, 1, 1], [desc.vs, 1, 1]
    f.bw, f.bh, f.offset = list(desc.blocks_w), list(desc.blocks_h), list(desc.offset)
    f.quant = [np.array(desc.quant[c][:], np.uint16) for c in range(3)]
    f.coef = coef
    return J.reconstruct(f), f


def test_the_picture_is_what_the_evaluation_scored(gpu_device, capture, run):
    out, log = run("--renderViews", "test", "--renderQuality", "100", "--renderSampling", "444")
    files = sorted(os.listdir(out + f"_{STEPS}_renders"))
    assert files == ["view_000.jpg"], files
    assert re.search(r"config: renderViews 1: every save also writes the test cameras as JPEG files \(quality 100, 4:4:4\)", log), log[-3000:]
    m = re.search(rf"render @{STEPS}: 1 views, (\d+) bytes, transform [\d.]+ ms \(device, events\), entropy coding [\d.]+ ms \(host, 1 threads, wall\)", log)
    assert m, log[-3000:]
    path = os.path.join(out + f"_{STEPS}_renders", "view_000.jpg")
    assert int(m.group(1)) == os.path.getsize(path)
    got, f = decode_file(path)
    assert got.shape == (3, H, W) and (f.hs[0], f.vs[0]) == (1, 1) and all((q == 1).all() for q in f.quant)
    assert got.std() > 5                                      # a picture, not a flat field
    ev = json.load(open(out + f"_{STEPS}_eval.json"))
    view = next(v for v in ev["views"] if v["camera"] == 0)
    target = capture[1]["view_000.ppm"].transpose(2, 0, 1).astype(np.float64) / 255.0
    rms = float(np.sqrt(np.mean((got.astype(np.float64) / 255.0 - target) ** 2)))
    print(f"rms of the decoded file {rms:.6f}, sqrt(mse) of the evaluation {np.sqrt(view['mse']):.6f}, bound {ROUND_TRIP_ERROR_Q100_444 / 255.0:.6f}")
    assert abs(rms - np.sqrt(view["mse"])) <= ROUND_TRIP_ERROR_Q100_444 / 255.0
    assert set(ev) == {"iteration", "n_splats", "sh_degree", "holdout", "views", "mean"}                 # the eval JSON is as it was


def test_all_cameras_default_sampling_and_off(gpu_device, capture, run):
    small = ("--maxImageWidth", "16")
    out_on, log_on = run("--renderViews", "all", *small)
    out_off, log_off = run(*small)
    files = sorted(os.listdir(out_on + f"_{STEPS}_renders"))
    assert files == [f"view_{k:03d}.jpg" for k in range(CAMS)], files
    assert re.search(rf"render @{STEPS}: {CAMS} views, \d+ bytes", log_on) and "(quality 90, 4:2:0)" in log_on
    for name in files:
        got, f = decode_file(os.path.join(out_on + f"_{STEPS}_renders", name))
        assert got.shape == (3, 12, 16) and (f.hs[0], f.vs[0]) == (2, 2)
    # off: nothing of the feature, and the same evaluation
    assert not os.path.exists(out_off + f"_{STEPS}_renders") and not [n for n in os.listdir(os.path.dirname(out_off)) if "render" in n]
    assert "render @" not in log_off and "config: render" not in log_off
    ev_on, ev_off = re.findall(rf"eval @{STEPS}: .*", log_on), re.findall(rf"eval @{STEPS}: .*", log_off)
    assert len(ev_on) == 1 and ev_on == ev_off
    assert open(out_on + f"_{STEPS}_eval.json").read() == open(out_off + f"_{STEPS}_eval.json").read()


def test_training_cameras_alone_and_the_environment_override(gpu_device, capture, tmp_path):
    """no camera is held out and only pictures are asked for: the rendering context is created by the first render"""
    out = str(tmp_path / "m" / "iteration")
    p = subprocess.run([DRIVER, "--inputPath", capture[0], "--maxIteration", "2", "--outputPath", out, "--maxImageWidth", "16"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, DVS_RENDER_VIEWS="2", DVS_RENDER_QUALITY="75", DVS_RENDER_SAMPLING="1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "eval @" not in p.stderr and "(quality 75, 4:4:4)" in p.stderr
    assert sorted(os.listdir(out + "_2_renders")) == [f"view_{k:03d}.jpg" for k in range(CAMS)]
    assert decode_file(os.path.join(out + "_2_renders", "view_003.jpg"))[0].shape == (3, 12, 16)


def test_every_user_of_the_evaluation_context_crosses_a_pass_boundary(gpu_device, capture, tmp_path):
    """--evalHoldout 3 holds out cameras 0, 3, 6: the evaluation context renders 3 views per pass, so the 8 written renders go through
    it as 3 + 3 + 2 and the 5 training cameras of the mesh export and of the importance prune (one occasion, iteration 12) as 3 + 2;
    the .spz export scores its decoded model through it as well. At 16x12 two runs of the command write the same bytes."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_RENDER_")}
    env.update(DVS_MESH_RESOLUTION="16", DVS_MESH_BOUNDS="-1.5,-1,2.5,1.5,1,4", DVS_IMPORTANCE_PRUNE="20", DVS_EXPORT_FORMATS="4")   # (the box of the points)
    runs = []
    for tag in ("a", "b"):
        out = str(tmp_path / tag / "iteration")
        p = subprocess.run([DRIVER, "--inputPath", capture[0], "--maxIteration", str(STEPS), "--maxImageWidth", "16", "--evalHoldout", "3", "--renderViews", "all",
                            "--refineStopIter", "5", "--pruneEvery", "12", "--outputPath", out], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        files = {}
        for d, _, names in os.walk(os.path.dirname(out)):
            files.update({os.path.relpath(os.path.join(d, n), os.path.dirname(out)): open(os.path.join(d, n), "rb").read() for n in names})
        runs.append((p.stderr, files))
    log, files = runs[0]
    assert sorted(n for n in files if n.endswith(".jpg")) == [f"iteration_{STEPS}_renders/view_{k:03d}.jpg" for k in range(CAMS)], sorted(files)
    ev = json.loads(files[f"iteration_{STEPS}_eval.json"])
    assert [v["camera"] for v in ev["views"]] == [0, 3, 6] and set(ev["exports"]["spz"]) == {"psnr", "ssim", "l1", "mse"}
    assert re.search(rf"render @{STEPS}: {CAMS} views, ", log), log[-3000:]
    assert re.findall(rf"mesh @{STEPS}: .* trunc \S+, (\d+) views; ", log) == ["5"], log[-3000:]
    assert re.findall(r"importance prune @(\d+): \d+ -> \d+ splats, (\d+) views, ", log) == [("12", "5")], log[-3000:]
    assert {f"iteration_{STEPS}.ply", f"iteration_{STEPS}.spz", f"iteration_{STEPS}_mesh.ply"} <= set(files)
    assert sorted(files) == sorted(runs[1][1])
    assert [n for n in sorted(files) if files[n] != runs[1][1][n]] == []


def test_bad_flag_values_are_command_line_errors(tmp_path):
    for flag, value in (("--renderViews", "bogus"), ("--renderSampling", "422"), ("--renderQuality", "0")):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), flag, value], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "Command Line Error" in p.stdout and value in p.stdout, (flag, p.stdout)


def test_render_camera_to_jpeg_through_the_class(gpu_device, tmp_path):
    exe = str(tmp_path / "render_one")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hosts", "render_one.cpp"), "-o", exe,
                           "-L", LIB, "-lgstrain", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    jpg = str(tmp_path / "camera_1.jpg")
    p = subprocess.run([exe, "synthetic:N=2000,W=64,H=48,cams=3,sh=1,seed=4", "5", jpg], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "before_load 0, camera 1 1, camera -1 0, past the end 0, missing directory 0, iterations 6, terminated 0" in p.stdout, p.stdout + p.stderr
    got, f = decode_file(jpg)
    assert got.shape == (3, 48, 64) and (f.hs[0], f.vs[0]) == (1, 1) and got.std() > 1
    assert not os.path.exists(jpg + ".missing")
