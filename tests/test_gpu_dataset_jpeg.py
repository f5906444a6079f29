"""JPEG ingestion end to end on the GPU. A 3-camera capture of 40x24 JPEGs at 4:2:0 (three fixtures of tests/golden/jpeg/: standard,
optimised and restart-marker tables) and the same capture with the images written as PPM from tests/jpeg_ref.py's pixels go through
`gaussian_train` for 20 steps (DVS_LOSS_EVERY=1 logs every step's loss). The device reconstructs what jpeg_ref defines, so nothing
past the loader can tell the two captures apart — and every comparison below is `==` on the log lines, made where the trainer itself
is reproducible from run to run.

What is reproducible. The composite backward adds each tile's total for a splat into that splat's gradient row with ONE fp32 atomic
per tile (csrc/render_tr.hip), so a row is a sum of as many addends as the view has tiles that the splat touches, in the order the
workgroups arrive. A 40x24 view has 3 x 2 tiles of 16 x 16: up to six addends, the order matters in the last bit, and two runs of the
SAME capture already differ from the first optimizer step on (measured on the PPM capture alone: six runs, six different `eval @20`
lines, losses that differ in the sixth decimal). Everything before the first backward is free of atomics: the `eval @0` line
(forward + dvs_image_metrics_views on the held-out view's stored bytes) and the loss of step 0 (forward + loss of a training view).
At --maxImageWidth 20 the views are 20x12 = 2 x 1 tiles: a row receives at most two addends into a zeroed cell, fp32 addition is
commutative, so the whole trajectory is order-independent and all 20 losses and the `eval @20` line are compared exactly.
  40x24 (factor 1):  `eval @0` and the step-0 loss identical, JPEG against PPM, with every view held out once (the capture is also
                     written with its three pictures rotated, since --eval holds out view 0 only), and 1 load thread against 8
  20x12 (factor 2):  `eval @0`, all 20 losses and `eval @20` identical, JPEG against PPM and 1 load thread against 8"""
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import jpeg_ref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
FIX = os.path.join(ROOT, "tests", "golden", "jpeg")
FILES = ["c420_40x24", "c420_40x24_opt", "c420_40x24_rst3"]
W, H, STEPS = 40, 24, 20


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    """captures(rot) -> (jpeg capture, ppm capture) with picture (k + rot) % 3 as view k: one sparse model (the image names end in .jpg
    in both), 300 points in front of the cameras"""
    cache = {}

    def make(rot=0):
        if rot in cache:
            return cache[rot]
        r = np.random.default_rng(12)
        cameras = [dict(id=k + 1, model="PINHOLE", width=W, height=H, params=[36.0, 36.0, W / 2.0, H / 2.0]) for k in range(3)]
        images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.3 * (k - 1), 0.05 * k, 0.0]), camera_id=k + 1, name=f"view_{k}.jpg")
                  for k in range(3)]
        points = [dict(id=k + 1, xyz=np.array([r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), r.uniform(2.5, 4.0)]), rgb=r.integers(0, 256, 3)) for k in range(300)]
        jpeg_dir, ppm_dir = str(tmp_path_factory.mktemp("capture_jpeg")), str(tmp_path_factory.mktemp("capture_ppm"))
        CR.write_dataset(jpeg_dir, cameras, images, points, {})
        CR.write_dataset(ppm_dir, cameras, images, points, {})
        for k in range(3):
            src = os.path.join(FIX, FILES[(k + rot) % 3] + ".jpg")
            shutil.copy(src, os.path.join(jpeg_dir, "images", f"view_{k}.jpg"))
            CR.write_ppm(os.path.join(ppm_dir, "images", f"view_{k}.ppm"), np.ascontiguousarray(J.decode(open(src, "rb").read()).transpose(1, 2, 0)))
        cache[rot] = (jpeg_dir, ppm_dir)
        return cache[rot]
    return make


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(capture, extra args, threads) -> (eval @0 line, [20 loss lines], eval @20 line, stderr), each distinct run made once"""
    cache = {}

    def go(capture, extra=(), threads=None):
        key = (capture, tuple(extra), threads)
        if key not in cache:
            out = str(tmp_path_factory.mktemp("out") / "iteration")
            env = dict(os.environ, DVS_LOSS_EVERY="1")
            env.pop("DVS_LOAD_THREADS", None)
            if threads is not None:
                env["DVS_LOAD_THREADS"] = str(threads)
            p = subprocess.run([DRIVER, "--inputPath", capture, "--maxIteration", str(STEPS), "--eval", "--outputPath", out] + list(extra),
                               capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
            ev0, ev20 = re.findall(r"eval @0: .*", p.stderr), re.findall(rf"eval @{STEPS}: .*", p.stderr)
            losses = re.findall(r"Iteraions \d+, loss : [-\d.enaif+]+", p.stderr)
            assert len(ev0) == 1 and len(ev20) == 1 and len(losses) == STEPS, p.stderr[-3000:]
            assert all("nan" not in l and "inf" not in l for l in losses)
            cache[key] = (ev0[0], losses, ev20[0], p.stderr)
        return cache[key]
    return go


HALF = ("--maxImageWidth", "20")


def test_full_size_eval_at_0_and_first_loss_identical(gpu_device, captures, run):
    jpeg_dir, ppm_dir = captures()
    ev_j, loss_j, _, log_j = run(jpeg_dir)
    ev_p, loss_p, _, log_p = run(ppm_dir)
    print(ev_j, loss_j[0], loss_j[-1], loss_p[-1], sep="\n")
    m = re.search(r"dataset: jpeg: 3 of 3 images, entropy decode [\d.]+ ms \(host, 8 threads, wall\), reconstruction [\d.]+ ms \(device, events\)", log_j)
    assert m, log_j[-3000:]
    print(m.group(0))
    assert "dataset: jpeg:" not in log_p
    assert re.search(rf"dataset: 3 cameras \(PINHOLE\), {W}x{H}, 300 points \(0 dropped\)", log_j)
    assert ev_j == ev_p
    assert loss_j[0] == loss_p[0] and loss_j[0].startswith("Iteraions 0,")
    assert len(set(loss_j)) > 1


@pytest.mark.parametrize("rot", [1, 2])
def test_full_size_every_view_held_out_once(gpu_device, captures, run, rot):
    jpeg_dir, ppm_dir = captures(rot)
    ev_j, loss_j, _, _ = run(jpeg_dir)
    ev_p, loss_p, _, _ = run(ppm_dir)
    assert ev_j == ev_p and loss_j[0] == loss_p[0]
    assert ev_j != run(captures()[0])[0]                                     # another picture is the held-out one


def test_the_factor_2_path_trains_identically(gpu_device, captures, run):
    jpeg_dir, ppm_dir = captures()
    ev_j, loss_j, end_j, log_j = run(jpeg_dir, HALF)
    ev_p, loss_p, end_p, _ = run(ppm_dir, HALF)
    assert f"{W}x{H} -> {W // 2}x{H // 2} (1/2)" in log_j
    assert ev_j == ev_p
    assert loss_j == loss_p
    assert end_j == end_p
    assert ev_j != run(jpeg_dir)[0] and len(set(loss_j)) > 1


def test_one_load_thread_against_the_default(gpu_device, captures, run):
    jpeg_dir, _ = captures()
    ev_1, loss_1, end_1, log_1 = run(jpeg_dir, HALF, 1)
    ev_d, loss_d, end_d, _ = run(jpeg_dir, HALF)
    assert "(host, 1 threads, wall)" in log_1
    assert ev_1 == ev_d and loss_1 == loss_d and end_1 == end_d
    ev_1, loss_1, _, _ = run(jpeg_dir, (), 1)
    ev_d, loss_d, _, _ = run(jpeg_dir)
    assert ev_1 == ev_d and loss_1[0] == loss_d[0]


def test_a_rejected_jpeg_stops_the_load_with_its_message(gpu_device, captures, tmp_path):
    jpeg_dir, _ = captures()
    bad = str(tmp_path / "bad")
    shutil.copytree(jpeg_dir, bad)
    shutil.copy(os.path.join(FIX, "progressive.jpg"), os.path.join(bad, "images", "view_1.jpg"))
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "progressive JPEG" in p.stderr and "view_1.jpg" in p.stderr and "load data failed" in p.stdout
    shutil.copy(os.path.join(FIX, "c420_37x29.jpg"), os.path.join(bad, "images", "view_1.jpg"))
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "view_1.jpg is 37x29 but its camera 2 is 40x24" in p.stderr
