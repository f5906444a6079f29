"""Distorted COLMAP cameras end to end on the GPU, on the pattern of tests/test_gpu_dataset_jpeg.py (which explains what is reproducible
from run to run and why: everything before the first backward at 40x24, the whole trajectory at 20x12). 3 cameras at 40x24, PPM
pictures of smooth random content, 300 points, `gaussian_train` for 20 steps with DVS_LOSS_EVERY=1:
  capture A   SIMPLE_RADIAL (k = +0.3), RADIAL and OPENCV cameras and the raw pictures;
  capture B   PINHOLE cameras with the same fx, fy, cx, cy; its pictures are tests/undistort_ref.py's undistorted bytes and its
              masks/*.pgm are the restatement's masks times 255.
The loader undistorts A on the device into what undistort_ref defines, so nothing past the loader can tell A from B when both run with
--useMask 1: every comparison is `==` on the log lines. A without --useMask gives the same `eval @0` (it has no mask files: the mask
is the validity either way) and its log carries the restatement's invalid count. With source-space mask files on two views of A and the
restatement's warped masks in B the lines are identical again. Pinhole views beside a distorted one, without --useMask, train as they
do with all-255 mask files under --useMask. An OPENCV_FISHEYE camera stops the load with a message that names it."""
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import undistort_ref as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
W, H, STEPS = 40, 24, 20
MODELS = [("SIMPLE_RADIAL", [36.0, 20.0, 12.0, 0.3]), ("RADIAL", [35.0, 20.5, 11.5, 0.25, -0.1]), ("OPENCV", [36.0, 34.5, 19.0, 12.75, 0.21, -0.06, 0.013, -0.009])]
HALF = ("--maxImageWidth", "20")
MASK = ("--useMask", "1")


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    """captures(source_masks) -> (capture A, capture B, the restatement's invalid pixels over the three views); with source_masks, views
    0 and 1 of A carry a mask file in the source image's geometry and B the restatement's warped masks"""
    cache = {}

    def make(source_masks=False):
        if source_masks in cache:
            return cache[source_masks]
        r = np.random.default_rng(12)
        images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.3 * (k - 1), 0.05 * k, 0.0]), camera_id=k + 1, name=f"view_{k}.ppm")
                  for k in range(3)]
        points = [dict(id=k + 1, xyz=np.array([r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), r.uniform(2.5, 4.0)]), rgb=r.integers(0, 256, 3)) for k in range(300)]
        cams_a = [dict(id=k + 1, model=m, width=W, height=H, params=p) for k, (m, p) in enumerate(MODELS)]
        cams_b = [dict(id=k + 1, model="PINHOLE", width=W, height=H, params=list(U.split_params(U.MODEL_IDS[m], p)[:4])) for k, (m, p) in enumerate(MODELS)]
        pix_a, pix_b, masks_a, masks_b, invalid = {}, {}, {}, {}, 0
        for k, (m, p) in enumerate(MODELS):
            src = U.smooth_image(W, H, 3, seed=40 + k)
            src_mask = None
            if source_masks and k < 2:
                src_mask = np.ones((H, W), np.uint8)
                src_mask[3 + 4 * k:15 + 2 * k, 5 + 9 * k:22 + 9 * k] = 0
                masks_a[f"view_{k}.ppm"] = src_mask * 200                        # (> 127 is trainable)
            dst, mask, n = U.undistort(src, U.descriptor(U.MODEL_IDS[m], p, W, H), src_mask)
            assert 0 < n < W * H // 3 and mask.sum() > W * H // 3
            invalid += n
            pix_a[f"view_{k}.ppm"], pix_b[f"view_{k}.ppm"] = src.transpose(1, 2, 0), dst.transpose(1, 2, 0)
            masks_b[f"view_{k}.ppm"] = (mask * 255).astype(np.uint8)
        a, b = str(tmp_path_factory.mktemp("capture_distorted")), str(tmp_path_factory.mktemp("capture_pinhole"))
        CR.write_dataset(a, cams_a, images, points, pix_a, masks=masks_a)
        CR.write_dataset(b, cams_b, images, points, pix_b, masks=masks_b)
        cache[source_masks] = (a, b, invalid)
        return cache[source_masks]
    return make


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(capture, extra args, steps) -> (eval @0 line, [the loss lines], the last eval line, stderr), each distinct run made once"""
    cache = {}

    def go(capture, extra=(), steps=STEPS):
        key = (capture, tuple(extra), steps)
        if key not in cache:
            out = str(tmp_path_factory.mktemp("out") / "iteration")
            p = subprocess.run([DRIVER, "--inputPath", capture, "--maxIteration", str(steps), "--eval", "--outputPath", out] + list(extra),
                               capture_output=True, text=True, timeout=300, env=dict(os.environ, DVS_LOSS_EVERY="1"))
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
            ev0, ev20 = re.findall(r"eval @0: .*", p.stderr), re.findall(rf"eval @{steps}: .*", p.stderr)
            losses = re.findall(r"Iteraions \d+, loss : [-\d.enaif+]+", p.stderr)
            assert len(ev0) == 1 and len(ev20) == 1 and len(losses) == steps, p.stderr[-3000:]
            assert all("nan" not in l and "inf" not in l for l in losses)
            cache[key] = (ev0[0], losses, ev20[0], p.stderr)
        return cache[key]
    return go


def test_full_size_eval_at_0_and_first_loss_identical(gpu_device, captures, run):
    a, b, invalid = captures()
    ev_a, loss_a, _, log_a = run(a, MASK)
    ev_b, loss_b, _, log_b = run(b, MASK)
    print(ev_a, loss_a[0], loss_a[-1], loss_b[-1], sep="\n")
    assert re.search(rf"dataset: 3 cameras \(mixed models\), {W}x{H}, 300 points \(0 dropped\)", log_a), log_a[-3000:]
    assert re.search(rf"dataset: 3 cameras \(PINHOLE\), {W}x{H}, 300 points \(0 dropped\)", log_b)
    assert "dataset: undistort:" in log_a and "dataset: undistort:" not in log_b
    assert ev_a == ev_b
    assert loss_a[0] == loss_b[0] and loss_a[0].startswith("Iteraions 0,")
    assert len(set(loss_a)) > 1


def test_the_factor_2_path_trains_identically(gpu_device, captures, run):
    a, b, _ = captures()
    ev_a, loss_a, end_a, log_a = run(a, MASK + HALF)
    ev_b, loss_b, end_b, _ = run(b, MASK + HALF)
    assert f"{W}x{H} -> {W // 2}x{H // 2} (1/2)" in log_a
    assert ev_a == ev_b
    assert loss_a == loss_b
    assert end_a == end_b
    assert ev_a != run(a, MASK)[0] and len(set(loss_a)) > 1


def test_without_usemask_the_mask_is_the_validity(gpu_device, captures, run):
    a, b, invalid = captures()
    ev, loss, _, log = run(a)
    assert ev == run(a, MASK)[0] and loss[0] == run(a, MASK)[1][0]
    m = re.search(r"dataset: undistort: 3 of 3 images \(SIMPLE_RADIAL, RADIAL, OPENCV\), ([\d.]+) ms \(device, events\), (\d+) of (\d+) pixels have no source "
                  r"and are masked out", log)
    assert m, log[-3000:]
    print(m.group(0))
    assert int(m.group(2)) == invalid and int(m.group(3)) == 3 * W * H
    assert ev != run(b)[0]                                                   # B without its mask files scores the blank pixels too


def test_source_masks_are_warped_with_the_view(gpu_device, captures, run):
    a, b, _ = captures(True)
    ev_a, loss_a, _, _ = run(a, MASK)
    ev_b, loss_b, _, _ = run(b, MASK)
    assert ev_a == ev_b and loss_a[0] == loss_b[0]
    assert ev_a != run(captures()[0], MASK)[0]                               # the held-out view's mask file counts
    ev_h, loss_h, end_h, _ = run(a, MASK + HALF)
    assert (ev_h, loss_h, end_h) == run(b, MASK + HALF)[:3]


def test_a_pinhole_view_beside_a_distorted_one_trains_everywhere(gpu_device, tmp_path, run):
    """without --useMask a capture with one distorted camera carries a mask on every view, all ones on its pinhole views: the same
    capture with an all-255 masks/<stem>.pgm on the pinhole views and --useMask gives the same lines (4 steps)"""
    r = np.random.default_rng(12)
    models = [("PINHOLE", [36.0, 35.0, 20.0, 12.0]), MODELS[1], ("PINHOLE", [34.0, 36.0, 19.5, 12.5])]
    cams = [dict(id=k + 1, model=m, width=W, height=H, params=p) for k, (m, p) in enumerate(models)]
    images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.3 * (k - 1), 0.05 * k, 0.0]), camera_id=k + 1, name=f"view_{k}.ppm") for k in range(3)]
    points = [dict(id=k + 1, xyz=np.array([r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), r.uniform(2.5, 4.0)]), rgb=r.integers(0, 256, 3)) for k in range(300)]
    pixels = {f"view_{k}.ppm": U.smooth_image(W, H, 3, seed=40 + k).transpose(1, 2, 0) for k in range(3)}
    a, b = str(tmp_path / "plain"), str(tmp_path / "ones")
    CR.write_dataset(a, cams, images, points, pixels)
    CR.write_dataset(b, cams, images, points, pixels, masks={f"view_{k}.ppm": np.full((H, W), 255, np.uint8) for k in (0, 2)})
    for extra in ((), HALF):
        ev_a, loss_a, end_a, log_a = run(a, extra, 4)
        ev_b, loss_b, end_b, _ = run(b, MASK + extra, 4)
        assert "dataset: 3 cameras (mixed models)" in log_a and "dataset: undistort: 1 of 3 images (RADIAL)" in log_a, log_a[-3000:]
        assert ev_a == ev_b and loss_a[0] == loss_b[0] and len(set(loss_a)) > 1
        if extra:                                                            # 20x12: the whole trajectory is reproducible
            assert loss_a == loss_b and end_a == end_b


def test_a_fisheye_camera_stops_the_load_with_its_name(gpu_device, captures, tmp_path):
    a, _, _ = captures()
    bad = str(tmp_path / "fisheye")
    shutil.copytree(a, bad)
    for f in ("cameras.bin", "images.bin", "points3D.bin"):                  # leave the text model only
        os.remove(os.path.join(bad, "sparse/0", f))
    cams = [dict(id=k + 1, model=m, width=W, height=H, params=p) for k, (m, p) in enumerate(MODELS)]
    images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.zeros(3), camera_id=k + 1, name=f"view_{k}.ppm") for k in range(3)]
    files = CR.sparse_txt(cams, images, [dict(id=1, xyz=np.array([0.0, 0.0, 3.0]), rgb=[1, 2, 3])])
    files["cameras.txt"] = files["cameras.txt"].replace(b"2 RADIAL 40 24 35.0 20.5 11.5 0.25 -0.1", b"2 OPENCV_FISHEYE 40 24 35.0 35.0 20.5 11.5 0.01 0.0 0.0 0.0")
    assert b"OPENCV_FISHEYE" in files["cameras.txt"]
    for name, data in files.items():
        open(os.path.join(bad, "sparse/0", name), "wb").write(data)
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "camera model OPENCV_FISHEYE is not supported" in p.stderr and "load data failed" in p.stdout
    assert "SIMPLE_RADIAL, RADIAL and OPENCV are undistorted by the loader" in p.stderr
