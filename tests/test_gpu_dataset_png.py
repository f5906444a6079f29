"""PNG ingestion end to end on the GPU, on the pattern of tests/test_gpu_dataset_jpeg.py (which explains what is reproducible from run to
run and why: everything before the first backward at 40x24, the whole trajectory at 20x12). One 3-camera capture at 40x24 (smooth random
pictures, 300 points, block masks) is written once as PPM + PGM masks and then as PNG in these variants, all from tests/png_ref.py's
writer with the row filters cycling 0..4:
  rgb8    RGB8 pictures, masks/<stem>.png (8-bit gray)
  rgb16   RGB16 pictures with v = 257 b, masks/<image name>.png (gray + alpha: gray 255 everywhere, the mask in the alpha channel)
  rgba8   RGBA8 pictures whose alpha is 255 x the PGM mask, no mask files
  bit1    RGB8 pictures, view 0's mask a 1-bit gray PNG, the other masks PGM
PNG is lossless and the loader reconstructs what png_ref defines, so nothing past the loader can tell a PNG capture from the PPM one:
`gaussian_train` runs for a few steps with DVS_LOSS_EVERY=1 and every comparison is `==` on the log lines, with and without --useMask,
at factor 1 and at --maxImageWidth 20 (factor 2). One OPENCV variant takes a PNG picture with a PNG mask through the undistortion; a
truncated PNG stops the load with its message; one load thread gives the same lines as the default. RGBA8 pictures beside PGM masks train
as the PPM capture whose masks are the product of the alpha and the PGM."""
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import png_ref as P
import undistort_ref as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
W, H, STEPS = 40, 24, 4
HALF = ("--maxImageWidth", "20")
MASK = ("--useMask", "1")
VARIANTS = ["rgb8", "rgb16", "rgba8", "bit1"]


def _pictures():
    return [np.ascontiguousarray(U.smooth_image(W, H, 3, seed=70 + k).transpose(1, 2, 0)) for k in range(3)]          # [H][W][3]


def _masks():
    out = []
    for k in range(3):
        m = np.ones((H, W), np.uint8)
        m[2 + 3 * k:13 + 2 * k, 4 + 7 * k:19 + 7 * k] = 0
        out.append(m)
    return out


def _sparse(model="PINHOLE", params=(36.0, 36.0, W / 2.0, H / 2.0), ext=".png"):
    r = np.random.default_rng(12)
    cameras = [dict(id=k + 1, model=model, width=W, height=H, params=list(params)) for k in range(3)]
    images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.3 * (k - 1), 0.05 * k, 0.0]), camera_id=k + 1, name=f"view_{k}{ext}") for k in range(3)]
    points = [dict(id=k + 1, xyz=np.array([r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), r.uniform(2.5, 4.0)]), rgb=r.integers(0, 256, 3)) for k in range(300)]
    return cameras, images, points


def _png(samples, depth, ctype, **kw):
    h = samples.shape[0]
    return P.write_image(W, h, depth, ctype, samples.reshape(h, -1), split=57, **kw)


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _write_variant(root, variant, pictures, masks):
    for k, (px, m) in enumerate(zip(pictures, masks)):
        img, msk = os.path.join(root, "images", f"view_{k}.png"), os.path.join(root, "masks")
        px = px.astype(np.int64)
        if variant == "rgb8":
            _write(img, _png(px, 8, 2))
            _write(os.path.join(msk, f"view_{k}.png"), _png(m.astype(np.int64) * 200, 8, 0))
        elif variant == "rgb16":
            _write(img, _png(px * 257, 16, 2))
            ga = np.stack([np.full((H, W), 255, np.int64), m.astype(np.int64) * 255], -1)
            _write(os.path.join(msk, f"view_{k}.png.png"), _png(ga, 8, 4))
        elif variant == "rgba8":
            _write(img, _png(np.concatenate([px, m[..., None].astype(np.int64) * 255], -1), 8, 6))
        elif variant == "bit1":
            _write(img, _png(px, 8, 2))
            if k == 0:
                _write(os.path.join(msk, "view_0.png"), _png(m.astype(np.int64), 1, 0))
            else:
                os.makedirs(msk, exist_ok=True)
                CR.write_pgm(os.path.join(msk, f"view_{k}.pgm"), m * 255)


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    """{"ppm": the PPM + PGM capture, variant: its PNG capture}: one sparse model, the image names end in .png in all of them"""
    pictures, masks = _pictures(), _masks()
    cameras, images, points = _sparse()
    out = {}
    for name in ["ppm"] + VARIANTS:
        root = str(tmp_path_factory.mktemp("capture_" + name))
        if name == "ppm":
            CR.write_dataset(root, cameras, images, points, {f"view_{k}.png": pictures[k] for k in range(3)}, masks={f"view_{k}.png": masks[k] * 255 for k in range(3)})
        else:
            CR.write_dataset(root, cameras, images, points, {})
            _write_variant(root, name, pictures, masks)
        out[name] = root
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(capture, extra args, threads) -> (eval @0 line, [loss lines], eval @STEPS line, stderr), each distinct run made once, each a
    fresh child process under its own time limit"""
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
                               capture_output=True, text=True, timeout=120, env=env)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
            ev0, end = re.findall(r"eval @0: .*", p.stderr), re.findall(rf"eval @{STEPS}: .*", p.stderr)
            losses = re.findall(r"Iteraions \d+, loss : [-\d.enaif+]+", p.stderr)
            assert len(ev0) == 1 and len(end) == 1 and len(losses) == STEPS, p.stderr[-3000:]
            assert all("nan" not in l and "inf" not in l for l in losses)
            cache[key] = (ev0[0], losses, end[0], p.stderr)
        return cache[key]
    return go


def _compare(a, b, half):
    assert a[0] == b[0]                                                      # eval @0
    assert a[1][0] == b[1][0] and a[1][0].startswith("Iteraions 0,")          # the first loss line
    if half:                                                                 # 20x12: the whole trajectory is reproducible
        assert a[1] == b[1] and a[2] == b[2]
    assert len(set(a[1])) > 1


@pytest.mark.parametrize("half", [False, True], ids=["factor1", "factor2"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "useMask"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_png_capture_trains_as_the_ppm_capture(gpu_device, captures, run, variant, mask, half):
    extra = (MASK if mask else ()) + (HALF if half else ())
    png, ppm = run(captures[variant], extra), run(captures["ppm"], extra)
    log = png[3]
    n_masks = {"rgb8": 3, "rgb16": 3, "rgba8": 0, "bit1": 1}[variant] if mask else 0
    m = re.search(rf"dataset: png: 3 of 3 images, {n_masks} masks, inflate [\d.]+ ms \(host, 8 threads, wall\), reconstruction [\d.]+ ms \(device, events\)", log)
    assert m, log[-3000:]
    print(m.group(0), png[0], png[1][0], sep="\n")
    assert "dataset: png:" not in ppm[3]
    assert re.search(rf"dataset: 3 cameras \(PINHOLE\), {W}x{H}", log)
    if half:
        assert f"{W}x{H} -> {W // 2}x{H // 2} (1/2)" in log
    assert ("3 of 3 images have alpha; it is ignored without useMask" in log) == (variant == "rgba8" and not mask)
    _compare(png, ppm, half)


def test_the_mask_and_the_size_matter(gpu_device, captures, run):
    """what the comparisons above could not tell apart if the mask or the size were ignored"""
    first = lambda r: (r[0], r[1][0])                                        # eval @0 and the first loss line
    assert first(run(captures["ppm"], MASK)) != first(run(captures["ppm"]))
    assert first(run(captures["rgba8"], MASK)) != first(run(captures["rgba8"]))
    assert run(captures["ppm"], HALF)[0] != run(captures["ppm"])[0]


def test_opencv_camera_png_picture_and_png_mask_through_the_undistortion(gpu_device, tmp_path, run):
    pictures, masks = _pictures(), _masks()
    cameras, images, points = _sparse("OPENCV", (36.0, 34.5, 19.0, 12.75, 0.21, -0.06, 0.013, -0.009))
    a, b = str(tmp_path / "png"), str(tmp_path / "ppm")
    CR.write_dataset(a, cameras, images, points, {})
    _write_variant(a, "rgb8", pictures, masks)
    CR.write_dataset(b, cameras, images, points, {f"view_{k}.png": pictures[k] for k in range(3)}, masks={f"view_{k}.png": masks[k] * 255 for k in range(3)})
    png, ppm = run(a, MASK), run(b, MASK)
    assert "dataset: undistort: 3 of 3 images (OPENCV)" in png[3] and "dataset: png: 3 of 3 images, 3 masks" in png[3]
    _compare(png, ppm, False)
    png, ppm = run(a, MASK + HALF), run(b, MASK + HALF)
    _compare(png, ppm, True)


def test_a_pgm_mask_is_anded_with_the_picture_alpha(gpu_device, captures, tmp_path, run):
    """RGBA8 pictures whose alpha is 255 x the block masks AND masks/<stem>.pgm with other blocks, against the PPM capture whose PGM masks are
    the product of the two"""
    pictures, alpha = _pictures(), _masks()
    files = []
    for k in range(3):
        m = np.ones((H, W), np.uint8)
        m[5 + 2 * k:20 - k, 1 + 5 * k:12 + 6 * k] = 0
        files.append(m)
        both = alpha[k] & m
        assert (both != alpha[k]).any() and (both != m).any() and both.any()
    cameras, images, points = _sparse()
    a, b = str(tmp_path / "png"), str(tmp_path / "ppm")
    CR.write_dataset(a, cameras, images, points, {})
    _write_variant(a, "rgba8", pictures, alpha)
    os.makedirs(os.path.join(a, "masks"), exist_ok=True)
    for k in range(3):
        CR.write_pgm(os.path.join(a, "masks", f"view_{k}.pgm"), files[k] * 255)
    CR.write_dataset(b, cameras, images, points, {f"view_{k}.png": pictures[k] for k in range(3)}, masks={f"view_{k}.png": (alpha[k] & files[k]) * 255 for k in range(3)})
    png, ppm = run(a, MASK), run(b, MASK)
    assert "dataset: png: 3 of 3 images, 0 masks" in png[3] and "have alpha" not in png[3]
    _compare(png, ppm, False)
    assert (png[0], png[1][0]) != (run(captures["ppm"], MASK)[0], run(captures["ppm"], MASK)[1][0])       # the alpha alone is another mask
    png, ppm = run(a, MASK + HALF), run(b, MASK + HALF)
    _compare(png, ppm, True)


def test_a_truncated_png_stops_the_load_with_its_message(gpu_device, captures, tmp_path):
    bad = str(tmp_path / "bad")
    shutil.copytree(captures["rgb8"], bad)
    file = os.path.join(bad, "images", "view_1.png")
    data = open(file, "rb").read()
    _write(file, data[:len(data) // 2])
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "view_1.png: truncated" in p.stderr and "load data failed" in p.stdout, p.stderr[-2000:]
    _write(file, P.write_image(37, 29, 8, 2, np.zeros((29, 37 * 3), np.int64)))
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "view_1.png is 37x29 but its camera 2 is 40x24" in p.stderr, p.stderr[-2000:]
    _write(file, data)
    _write(os.path.join(bad, "masks", "view_2.png"), P.write_image(W, H, 8, 2, np.zeros((H, W * 3), np.int64)))
    p = subprocess.run([DRIVER, "--inputPath", bad, "--maxIteration", "1", "--useMask", "1", "--outputPath", str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "view_2.png has colour type 2; a PNG mask must be grayscale" in p.stderr, p.stderr[-2000:]


def test_one_load_thread_against_the_default(gpu_device, captures, run):
    one, default = run(captures["rgb8"], MASK + HALF, 1), run(captures["rgb8"], MASK + HALF)
    assert "dataset: png: 3 of 3 images, 3 masks" in one[3] and "(host, 1 threads, wall)" in one[3]
    assert one[:3] == default[:3]
    one, default = run(captures["rgb16"], MASK, 1), run(captures["rgb16"], MASK)
    assert one[0] == default[0] and one[1][0] == default[1][0]
