"""Dataset ingestion end to end on the GPU: 10 views of a 3000-splat synthetic scene at 96x64, rendered through divshot_amd.raster, go
to disk as a COLMAP capture (PPM images, PINHOLE cameras, the generating centres with their colours as the sparse points, written by
tests/colmap_ref.py); `gaussian_train --inputPath <dir> --maxIteration 300 --eval` trains from it. The dataset: and init: log lines carry
the written counts, the held-out PSNR at the end exceeds the one of the point-cloud start (the loader's `eval @0` line of the same
run), the saved PLY is finite, and a second run with --maxImageWidth 48 trains at 1/2."""
import json
import os
import re
import subprocess
import numpy as np
import pytest
import colmap_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
N, W, H, CAMS, ITERS = 3000, 96, 64, 10, 300
C0 = 0.28209479177387814


@pytest.fixture(scope="module")
def capture(gpu_device, tmp_path_factory):
    import torch
    import divshot_amd as dv
    from divshot_amd.raster import Rasterizer, params_to_device
    root = str(tmp_path_factory.mktemp("capture"))
    spec = dv.make_spec(N, W, H, sh_degree=0, n_cams=CAMS, seed=2)
    P = dv.synth_splats(spec)
    r = Rasterizer(0, max_splats=N, max_w=W, max_h=H)
    Pd = params_to_device(P, r.tdev)
    cameras, images, pixels = [], [], {}
    for ci in range(CAMS):
        cam = dv.synth_camera(spec, ci)
        img = r.forward(Pd, cam, sh_degree=0)
        torch.cuda.synchronize()
        name = f"view_{ci:03d}.ppm"
        pixels[name] = np.clip(np.rint(img.cpu().numpy().transpose(1, 2, 0) * 255.0), 0, 255).astype(np.uint8)
        view = np.array(list(cam.view), np.float64).reshape(4, 4)           # view[c][r]
        cameras.append(dict(id=ci + 1, model="PINHOLE", width=W, height=H, params=[cam.focal_x, cam.focal_y, W / 2.0, H / 2.0]))
        images.append(dict(id=ci + 1, q=CR.rotmat_to_qvec(view[:3, :3].T), t=view[3, :3], camera_id=ci + 1, name=name))
    r.close()
    rgb = np.clip(np.rint((0.5 + C0 * P["sh0"]) * 255.0), 0, 255).astype(np.uint8)
    points = [dict(id=k + 1, xyz=P["pos"][k], rgb=rgb[k]) for k in range(N)]
    CR.write_dataset(root, cameras, images, points, pixels)
    return root


def _run(args, out):
    p = subprocess.run([DRIVER, "--maxIteration", str(ITERS), "--eval", "--outputPath", out] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    return np.frombuffer(body, np.float32).reshape(n, 59)


def _psnr_at(log, it):
    m = re.search(rf"eval @{it}: \d+ views, PSNR ([-\d.e+]+) dB", log)
    assert m, log[-3000:]
    return float(m.group(1))


def test_training_from_a_capture_directory(capture, tmp_path):
    out = str(tmp_path / "full" / "iteration")
    p = _run(["--inputPath", capture], out)
    assert re.search(rf"dataset: {CAMS} cameras \(PINHOLE\), {W}x{H}, {N} points \(0 dropped\)", p.stderr), p.stderr[-3000:]
    assert re.search(rf"init: 3-NN scales for {N} points: [\d.]+ ms", p.stderr), p.stderr[-3000:]
    assert "evalHoldout 8: cameras 0 8" in p.stderr
    ev = json.load(open(out + f"_{ITERS}_eval.json"))
    start, end = _psnr_at(p.stderr, 0), ev["mean"]["psnr"]
    print(f"held-out PSNR: {start:.3f} dB at the point-cloud start, {end:.3f} dB after {ITERS} iterations")
    assert ev["iteration"] == ITERS and end == _psnr_at(p.stderr, ITERS)
    assert np.isfinite(start) and np.isfinite(end) and end > start
    ply = _read_ply(out + f"_{ITERS}.ply")
    assert len(ply) >= N and np.isfinite(ply).all()


def test_max_image_width_trains_at_half_size(capture, tmp_path):
    out = str(tmp_path / "half" / "iteration")
    p = _run(["--inputPath", capture, "--maxImageWidth", "48"], out)
    assert re.search(rf"dataset: {CAMS} cameras \(PINHOLE\), {W}x{H} -> {W // 2}x{H // 2} \(1/2\), {N} points \(0 dropped\)", p.stderr), p.stderr[-3000:]
    assert f"@ {W // 2}x{H // 2}" in p.stderr
    ev = json.load(open(out + f"_{ITERS}_eval.json"))
    assert ev["mean"]["psnr"] > _psnr_at(p.stderr, 0)
    assert np.isfinite(_read_ply(out + f"_{ITERS}.ply")).all()


def test_a_file_is_not_a_dataset(capture, tmp_path):
    p = subprocess.run([DRIVER, "--inputPath", os.path.join(capture, "images", "view_000.ppm"), "--maxIteration", "1", "--outputPath", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "not a directory" in p.stderr and "load data failed" in p.stdout
