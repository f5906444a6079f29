"""Rendered views as PNG files, end to end on the GPU, modelled on tests/test_gpu_render_views.py: the same kind of pinhole capture (8
cameras at 64x48, PPM targets, 300 sparse points) goes through `gaussian_train` for 10 steps.

`--renderViews all --renderFormat png --renderLayers color,depth,alpha` writes exactly <stem>.png, <stem>_depth.png and <stem>_alpha.png
per camera; every file decodes with tests/png_ref.py to the right size and type (RGB8, GRAY16, GRAY8); each depth file carries the tEXt
chunk depth_scale; depth is 0 wherever the alpha file is 0; the logged byte count is the sum of the files' sizes. The colour PNG is
lossless — the bytes b of the render — and the Q 100 / 4:4:4 JPEG of the same saved model (a second run, --load_itr with zero further
steps) decodes to within e = 4 levels of b per pixel, the round-trip error tests/test_jpeg_write_format.py derives for that JPEG path
(ROUND_TRIP_ERROR_Q100_444), so the two differ by at most e (seen on an MI355X: 4 levels).

Saturation: at --renderDepthScale 30000 every depth of this scene (the points lie at z 2.5 .. 4) passes 65535 / 30000 = 2.18; the
logged count is the number of 65535 samples in the depth files. Off: without the new flags, and with them at their defaults, the file list and the JPEG bytes are
those of a run that does not know the flags — compared between two runs at 16x12, where the trainer repeats from run to run.
renderCameraToPng through a host that links the class (tests/hosts/render_png_one.cpp): a decodable file per layer, false for a bad
index or layer."""
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import png_ref
from test_jpeg_write_format import ROUND_TRIP_ERROR_Q100_444

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
W, H, CAMS, STEPS = 64, 48, 8, 10


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
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
    return root


def train(capture, out, *extra, steps=STEPS):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_RENDER_")}
    p = subprocess.run([DRIVER, "--inputPath", capture, "--maxIteration", str(steps), "--outputPath", out] + list(extra), capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stderr


def read_png(path):
    """-> (samples int64 [H][W][channels], colour type, depth, {keyword: text}) through tests/png_ref.py"""
    data = open(path, "rb").read()
    f = png_ref.decode_filtered(data)
    rows = png_ref.unfilter(f.filtered, f.width, f.height, f.depth, f.ctype)
    text, at = {}, 8
    while at < len(data):
        n, ctype = struct.unpack(">I4s", data[at:at + 8])
        if ctype == b"tEXt":
            k, v = data[at + 8:at + 8 + n].split(b"\x00", 1)
            text[k.decode("latin-1")] = v.decode("latin-1")
        at += 12 + n
    rgb, _ = png_ref.decode(data)                              # (the whole reference decoder accepts the file too)
    assert rgb.shape == (3, f.height, f.width)
    return png_ref.samples_of(rows, f.width, f.depth, f.ctype), f.ctype, f.depth, text


def test_all_layers_of_all_cameras_and_the_jpeg_of_the_same_model(gpu_device, capture, tmp_path):
    from test_gpu_render_views import decode_file
    out = str(tmp_path / "png" / "iteration")
    log = train(capture, out, "--renderViews", "all", "--renderFormat", "png", "--renderLayers", "color,depth,alpha")
    d = out + f"_{STEPS}_renders"
    names = sorted(os.listdir(d))
    assert names == sorted(f"view_{k:03d}{s}.png" for k in range(CAMS) for s in ("", "_depth", "_alpha")), names
    assert re.search(r"config: renderViews 3: every save also writes the test and training cameras as PNG files \(layers color,depth,alpha, depth x 1000 as 16-bit gray", log), log[-3000:]
    m = re.search(rf"render @{STEPS}: {CAMS} views, {3 * CAMS} files, (\d+) bytes, filtering [\d.]+ ms \(device, events\), deflate [\d.]+ ms \(host, (\d+) threads, wall\), "
                  r"(\d+) depth samples saturated", log)
    assert m, log[-3000:]
    assert int(m.group(1)) == sum(os.path.getsize(os.path.join(d, n)) for n in names) and 1 <= int(m.group(2)) <= 8 and int(m.group(3)) == 0
    assert "transform" not in m.group(0) and "entropy" not in m.group(0)
    colour = {}
    for k in range(CAMS):
        c, ctype, depth, text = read_png(os.path.join(d, f"view_{k:03d}.png"))
        assert c.shape == (H, W, 3) and (ctype, depth) == (2, 8) and text == {} and c.std() > 5
        z, ctype, depth, text = read_png(os.path.join(d, f"view_{k:03d}_depth.png"))
        assert z.shape == (H, W, 1) and (ctype, depth) == (0, 16) and text == {"depth_scale": "1000"}
        a, ctype, depth, text = read_png(os.path.join(d, f"view_{k:03d}_alpha.png"))
        assert a.shape == (H, W, 1) and (ctype, depth) == (0, 8) and text == {}
        assert (z[a == 0] == 0).all()                          # no depth where nothing was rendered
        seen = z[a >= 128]                                     # where the splats cover the pixel the depth is the scene's: 2.5 .. 4 and some blur
        assert seen.size > 100 and 1500 < seen.min() and seen.max() < 6000, (seen.size, seen.min(), seen.max())
        colour[k] = c
    # the JPEG of the same parameters: a second run that loads the saved model and saves at once
    same = str(tmp_path / "jpg" / "iteration")
    os.makedirs(os.path.dirname(same))
    shutil.copy(out + f"_{STEPS}.ply", same + f"_{STEPS}.ply")
    log2 = train(capture, same, "--load_itr", str(STEPS), "--renderViews", "all", "--renderFormat", "jpg", "--renderQuality", "100", "--renderSampling", "444")
    assert "(resumed" in log2 and open(same + f"_{STEPS}.ply", "rb").read() == open(out + f"_{STEPS}.ply", "rb").read()
    assert sorted(os.listdir(same + f"_{STEPS}_renders")) == [f"view_{k:03d}.jpg" for k in range(CAMS)]
    worst = 0
    for k in range(CAMS):
        got, _ = decode_file(os.path.join(same + f"_{STEPS}_renders", f"view_{k:03d}.jpg"))
        worst = max(worst, int(np.abs(got.astype(np.int64) - colour[k].transpose(2, 0, 1)).max()))
    print(f"largest difference between the lossless PNG and the Q100 4:4:4 JPEG of one render: {worst} levels, bound {ROUND_TRIP_ERROR_Q100_444}")
    assert worst <= ROUND_TRIP_ERROR_Q100_444


def test_saturated_depth_samples_are_counted_and_a_subset_of_layers(gpu_device, capture, tmp_path):
    out = str(tmp_path / "sat" / "iteration")
    log = train(capture, out, "--maxImageWidth", "16", "--renderViews", "train", "--renderFormat", "png", "--renderLayers", "color,depth", "--renderDepthScale", "30000",
                "--eval", steps=4)
    d = out + "_4_renders"
    names = sorted(os.listdir(d))
    assert names == sorted(f"view_{k:03d}{s}.png" for k in range(1, CAMS) for s in ("", "_depth")), names      # camera 0 is held out
    m = re.search(rf"render @4: {CAMS - 1} views, {2 * (CAMS - 1)} files, (\d+) bytes, .* (\d+) depth samples saturated", log)
    assert m and int(m.group(1)) == sum(os.path.getsize(os.path.join(d, n)) for n in names), log[-3000:]
    full = 0
    for k in range(1, CAMS):
        z, ctype, depth, text = read_png(os.path.join(d, f"view_{k:03d}_depth.png"))
        assert z.shape == (12, 16, 1) and (ctype, depth) == (0, 16) and text == {"depth_scale": "30000"}
        full += int(np.count_nonzero(z == 65535))
    assert int(m.group(2)) == full and full > 0


def test_off_and_the_defaults_spelled_out_leave_the_jpeg_output_as_it_is(gpu_device, capture, tmp_path):
    small = ("--maxImageWidth", "16", "--renderViews", "all")
    out_a, out_b, out_none = (str(tmp_path / t / "iteration") for t in ("a", "b", "none"))
    log_a = train(capture, out_a, *small)
    log_b = train(capture, out_b, *small, "--renderFormat", "jpg", "--renderLayers", "color", "--renderDepthScale", "1000")
    log_none = train(capture, out_none, "--maxImageWidth", "16")
    for out, log in ((out_a, log_a), (out_b, log_b)):
        assert sorted(os.listdir(out + f"_{STEPS}_renders")) == [f"view_{k:03d}.jpg" for k in range(CAMS)]
        assert sorted(os.listdir(os.path.dirname(out))) == [f"iteration_{STEPS}.ply", f"iteration_{STEPS}_renders"]
        assert re.search(rf"render @{STEPS}: {CAMS} views, \d+ bytes, transform [\d.]+ ms \(device, events\), entropy coding [\d.]+ ms \(host, \d+ threads, wall\)$", log, re.M), log[-3000:]
        assert "as JPEG files (quality 90, 4:2:0)" in log and "PNG" not in log and "deflate" not in log and "DVS_RENDER" not in log
    for k in range(CAMS):
        name = f"view_{k:03d}.jpg"
        assert open(os.path.join(out_a + f"_{STEPS}_renders", name), "rb").read() == open(os.path.join(out_b + f"_{STEPS}_renders", name), "rb").read(), name
    strip = lambda log: [re.sub(r"[\d.]+ ms", "ms", l) for l in log.splitlines() if "config: render" in l or "render @" in l]
    assert strip(log_a) == strip(log_b)
    assert sorted(os.listdir(os.path.dirname(out_none))) == [f"iteration_{STEPS}.ply"] and "render" not in log_none


def test_bad_environment_values_are_reported_once_and_ignored(gpu_device, capture, tmp_path):
    out = str(tmp_path / "env" / "iteration")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_RENDER_")}
    env.update(DVS_RENDER_VIEWS="1", DVS_RENDER_FORMAT="png", DVS_RENDER_LAYERS="9", DVS_RENDER_DEPTH_SCALE="-2", DVS_RENDER_PNG_LEVEL="12")
    p = subprocess.run([DRIVER, "--inputPath", capture, "--maxIteration", "2", "--outputPath", out, "--maxImageWidth", "16", "--eval"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    for var in ("DVS_RENDER_LAYERS='9'", "DVS_RENDER_DEPTH_SCALE='-2'", "DVS_RENDER_PNG_LEVEL='12'"):
        assert len(re.findall(re.escape(var) + r".*ignored", p.stderr)) == 1, (var, p.stderr[-3000:])
    assert sorted(os.listdir(out + "_2_renders")) == ["view_000.png"] and "layers color, depth x 1000 as 16-bit gray with 0 = no depth, zlib level 6" in p.stderr
    assert read_png(os.path.join(out + "_2_renders", "view_000.png"))[0].shape == (12, 16, 3)


def test_render_camera_to_png_through_the_class(gpu_device, tmp_path):
    exe = str(tmp_path / "render_png_one")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hosts", "render_png_one.cpp"), "-o", exe,
                           "-L", LIB, "-lgstrain", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    stem = str(tmp_path / "camera_1")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_RENDER_")}
    p = subprocess.run([exe, "synthetic:N=2000,W=64,H=48,cams=3,sh=1,seed=4", "5", stem], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "before_load 0, layers written 7, camera -1 0, past the end 0, bad layers 0, missing directory 0, iterations 6, terminated 0" in p.stdout, p.stdout + p.stderr
    c, ctype, depth, _ = read_png(stem + "_1.png")
    assert c.shape == (48, 64, 3) and (ctype, depth) == (2, 8) and c.std() > 1
    z, ctype, depth, text = read_png(stem + "_2.png")
    assert z.shape == (48, 64, 1) and (ctype, depth) == (0, 16) and text == {"depth_scale": "1000"} and z.max() > 0
    a, ctype, depth, _ = read_png(stem + "_4.png")
    assert a.shape == (48, 64, 1) and (ctype, depth) == (0, 8) and a.max() > 0 and (z[a == 0] == 0).all()
    assert sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("camera_1")) == ["camera_1_1.png", "camera_1_2.png", "camera_1_4.png"]
