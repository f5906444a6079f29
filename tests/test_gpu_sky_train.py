"""The sky model through the product: `gaussian_train --enableBg 1` on a tiny capture written here (the helpers of tests/colmap_ref.py):
8 pinhole cameras at the origin on a ring, looking outward and 40 degrees upward (64x48, 90 degrees wide, so that the held-out camera 0
is covered by its two neighbours), PPM images that show a smooth function of the ray direction and nothing else, and 40 sparse points
below every camera's view so that the load succeeds.
150 steps with --eval, with and without the flag. With it: the `config: skyModel` line, enableBg absent from the IGNORED line,
it_150.sky of the right size with finite values whose texels along the held-out camera's rays reproduce the sky function (the error is
printed; the function lies in [0.2, 0.8], so an untrained texture is off by at least 0.2 everywhere and the mean error must be below
0.1), and a held-out PSNR strictly above the run without the flag (both printed). Without it: no .sky file, no skyModel line. A resume
from iteration 150 logs that it read the texture; a two-rank run (TCP test backend, DVS_SAVE_ALL_RANKS=1) saves identical .sky files."""
import os
import re
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import sky_ref as SR
from test_gpu_multirank import DRIVER, _plugin_run
from test_sky_ref import intrinsics_camera

pytestmark = pytest.mark.gpu
W, H, F, CAMS, STEPS, HS = 64, 48, 32.0, 8, 150, 16


def sky_function(d):
    """directions [...,3] -> rgb [...,3] in [0.2, 0.8]"""
    return 0.5 + 0.3 * np.stack([d[..., 0], d[..., 1], d[..., 2]], -1)


def ring_rotation(k):
    a, pitch = 2 * np.pi * k / CAMS, np.radians(40.0)
    f = np.array([np.sin(a) * np.cos(pitch), -np.sin(pitch), np.cos(a) * np.cos(pitch)])     # Y is down: up is -Y
    right = np.array([np.cos(a), 0.0, -np.sin(a)])
    return np.stack([right, np.cross(f, right), f])


def rays_of(k):
    cam = intrinsics_camera(ring_rotation(k), np.zeros(3), F, F, W / 2.0, H / 2.0, W, H)
    return SR.rays(cam.proj[:], W, H)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sky_capture"))
    cameras, images, pixels = [], [], {}
    for k in range(CAMS):
        name = f"view_{k:03d}.ppm"
        pixels[name] = np.clip(np.rint(sky_function(rays_of(k)) * 255.0), 0, 255).astype(np.uint8)
        cameras.append(dict(id=k + 1, model="PINHOLE", width=W, height=H, params=[F, F, W / 2.0, H / 2.0]))
        images.append(dict(id=k + 1, q=CR.rotmat_to_qvec(ring_rotation(k)), t=np.zeros(3), camera_id=k + 1, name=name))
    r = np.random.default_rng(3)
    ang, rad = r.uniform(0, 2 * np.pi, 40), r.uniform(1.0, 3.0, 40)
    xyz = np.stack([rad * np.sin(ang), np.full(40, 2.0), rad * np.cos(ang)], 1)              # on the ground, 2 units below the cameras
    points = [dict(id=i + 1, xyz=xyz[i], rgb=(120, 110, 100)) for i in range(40)]
    CR.write_dataset(root, cameras, images, points, pixels)
    return root


def run(capture, out, *extra, steps=STEPS, env=None):
    base = {k: v for k, v in os.environ.items() if k not in ("DVS_SKY_RESOLUTION", "DVS_SKY_LR")}
    base.update(DVS_SKY_LR="0.05")            # a texel is seen in about 2 of 7 steps: 0.05 x 40 updates reaches any value of the function
    base.update(env or {})
    p = subprocess.run([DRIVER, "--inputPath", capture, "--maxIteration", str(steps), "--eval", "--outputPath", out] + list(extra), capture_output=True,
                       text=True, timeout=300, env=base)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return p.stderr


def psnr_at(log, it):
    m = re.search(rf"eval @{it}: \d+ views, PSNR ([-\d.e+]+) dB", log)
    assert m, log[-3000:]
    return float(m.group(1))


def read_sky(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"DVSSKY1\0"
    w, h = np.frombuffer(raw[8:16], "<u4")
    assert len(raw) == 16 + int(w) * int(h) * 12
    return np.frombuffer(raw[16:], "<f4").reshape(int(h), int(w), 3)


@pytest.fixture(scope="module")
def trained(capture, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sky_runs"))
    on, off = os.path.join(tmp, "on", "it"), os.path.join(tmp, "off", "it")
    return dict(on=on, off=off, log_on=run(capture, on, "--enableBg", "1", "--skyResolution", str(HS)), log_off=run(capture, off))


def test_the_flag_trains_and_saves_a_sky_that_beats_the_constant_background(trained):
    log = trained["log_on"]
    assert re.search(rf"config: skyModel {2 * HS}x{HS}: ", log), log[-3000:]
    ignored = re.findall(r"config: IGNORED by this build:(.*)", log)
    assert all("enableBg" not in line for line in ignored)
    tex = read_sky(trained["on"] + f"_{STEPS}.sky")
    assert tex.shape == (HS, 2 * HS, 3) and np.isfinite(tex).all()
    d = rays_of(0)                                                           # camera 0 is the held-out one (0 % 8 == 0)
    err = np.abs(np.moveaxis(SR.lookup(tex, d), 0, -1) - sky_function(d))
    p_on, p_off = psnr_at(log, STEPS), psnr_at(trained["log_off"], STEPS)
    print(f"texels along the held-out camera's rays: mean |error| {err.mean():.4f}, max {err.max():.4f}; held-out PSNR {p_on:.3f} dB with the sky, {p_off:.3f} dB without")
    assert err.mean() < 0.1
    assert p_on > p_off


def test_without_the_flag_nothing_of_the_sky_appears(trained):
    assert "skyModel" not in trained["log_off"] and "sky texture" not in trained["log_off"] and "sky:" not in trained["log_off"]
    folder = os.path.dirname(trained["off"])
    assert not [f for f in os.listdir(folder) if ".sky" in f]
    assert os.path.exists(trained["off"] + f"_{STEPS}.ply")


def test_resume_reads_the_texture(capture, trained):
    log = run(capture, trained["on"], "--enableBg", "1", "--skyResolution", str(HS), "--load_itr", str(STEPS), steps=STEPS + 10)
    assert re.search(rf"sky: read the {2 * HS}x{HS} texture from .*_{STEPS}\.sky", log), log[-3000:]
    assert np.isfinite(read_sky(trained["on"] + f"_{STEPS + 10}.sky")).all()


def test_resume_without_a_texture_starts_from_zero_and_says_so(capture, trained):
    log = run(capture, trained["off"], "--enableBg", "1", "--skyResolution", str(HS), "--load_itr", str(STEPS), steps=STEPS + 2)
    assert "the texture starts from zero" in log, log[-3000:]


def test_two_ranks_keep_identical_textures(capture, tmp_path):
    steps = 20
    out, res = _plugin_run(tmp_path, "two", ["--inputPath", capture, "--maxIteration", str(steps), "--enableBg", "1", "--skyResolution", str(HS)], 2,
                           extra_env={"DVS_SKY_LR": "0.05"}, timeout=300)
    a, b = open(out + f"_{steps}.sky", "rb").read(), open(out + f"_{steps}.sky.rank1", "rb").read()
    assert a == b and len(a) == 16 + 2 * HS * HS * 12
    assert np.abs(read_sky(out + f"_{steps}.sky")).max() > 0
