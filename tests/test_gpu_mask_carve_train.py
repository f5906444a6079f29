"""The mask carve through the product: `gaussian_train` on a capture written here (the helpers of tests/colmap_ref.py): 4 pinhole cameras
of 96x64 on a ring around the origin, 400 sparse points — 200 inside a ball around the origin (the object), 200 scattered around and
behind it — PPM pictures, and PGM masks that are the ball's projected disc.

Run A trains 7 steps with --useMask 1 and saves; run B is the same with --maskCarve 50: no prune occasion falls inside, so the carve
runs once, before the save. B's PLY must hold, row for row and bit for bit, the rows of A's PLY that prune.foreground_votes +
prune.foreground_plan(..., 50) keep, computed here from A's PLY over the same four cameras with the evaluation's options; kept and
removed are at least 50 splats each, and B's log carries the `mask carve @7:` line with the same two counts.
Both runs pass --maxImageWidth 24, so the 96x64 views are trained at 24x16 (factor 4, 2 x 1 tiles): comparing two RUNS bit for bit needs
a trainer that repeats from run to run, and it does only while a view has at most two tiles (tests/test_gpu_dataset_jpeg.py explains
why: one fp32 atomic per tile and splat in the composite backward). The cameras here are those of dvs_camera_downscale and a mask pixel
is foreground when any of its 4x4 source pixels is, which is what the loader's box filter leaves nonzero.
A view that went through the undistortion keeps its validity apart when the carve is on at load: on the distorted capture of
tests/test_gpu_dataset_undistort.py with source masks (A) the blank pixels vote for nothing, on its pinhole twin (B: the restatement's
warped masks as files, so blank and masked-out pixels are one) they vote background. The two train identically at 20x12 (that file
asserts it), fg is the same and bg can only be larger in B, so what B keeps is a subset of what A keeps, row for row.
Without --useMask, --maskCarve 50 writes the PLY of the run without either flag, bit for bit, and logs the `inactive` line once.
DVS_MASK_CARVE=50 behaves as the flag does."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, prune
from divshot_amd.raster import Rasterizer, params_to_device
import colmap_ref as CR
from test_gpu_multirank import DRIVER, _read_ply_rows
from test_gpu_dataset_undistort import captures  # noqa: F401  (the fixture: distorted capture and its pinhole twin)
from test_sky_ref import intrinsics_camera

pytestmark = pytest.mark.gpu
W, H, F, D, CAMS, STEPS = 96, 64, 96.0, 4, 4, 7          # D: the factor --maxImageWidth 24 gives
DIST, BALL, MASK_BALL = 4.0, 0.7, 0.85
LINE = r"mask carve @(\d+): (\d+) -> (\d+) splats, (\d+) views, (\d+) never taken, votes [\d.]+ ms, plan\+compact [\d.]+ ms"


def pose(k):
    """world -> camera rotation (rows: right, down, forward; Y is down) and translation of camera k, which looks at the origin"""
    a = 2 * np.pi * k / CAMS + 0.3
    centre = DIST * np.array([np.sin(a), -0.25, -np.cos(a)]) / np.linalg.norm([1.0, 0.25])
    f = -centre / np.linalg.norm(centre)
    right = np.cross([0.0, 1.0, 0.0], f); right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(f, right), f])
    return R, -R @ centre


def disc():
    ys, xs = np.mgrid[0:H, 0:W]
    radius = F * MASK_BALL / np.sqrt(DIST * DIST - MASK_BALL * MASK_BALL)
    return (xs - W / 2.0 + 0.5) ** 2 + (ys - H / 2.0 + 0.5) ** 2 <= radius * radius


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("carve_capture"))
    r = np.random.default_rng(21)
    cameras, images, pixels, masks = [], [], {}, {}
    inside = disc()
    for k in range(CAMS):
        name = f"view_{k}.ppm"
        R, t = pose(k)
        q = CR.rotmat_to_qvec(R)
        px = r.integers(70, 110, (H, W, 3))
        px[inside] = (200, 80, 60) + r.integers(-10, 10, (int(inside.sum()), 3))
        pixels[name] = px.astype(np.uint8)
        masks[name] = inside.astype(np.uint8) * 255
        cameras.append(dict(id=k + 1, model="PINHOLE", width=W, height=H, params=[F, F, W / 2.0, H / 2.0]))
        images.append(dict(id=k + 1, q=q, t=t, camera_id=k + 1, name=name))
    v = r.normal(size=(200, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    ball = v * BALL * r.uniform(0, 1, (200, 1)) ** (1 / 3)
    far = np.zeros((0, 3))
    while len(far) < 200:
        p = r.uniform(-3.0, 3.0, (400, 3))
        far = np.concatenate([far, p[np.linalg.norm(p, axis=1) > 1.5]])[:200]
    points = [dict(id=i + 1, xyz=p, rgb=(200, 80, 60) if i < 200 else (90, 90, 90)) for i, p in enumerate(np.concatenate([ball, far]))]
    CR.write_dataset(root, cameras, images, points, pixels, masks=masks)
    return dict(root=root, images=images)


def run(capture, out, *extra, env=None):
    base = {k: v for k, v in os.environ.items() if k != "DVS_MASK_CARVE"}
    base.update(env or {})
    p = subprocess.run([DRIVER, "--inputPath", capture["root"], "--maxIteration", str(STEPS), "--maxImageWidth", str(W // D), "--outputPath", out] + list(extra),
                       capture_output=True, text=True, timeout=300, env=base)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return p.stderr


@pytest.fixture(scope="module")
def runs(gpu_device, capture, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("carve_runs"))
    out = {k: os.path.join(tmp, k, "it") for k in ("a", "b")}
    return dict(out=out, log_a=run(capture, out["a"], "--useMask", "1"), log_b=run(capture, out["b"], "--useMask", "1", "--maskCarve", "50"), tmp=tmp)


def ply(out):
    return out + f"_{STEPS}.ply"


def trainer_cameras(capture):
    """the loader's cameras: dvs_make_camera_intrinsics on the file's rotation (COLMAP's formula in double, rounded) and dvs_camera_downscale"""
    cams = []
    for im in capture["images"]:
        full = intrinsics_camera(CR.qvec_to_rotmat(im["q"]), np.asarray(im["t"], np.float64), F, F, W / 2.0, H / 2.0, W, H)
        low = dv.Camera()
        _lib.check(dv.lib.dvs_camera_downscale(C.byref(full), D, C.byref(low)), "dvs_camera_downscale")
        cams.append(low)
    return cams


def test_the_carve_keeps_exactly_the_rows_the_votes_keep(gpu_device, capture, runs):
    rows_a, rows_b = _read_ply_rows(ply(runs["out"]["a"])), _read_ply_rows(ply(runs["out"]["b"]))
    n = rows_a.shape[0]
    assert n == 400 and "mask carve" not in runs["log_a"] and "maskCarve" not in runs["log_a"]
    P = {"pos": rows_a[:, 0:3], "sh0": rows_a[:, 3:6], "shN": rows_a[:, 6:51].reshape(n, 3, 15).transpose(0, 2, 1), "opacity": rows_a[:, 51],
         "scale": rows_a[:, 52:55], "rot": rows_a[:, 55:59]}
    P = params_to_device({k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}, gpu_device)
    fg_low = disc().reshape(H // D, D, W // D, D).any(axis=(1, 3)).astype(np.float32)
    fg = [torch.from_numpy(fg_low).to(gpu_device) for _ in range(CAMS)]
    r = Rasterizer(0, max_splats=1024, max_w=W // D, max_h=H // D, max_views=CAMS)
    r.forward_views(P, trainer_cameras(capture), sh_degree=3, antialias=False)
    votes_fg, votes_bg = prune.foreground_votes(r, fg)
    action, offsets, count = prune.foreground_plan(votes_fg, votes_bg, 50)
    r.close()
    keep = action.cpu().numpy() == 0
    print(f"kept {count} of {n}; of the ball's 200 points {int(keep[:200].sum())}, of the scattered 200 {int(keep[200:].sum())}")
    assert count == int(keep.sum()) and count >= 50 and n - count >= 50
    assert rows_b.shape == (count, 59)
    assert np.array_equal(rows_b.view(np.uint32), rows_a[keep].view(np.uint32))
    found = re.findall(LINE, runs["log_b"])
    assert len(found) == 1, runs["log_b"][-3000:]
    it, a, b, views, never = (int(v) for v in found[0])
    assert (it, a, b, views) == (STEPS, n, count, CAMS) and 0 <= never <= n - count
    assert len(re.findall(r"config: maskCarve 50: at every prune occasion", runs["log_b"])) == 1


def test_without_masks_the_carve_is_inactive_and_changes_nothing(gpu_device, capture, runs):
    plain, carve = os.path.join(runs["tmp"], "c", "it"), os.path.join(runs["tmp"], "d", "it")
    log_plain = run(capture, plain)
    log_carve = run(capture, carve, "--maskCarve", "50")
    assert open(plain + f"_{STEPS}.ply", "rb").read() == open(carve + f"_{STEPS}.ply", "rb").read()
    assert len(re.findall(r"config: maskCarve 50: inactive: no training view has a mask \(useMask is off\)", log_carve)) == 1
    assert "mask carve @" not in log_carve and "maskCarve" not in log_plain and "mask carve" not in log_plain


def test_the_environment_variable_behaves_as_the_flag(gpu_device, capture, runs):
    out = os.path.join(runs["tmp"], "e", "it")
    log = run(capture, out, "--useMask", "1", env=dict(DVS_MASK_CARVE="50"))
    assert open(ply(out), "rb").read() == open(ply(runs["out"]["b"]), "rb").read()
    assert re.findall(LINE, log) == re.findall(LINE, runs["log_b"]) and len(re.findall(LINE, log)) == 1
    bad = run(capture, os.path.join(runs["tmp"], "f", "it"), "--useMask", "1", env=dict(DVS_MASK_CARVE="fifty"))
    assert len(re.findall(r"DVS_MASK_CARVE='fifty' is not a percentage", bad)) == 1 and "mask carve @" not in bad
    assert open(ply(os.path.join(runs["tmp"], "f", "it")), "rb").read() == open(ply(runs["out"]["a"]), "rb").read()


def test_blank_pixels_of_an_undistorted_view_vote_for_nothing(gpu_device, captures, tmp_path):
    a, b, _ = captures(True)
    rows, counts, logs = {}, {}, {}
    for tag, root in (("a", a), ("b", b)):
        out = os.path.join(str(tmp_path), tag, "it")
        logs[tag] = run(dict(root=root), out, "--useMask", "1", "--maskCarve", "50")
        found = re.findall(LINE, logs[tag])
        assert len(found) == 1, logs[tag][-3000:]
        counts[tag] = (int(found[0][1]), int(found[0][2]))
        rows[tag] = _read_ply_rows(ply(out))
        assert rows[tag].shape[0] == counts[tag][1]
    print(f"distorted capture: {counts['a'][0]} -> {counts['a'][1]}; pinhole twin: {counts['b'][0]} -> {counts['b'][1]}")
    assert "the blank pixels of the undistorted views vote for nothing" in logs["a"] and "blank pixels" not in logs["b"]
    assert counts["a"][0] == counts["b"][0] == 300 and 0 < counts["b"][1] <= counts["a"][1] < 300
    kept_a = {r.tobytes() for r in rows["a"]}
    assert all(r.tobytes() in kept_a for r in rows["b"])
