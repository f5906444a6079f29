"""dvs_make_camera_intrinsics (include/dvs_scene.h) without a GPU. With the principal point at the image centre and focal lengths derived
from a field of view the camera equals dvs_make_camera's bit for bit. With the principal point off centre the fp64 oracle draws a
camera-space point (X, Y, Z) at (fx X / Z + cx - 0.5, fy Y / Z + cy - 0.5): COLMAP puts a pixel's centre at i + 0.5, the rasterizer at i.
The bar is the one DESIGN section 8 row 6 reports for dvs_camera_downscale: 6e-7 px.

What that bar admits. Two things separate the oracle's mean from the formula, neither of them in the function under test:
  - proj is stored in float32: a generic entry carries a relative rounding error of 2^-24, worth up to (W / 2) * 1.2e-7 px. The cameras
    below are chosen so that every entry of view and proj is exactly representable (axis-aligned rotations, dyadic translations and
    intrinsics, power-of-two image sizes); generic rotations are covered by the bit-for-bit comparison with dvs_make_camera.
  - the rasterizer divides by w + 1e-7 (its own convention, oracle/dvs_oracle.hpp), which moves a mean by (W / 2) |ndc| 1e-7 / Z px.
    With Z >= 6, |ndc| <= 1.3 and W = 32 that is at most 3.5e-7 px (half of it at the level camera)."""
import ctypes as C
import math
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import _lib
from oracle.oracle import Oracle
from resolution_ref import camera_fields, same_bits

INVALID = 1
BAR = 6e-7                                                   # px; DESIGN section 8 row 6
W, H = 32, 16


def intrinsics_camera(R, t, fx, fy, cx, cy, w, h):
    cam = _lib.Camera()
    R = np.ascontiguousarray(R, np.float32)
    t = np.ascontiguousarray(t, np.float32)
    _lib.check(_lib.lib.dvs_make_camera_intrinsics(R.ctypes.data, t.ctypes.data, fx, fy, cx, cy, w, h, C.byref(cam)), "dvs_make_camera_intrinsics")
    return cam


@pytest.mark.parametrize("w,h,fov", [(142, 110, 60.0), (1920, 1080, 47.5), (96, 64, 73.0), (33, 17, 90.0)])
def test_centred_case_equals_make_camera_bit_for_bit(w, h, fov):
    spec = dv.make_spec(10, w, h, sh_degree=1, n_cams=5, seed=3, fov_x_deg=fov)
    tanx = math.tan(0.5 * float(np.float32(fov)) * 3.14159265358979323846 / 180.0)
    tany = tanx * h / w
    fx, fy = w / (2.0 * tanx), h / (2.0 * tany)
    for ci in range(5):
        want = dv.synth_camera(spec, ci)                                     # dvs_make_camera on a rotated, translated pose
        view = np.array(list(want.view), np.float32).reshape(4, 4)          # view[c][r]
        R, t = view[:3, :3].T.copy(), view[3, :3].copy()
        got = intrinsics_camera(R, t, fx, fy, w / 2.0, h / 2.0, w, h)
        assert bytes(got) == bytes(want), {k: (v, camera_fields(want)[k]) for k, v in camera_fields(got).items() if not same_bits(v, camera_fields(want)[k])}


def test_argument_checks():
    f = _lib.lib.dvs_make_camera_intrinsics
    R, t, out = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), _lib.Camera()
    good = [R.ctypes.data, t.ctypes.data, 40.0, 41.0, 16.5, 8.25, W, H, C.byref(out)]
    assert f(*good) == 0 and out.focal_x == 40.0 and out.focal_y == 41.0 and (out.width, out.height) == (W, H)
    assert out.tan_fovx == np.float32(W / 80.0) and out.tan_fovy == np.float32(H / 82.0)
    for i, bad in [(0, None), (1, None), (8, None), (2, 0.0), (3, -1.0), (2, float("nan")), (4, float("inf")), (5, float("nan")), (6, 0), (7, -3)]:
        args = list(good)
        args[i] = bad
        assert f(*args) == INVALID, (i, bad)


# rotations and translations whose float32 entries are exact, and intrinsics for which 2 f / size and 2 c / size - 1 are dyadic
POSES = [(np.eye(3), [0.0, 0.0, 0.0]),
         ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0.25, -0.5, 1.0]),
         ([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [-0.125, 0.375, 2.0])]
INTRINSICS = [(40.0, 20.0, 18.625, 5.75), (24.0, 28.0, 12.5, 9.125), (36.0, 36.0, 16.0, 8.0)]


@pytest.fixture(scope="module")
def scene():
    """600 splats with the parameters of the synthetic generator and centres spread over the frustum at depths 6 .. 12"""
    spec = dv.make_spec(600, W, H, sh_degree=1, seed=11)
    P = dv.synth_splats(spec)
    r = np.random.default_rng(5)
    z = r.uniform(6.0, 12.0, 600)
    P["pos"] = np.stack([r.uniform(-0.45, 0.45, 600) * z, r.uniform(-0.3, 0.3, 600) * z, z], 1).astype(np.float32)
    return P


@pytest.mark.parametrize("pose", range(len(POSES)))
@pytest.mark.parametrize("intr", range(len(INTRINSICS)))
def test_off_centre_principal_point_lands_where_colmap_says(scene, pose, intr):
    R, t = POSES[pose]
    fx, fy, cx, cy = INTRINSICS[intr]
    cam = intrinsics_camera(R, t, fx, fy, cx, cy, W, H)
    # the inputs are what the docstring says they are: nothing is lost when view and proj are stored as float32
    proj = np.array(list(cam.proj), np.float64).reshape(4, 4)               # proj[c][r]
    Rd, td = np.asarray(R, np.float64), np.asarray(t, np.float64)
    assert np.array_equal(proj[:3, 0], 2 * fx / W * Rd[0] + (2 * cx / W - 1) * Rd[2]) and proj[3, 0] == 2 * fx / W * td[0] + (2 * cx / W - 1) * td[2]
    assert np.array_equal(proj[:3, 1], 2 * fy / H * Rd[1] + (2 * cy / H - 1) * Rd[2]) and proj[3, 1] == 2 * fy / H * td[1] + (2 * cy / H - 1) * td[2]
    assert np.array_equal(proj[:3, 3], Rd[2]) and proj[3, 3] == td[2]
    cam_pts = scene["pos"].astype(np.float64) @ Rd.T + td                    # (X, Y, Z), exact in float64
    o = Oracle(np.float64)
    seen = 0
    for d, c in ((1, cam), (2, dv.camera_downscale(cam, 2))):
        o.forward(scene, c, sh_degree=1)
        m, radii, depth = o.get("mean2d").copy(), o.get("radii").copy(), o.get("depth").copy()
        vis = radii > 0
        seen += int(vis.sum())
        X, Y, Z = cam_pts[vis, 0], cam_pts[vis, 1], cam_pts[vis, 2]
        assert np.array_equal(depth[vis], Z)
        want = np.stack([(fx * X / Z + cx - 0.5 + 0.5) / d - 0.5, (fy * Y / Z + cy - 0.5 + 0.5) / d - 0.5], 1)
        err = np.abs(m[vis] - want).max()
        print(f"pose {pose} intrinsics {intr} 1/{d}: {int(vis.sum())} splats, worst {err:.3e} px")
        assert err <= BAR, (pose, intr, d, err)
    assert seen > 600                                                       # most splats are inside both images
