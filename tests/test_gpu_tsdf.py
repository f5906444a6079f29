"""dvs_tsdf_integrate against the fp64 restatement tests/tsdf_ref.py: a 20x17x13 grid, three 33x29 cameras with an off-centre principal
point looking at analytic depth images of a sphere in front of a plane (built in numpy). Camera 0 is masked in a rectangle, camera 2
stands inside the grid's extent so that part of the grid is behind it, a strip of every alpha image is 0.4. The poses are generic
(no axis-aligned symmetry), chosen on the CPU so that the voxels the reference excludes stay <= 2 %."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, mesh
import tsdf_ref as TR

pytestmark = pytest.mark.gpu
W, H = 33, 29
DIMS, ORIGIN, VOXEL, TRUNC = (20, 17, 13), (-0.97, -0.83, -0.61), 0.1, 0.3
RADIUS, PLANE_Z = 0.45, 0.5


def look_at(pos, tilt):
    pos = np.asarray(pos, np.float64)
    z = -pos / np.linalg.norm(pos)
    up = np.array([np.sin(tilt), np.cos(tilt), 0.1])
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ pos


def camera(R, t):
    cam = dv.Camera()
    R32, t32 = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(t, np.float32)
    _lib.check(dv.lib.dvs_make_camera_intrinsics(R32.ctypes.data, t32.ctypes.data, 30.0, 31.0, 16.3, 14.1, W, H, C.byref(cam)), "dvs_make_camera_intrinsics")
    return cam


def make_cams():
    cams = []
    for pos, tilt in (((0.13, -0.21, -2.4), 0.05), ((2.3, 0.17, -0.31), -0.08), ((0.05, 0.07, -0.55), 0.03)):
        R, t = look_at(pos, tilt)
        if len(cams) == 2:                                    # camera 2 looks along +z from inside the grid's extent
            R, t = np.eye(3), -np.asarray(pos, np.float64)
        cams.append(camera(R, t))
    return cams


def render_analytic(cam, view=None):
    """-> depth, alpha, rgb of the sphere |p| = RADIUS and the plane z = PLANE_Z seen by cam (view-space z of the nearest hit); with
    `view` (0..15) the green channel carries the view's index, so that no two views' colour maps are interchangeable"""
    V = TR.mat(cam.view)
    R, t = V[:3, :3], V[:3, 3]
    o = -R.T @ t
    y, x = np.mgrid[0:H, 0:W]
    d_cam = np.stack([(x + 0.5 - 16.3) / 30.0, (y + 0.5 - 14.1) / 31.0, np.ones((H, W))], -1)
    d = d_cam @ R
    b = d @ o; a = (d * d).sum(-1); c = o @ o - RADIUS ** 2
    disc = b * b - a * c
    s_sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    s_sph = np.where(s_sph > 0, s_sph, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        s_pl = np.where(np.abs(d[..., 2]) > 1e-9, (PLANE_Z - o[2]) / d[..., 2], np.inf)
    s_pl = np.where(s_pl > 0, s_pl, np.inf)
    s = np.minimum(s_sph, s_pl)
    hit = np.isfinite(s)
    alpha = np.where(hit, 1.0, 0.0)
    alpha[:, 3:6] = np.where(hit[:, 3:6], 0.4, 0.0)          # a strip below the 0.5 threshold
    depth = np.where(hit, s, 0.0)
    rgb = np.stack([0.5 + 0.5 * np.sin(0.3 * x + 0.1 * y), x / W + 0 * y, np.where(s_sph <= s_pl, 0.9, 0.2) + 0 * x], 0)
    if view is not None:
        rgb[1] = (view + x / W) / 16
    return depth.astype(np.float32), alpha.astype(np.float32), rgb.astype(np.float32)


@pytest.fixture(scope="module")
def case():
    cams = make_cams()
    maps = [render_analytic(c) for c in cams]
    depth, alpha, rgb = (np.stack([m[k] for m in maps]) for k in range(3))
    mask0 = np.ones((H, W), np.float32); mask0[8:15, 10:20] = 0.0
    masks = [mask0, None, None]
    nx, ny, nz = DIMS
    state = (np.ones((nz, ny, nx)), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx, 3)))
    excl = TR.integrate(state, ORIGIN, VOXEL, DIMS, cams, depth, alpha, rgb, masks, TRUNC)
    return cams, depth, alpha, rgb, masks, state, excl


def gpu_integrate(case, gpu_device, chunks):
    cams, depth, alpha, rgb, masks, _, _ = case
    g = mesh.TsdfGrid(ORIGIN, VOXEL, DIMS)
    for lo, hi in chunks:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(gpu_device)
        g.integrate(cams[lo:hi], dev(depth), dev(alpha), dev(rgb), TRUNC, masks=[None if m is None else torch.from_numpy(m).to(gpu_device) for m in masks[lo:hi]])
    return g.download()


def test_reference_exercises_every_rule(case):
    cams, depth, alpha, rgb, masks, (tsdf, weight, col), excl = case
    print(f"excluded voxels: {int(excl.sum())} of {excl.size}")
    assert excl.mean() <= 0.02
    assert set(np.unique(weight)) >= {0.0, 1.0, 2.0, 3.0}
    assert (tsdf < 0).any() and (tsdf == 1.0).any() and ((tsdf > 0) & (tsdf < 1)).any()
    p = TR.voxel_centres(ORIGIN, VOXEL, DIMS)
    assert ((p @ TR.mat(cams[2].view)[:3, :3].T + TR.mat(cams[2].view)[:3, 3])[..., 2] < 0).any(), "nothing behind camera 2"


def test_matches_the_reference(case, gpu_device):
    _, _, _, _, _, (tsdf, weight, col), excl = case
    t, w, c = gpu_integrate(case, gpu_device, [(0, 3)])
    keep = ~excl
    assert np.array_equal(w[keep], weight[keep])
    t_err, c_err = np.abs(t - tsdf)[keep].max(), np.abs(c - col)[keep].max()
    print(f"tsdf err {t_err:.3e}, rgb err {c_err:.3e}")
    assert t_err <= 1e-5 and c_err <= 1e-5


def test_one_call_equals_three_calls_bit_for_bit(case, gpu_device):
    one = gpu_integrate(case, gpu_device, [(0, 3)])
    three = gpu_integrate(case, gpu_device, [(0, 1), (1, 2), (2, 3)])
    for a, b in zip(one, three):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_oversized_dims_are_refused(gpu_device):
    big = (C.c_int32 * 3)(1025, 8, 8)
    assert dv.lib.dvs_tsdf_bytes(big) == 0 and dv.lib.dvs_mesh_scratch_bytes(big) == 0
    desc = _lib.TsdfGridDesc()
    assert dv.lib.dvs_tsdf_create((C.c_float * 3)(0, 0, 0), 0.1, big, C.byref(desc)) == 1          # DVS_ERR_INVALID
    with pytest.raises(dv.DvsError):
        mesh.TsdfGrid((0, 0, 0), 0.1, (8, 1025, 8))
    g = mesh.TsdfGrid((0, 0, 0), 0.1, (8, 8, 8))
    g.desc.dims[2] = 1025
    z = torch.zeros((1, 3, H, W), device=gpu_device)
    cam = make_cams()[:1]
    assert dv.lib.dvs_tsdf_integrate(None, C.byref(g.desc), (dv.Camera * 1)(*cam), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, W, H, 0.3) == 1
    assert dv.lib.dvs_tsdf_clear(None, C.byref(g.desc)) == 1


# ---- sixteen views in one call ------------------------------------------------------------------------------------------------------
# dvs_tsdf_integrate takes up to 16 views per call and the kernel finds each view's camera and mask pointer in its argument block by
# the view's index. Sixteen cameras on a spiral over the half-space in front of the plane; camera 11 looks along +z from inside the
# grid's extent; every view's green channel carries its index; masks on views 5 and 15 only. A voxel is excluded when it is within 1e-3
# pixel of a rounding boundary in some view (about 0.4 % of the voxels per view): the cap grows from the three views' 2 % to 10 %.
N16, MASKED16, INSIDE16 = 16, (5, 15), 11
BAR = 1e-5


def make_cams16():
    cams = []
    for n in range(N16):
        th, ph, dist = 0.25 + 0.05 * n, 0.4 + 2.39996 * n, 2.2 + 0.03 * n          # (the golden angle: no two azimuths alike)
        pos = dist * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])
        R, t = look_at(pos, 0.04 * (n - 8))
        if n == INSIDE16:
            pos = np.array([-0.63, 0.41, -0.55])
            R, t = np.eye(3), -pos
        cams.append(camera(R, t))
    return cams


def reference16(cams, maps, masks, views):
    nx, ny, nz = DIMS
    depth, alpha, rgb = (np.stack([maps[v][k] for v in views]) for k in range(3))
    state = (np.ones((nz, ny, nx)), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx, 3)))
    excl = TR.integrate(state, ORIGIN, VOXEL, DIMS, [cams[v] for v in views], depth, alpha, rgb, [masks[v] for v in views], TRUNC)
    return state, excl


def build_case16():
    """the 16-view input and its reference, with every condition on the input asserted: CPU only"""
    cams = make_cams16()
    maps = [render_analytic(c, view=v) for v, c in enumerate(cams)]
    masks = [None] * N16
    for v in MASKED16:
        hit = (maps[v][1] >= 0.5)
        m = np.ones((H, W), np.float32); m[8:15, 10:20] = 0.0
        assert hit[8:15, 10:20].all(), f"view {v}'s mask rectangle leaves the region the view hits"
        masks[v] = m
    every = list(range(N16))
    (tsdf, weight, col), excl = reference16(cams, maps, masks, every)
    print(f"16 views: excluded voxels {int(excl.sum())} of {excl.size} ({100 * excl.mean():.2f} %), max weight {int(weight.max())}")
    assert excl.mean() <= 0.10
    assert weight.max() >= 12 and set(np.unique(weight)) >= set(float(k) for k in range(13))
    keep = ~excl

    def differs(other):
        (t2, _, c2), _ = other
        return max(np.abs(t2 - tsdf)[keep].max(), np.abs(c2 - col)[keep].max())
    for v in every:                                          # no camera or map reduces to another: leaving one out shows
        d = differs(reference16(cams, maps, masks, [u for u in every if u != v]))
        assert d > 100 * BAR, f"leaving out view {v} changes the reference by {d:.2e} only"
    for v in range(N16 - 1):                                 # ... nor does reading the neighbour's maps or camera instead
        swapped = every.copy(); swapped[v], swapped[v + 1] = swapped[v + 1], swapped[v]
        d_maps = differs(reference16(cams, [maps[u] for u in swapped], masks, every))
        d_cams = differs(reference16([cams[u] for u in swapped], maps, masks, every))
        assert min(d_maps, d_cams) > 100 * BAR, (v, d_maps, d_cams)
    for v in MASKED16:                                       # the masks change the result, each on its own
        d = differs(reference16(cams, maps, [None if u == v else m for u, m in enumerate(masks)], every))
        assert d > 100 * BAR, f"view {v}'s mask changes the reference by {d:.2e} only"
        moved = masks.copy(); moved[v], moved[v - 1] = None, masks[v]          # ... and on its own view: not on the one before
        d = differs(reference16(cams, maps, moved, every))
        assert d > 100 * BAR, f"view {v}'s mask on view {v - 1} changes the reference by {d:.2e} only"
    p = TR.voxel_centres(ORIGIN, VOXEL, DIMS)
    V = TR.mat(cams[INSIDE16].view)
    assert ((p @ V[:3, :3].T + V[:3, 3])[..., 2] < 0).any(), "nothing behind the camera inside the grid"
    depth, alpha, rgb = (np.stack([m[k] for m in maps]) for k in range(3))
    return cams, depth, alpha, rgb, masks, (tsdf, weight, col), excl


@pytest.fixture(scope="module")
def case16():
    return build_case16()


def test_sixteen_views_match_the_reference(case16, gpu_device):
    _, _, _, _, _, (tsdf, weight, col), excl = case16
    t, w, c = gpu_integrate(case16, gpu_device, [(0, N16)])
    keep = ~excl
    assert np.array_equal(w[keep], weight[keep])
    t_err, c_err = np.abs(t - tsdf)[keep].max(), np.abs(c - col)[keep].max()
    print(f"tsdf err {t_err:.3e}, rgb err {c_err:.3e}")
    assert t_err <= BAR and c_err <= BAR


def test_one_call_equals_two_and_sixteen_calls_bit_for_bit(case16, gpu_device):
    one = gpu_integrate(case16, gpu_device, [(0, 16)])
    two = gpu_integrate(case16, gpu_device, [(0, 8), (8, 16)])
    sixteen = gpu_integrate(case16, gpu_device, [(v, v + 1) for v in range(N16)])
    for a, b, c in zip(one, two, sixteen):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_seventeen_views_are_refused(case16, gpu_device):
    cams = case16[0]
    g = mesh.TsdfGrid(ORIGIN, VOXEL, DIMS)
    z = torch.zeros((17, 3, H, W), device=gpu_device)
    arr = (dv.Camera * 17)(*(cams + cams[:1]))
    assert dv.lib.dvs_tsdf_integrate(None, C.byref(g.desc), arr, 17, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, W, H, TRUNC) == 1   # DVS_ERR_INVALID
    assert dv.lib.dvs_tsdf_integrate(None, C.byref(g.desc), arr, 16, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, W, H, TRUNC) == 0
    torch.cuda.synchronize()
    t, w, _ = g.download()
    assert (t == 1.0).all() and (w == 0.0).all()             # (alpha 0 everywhere: the accepted call fused nothing, the refused one ran nothing)
