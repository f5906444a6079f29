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


def make_cams():
    cams = []
    for pos, tilt in (((0.13, -0.21, -2.4), 0.05), ((2.3, 0.17, -0.31), -0.08), ((0.05, 0.07, -0.55), 0.03)):
        R, t = look_at(pos, tilt)
        if len(cams) == 2:                                    # camera 2 looks along +z from inside the grid's extent
            R, t = np.eye(3), -np.asarray(pos, np.float64)
        cam = dv.Camera()
        R32, t32 = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(t, np.float32)
        _lib.check(dv.lib.dvs_make_camera_intrinsics(R32.ctypes.data, t32.ctypes.data, 30.0, 31.0, 16.3, 14.1, W, H, C.byref(cam)), "dvs_make_camera_intrinsics")
        cams.append(cam)
    return cams


def render_analytic(cam):
    """-> depth, alpha, rgb of the sphere |p| = RADIUS and the plane z = PLANE_Z seen by cam (view-space z of the nearest hit)"""
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
