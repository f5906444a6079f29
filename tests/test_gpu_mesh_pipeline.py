"""Mesh extraction end to end. Python: 4000 opaque splats of scale 0.25 voxel on the unit sphere, six cameras on the axes, 96x96 images,
depth_maps -> TsdfGrid at resolution 48 over [-1.5, 1.5]^3 -> extract; the median of | |v| - 1 | must stay within 2 voxels (depth within
the shell's +-3 sigma = 0.75 voxel, 0.5 voxel of interpolation, 0.5 voxel of nearest-pixel sampling). CLI: --meshResolution writes
<out>_<it>_mesh.ply whose counts are the log line's; without the flag nothing is written; --exportMesh keeps its IGNORED line."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, mesh
from divshot_amd.raster import Rasterizer, params_to_device
import mesh_ref as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")


def axis_camera(pos, size):
    pos = np.asarray(pos, np.float64)
    z = -pos / np.linalg.norm(pos)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.ascontiguousarray(np.stack([x, y, z]), np.float32)
    t = np.ascontiguousarray(-np.stack([x, y, z]) @ pos, np.float32)
    cam = dv.Camera()
    _lib.check(dv.lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, 60.0, size, size, C.byref(cam)), "dvs_make_camera")
    return cam


def test_python_end_to_end(gpu_device):
    n, res, size = 4000, 48, 96
    voxel = 3.0 / res
    r = np.random.default_rng(5)
    pos = r.normal(0, 1, (n, 3)); pos /= np.linalg.norm(pos, axis=1, keepdims=True)
    P = {"pos": pos, "sh0": r.uniform(-1, 1, (n, 3)), "shN": np.zeros((n, 15, 3)), "opacity": np.full(n, 6.0),
         "scale": np.full((n, 3), np.log(0.25 * voxel)), "rot": np.tile([1.0, 0, 0, 0], (n, 1))}
    P = params_to_device({k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}, gpu_device)
    cams = [axis_camera(p, size) for p in ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3))]
    ras = Rasterizer(0, max_splats=4096, max_w=size, max_h=size, max_views=6)
    rgb = ras.forward_views(P, cams, sh_degree=0)
    depth, alpha = mesh.depth_maps(ras)
    grid = mesh.TsdfGrid((-1.5, -1.5, -1.5), voxel, (res + 1, res + 1, res + 1))
    grid.integrate(cams, depth, alpha, rgb, 4 * voxel)
    xyz, col, tri = grid.extract()
    ras.close()
    assert len(xyz) > 100 and len(tri) > 100
    assert tri.max() < len(xyz)
    assert (xyz >= -1.5).all() and (xyz <= 1.5).all()
    med = float(np.median(np.abs(np.linalg.norm(xyz.astype(np.float64), axis=1) - 1.0)))
    print(f"{len(xyz)} vertices, {len(tri)} triangles, median | |v| - 1 | = {med / voxel:.3f} voxel")
    assert med <= 2 * voxel


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    def go(extra, env_extra=None):
        out = str(tmp_path_factory.mktemp("out") / "iteration")
        env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_MESH_")}
        env.update(env_extra or {})
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=20000,W=256,H=192,cams=8,sh=1,seed=9", "--maxIteration", "60", "--outputPath", out] + extra,
                           capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        return out, p.stderr
    return go


def check_mesh_file(out, log):
    path = out + "_60_mesh.ply"
    assert os.path.exists(path), log[-3000:]
    xyz, rgb, tri = MR.parse_mesh_ply(path)
    lines = re.findall(r"mesh @60: (\d+) vertices, (\d+) triangles, grid (\d+)x(\d+)x(\d+), voxel (\S+), bounds ([^ ]+)[ ,]", log)
    assert lines, log[-3000:]
    nv, nt = int(lines[-1][0]), int(lines[-1][1])
    assert (len(xyz), len(tri)) == (nv, nt)
    b = [float(v) for v in lines[-1][6].rstrip(",").split(",")]
    assert len(b) == 6
    if nv:
        assert tri.max() < nv
        assert (xyz >= np.array(b[:3]) - 1e-5).all() and (xyz <= np.array(b[3:]) + 1e-5).all()
    return nv, nt


def test_cli_writes_the_mesh(run):
    out, log = run(["--meshResolution", "32"])
    assert re.search(r"config: meshResolution 32:", log), log[-3000:]
    check_mesh_file(out, log)


def test_cli_without_the_flag_writes_no_mesh(run):
    out, log = run([])
    assert not os.path.exists(out + "_60_mesh.ply") and "mesh @" not in log and "config: meshResolution" not in log
    assert os.path.exists(out + "_60.ply")


def test_cli_export_mesh_flag_keeps_its_meaning_and_bounds_override(run):
    """--exportMesh 1 still lands in the IGNORED line; with DVS_MESH_BOUNDS around the synthetic scene's splats (they lie at z in [2, 12],
    outside the cube of 3 x extent about the cameras, so the default box is empty there) the mesh is not empty"""
    out, log = run(["--meshResolution", "32", "--exportMesh", "1"], {"DVS_MESH_BOUNDS": "-3,-2.5,2,3,2.5,8"})
    ign = [ln for ln in log.splitlines() if "IGNORED by this build:" in ln]
    assert ign and "exportMesh" in ign[0] and "normalConsistencyLoss" in ign[0]
    nv, nt = check_mesh_file(out, log)
    assert nv > 0 and nt > 0
