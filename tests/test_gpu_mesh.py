"""dvs_mesh_extract_* against the numpy restatement tests/mesh_ref.py on grids uploaded directly: a 24x21x19 grid holding the exact signed
distance (in voxels) of a sphere of radius 7 voxels about a generic centre, fully observed; the same with weight 0 in a slab; an
all-positive grid. Positions are compared in voxels: origin and voxel are binary fractions, so the kernel's only roundings are those of
a / (a - b) and of i + t (half an ulp of 24: 1e-6 voxel), ten times inside the 1e-5 bar."""
import numpy as np
import pytest
from divshot_amd import mesh
import mesh_ref as MR

pytestmark = pytest.mark.gpu
NX, NY, NZ = 24, 21, 19
ORIGIN, VOXEL = (-1.5, -1.25, -1.0), 0.125
CENTRE, RADIUS = np.array([11.3, 10.2, 9.1]), 7.0


def sphere_grid():
    k, j, i = np.mgrid[0:NZ, 0:NY, 0:NX]
    tsdf = (np.sqrt((i - CENTRE[0]) ** 2 + (j - CENTRE[1]) ** 2 + (k - CENTRE[2]) ** 2) - RADIUS).astype(np.float32)
    rgb = np.stack([i / NX, j / NY, k / NZ], -1).astype(np.float32)
    return tsdf, rgb


def extract(tsdf, weight, rgb):
    g = mesh.TsdfGrid(ORIGIN, VOXEL, (NX, NY, NZ))
    g.upload(tsdf, weight, rgb)
    return g.extract()


@pytest.fixture(scope="module")
def full(gpu_device):
    tsdf, rgb = sphere_grid()
    w = np.ones_like(tsdf)
    return extract(tsdf, w, rgb), MR.marching_tets(tsdf, w, rgb, ORIGIN, VOXEL)


def test_sphere_equals_the_reference(full):
    (xyz, rgb, tri), (rxyz, rrgb, rtri) = full
    assert len(xyz) == len(rxyz) > 500 and len(tri) == len(rtri) > 1000
    assert np.array_equal(tri.astype(np.int64), rtri)
    err = np.abs(xyz.astype(np.float64) - rxyz).max() / VOXEL
    print(f"{len(xyz)} vertices, {len(tri)} triangles, position error {err:.3e} voxel")
    assert err <= 1e-5
    assert np.abs(rgb.astype(int) - rrgb.astype(int)).max() <= 1          # (a byte may round the other way at an exact .5)


def test_sphere_is_closed_oriented_and_on_the_surface(full):
    (xyz, _, tri), _ = full
    t = tri.astype(np.int64)
    half = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = half[:, 0] * (len(xyz) + 1) + half[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge is used twice"
    rev = half[:, 1] * (len(xyz) + 1) + half[:, 0]
    assert np.array_equal(np.sort(key), np.sort(rev)), "an edge without its opposite: not closed or not consistently wound"
    E = len(key) // 2
    assert len(np.unique(t)) == len(xyz)
    assert len(xyz) - E + len(t) == 2
    p = (xyz.astype(np.float64) - np.array(ORIGIN)) / VOXEL - CENTRE
    assert np.abs(np.linalg.norm(p, axis=1) - RADIUS).max() <= 0.5
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    n = np.cross(b - a, c - a)
    live = np.linalg.norm(n, axis=1) > 1e-12
    assert ((n * (a + b + c)).sum(1)[live] > 0).all()
    assert live.mean() > 0.99


def test_partly_unobserved(gpu_device):
    tsdf, rgb = sphere_grid()
    w = np.ones_like(tsdf)
    w[:, :, 14:16] = 0.0
    xyz, _, tri = extract(tsdf, w, rgb)
    rxyz, _, rtri = MR.marching_tets(tsdf, w, rgb, ORIGIN, VOXEL)
    assert len(tri) > 500 and np.array_equal(tri.astype(np.int64), rtri) and len(xyz) == len(rxyz)
    p = (xyz.astype(np.float64) - np.array(ORIGIN)) / VOXEL
    cen = (p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]]) / 3           # strictly inside the triangle's cell
    i, j, k = (np.floor(cen[:, a]).astype(int) for a in range(3))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                assert (w[k + dz, j + dy, i + dx] > 0).all(), "a triangle in a cell with an unobserved corner"


def test_no_surface(gpu_device):
    tsdf = np.full((NZ, NY, NX), 0.7, np.float32)
    xyz, rgb, tri = extract(tsdf, np.ones_like(tsdf), None)
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and tri.shape == (0, 3)
