"""dvs_mesh_decimate_count / _write (mesh.decimate_mesh) against the numpy restatement tests/mesh_decimate_ref.py, byte for byte: every
array is compared with tobytes() and the info dicts must be equal. No input holds a NaN or an infinity, so equal bytes are equal values.

Sizes. The vertex sort and the triangle sorts work in partitions of dvs_fe_part_for(n) = 256 threads x 8 keys = 2048 keys for every n
up to 1.5 million (frontend.hip), and the scans in tiles of DVS_SCAN_TILE = 2048 words: 2049 vertices are the smallest count that
needs a second sort partition and a second scan tile (one element in it), 4097 a third of each, 5000 an odd count inside the third;
12000 triangles are six partitions of the triangle sorts, the last one partly filled."""
import numpy as np
import pytest
from divshot_amd import mesh
import mesh_decimate_ref as DR

pytestmark = pytest.mark.gpu


def check(xyz, rgb, tri, origin, cell, ncell, normals=None):
    """runs both, asserts equality, -> the reference's outputs"""
    got = mesh.decimate_mesh(xyz, rgb, tri, origin, cell, ncell, normals=normals)
    ref = DR.decimate(xyz, rgb, tri, origin, cell, ncell, normals=normals)
    print(ref[4])
    assert got[4] == ref[4], (got[4], ref[4])
    for name, g, r in zip(("xyz", "rgb", "tri"), got[:3], ref[:3]):
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, g.shape, r.dtype, r.shape)
        assert g.tobytes() == r.tobytes(), (name, int((g != r).sum()))
    if normals is None:
        assert got[3] is None and ref[3] is None
    else:
        assert got[3].shape == ref[3].shape and not np.isnan(ref[3]).any()
        assert got[3].tobytes() == ref[3].tobytes(), ("normals", int((got[3] != ref[3]).sum()))
    return ref


@pytest.mark.parametrize("nv", [5000, 4097, 2049])
def test_random_soup(gpu_device, nv):
    rng = np.random.default_rng(nv)
    xyz = rng.random((nv, 3), dtype=np.float32)
    nrm = rng.standard_normal((nv, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (nv, 3), dtype=np.uint8)
    tri = rng.integers(0, nv, (12000, 3)).astype(np.uint32)
    # cells of 0.2 from the cube's corner: x has spare cells, y fits exactly (a point at 1.0 - ulp is in the last), z is clamped from 0.6 on
    ref = check(xyz, rgb, tri, (0.0, 0.0, 0.0), 0.2, (7, 5, 3), normals=nrm)
    info = ref[4]
    assert info["n_clusters"] == 5 * 5 * 3 and info["n_degenerate"] > 100 and info["n_duplicate"] > 100 and info["out_triangles"] > 5000
    # and without normals
    check(xyz, rgb, tri, (0.0, 0.0, 0.0), 0.2, (7, 5, 3))


def test_one_cell_collapses_everything(gpu_device):
    rng = np.random.default_rng(1)
    xyz = rng.random((300, 3), dtype=np.float32)
    rgb = rng.integers(0, 256, (300, 3), dtype=np.uint8)
    tri = rng.integers(0, 300, (500, 3)).astype(np.uint32)
    ref = check(xyz, rgb, tri, (-1.0, -1.0, -1.0), 4.0, (1, 1, 1), normals=xyz)
    assert ref[4] == {"out_vertices": 0, "out_triangles": 0, "n_clusters": 1, "n_degenerate": 500, "n_duplicate": 0, "n_bad": 0}
    assert ref[0].shape == (0, 3) and ref[2].shape == (0, 3)


def test_finest_lattice_merges_nothing(gpu_device):
    """1024^3 cells of 2^-10: 600 points at the centres of distinct cells (q is exact). The output is the input without its unused
    vertices, in key order"""
    rng = np.random.default_rng(2)
    cells = rng.choice(1024 ** 3, 600, replace=False)
    ijk = np.stack([cells % 1024, (cells // 1024) % 1024, cells // (1024 * 1024)], -1)
    cell = np.float32(2.0 ** -10)
    xyz = ((ijk + 0.5) * float(cell)).astype(np.float32)
    rgb = rng.integers(0, 256, (600, 3), dtype=np.uint8)
    nrm = rng.standard_normal((600, 3)).astype(np.float32)
    tri = rng.integers(0, 450, (800, 3)).astype(np.uint32)           # vertices 450.. are unused
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    oxyz, orgb, otri, onrm, info = check(xyz, rgb, tri, (0.0, 0.0, 0.0), cell, (1024, 1024, 1024), normals=nrm)
    assert info["n_clusters"] == 600 and info["n_degenerate"] == 0 and info["n_bad"] == 0
    used = np.unique(tri)
    order = used[np.argsort(cells[used], kind="stable")]
    assert info["out_vertices"] == len(used)
    assert oxyz.tobytes() == xyz[order].tobytes() and orgb.tobytes() == rgb[order].tobytes()   # (a mean of one is the value: x / 1.0f)
    rank = np.full(600, -1)
    rank[order] = np.arange(len(order))
    canon = {DR.rotate_min_first(*r) for r in rank[tri].tolist()}
    assert info["out_triangles"] == len(canon) and info["n_duplicate"] == len(tri) - len(canon)


def highest_cell_fixture():
    """1024^3 cells of 2^-10 again (q is exact): 294 vertices alone in cells spread over the lattice, among them the two neighbours of the
    last cell in key order, and six in the last cell (1023, 1023, 1023), whose key 2^30 - 1 has every one of the 30 bits set — one of the
    six on the far corner, clamped into it. Every triangle has a corner in the last cell. -> xyz, rgb, nrm, tri, cell"""
    rng = np.random.default_rng(4)
    top = 1024 ** 3 - 1
    cells = np.concatenate([rng.choice(top - 2, 292, replace=False), [top - 2, top - 1]])
    ijk = np.stack([cells % 1024, (cells // 1024) % 1024, cells // (1024 * 1024)], -1)
    cell = np.float32(2.0 ** -10)
    inside = 1023 + np.array([[0.5, 0.5, 0.5], [0.125, 0.75, 0.25], [0.875, 0.0, 0.625], [0.0, 0.0, 0.0], [0.25, 0.5, 0.875]])
    xyz = np.concatenate([(ijk + 0.5) * float(cell), inside * float(cell), [[1.0, 1.0, 1.0]]]).astype(np.float32)
    perm = rng.permutation(300)                                          # the six are not the last six indices
    xyz = xyz[perm]
    members = np.nonzero(np.isin(perm, np.arange(294, 300)))[0]
    others = np.nonzero(~np.isin(perm, np.arange(294, 300)))[0]
    rgb = rng.integers(0, 256, (300, 3), dtype=np.uint8)
    nrm = rng.standard_normal((300, 3)).astype(np.float32)
    tri = np.stack([rng.choice(members, 200), rng.choice(others, 200), rng.choice(others, 200)], -1)
    tri = np.concatenate([tri, tri[:20, [1, 2, 0]], [[members[0], members[1], others[0]]]]).astype(np.uint32)      # rotations repeat, one collapses
    return xyz, rgb, nrm, tri, cell


def test_highest_cell_is_a_cell(gpu_device):
    """a full 30-bit key sits next to the bit that marks "no cell" in the shared clustering (cell_cluster.hip): the last cell's vertices
    form a cluster like any other, the last one, and its triangles survive"""
    xyz, rgb, nrm, tri, cell = highest_cell_fixture()
    dims = (1024, 1024, 1024)
    keys = DR.cell_keys(xyz, (0.0, 0.0, 0.0), cell, dims)
    assert keys.max() == 2 ** 30 - 1 and (keys == 2 ** 30 - 1).sum() == 6 and len(np.unique(keys)) == 295
    oxyz, _, otri, _, info = check(xyz, rgb, tri, (0.0, 0.0, 0.0), cell, dims, normals=nrm)
    assert info["n_clusters"] == 295 and info["n_bad"] == 0 and info["n_degenerate"] >= 1 and info["n_duplicate"] >= 20
    assert info["out_triangles"] > 100 and DR.cell_keys(oxyz, (0.0, 0.0, 0.0), cell, dims)[-1] == 2 ** 30 - 1
    assert (otri == info["out_vertices"] - 1).any(1).all(), "every kept triangle has a corner in the last cluster"


def test_member_order_of_a_large_cell(gpu_device):
    """3000 vertices in one cell whose fp32 sums depend on the order of the additions (magnitudes over five decades, mixed signs for the
    normals), walked by one lane; two more cells so that triangles survive"""
    rng = np.random.default_rng(3)
    n = 3000
    xyz = np.empty((n + 2, 3), np.float32)
    xyz[:n] = (10.0 ** rng.uniform(-3, 2.99, (n, 3))).astype(np.float32)              # all inside [0, 1000)^3: cell (0, 0, 0)
    xyz[n] = (1500.0, 10.0, 10.0)
    xyz[n + 1] = (2500.0, 10.0, 10.0)
    nrm = (rng.standard_normal((n + 2, 3)) * 10.0 ** rng.uniform(-3, 3, (n + 2, 3))).astype(np.float32)
    rgb = rng.integers(0, 256, (n + 2, 3), dtype=np.uint8)
    fwd = np.float32(0)
    for v in xyz[:n, 0]:
        fwd = np.float32(fwd + v)
    rev = np.float32(0)
    for v in xyz[:n, 0][::-1]:
        rev = np.float32(rev + v)
    assert fwd != rev, "the fixture must tell the orders apart"
    tri = np.array([[int(v), n, n + 1] for v in rng.integers(0, n, 40)] + [[n + 1, n, 7]], np.uint32)
    ref = check(xyz, rgb, tri, (0.0, 0.0, 0.0), 1000.0, (4, 1, 1), normals=nrm)
    assert ref[4] == {"out_vertices": 3, "out_triangles": 2, "n_clusters": 3, "n_degenerate": 0, "n_duplicate": 39, "n_bad": 0}


def test_duplicates_by_hand(gpu_device):
    xyz = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]], np.float32)
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    tri = np.array([[1, 2, 0], [2, 0, 1], [0, 1, 2], [0, 2, 1]], np.uint32)           # three rotations and the mirror image
    oxyz, orgb, otri, _, info = check(xyz, rgb, tri, (0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    assert info["n_duplicate"] == 2 and info["out_triangles"] == 2 and info["out_vertices"] == 3
    assert otri.tolist() == [[1, 2, 0], [0, 2, 1]]                   # the first rotation as it was given (not rotated), and the mirror
    assert oxyz.tobytes() == xyz.tobytes() and orgb.tobytes() == rgb.tobytes()


def test_bad_indices_and_clamped_positions(gpu_device):
    rng = np.random.default_rng(5)
    nv = 200
    xyz = (rng.random((nv, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    xyz[0] = (0.0, 0.0, 0.0)                                         # exactly at the origin: cell 0
    xyz[1] = (-0.25, -3.0, -1e-6)                                    # below it: clamped to cell 0
    xyz[2] = (4.0, 7.5, 1e6)                                         # at and beyond the last cell's far face: the last cell
    xyz[3] = (np.nextafter(np.float32(4.0), np.float32(0)), 2.0, 2.0)
    assert np.isfinite(xyz).all()
    rgb = rng.integers(0, 256, (nv, 3), dtype=np.uint8)
    nrm = rng.standard_normal((nv, 3)).astype(np.float32)
    tri = rng.integers(0, nv, (400, 3)).astype(np.uint32)
    tri[::7, 1] = nv                                                 # the first index that is out of range
    tri[3::11, 2] = 0xFFFFFFFF
    tri[5::13, 0] = nv + 1000
    tri[:6] = [[0, 2, 50], [1, 2, 51], [0, 1, 2], [3, 2, 0], [0, 3, 60], [nv - 1, 0, 2]]
    ref = check(xyz, rgb, tri, (0.0, 0.0, 0.0), 1.0, (4, 4, 4), normals=nrm)
    keys = DR.cell_keys(xyz, (0.0, 0.0, 0.0), 1.0, (4, 4, 4))
    assert keys[0] == 0 and keys[1] == 0 and keys[2] == 63 and keys[3] == (2 * 4 + 2) * 4 + 3
    assert ref[4]["n_bad"] == int((tri.astype(np.int64) >= nv).any(1).sum()) > 50 and ref[4]["n_degenerate"] >= 1


@pytest.mark.parametrize("with_normals", [False, True])
def test_empty_inputs(gpu_device, with_normals):
    z3 = np.zeros((0, 3), np.float32)
    nothing = {"out_vertices": 0, "out_triangles": 0, "n_clusters": 0, "n_degenerate": 0, "n_duplicate": 0, "n_bad": 0}
    ref = check(z3, np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint32), (0.0, 0.0, 0.0), 1.0, (2, 2, 2), normals=z3 if with_normals else None)
    assert ref[4] == nothing
    # no vertex: every triangle is bad
    ref = check(z3, np.zeros((0, 3), np.uint8), np.array([[0, 1, 2], [5, 5, 5]], np.uint32), (0.0, 0.0, 0.0), 1.0, (2, 2, 2),
                normals=z3 if with_normals else None)
    assert ref[4] == dict(nothing, n_bad=2)
    # no triangle: the cells are counted, nothing comes out
    xyz = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [1.6, 0.5, 0.5]], np.float32)
    ref = check(xyz, np.zeros((3, 3), np.uint8), np.zeros((0, 3), np.uint32), (0.0, 0.0, 0.0), 1.0, (2, 2, 2), normals=xyz if with_normals else None)
    assert ref[4] == dict(nothing, n_clusters=2)


# ---- a sphere through the device's own extraction -----------------------------------------------------------------------------------
N, RADIUS, CENTRE = 40, 15.0, np.array([19.3, 20.2, 19.1])          # the fixture of tests/test_mesh_decimate_format.py
ORIGIN, VOXEL = (-2.5, -2.5, -2.5), 0.125


@pytest.fixture(scope="module")
def extracted(gpu_device):
    k, j, i = np.mgrid[0:N, 0:N, 0:N]
    tsdf = (np.sqrt((i - CENTRE[0]) ** 2 + (j - CENTRE[1]) ** 2 + (k - CENTRE[2]) ** 2) - RADIUS).astype(np.float32)
    rgb = np.stack([i / N, j / N, k / N], -1).astype(np.float32)
    g = mesh.TsdfGrid(ORIGIN, VOXEL, (N, N, N))
    g.upload(tsdf, np.ones_like(tsdf), rgb)
    return g.extract(normals=True)


@pytest.mark.parametrize("factor", [2, 3])
def test_extracted_sphere(extracted, factor):
    xyz, rgb, tri, nrm = extracted
    assert len(xyz) > 10000 and len(tri) > 20000
    origin, cell, ncell = DR.lattice(ORIGIN, VOXEL, (N, N, N), factor)
    oxyz, _, otri, onrm, info = check(xyz, rgb, tri, origin, cell, ncell, normals=nrm)
    assert 0 < info["out_triangles"] < len(tri) // 8
    length = np.linalg.norm(onrm.astype(np.float64), axis=1)
    assert (np.abs(length - 1) <= 1e-5).all()
    p = oxyz.astype(np.float64) - (np.array(ORIGIN) + CENTRE * VOXEL)
    assert ((onrm * p).sum(1) > 0).all(), "a merged normal that points into the sphere"
