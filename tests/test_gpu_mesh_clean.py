"""dvs_mesh_components, dvs_mesh_clean_* and dvs_mesh_extract_normals against tests/mesh_clean_ref.py.
Components and clean-up are integer work: every comparison is exact. Normals: the kernel and the float32 reference perform the same
operations up to the final square root and division, so 1e-5 absolute per component (about 100 fp32 ulp of a unit vector) bounds them."""
import numpy as np
import pytest
from divshot_amd import mesh
import mesh_clean_ref as CR

pytestmark = pytest.mark.gpu


def strip(first, n_tri):
    """a triangle strip over the vertices first .. first + n_tri + 1"""
    k = np.arange(n_tri)
    return np.stack([k, k + 1, k + 2], 1).astype(np.int64) + first


def check_components(tri, nv, expect_bad=0):
    label, n_bad = mesh.mesh_components(np.asarray(tri, np.uint32).reshape(-1, 3), nv)
    ref, ref_bad = CR.components(tri, nv)
    assert label.dtype == np.uint32 and label.shape == (nv,)
    assert np.array_equal(label, ref)
    assert n_bad == ref_bad == expect_bad
    return label


# ---- 1. components on hand-made index buffers --------------------------------------------------------------------------------------
def test_shuffled_strip_is_one_component(gpu_device):
    r = np.random.default_rng(41)
    tri = strip(0, 4097)
    nv = 4099
    perm = r.permutation(nv)
    tri = perm[tri][r.permutation(len(tri))]
    for row in tri:                                          # the corners' order inside a triangle too
        r.shuffle(row)
    label = check_components(tri, nv)
    assert (label == 0).all()


def test_isolated_triangles_and_unused_vertices(gpu_device):
    tri = np.arange(3000).reshape(1000, 3)
    label = check_components(tri, 3500)
    assert np.array_equal(label[:3000], np.repeat(np.arange(0, 3000, 3), 3)) and np.array_equal(label[3000:], np.arange(3000, 3500))


def test_two_strips_sharing_one_vertex(gpu_device):
    a, b = strip(0, 300), strip(302, 300)                    # vertices 0..301 and 302..603
    b[b == 302] = 150                                        # ... the second strip's first vertex is the first strip's vertex 150
    label = check_components(np.concatenate([b, a]), 604)
    assert (np.delete(label, 302) == 0).all() and label[302] == 302


def test_fan_on_the_last_vertex(gpu_device):
    nv = 6001
    k = np.arange(3000)
    tri = np.stack([2 * k, 2 * k + 1, np.full(3000, nv - 1)], 1)
    label = check_components(tri, nv)
    assert (label == 0).all()


def test_repeated_index_and_bad_indices(gpu_device):
    label = check_components([[5, 5, 2]], 8)
    assert label.tolist() == [0, 1, 2, 3, 4, 2, 6, 7]
    tri = [[0, 1, 2], [3, 4, 9], [5, 6, 7], [4, 0xFFFFFFFF, 3], [7, 8, 8]]
    label = check_components(tri, 9, expect_bad=2)
    assert label.tolist() == [0, 0, 0, 3, 4, 5, 5, 5, 5]


def test_empty_inputs(gpu_device):
    label, n_bad = mesh.mesh_components(np.zeros((0, 3), np.uint32), 7)
    assert label.tolist() == list(range(7)) and n_bad == 0
    label, n_bad = mesh.mesh_components(np.array([[0, 1, 2]], np.uint32), 0)
    assert label.shape == (0,) and n_bad == 1
    label, n_bad = mesh.mesh_components(np.zeros((0, 3), np.uint32), 0)
    assert label.shape == (0,) and n_bad == 0
    z3 = np.zeros((0, 3))
    xyz, rgb, tri, nrm, info = mesh.clean_mesh(z3, z3, z3, 100)
    assert xyz.shape == rgb.shape == tri.shape == (0, 3) and nrm is None and not any(info.values())
    xyz, rgb, tri, nrm, info = mesh.clean_mesh(np.ones((4, 3)), np.ones((4, 3)), z3, 0, normals=np.ones((4, 3)))
    assert xyz.shape == tri.shape == nrm.shape == (0, 3) and not any(info.values())


# ---- 2. the keep rule at its boundary ----------------------------------------------------------------------------------------------
def hand_mesh(sizes, seed=3):
    """components of the given triangle counts (strips), some vertices no triangle uses in between, vertex ids permuted so that the
    components interleave, triangles shuffled; vertex data that tells the vertices apart"""
    r = np.random.default_rng(seed)
    parts, first = [], 0
    for s in sizes:
        parts.append(strip(first, s))
        first += s + 2 + 3                                   # three unreferenced vertices behind each component
    nv = first
    perm = r.permutation(nv)
    tri = perm[np.concatenate(parts)]
    tri = tri[r.permutation(len(tri))]
    xyz = r.normal(0, 1, (nv, 3)).astype(np.float32)
    rgb = r.integers(0, 256, (nv, 3)).astype(np.uint8)
    nrm = r.normal(0, 1, (nv, 3)).astype(np.float32)
    return xyz, rgb, tri.astype(np.uint32), nrm


def check_clean(xyz, rgb, tri, min_bp, nrm):
    got = mesh.clean_mesh(xyz, rgb, tri, min_bp, normals=nrm)
    ref = CR.clean(xyz, rgb, tri, min_bp, normals=nrm)
    assert got[4] == ref[4], (got[4], ref[4])
    for g, r_, name in zip(got[:4], ref[:4], ("xyz", "rgb", "tri", "normals")):
        if r_ is None:
            assert g is None, name
        else:
            assert g.dtype == r_.dtype and g.shape == r_.shape and g.tobytes() == r_.tobytes(), name
    return got


@pytest.mark.parametrize("min_bp,kept", [(700, 2), (701, 1), (0, 2), (10000, 1)])
def test_keep_rule_boundary(gpu_device, min_bp, kept):
    xyz, rgb, tri, nrm = hand_mesh([100, 7])
    assert 7 * 10000 == 100 * 700
    got = check_clean(xyz, rgb, tri, min_bp, nrm)
    info = got[4]
    assert info["n_components"] == 2 and info["largest"] == 100 and info["kept_components"] == kept and info["n_bad"] == 0
    assert info["kept_triangles"] == (107 if kept == 2 else 100) and info["kept_vertices"] == (102 + 9 if kept == 2 else 102)
    check_clean(xyz, rgb, tri, min_bp, None)                 # ... and without normals


def test_tie_for_largest_keeps_both_and_bad_triangles_are_dropped(gpu_device):
    xyz, rgb, tri, nrm = hand_mesh([40, 9, 40, 1], seed=8)
    tri = np.concatenate([tri[:30], np.array([[1, 2, len(xyz)], [0xFFFFFFFF, 0, 0]], np.uint32), tri[30:]])
    got = check_clean(xyz, rgb, tri, 10000, nrm)
    assert got[4] == dict(n_components=4, largest=40, kept_components=2, kept_vertices=84, kept_triangles=80, n_bad=2)
    got = check_clean(xyz, rgb, tri, 0, nrm)
    assert got[4]["kept_components"] == 4 and got[4]["kept_triangles"] == 90 and got[4]["kept_vertices"] == 42 + 11 + 42 + 3


# ---- 2b. compaction past 256 block sums ---------------------------------------------------------------------------------------------
BIG_STRIP, BIG_ISOLATED = 400000, 200000


def big_mesh():
    """one strip of 400 000 triangles over 400 002 vertices, then 200 000 isolated triangles on their own 600 000 vertices; triangles
    shuffled, corners shuffled inside each triangle, vertex ids permuted -> (xyz, rgb, tri, normals, in_strip [nt], perm)"""
    r = np.random.default_rng(17)
    nv = BIG_STRIP + 2 + 3 * BIG_ISOLATED
    tri = np.concatenate([strip(0, BIG_STRIP), BIG_STRIP + 2 + np.arange(3 * BIG_ISOLATED).reshape(-1, 3)])
    perm = r.permutation(nv)
    order = r.permutation(len(tri))
    tri = r.permuted(perm[tri][order], axis=1)
    xyz = r.normal(0, 1, (nv, 3)).astype(np.float32)
    rgb = r.integers(0, 256, (nv, 3)).astype(np.uint8)
    nrm = r.normal(0, 1, (nv, 3)).astype(np.float32)
    return xyz, rgb, tri.astype(np.uint32), nrm, order < BIG_STRIP, perm


def test_compaction_past_256_block_sums(gpu_device):
    """1 000 002 vertices are 489 block sums of the shared scan and 600 000 triangles 293: k_scan_block_sums runs two rounds for each,
    and the second needs the first's carry. With min_bp = 1 an isolated triangle goes (1 x 10 000 < 400 000 x 1)."""
    xyz, rgb, tri, nrm, in_strip, perm = big_mesh()
    nv, nt = len(xyz), len(tri)
    assert nv == 1000002 and nt == 600000 and (nv + 2047) // 2048 == 489 and (nt + 2047) // 2048 == 293
    # the expectation by construction: the strip's vertices in ascending (permuted) index, its triangles in input order
    used = np.zeros(nv, bool)
    used[perm[:BIG_STRIP + 2]] = True
    remap = np.cumsum(used) - 1
    want_tri = remap[tri[in_strip].astype(np.int64)].astype(np.uint32)
    # what the second round's carry is worth: kept vertices and triangles on both sides of element 524 288
    assert 10000 < used[:524288].sum() < used.sum() - 10000 and 10000 < in_strip[:524288].sum() < in_strip.sum() - 10000
    ref = CR.clean(xyz, rgb, tri, 1, normals=nrm)
    want_info = dict(n_components=200001, largest=400000, kept_components=1, kept_vertices=400002, kept_triangles=400000, n_bad=0)
    assert ref[4] == want_info
    assert ref[2].tobytes() == want_tri.tobytes() and ref[0].tobytes() == xyz[used].tobytes()       # the restatement agrees with the construction
    got = mesh.clean_mesh(xyz, rgb, tri, 1, normals=nrm)
    assert got[4] == want_info, got[4]
    for g, r_, name in zip(got[:4], ref[:4], ("xyz", "rgb", "tri", "normals")):
        assert g.dtype == r_.dtype and g.shape == r_.shape and g.tobytes() == r_.tobytes(), name
    # min_bp = 0: everything is kept and the compaction is the identity
    got = mesh.clean_mesh(xyz, rgb, tri, 0, normals=nrm)
    assert got[4] == dict(n_components=200001, largest=400000, kept_components=200001, kept_vertices=nv, kept_triangles=nt, n_bad=0), got[4]
    for g, r_, name in zip(got[:4], (xyz, rgb, tri, nrm), ("xyz", "rgb", "tri", "normals")):
        assert g.dtype == r_.dtype and g.shape == r_.shape and g.tobytes() == r_.tobytes(), name


# ---- 3. on an extracted mesh, 4. normals -------------------------------------------------------------------------------------------
NX, NY, NZ = 24, 16, 16
ORIGIN, VOXEL = (-1.5, -1.0, -1.0), 0.125
BIG, SMALL = (np.array([7.3, 7.6, 7.9]), 5.0), (np.array([19.4, 8.2, 7.7]), 2.0)


def two_spheres():
    k, j, i = np.mgrid[0:NZ, 0:NY, 0:NX]
    d = [np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r for c, r in (BIG, SMALL)]
    tsdf = np.minimum(d[0], d[1]).astype(np.float32)
    rgb = np.stack([i / NX, j / NY, k / NZ], -1).astype(np.float32)
    return tsdf, rgb


def run_two_spheres():
    tsdf, rgb = two_spheres()
    g = mesh.TsdfGrid(ORIGIN, VOXEL, (NX, NY, NZ))
    g.upload(tsdf, np.ones_like(tsdf), rgb)
    m = g.extract(normals=True)
    label, n_bad = mesh.mesh_components(m[2], len(m[0]))
    top = mesh.clean_mesh(m[0], m[1], m[2], 10000, normals=m[3])
    all_ = mesh.clean_mesh(m[0], m[1], m[2], 100, normals=m[3])
    return m, label, n_bad, top, all_


@pytest.fixture(scope="module")
def spheres(gpu_device):
    return run_two_spheres(), run_two_spheres()


def test_extracted_spheres_are_two_components(spheres):
    (m, label, n_bad, top, all_), _ = spheres
    xyz, rgb, tri, nrm = m
    assert n_bad == 0 and len(np.unique(label)) == 2
    p = (xyz.astype(np.float64) - np.array(ORIGIN)) / VOXEL
    near_big = np.linalg.norm(p - BIG[0], axis=1) < BIG[1] + 1
    assert near_big.any() and (~near_big).any() and len(np.unique(label[near_big])) == 1 and len(np.unique(label[~near_big])) == 1
    # the largest alone: the big sphere, still closed (every edge used by exactly two triangles, once in each direction)
    cxyz, crgb, ctri, cnrm, info = top
    assert info["n_components"] == 2 and info["kept_components"] == 1 and info["kept_vertices"] == int(near_big.sum()) == len(cxyz)
    assert cxyz.tobytes() == xyz[near_big].tobytes() and crgb.tobytes() == rgb[near_big].tobytes() and cnrm.tobytes() == nrm[near_big].tobytes()
    t = ctri.astype(np.int64)
    assert len(t) == info["kept_triangles"] == info["largest"] and t.max() == len(cxyz) - 1
    half = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    und, uses = np.unique(np.sort(half, 1), axis=0, return_counts=True)
    assert (uses == 2).all()
    key, rev = half[:, 0] * len(cxyz) + half[:, 1], half[:, 1] * len(cxyz) + half[:, 0]
    assert len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))
    assert len(cxyz) - len(und) + len(t) == 2
    # 1 %: the small sphere has more than that, the mesh comes back unchanged
    axyz, argb, atri, anrm, ainfo = all_
    assert ainfo["kept_components"] == 2 and ainfo["largest"] * 100 <= 10000 * (len(tri) - ainfo["largest"])
    assert axyz.tobytes() == xyz.tobytes() and argb.tobytes() == rgb.tobytes() and atri.tobytes() == tri.tobytes() and anrm.tobytes() == nrm.tobytes()
    ref = CR.clean(xyz, rgb, tri, 10000, normals=nrm)
    assert ref[4] == info and ref[2].tobytes() == ctri.tobytes()


def test_two_runs_return_identical_bytes(spheres):
    a, b = spheres

    def flat(run):
        m, label, n_bad, top, all_ = run
        return [x.tobytes() for x in m] + [label.tobytes()] + [x.tobytes() for x in top[:4]] + [x.tobytes() for x in all_[:4]] + [repr(top[4]), repr(all_[4])]
    assert flat(a) == flat(b)


def check_normals(tsdf, weight, nrm):
    ref = CR.normals(tsdf, weight)
    assert nrm.shape == ref.shape and nrm.dtype == np.float32
    err = float(np.abs(nrm.astype(np.float64) - ref).max())
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    zero = (nrm == 0).all(1)
    assert np.array_equal(zero, (ref == 0).all(1))
    print(f"{len(nrm)} normals, {int(zero.sum())} zero, max |kernel - float32 reference| {err:.3e}, max | |n| - 1 | {np.abs(length[~zero] - 1).max():.3e}")
    assert err <= 1e-5
    assert np.abs(length[~zero] - 1).max() <= 1e-5
    return zero


def test_normals_on_the_sphere(spheres):
    (m, label, _, top, _), _ = spheres
    tsdf, _ = two_spheres()
    check_normals(tsdf, np.ones_like(tsdf), m[3])
    xyz, _, tri, nrm, _ = top                                # the radius-5 sphere alone
    assert not (nrm == 0).all(1).any()
    p = (xyz.astype(np.float64) - np.array(ORIGIN)) / VOXEL - BIG[0]
    assert ((nrm * p).sum(1) > 0).all(), "a normal that points into the sphere"
    t = tri.astype(np.int64)
    fn = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])          # length = twice the area: the weights
    mean = np.zeros_like(p)
    for c in range(3):
        np.add.at(mean, t[:, c], fn)
    assert ((nrm * mean).sum(1) > 0).all(), "a normal against its faces' winding"


def test_normals_on_a_partly_unobserved_grid(gpu_device):
    """test_gpu_mesh.py's test_partly_unobserved grid, weight 0 in the slab i in {14, 15}: the voxels at i = 13 and i = 16 take the
    one-sided difference along x. (A vertex's voxel is a corner of a participating cell, so on every axis one of its neighbours is
    observed: the all-zero component is defined, and restated by the reference, but no vertex of an extraction reaches it.)"""
    nx, ny, nz = 24, 21, 19
    origin, voxel = (-1.5, -1.25, -1.0), 0.125
    centre, radius = np.array([11.3, 10.2, 9.1]), 7.0
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
    tsdf = (np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius).astype(np.float32)
    rgb = np.stack([i / nx, j / ny, k / nz], -1).astype(np.float32)
    w = np.ones_like(tsdf)
    w[:, :, 14:16] = 0.0
    g = mesh.TsdfGrid(origin, voxel, (nx, ny, nz))
    g.upload(tsdf, w, rgb)
    xyz, _, tri, nrm = g.extract(normals=True)
    assert len(tri) > 500
    zero = check_normals(tsdf, w, nrm)
    assert not zero.any()
    gr = CR.gradient(tsdf, w)
    assert (gr[:, :, 13, 0] == tsdf[:, :, 13] - tsdf[:, :, 12]).all() and (gr[:, :, 16, 0] == tsdf[:, :, 17] - tsdf[:, :, 16]).all()
    assert (CR.gradient(tsdf, np.zeros_like(w)) == 0).all()
    # vertices on edges that end at i = 13 or start at i = 16 exist: the one-sided branch reached the kernel's output
    p = (xyz.astype(np.float64) - np.array(origin)) / voxel
    assert ((p[:, 0] > 12) & (p[:, 0] <= 13)).any() and ((p[:, 0] >= 16) & (p[:, 0] < 17)).any()
