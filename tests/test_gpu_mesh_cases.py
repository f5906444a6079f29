"""dvs_mesh_extract_* against tests/mesh_ref.py where test_gpu_mesh.py's sphere does not go: a random-sign field that shows every cube
mask and every (tetrahedron, case) pair; random, planar and isolated unobserved voxels; grids one cell thick; vertices exactly on grid
corners; grids of 256 and 293 scan tiles, whose block sums go through k_scan_block_sums' last lane and its carry.

Every condition on an input (which masks occur, which scan tiles own vertices and triangles, ...) is computed from numpy and the
restatement alone, in the input builders, and asserted before the first GPU call: the builders run on a machine without a GPU.

Position bars, in voxels. Origin and voxel are binary fractions, so the kernel rounds a / (a - b) (relative 2^-24 of t <= 1) and i + t
(half an ulp of the index). Indices below 32: half an ulp is 2^-20 = 9.5e-7, bar 1e-5 (test_gpu_mesh.py's). Indices up to 128: half an
ulp is 2^-18 = 3.8e-6, bar 2e-5. |a - b| >= 0.1 keeps the division's condition number below 20."""
import time
import numpy as np
import pytest
from divshot_amd import mesh
import mesh_ref as MR

pytestmark = pytest.mark.gpu
VOXEL = 0.125
SCAN_TILE = 2048                                             # elements per block sum (csrc/dvs_kernels.h DVS_SCAN_TILE)
ROUND = 256 * SCAN_TILE                                      # elements per round of the block-sum loop: 524 288


def random_field(dims, seed, shell=True):
    """-> tsdf [nz,ny,nx] float32 with |tsdf| uniform in [0.05, 1] and a fair coin for the sign (the outer shell +1), rgb in [0, 1]"""
    nx, ny, nz = dims
    r = np.random.default_rng(seed)
    tsdf = (r.uniform(0.05, 1.0, (nz, ny, nx)) * np.where(r.random((nz, ny, nx)) < 0.5, -1.0, 1.0)).astype(np.float32)
    if shell:
        tsdf[0], tsdf[-1], tsdf[:, 0], tsdf[:, -1], tsdf[:, :, 0], tsdf[:, :, -1] = 1, 1, 1, 1, 1, 1
    rgb = r.random((nz, ny, nx, 3)).astype(np.float32)
    return tsdf, rgb


def cube_masks(tsdf):
    """[nz-1,ny-1,nx-1]: bit b of a cell's mask = its corner b (x + 2 y + 4 z) is inside"""
    nz, ny, nx = tsdf.shape
    inside = tsdf < 0
    m = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for b in range(8):
        dx, dy, dz = MR.corner_xyz(b)
        m |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << b
    return m


def full_cells(weight):
    nz, ny, nx = weight.shape
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for b in range(8):
        dx, dy, dz = MR.corner_xyz(b)
        ok &= weight[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] > 0
    return ok


def tet_cases(masks):
    """the (tetrahedron, case) pairs the cube masks select: case bit q = the tetrahedron's vertex q is inside"""
    seen = set()
    for m in np.unique(masks):
        for t, tet in enumerate(MR.tets()):
            seen.add((t, sum(((int(m) >> tet[q]) & 1) << q for q in range(4))))
    return seen


def extract(dims, origin, tsdf, weight, rgb):
    g = mesh.TsdfGrid(origin, VOXEL, dims)
    g.upload(tsdf, weight, rgb)
    return g.extract()


def directed_edges(tri, nv):
    t = tri.astype(np.int64)
    half = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return half[:, 0] * (nv + 1) + half[:, 1], half[:, 1] * (nv + 1) + half[:, 0]


def check_against(got, ref, origin, pos_bar, exact_pos=False):
    (xyz, rgb, tri), (rxyz, rrgb, rtri) = got, ref
    assert len(xyz) == len(rxyz) and len(tri) == len(rtri), (len(xyz), len(rxyz), len(tri), len(rtri))
    assert np.array_equal(tri.astype(np.int64), rtri)
    if not len(xyz):
        return
    if exact_pos:
        assert np.array_equal(xyz.view(np.uint32), rxyz.astype(np.float32).view(np.uint32)), "a position differs from the rounded reference"
    err = np.abs(xyz.astype(np.float64) - rxyz).max() / VOXEL
    print(f"{len(xyz)} vertices, {len(tri)} triangles, position error {err:.3e} voxel")
    assert err <= pos_bar
    assert np.abs(rgb.astype(int) - rrgb.astype(int)).max() <= 1


def triangle_cells(xyz, tri, origin):
    p = (xyz.astype(np.float64) - np.array(origin)) / VOXEL
    cen = (p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]]) / 3           # strictly inside the triangle's cell
    return tuple(np.floor(cen[:, a]).astype(int) for a in range(3))


# ---- A. every cell case on a random-sign field --------------------------------------------------------------------------------------
A_DIMS, A_ORIGIN = (20, 18, 16), (0.0, 0.0, 0.0)


def build_a():
    tsdf, rgb = random_field(A_DIMS, 7)
    masks = cube_masks(tsdf)
    assert len(np.unique(masks)) == 256, "a cube mask does not occur"
    cases = tet_cases(masks)
    assert {(t, m) for t in range(6) for m in range(1, 15)} <= cases, "a (tetrahedron, case) pair does not occur"
    w = np.ones_like(tsdf)
    return tsdf, w, rgb, MR.marching_tets(tsdf, w, rgb, A_ORIGIN, VOXEL)


@pytest.fixture(scope="module")
def field_a():
    return build_a()


@pytest.fixture(scope="module")
def extracted_a(field_a, gpu_device):
    tsdf, w, rgb, ref = field_a
    return extract(A_DIMS, A_ORIGIN, tsdf, w, rgb)


def test_random_signs_every_case(field_a, extracted_a):
    ref = field_a[3]
    assert len(ref[0]) > 10000 and len(ref[2]) > 30000
    check_against(extracted_a, ref, A_ORIGIN, 1e-5)


def test_random_signs_closed_and_consistently_wound(extracted_a):
    """without the reference: the shell is outside, so the surface is closed inside the grid"""
    xyz, col, tri = extracted_a
    key, rev = directed_edges(tri, len(xyz))
    assert len(np.unique(key)) == len(key), "a directed edge is used twice"
    assert np.array_equal(np.sort(key), np.sort(rev)), "an edge without its opposite: not closed or not consistently wound"
    assert len(np.unique(tri)) == len(xyz), "a vertex no triangle uses"


# ---- B. holes, thin grids, corner-exact vertices ------------------------------------------------------------------------------------
def build_holes():
    tsdf, rgb = random_field(A_DIMS, 7)
    nx, ny, nz = A_DIMS
    r = np.random.default_rng(11)
    w = np.where(r.random((nz, ny, nx)) < 0.10, 0.0, 1.0).astype(np.float32)
    w[:, 11, :] = 0.0                                        # a full plane along y and one along z
    w[5, :, :] = 0.0
    cells = full_cells(w)
    assert 1000 < cells.sum() < cells.size // 2             # (0.9^8 = 43 % of the cells keep their 8 corners, less the two planes')
    # isolated holes: an unobserved voxel all of whose 26 neighbours are observed
    pad = np.pad(w, 1, constant_values=1.0)
    nb = sum(pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] > 0 for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert ((w == 0) & (nb == 26)).sum() >= 5
    ref = MR.marching_tets(tsdf, w, rgb, A_ORIGIN, VOXEL)
    # every edge kind has crossed edges with a vertex (a participating cell around them) and without (none)
    eids = kinds_with_vertex(ref)
    for kind in range(1, 8):
        d = MR.corner_xyz(kind)
        a = (tsdf < 0)[:nz - d[2], :ny - d[1], :nx - d[0]]; b = (tsdf < 0)[d[2]:, d[1]:, d[0]:]
        crossed = int((a != b).sum())
        assert 0 < eids[kind] < crossed, (kind, eids[kind], crossed)
    return tsdf, w, rgb, ref


def kinds_with_vertex(ref):
    """how many of the reference's vertices lie on an edge of each kind (kind = the corner the edge runs to, 1..7): from the positions.
    A vertex p + t d with 0 < t < 1 has a fractional part on exactly the axes of d"""
    p = ref[0] / VOXEL
    frac = np.abs(p - np.round(p)) > 1e-9
    kind = frac[:, 0] * 1 + frac[:, 1] * 2 + frac[:, 2] * 4
    return np.bincount(kind, minlength=8)


def test_random_holes(gpu_device):
    tsdf, w, rgb, ref = build_holes()
    xyz, col, tri = got = extract(A_DIMS, A_ORIGIN, tsdf, w, rgb)
    check_against(got, ref, A_ORIGIN, 1e-5)
    assert len(tri) > 1000
    i, j, k = triangle_cells(xyz, tri, A_ORIGIN)
    for b in range(8):
        dx, dy, dz = MR.corner_xyz(b)
        assert (w[k + dz, j + dy, i + dx] > 0).all(), "a triangle in a cell with an unobserved corner"
    assert len(np.unique(tri)) == len(xyz), "a vertex no triangle uses"


THIN = [(2, 2, 9), (2, 7, 2), (5, 2, 2)]


@pytest.mark.parametrize("dims", THIN)
def test_thin_grids(gpu_device, dims):
    tsdf, rgb = random_field(dims, 23 + sum(dims), shell=False)
    assert len(np.unique(cube_masks(tsdf))) >= min(4, (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1))
    w = np.ones_like(tsdf)
    ref = MR.marching_tets(tsdf, w, rgb, A_ORIGIN, VOXEL)
    assert len(ref[2]) >= 6
    check_against(extract(dims, A_ORIGIN, tsdf, w, rgb), ref, A_ORIGIN, 1e-5)


ONE_CELL_MASKS = [0x01, 0x7F, 0x69, 0x96, 0x80, 0xFE, 0x3C, 0xA5, 0x5A, 0x0F, 0x00, 0xFF]


def test_one_cell_grid(gpu_device):
    r = np.random.default_rng(5)
    for m in ONE_CELL_MASKS:
        mag = r.uniform(0.05, 1.0, 8)
        tsdf = np.array([-mag[b] if (m >> b) & 1 else mag[b] for b in range(8)], np.float32).reshape(2, 2, 2)
        assert int(cube_masks(tsdf)[0, 0, 0]) == m
        rgb = r.random((2, 2, 2, 3)).astype(np.float32)
        w = np.ones_like(tsdf)
        ref = MR.marching_tets(tsdf, w, rgb, A_ORIGIN, VOXEL)
        assert (len(ref[2]) == 0) == (m in (0x00, 0xFF))
        check_against(extract((2, 2, 2), A_ORIGIN, tsdf, w, rgb), ref, A_ORIGIN, 1e-5)


C_DIMS, C_ORIGIN, C_SEED = (6, 5, 4), (-1.5, -1.25, -1.0), 0
C_VALUES = np.array([-1.0, -0.25, -0.0, 0.0, 0.25, 1.0], np.float32)


def build_corner_exact():
    nx, ny, nz = C_DIMS
    r = np.random.default_rng(C_SEED)
    tsdf = C_VALUES[r.integers(0, 6, (nz, ny, nx))]
    rgb = r.random((nz, ny, nx, 3)).astype(np.float32)
    bits = tsdf.view(np.uint32)
    for kind in range(1, 8):                                 # both zeros at both ends of an edge of every kind, the other end inside
        d = MR.corner_xyz(kind)
        lo, hi = (slice(0, nz - d[2]), slice(0, ny - d[1]), slice(0, nx - d[0])), (slice(d[2], nz), slice(d[1], ny), slice(d[0], nx))
        for zero in (0x00000000, 0x80000000):
            assert ((bits[lo] == zero) & (tsdf[hi] < 0)).any(), (kind, hex(zero), "t = 0")
            assert ((tsdf[lo] < 0) & (bits[hi] == zero)).any(), (kind, hex(zero), "t = 1")
    w = np.ones_like(tsdf)
    ref = MR.marching_tets(tsdf, w, rgb, C_ORIGIN, VOXEL)
    # Bit for bit is a fair demand here: t is 0, 1, 1/2, 1/5 or 4/5, and at these indices and this origin the float32 evaluation
    # origin + (i + t) * voxel (products by 0, 1 and 0.125 are exact) rounds to the float64 result's float32 neighbour.
    for t in (0.0, 0.2, 0.5, 0.8, 1.0):
        for axis, n in enumerate(C_DIMS):
            for i in range(n):
                f32 = np.float32(C_ORIGIN[axis]) + (np.float32(i) + np.float32(t)) * np.float32(VOXEL)
                assert f32 == np.float32(C_ORIGIN[axis] + (i + t) * VOXEL), (t, axis, i)
    tt = (ref[0] - np.array(C_ORIGIN)) / VOXEL
    tt = np.abs(tt - np.round(tt))
    assert (tt.max(1) < 1e-12).sum() >= 14 and (tt.max(1) > 0.1).sum() >= 14          # vertices on corners and vertices inside edges
    deg = (ref[2][:, 0] == ref[2][:, 1]) | (ref[2][:, 1] == ref[2][:, 2]) | (ref[2][:, 0] == ref[2][:, 2])
    assert not deg.any()                                     # (indices are edges: distinct even where positions coincide)
    q = ref[0][ref[2]]
    assert (np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1) < 1e-15).any(), "no triangle of zero area"
    return tsdf, w, rgb, ref


def test_vertices_on_grid_corners(gpu_device):
    tsdf, w, rgb, ref = build_corner_exact()
    check_against(extract(C_DIMS, C_ORIGIN, tsdf, w, rgb), ref, C_ORIGIN, 1e-5, exact_pos=True)


# ---- C. the scan past 256 block sums ------------------------------------------------------------------------------------------------
def slab_grid(dims, slabs, seed):
    """random signs in the observed slabs [(z0, z1, y0, y1)] (inclusive, all x), weight 0 elsewhere"""
    tsdf, rgb = random_field(dims, seed, shell=False)
    w = np.zeros_like(tsdf)
    for z0, z1, y0, y1 in slabs:
        w[z0:z1 + 1, y0:y1 + 1, :] = 1.0
    return tsdf, w, rgb


def owners(tsdf, w, ref, origin):
    """the linear voxel index that owns each reference vertex (its edge's lower end) and each reference triangle (its cell's lower
    corner), from the reference's output"""
    nz, ny, nx = tsdf.shape
    p = (ref[0] - np.array(origin)) / VOXEL
    lo = np.floor(p + 1e-9).astype(np.int64)                 # |t| in (0, 1): |tsdf| >= 0.05, no vertex on a corner
    v_owner = (lo[:, 2] * ny + lo[:, 1]) * nx + lo[:, 0]
    q = p[ref[2]].mean(1)
    c = np.floor(q).astype(np.int64)
    t_owner = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    return v_owner, t_owner


SCAN_GRIDS = {
    # 524 288 voxels, 256 block sums: one round, its last lane in use. A z-layer is two tiles; the last layer (tiles 254, 255) owns
    # vertices (in-layer edges) but no cell, so the last tile that can own a triangle is 253.
    "one_round": ((64, 64, 128), [(0, 1, 0, 9), (60, 62, 10, 31), (126, 127, 40, 63)], (0, 255), (0, 253)),
    # 599 040 voxels, 293 block sums: a second round of 37, the last tile half full. Linear index 524 288 is voxel (32, 85, 56); the last
    # layer starts in tile 288, the last tile that can own a triangle is 287 (z = 63).
    "two_rounds": ((96, 96, 65), [(0, 1, 0, 4), (55, 57, 74, 92), (63, 64, 84, 95)], (0, 255, 256, 292), (0, 255, 256, 287)),
}
_scan_inputs = {}


def build_scan(name):
    if name not in _scan_inputs:
        dims, slabs, v_tiles, t_tiles = SCAN_GRIDS[name]
        nx, ny, nz = dims
        n = nx * ny * nz
        assert (n + SCAN_TILE - 1) // SCAN_TILE == (256 if name == "one_round" else 293) and v_tiles[-1] == (n - 1) // SCAN_TILE
        last_cell = ((nz - 2) * ny + ny - 2) * nx + nx - 2
        assert t_tiles[-1] == last_cell // SCAN_TILE
        tsdf, w, rgb = slab_grid(dims, slabs, 31)
        t0 = time.perf_counter()
        ref = MR.marching_tets(tsdf, w, rgb, A_ORIGIN, VOXEL)
        print(f"{name}: reference {time.perf_counter() - t0:.1f} s, {len(ref[0])} vertices, {len(ref[2])} triangles")
        assert len(ref[0]) > 10000 and len(ref[2]) > 10000
        v_owner, t_owner = owners(tsdf, w, ref, A_ORIGIN)
        assert (np.diff(v_owner) >= 0).all() and (np.diff(t_owner) >= 0).all()       # the output order is the owners' order
        for tile in v_tiles:
            assert (v_owner // SCAN_TILE == tile).any(), f"no vertex owned by a voxel of scan tile {tile}"
        for tile in t_tiles:
            assert (t_owner // SCAN_TILE == tile).any(), f"no triangle owned by a voxel of scan tile {tile}"
        if n > ROUND:
            for own in (v_owner, t_owner):
                assert 1000 < (own < ROUND).sum() < len(own) - 1000, "the second round's carry is (nearly) zero or (nearly) unused"
            assert (v_owner // (nx * ny) == 56).any() and ROUND // (nx * ny) == 56
        _scan_inputs[name] = (dims, tsdf, w, rgb, ref)
    return _scan_inputs[name]


@pytest.mark.parametrize("name", list(SCAN_GRIDS))
def test_scan_block_sums_through_the_extraction(gpu_device, name):
    dims, tsdf, w, rgb, ref = build_scan(name)
    got = extract(dims, A_ORIGIN, tsdf, w, rgb)
    check_against(got, ref, A_ORIGIN, 2e-5)
    again = extract(dims, A_ORIGIN, tsdf, w, rgb)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes(), "two extractions of one grid differ"
