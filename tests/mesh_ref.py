"""numpy restatement of include/dvs_mesh.h's marching tetrahedra (fp64), independent of csrc/mesh.hip: vertices are discovered per
cell and numbered afterwards by sorting their edge ids; the winding is decided per triangle from the tetrahedron's own geometry."""
import itertools
import numpy as np

PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def corner_xyz(b):
    return np.array([b & 1, (b >> 1) & 1, (b >> 2) & 1])


def tets():
    """the six tetrahedra of a cell as 4 corner numbers each: 0 -> +axis p0 -> +axis p1 -> 7"""
    return [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in PERMS]


def parse_mesh_ply(path):
    """-> (xyz float32 [nv,3], rgb uint8 [nv,3], tri uint32 [nt,3]) of a file write_mesh_ply wrote; asserts the header"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0", head[:2]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nt = int([h for h in head if h.startswith("element face")][0].split()[-1])
    props = [h for h in head if h.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                     "property uchar blue", "property list uchar uint vertex_indices"], props
    vt = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("idx", "<u4", 3)])
    assert len(blob) == end + nv * vt.itemsize + nt * ft.itemsize, (len(blob), end, nv, nt)
    v = np.frombuffer(blob, vt, nv, end)
    f = np.frombuffer(blob, ft, nt, end + nv * vt.itemsize)
    assert (f["k"] == 3).all()
    return v["xyz"].copy(), v["rgb"].copy(), f["idx"].copy()


def build_mesh_ply(xyz, rgb, tri):
    """the bytes write_mesh_ply must produce"""
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(tri)}\nproperty list uchar uint vertex_indices\n"
            "end_header\n").encode()
    v = np.zeros(len(xyz), np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    v["xyz"], v["rgb"] = xyz, rgb
    f = np.zeros(len(tri), np.dtype([("k", "u1"), ("idx", "<u4", 3)]))
    f["k"], f["idx"] = 3, tri
    return head + v.tobytes() + f.tobytes()


def marching_tets(tsdf, weight, rgb, origin, voxel):
    """tsdf, weight [nz,ny,nx], rgb [nz,ny,nx,3] -> (xyz [nv,3] fp64, rgb uint8 [nv,3], tri int64 [nt,3])"""
    tsdf = np.asarray(tsdf, np.float64); weight = np.asarray(weight, np.float64); rgb = np.asarray(rgb, np.float64)
    nz, ny, nx = tsdf.shape
    ok = weight > 0
    inside = tsdf < 0
    cell = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for b in range(8):
        dx, dy, dz = corner_xyz(b)
        cell &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    tris = []                                             # (edge id a, edge id b, edge id c) in output order
    for k, j, i in zip(*np.nonzero(cell)):
        s = [inside[k + corner_xyz(b)[2], j + corner_xyz(b)[1], i + corner_xyz(b)[0]] for b in range(8)]
        if all(s) or not any(s):
            continue
        base = np.array([i, j, k])

        def edge_id(ca, cb):                              # grid edge between two corners of this cell, ca a sub-mask of cb
            p = base + corner_xyz(ca)
            return ((p[2] * ny + p[1]) * nx + p[0]) * 7 + ((ca ^ cb) - 1)
        for tet in tets():
            ins = [q for q in range(4) if s[tet[q]]]
            outs = [q for q in range(4) if not s[tet[q]]]
            if len(ins) in (0, 4):
                continue
            if len(ins) == 1:
                poly = [(ins[0], o) for o in outs]
            elif len(ins) == 3:
                poly = [(q, outs[0]) for q in ins]
            else:
                poly = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
            pts = [0.5 * (corner_xyz(tet[a]) + corner_xyz(tet[b])) for a, b in poly]
            out_dir = np.mean([corner_xyz(tet[q]) for q in outs], 0) - np.mean([corner_xyz(tet[q]) for q in ins], 0)
            ids = [edge_id(tet[min(a, b)], tet[max(a, b)]) for a, b in poly]
            for t3 in ([0, 1, 2], [0, 2, 3])[:len(poly) - 2]:
                nrm = np.cross(pts[t3[1]] - pts[t3[0]], pts[t3[2]] - pts[t3[0]])
                assert abs(nrm @ out_dir) > 1e-9
                if nrm @ out_dir < 0:
                    t3 = [t3[0], t3[2], t3[1]]
                tris.append([ids[q] for q in t3])
    if not tris:
        return np.zeros((0, 3)), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int64)
    tris = np.array(tris, np.int64)
    eids = np.unique(tris)                                # sorted: vertex order is edge-id order
    tri = np.searchsorted(eids, tris)
    vox, kind = eids // 7, eids % 7 + 1
    pi, pj, pk = vox % nx, (vox // nx) % ny, vox // (nx * ny)
    d = np.stack([kind & 1, (kind >> 1) & 1, (kind >> 2) & 1], 1)
    a = tsdf[pk, pj, pi]; b = tsdf[pk + d[:, 2], pj + d[:, 1], pi + d[:, 0]]
    t = a / (a - b)
    xyz = np.asarray(origin, np.float64) + (np.stack([pi, pj, pk], 1) + t[:, None] * d) * voxel
    ca = rgb[pk, pj, pi]; cb = rgb[pk + d[:, 2], pj + d[:, 1], pi + d[:, 0]]
    col = np.floor(np.clip(ca + t[:, None] * (cb - ca), 0, 1) * 255 + 0.5).astype(np.uint8)
    return xyz, col, tri
