"""Restatement of include/dvs_mesh.h's mesh clean-up, independent of csrc/mesh_clean.hip: a plain union-find over the index buffer,
the integer keep rule, the order-preserving compaction, the normals' formula in float32 operation by operation, and a parser of the
mesh PLY that accepts the optional nx ny nz. numpy only."""
import numpy as np


def components(tri, n_vertices):
    """-> (label uint32 [n_vertices]: the smallest vertex index of each vertex's component, n_bad); triangles with an index >=
    n_vertices are ignored and counted"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    n_bad = 0
    for a, b, c in tri.tolist():
        if max(a, b, c) >= n_vertices:
            n_bad += 1
            continue
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n_vertices)], np.uint32).reshape(n_vertices), n_bad


def keeps(c, largest, min_bp):
    """the rule, in Python integers"""
    return c > 0 and int(c) * 10000 >= int(largest) * int(min_bp)


def clean(xyz, rgb, tri, min_bp, normals=None):
    """-> (xyz, rgb, tri uint32, normals or None, info dict) of dvs_mesh_clean_count / _write"""
    xyz = np.asarray(xyz); rgb = np.asarray(rgb)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nv = len(xyz)
    label, n_bad = components(tri, nv)
    valid = (tri < nv).all(1) if len(tri) else np.zeros(0, bool)
    cnt = np.zeros(max(nv, 1), np.int64)
    for t in np.nonzero(valid)[0]:
        cnt[label[tri[t, 0]]] += 1
    roots = [v for v in range(nv) if label[v] == v and cnt[v] > 0]
    largest = max([int(cnt[r]) for r in roots], default=0)
    kept_roots = {r for r in roots if keeps(cnt[r], largest, min_bp)}
    tkeep = np.array([bool(valid[t]) and int(label[tri[t, 0]]) in kept_roots for t in range(len(tri))], bool)
    used = np.zeros(nv, bool)
    used[tri[tkeep].reshape(-1)] = True                      # "the vertices used by a kept triangle", from the triangles themselves
    remap = np.cumsum(used) - 1
    out_tri = remap[tri[tkeep]].astype(np.uint32).reshape(-1, 3)
    info = dict(n_components=len(roots), largest=largest, kept_components=len(kept_roots), kept_vertices=int(used.sum()),
                kept_triangles=int(tkeep.sum()), n_bad=n_bad)
    return xyz[used], rgb[used], out_tri, None if normals is None else np.asarray(normals)[used], info


def gradient(tsdf, weight):
    """float32 [nz,ny,nx,3]: per axis the central difference / 2 where both neighbours are inside the grid with weight > 0, the one-sided
    difference with the voxel itself where one is, 0 where none"""
    tsdf = np.asarray(tsdf, np.float32); ok = np.asarray(weight) > 0
    g = np.zeros(tsdf.shape + (3,), np.float32)
    for axis_xyz, ax in ((0, 2), (1, 1), (2, 0)):            # x is the last array axis
        n = tsdf.shape[ax]
        t = np.moveaxis(tsdf, ax, 0); o = np.moveaxis(ok, ax, 0)
        lo_ok = np.zeros_like(o); hi_ok = np.zeros_like(o)
        lo_ok[1:] = o[:-1]; hi_ok[:-1] = o[1:]
        lo = np.zeros_like(t); hi = np.zeros_like(t)
        lo[1:] = t[:-1]; hi[:-1] = t[1:]
        both = ((hi - lo) * np.float32(0.5)).astype(np.float32)
        r = np.where(lo_ok & hi_ok, both, np.where(hi_ok, hi - t, np.where(lo_ok, t - lo, np.float32(0)))).astype(np.float32)
        assert n == r.shape[0]
        g[..., axis_xyz] = np.moveaxis(r, 0, ax)
    return g


def crossed_edges(tsdf, weight):
    """the extraction's vertices in its order (edge id = voxel index * 7 + kind - 1) -> (pi, pj, pk, d [n,3]) of each vertex's edge p -> p + d"""
    tsdf = np.asarray(tsdf, np.float32); ok = np.asarray(weight) > 0
    nz, ny, nx = tsdf.shape
    cell = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for b in range(8):
        dx, dy, dz = b & 1, (b >> 1) & 1, (b >> 2) & 1
        cell &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    inside = tsdf < 0
    ids = []
    for kind in range(1, 8):
        d = (kind & 1, (kind >> 1) & 1, (kind >> 2) & 1)
        # the edge (p, p + d) is used by the cells p - s for the corners s with s & kind == 0
        used = np.zeros((nz, ny, nx), bool)
        for s in range(8):
            if s & kind:
                continue
            sx, sy, sz = s & 1, (s >> 1) & 1, (s >> 2) & 1
            used[sz:sz + nz - 1, sy:sy + ny - 1, sx:sx + nx - 1] |= cell
        cross = np.zeros((nz, ny, nx), bool)
        a = inside[:nz - d[2], :ny - d[1], :nx - d[0]]; b_ = inside[d[2]:, d[1]:, d[0]:]
        cross[:nz - d[2], :ny - d[1], :nx - d[0]] = a != b_
        k, j, i = np.nonzero(used & cross)
        ids.append(((k * ny + j) * nx + i) * 7 + (kind - 1))
    eids = np.sort(np.concatenate(ids))
    vox, kind = eids // 7, eids % 7 + 1
    return vox % nx, (vox // nx) % ny, vox // (nx * ny), np.stack([kind & 1, (kind >> 1) & 1, (kind >> 2) & 1], 1)


def normals(tsdf, weight):
    """float32 [nv,3] of dvs_mesh_extract_normals: n = (1 - t) g(p) + t g(p + d) in float32, over sqrt((x x + y y) + z z), or 0 when that
    sum of squares is < 1e-30"""
    tsdf = np.asarray(tsdf, np.float32)
    g = gradient(tsdf, weight)
    pi, pj, pk, d = crossed_edges(tsdf, weight)
    a = tsdf[pk, pj, pi]; b = tsdf[pk + d[:, 2], pj + d[:, 1], pi + d[:, 0]]
    t = (a / (a - b)).astype(np.float32)
    s = (np.float32(1) - t).astype(np.float32)
    gp = g[pk, pj, pi]; gq = g[pk + d[:, 2], pj + d[:, 1], pi + d[:, 0]]
    n = ((s[:, None] * gp).astype(np.float32) + (t[:, None] * gq).astype(np.float32)).astype(np.float32)
    len2 = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(np.float32) + n[:, 2] * n[:, 2]).astype(np.float32)
    live = len2 >= np.float32(1e-30)
    out = np.zeros_like(n)
    out[live] = n[live] / np.sqrt(len2[live])[:, None]
    return out


def parse_mesh_ply(path):
    """-> (xyz float32 [nv,3], rgb uint8 [nv,3], tri uint32 [nt,3], normals float32 [nv,3] or None) of a file write_mesh_ply wrote,
    with or without nx ny nz; asserts the header"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0", head[:2]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nt = int([h for h in head if h.startswith("element face")][0].split()[-1])
    props = [h for h in head if h.startswith("property")]
    pos = ["property float x", "property float y", "property float z"]
    nrm = ["property float nx", "property float ny", "property float nz"]
    col = ["property uchar red", "property uchar green", "property uchar blue", "property list uchar uint vertex_indices"]
    assert props in (pos + col, pos + nrm + col), props
    has_n = props == pos + nrm + col
    vt = np.dtype([("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if has_n else []) + [("rgb", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("idx", "<u4", 3)])
    assert vt.itemsize == (27 if has_n else 15)
    assert len(blob) == end + nv * vt.itemsize + nt * ft.itemsize, (len(blob), end, nv, nt)
    v = np.frombuffer(blob, vt, nv, end)
    f = np.frombuffer(blob, ft, nt, end + nv * vt.itemsize)
    assert (f["k"] == 3).all()
    return v["xyz"].copy(), v["rgb"].copy(), f["idx"].copy(), (v["n"].copy() if has_n else None)
