"""numpy restatement of dvs_mesh_decimate_count / _write (include/dvs_mesh.h), written from the definition: float32 operation by
operation, Python integers for the colour rule, a dictionary for the duplicates, no sort of triangles and no scan. Not shared with
the kernels in any part."""
import numpy as np

F32 = np.float32


def cell_keys(xyz, origin, cell, ncell):
    """-> int64 [nv]: key = (i_z * ncell_y + i_y) * ncell_x + i_x with, per axis, q = (x - origin) / cell in float32; i = 0 if !(q >= 0)
    (a NaN too), ncell - 1 if q >= float32(ncell), else the truncation of q"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    idx = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            q = (xyz[:, a] - F32(origin[a])) / F32(cell)
            assert q.dtype == F32
            n = int(ncell[a])
            low = ~(q >= F32(0))
            high = ~low & (q >= F32(n))
            mid = ~low & ~high
            i = np.zeros(len(q), np.int64)
            i[high] = n - 1
            i[mid] = np.trunc(q[mid]).astype(np.int64)
            idx.append(i)
    return (idx[2] * int(ncell[1]) + idx[1]) * int(ncell[0]) + idx[0]


def rotate_min_first(a, b, c):
    """the rotation of (a, b, c) whose first entry is the smallest (a, b, c distinct); the winding is kept"""
    m = min(a, b, c)
    return (a, b, c) if m == a else (b, c, a) if m == b else (c, a, b)


def decimate(xyz, rgb, tri, origin, cell, ncell, normals=None):
    """-> (xyz float32, rgb uint8, tri uint32, normals float32 or None, info dict of dvs_mesh_decimate_info)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nv = len(xyz)
    keys = cell_keys(xyz, origin, cell, ncell)
    occupied = sorted(set(keys.tolist()))                       # the clusters in key order
    number = {k: c for c, k in enumerate(occupied)}
    cluster_of = [number[k] for k in keys.tolist()]
    members = [[] for _ in occupied]
    for v in range(nv):                                          # ascending vertex index inside every cluster
        members[cluster_of[v]].append(v)

    n_bad = n_degenerate = n_duplicate = 0
    seen = {}
    kept = []                                                    # (original triangle index order) cluster triples, corner order as given
    for t in range(len(tri)):
        v0, v1, v2 = (int(x) for x in tri[t])
        if v0 >= nv or v1 >= nv or v2 >= nv:
            n_bad += 1
            continue
        c = (cluster_of[v0], cluster_of[v1], cluster_of[v2])
        if c[0] == c[1] or c[1] == c[2] or c[0] == c[2]:
            n_degenerate += 1
            continue
        canon = rotate_min_first(*c)
        if canon in seen:                                        # an earlier (smaller) triangle index holds it
            n_duplicate += 1
            continue
        seen[canon] = t
        kept.append(c)

    used = sorted({c for k in kept for c in k})                  # clusters some kept triangle uses, in key order
    new_index = {c: o for o, c in enumerate(used)}
    out_tri = np.array([[new_index[c] for c in k] for k in kept], np.uint32).reshape(-1, 3)
    out_xyz = np.zeros((len(used), 3), F32)
    out_rgb = np.zeros((len(used), 3), np.uint8)
    out_nrm = None if normals is None else np.zeros((len(used), 3), F32)
    nrm = None if normals is None else np.asarray(normals, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for o, c in enumerate(used):
            m = members[c]
            count = len(m)
            for a in range(3):
                s = xyz[m[0], a]
                for v in m[1:]:
                    s = F32(s + xyz[v, a])
                out_xyz[o, a] = F32(s / F32(count))
                total = sum(int(rgb[v, a]) for v in m)
                out_rgb[o, a] = (2 * total + count) // (2 * count)
            if nrm is not None:
                n = [nrm[m[0], a] for a in range(3)]
                for v in m[1:]:
                    n = [F32(n[a] + nrm[v, a]) for a in range(3)]
                l2 = F32(F32(F32(n[0] * n[0]) + F32(n[1] * n[1])) + F32(n[2] * n[2]))
                if l2 < F32(1e-30):
                    out_nrm[o] = 0
                else:
                    length = np.sqrt(l2)
                    assert length.dtype == F32
                    out_nrm[o] = [F32(n[a] / length) for a in range(3)]
    info = {"out_vertices": len(used), "out_triangles": len(kept), "n_clusters": len(occupied), "n_degenerate": n_degenerate,
            "n_duplicate": n_duplicate, "n_bad": n_bad}
    return out_xyz, out_rgb, out_tri, out_nrm, info


def lattice(lo, voxel, dims, factor):
    """the plugin's lattice for --meshDecimate `factor` over a grid at `lo` with `dims` voxels of edge `voxel` (all float32): the voxel lattice
    shifted by half a voxel -> (origin float32 [3], cell float32, ncell [3])"""
    voxel = F32(voxel)
    origin = np.array([F32(F32(lo[a]) - F32(F32(0.5) * voxel)) for a in range(3)], F32)
    return origin, F32(F32(factor) * voxel), [(int(dims[a]) + factor - 1) // factor for a in range(3)]
