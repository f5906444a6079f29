"""numpy restatement of the export transform (include/dvs_export.h, last section: dvs_similarity_*, dvs_sh_rotation, dvs_transform_splats,
dvs_transform_points) — TEST INFRASTRUCTURE, not product code: the yardstick csrc/transform.hip is compared with bit for bit. Every fp32
result is formed operation by operation on np.float32 arrays (one IEEE operation per numpy call, nothing fused); the fp64 variant runs
the same formulas in float64 with band matrices solved in float64."""
import math
import numpy as np

f32, f64 = np.float32, np.float64
BANDS = ((0, 3, 0), (3, 5, 9), (8, 7, 34))               # (first coefficient, size, offset into D[83]) of bands 1, 2, 3

# the constants of csrc/dvs_device.h, fp32 values
C1 = f64(f32(0.4886025119029199))
C2 = [f64(f32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
C3 = [f64(f32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                            1.445305721320277, -0.5900435899266435)]


def basis15(d):
    """the 15 basis functions above the dc term at unit directions d [m,3], float64 (dvs_sh_basis)"""
    d = np.asarray(d, f64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], axis=1)


def sh_rotation64(R, basis=basis15, samples=96):
    """the three band matrices in float64 as one [83] vector: least squares of Y(R d) D = Y(d) over a Fibonacci spiral of directions"""
    R = np.asarray(R, f64).reshape(3, 3)
    k = np.arange(samples, dtype=f64)
    z = 1.0 - (2.0 * k + 1.0) / samples
    rad = np.sqrt(1.0 - z * z)
    d = np.stack([rad * np.cos(2.399963229728653 * k), rad * np.sin(2.399963229728653 * k), z], axis=1)
    y0, y1 = basis(d), basis(d @ R.T)
    out = np.zeros(83, f64)
    for first, m, off in BANDS:
        D = np.linalg.lstsq(y1[:, first:first + m], y0[:, first:first + m], rcond=None)[0]
        out[off:off + m * m] = D.reshape(-1)
    return out


def quat_of_rotation(R):
    """the unit quaternion (w, x, y, z) of a row-major rotation matrix, float64, branch and operation order of tf_quat_of"""
    R = [f64(v) for v in np.asarray(R, f32).reshape(9)]
    tr = (R[0] + R[4]) + R[8]
    if tr >= R[0] and tr >= R[4] and tr >= R[8]:
        S = np.sqrt(tr + 1.0) * 2.0
        q = [0.25 * S, (R[7] - R[5]) / S, (R[2] - R[6]) / S, (R[3] - R[1]) / S]
    elif R[0] >= R[4] and R[0] >= R[8]:
        S = np.sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0
        q = [(R[7] - R[5]) / S, 0.25 * S, (R[1] + R[3]) / S, (R[2] + R[6]) / S]
    elif R[4] >= R[8]:
        S = np.sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0
        q = [(R[2] - R[6]) / S, (R[1] + R[3]) / S, 0.25 * S, (R[5] + R[7]) / S]
    else:
        S = np.sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0
        q = [(R[3] - R[1]) / S, (R[2] + R[6]) / S, (R[5] + R[7]) / S, 0.25 * S]
    ln = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.array([v / ln for v in q], f64)


def _row(r, x, y, z):
    return (r[0] * x + r[1] * y) + r[2] * z


def transform_points(R, t, s, xyz, normals=None, dtype=f32):
    R, t, s = np.asarray(R, dtype).reshape(3, 3), np.asarray(t, dtype).reshape(3), dtype(s)
    xyz = np.asarray(xyz, dtype).reshape(-1, 3)
    out = np.stack([_row(R[k], xyz[:, 0], xyz[:, 1], xyz[:, 2]) * s + t[k] for k in range(3)], axis=1)
    if normals is None:
        return out, None
    nr = np.asarray(normals, dtype).reshape(-1, 3)
    return out, np.stack([_row(R[k], nr[:, 0], nr[:, 1], nr[:, 2]) for k in range(3)], axis=1)


def rotate_sh(D, shN, degree, dtype=f32):
    """shN [n,45] -> [n,45]: bands 1..degree rotated, the rest copied"""
    D = np.asarray(D, dtype).reshape(83)
    v = np.asarray(shN, dtype).reshape(-1, 15, 3)
    out = v.copy()
    for band, (first, m, off) in enumerate(BANDS, start=1):
        if band > degree:
            break
        M = D[off:off + m * m].reshape(m, m)
        for j in range(m):
            acc = M[j, 0] * v[:, first, :]
            for k in range(1, m):
                acc = acc + M[j, k] * v[:, first + k, :]
            out[:, first + j, :] = acc
    return out.reshape(-1, 45)


def transform_splats(R, t, s, D, pos, shN, scale, rot, degree, dtype=f32):
    """-> dict pos, shN ([n,45], or None when shN is None), scale, rot of dvs_transform_splats"""
    pos_out, _ = transform_points(R, t, s, pos, None, dtype)
    ls = dtype(math.log(float(f32(s))))                    # the log in fp64 of the fp32 s, rounded once
    scale_out = np.asarray(scale, dtype).reshape(-1, 3) + ls
    a = quat_of_rotation(R).astype(dtype)
    q = np.asarray(rot, dtype).reshape(-1, 4)
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rot_out = np.stack([((a[0] * qw - a[1] * qx) - a[2] * qy) - a[3] * qz,
                        ((a[0] * qx + a[1] * qw) + a[2] * qz) - a[3] * qy,
                        ((a[0] * qy - a[1] * qz) + a[2] * qw) + a[3] * qx,
                        ((a[0] * qz + a[1] * qy) - a[2] * qx) + a[3] * qw], axis=1)
    return {"pos": pos_out, "shN": None if shN is None else rotate_sh(D, shN, degree, dtype), "scale": scale_out, "rot": rot_out}


def similarity_inverse(R, t, s):
    """(R', t', s') of dvs_similarity_inverse, float32 from float64"""
    R, t, s = np.asarray(R, f32).reshape(3, 3).astype(f64), np.asarray(t, f32).astype(f64), f64(f32(s))
    return R.T.astype(f32), (-(R.T @ t) / s).astype(f32), f32(1.0 / s)


def tiled(shN, pad=0.0):
    """[n][45] -> DVS_SHN_TILED, whole tiles; the pads and the lanes past n hold `pad`"""
    shN = np.asarray(shN, f32).reshape(-1, 45)
    n = len(shN)
    tiles = (n + 63) // 64
    full = np.full((tiles * 64, 48), pad, f32)
    full[:n, :45] = shN
    return np.ascontiguousarray(full.reshape(tiles, 64, 12, 4).transpose(0, 2, 1, 3)).reshape(-1)


def quat_to_matrix(q):
    """rotation matrices [n,3,3] of (w, x, y, z) quaternions, normalised first, float64 (dvs_quat_to_rot)"""
    q = np.asarray(q, f64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


# ---- the render-invariance scene of tests/test_gpu_transform.py: built here so that the CPU oracle and the GPU test share it ------------
INVARIANCE_SEED = 3
INVARIANCE_TRS = ([0.5, -1.0, 2.0], [0.3, -0.7, 1.1], 2.5)


def invariance_scene(seed=INVARIANCE_SEED, n=500, size=64, fov_deg=60.0):
    """-> (model dict in the A0 layout, Rc [3,3] world->camera, cc [3] camera centre): n splats in front of a camera at the origin looking
    along +z, every depth in [2, 6], inside the field of view, SH degree 3 with strong higher bands"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 6.0, n)
    half = 0.9 * math.tan(math.radians(fov_deg) / 2)
    xy = rng.uniform(-half, half, (n, 2)) * z[:, None]
    model = {"pos": np.concatenate([xy, z[:, None]], axis=1).astype(f32),
             "sh0": rng.uniform(-0.5, 1.5, (n, 3)).astype(f32),
             "shN": (0.4 * rng.normal(size=(n, 15, 3))).astype(f32),
             "opacity": rng.uniform(-1.0, 2.0, n).astype(f32),
             "scale": rng.uniform(-2.6, -1.6, (n, 3)).astype(f32),
             "rot": rng.normal(size=(n, 4)).astype(f32)}
    return model, np.eye(3), np.zeros(3)


def moved_camera(R, t, s, Rc, cc):
    """the camera (Rc, cc) under p' = s R p + t: centre s R cc + t, world->camera rotation Rc R^T; -> (Rc', translation t' = -Rc' centre')"""
    R, t, Rc, cc = (np.asarray(v, f64) for v in (R, t, Rc, cc))
    R = R.reshape(3, 3)
    centre = float(s) * (R @ cc) + t
    Rn = Rc @ R.T
    return Rn, -Rn @ centre
