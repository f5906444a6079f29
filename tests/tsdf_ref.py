"""fp64 restatement of dvs_tsdf_integrate (include/dvs_mesh.h), view after view over the whole grid at once. The pixel is written the
way the issue states it — focal * x / zc + (size - 1) / 2 plus the principal-point offset, which is recovered from proj = P view as
P = proj view^-1 — not the ndc form the kernel evaluates."""
import numpy as np


def mat(m):
    """dvs_camera's 16 floats (element [c*4+r]) as the 4x4 matrix that multiplies column vectors"""
    return np.array(list(m), np.float64).reshape(4, 4).T


def voxel_centres(origin, voxel, dims):
    nx, ny, nz = dims
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
    o32 = np.asarray(origin, np.float32).astype(np.float64)
    return np.stack([o32[0] + i * float(np.float32(voxel)), o32[1] + j * float(np.float32(voxel)), o32[2] + k * float(np.float32(voxel))], -1)


def integrate(state, origin, voxel, dims, cams, depth, alpha, rgb, masks, trunc):
    """state = (tsdf, weight, rgb) fp64 [nz,ny,nx(,3)], updated in place and returned with `excluded` [nz,ny,nx] bool: voxels within 1e-3
    of a pixel rounding boundary, 1e-4 trunc of sdf = -trunc or 1e-4 of zc = 0.01 in some view"""
    tsdf, weight, col = state
    p = voxel_centres(origin, voxel, dims)
    excl = np.zeros(tsdf.shape, bool)
    trunc = float(np.float32(trunc))
    for v, cam in enumerate(cams):
        W, H = cam.width, cam.height
        V = mat(cam.view); P = mat(cam.proj) @ np.linalg.inv(V)
        pc = p @ V[:3, :3].T + V[:3, 3]
        zc = pc[..., 2]
        excl |= np.abs(zc - 0.01) < 1e-4
        ok = zc > 0.01
        zs = np.where(ok, zc, 1.0)
        u = cam.focal_x * pc[..., 0] / zs + (W - 1) / 2 + P[0, 2] * W / 2
        r = cam.focal_y * pc[..., 1] / zs + (H - 1) / 2 + P[1, 2] * H / 2
        for q in (u, r):
            excl |= ok & (np.abs(q + 0.5 - np.round(q + 0.5)) < 1e-3)
        ui, ri = np.floor(u + 0.5).astype(np.int64), np.floor(r + 0.5).astype(np.int64)
        ok &= (ui >= 0) & (ui < W) & (ri >= 0) & (ri < H)
        ui, ri = np.clip(ui, 0, W - 1), np.clip(ri, 0, H - 1)
        ok &= ~(alpha[v][ri, ui] < 0.5)
        if masks is not None and masks[v] is not None:
            ok &= masks[v][ri, ui] != 0
        sdf = depth[v][ri, ui].astype(np.float64) - zc
        excl |= ok & (np.abs(sdf + trunc) < 1e-4 * trunc)
        ok &= ~(sdf < -trunc)
        t = np.minimum(1.0, sdf / trunc)
        w1 = weight + 1.0
        tsdf[...] = np.where(ok, (tsdf * weight + t) / w1, tsdf)
        pix = np.stack([rgb[v][c][ri, ui] for c in range(3)], -1).astype(np.float64)
        col[...] = np.where(ok[..., None], (col * weight[..., None] + pix) / w1[..., None], col)
        weight[...] = np.where(ok, w1, weight)
    return excl
