"""numpy restatement of include/dvs_region.h in float64: the region of three vectors and a box, which centres lie inside it, which pixels'
rays cross it. The inputs are the float32 values the library is given (the region's 18 floats, the camera's fields); everything after
that is float64, so the comparison with the device is exact away from the faces and edges — `near` marks what is left out."""
import numpy as np

KEEP, PRUNE = 0, 3


def rotation(rot):
    """glm::quat(vec3 euler) -> matrix: R = Rz(rot.z) Ry(rot.y) Rx(rot.x), angles in radians"""
    rx, ry, rz = (float(v) for v in rot)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def from_trs(pos, rot, scale):
    """-> (w2b [3,4], b2w [4,4]) in float64: F = T(pos) R(rot) S(scale) and the first three rows of its inverse"""
    pos, scale = np.asarray(pos, np.float64), np.asarray(scale, np.float64)
    F = np.eye(4)
    F[:3, :3] = rotation(rot) @ np.diag(scale)
    F[:3, 3] = pos
    return np.linalg.inv(F)[:3], F


def local(points, w2b):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    w = np.asarray(w2b, np.float64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        return p @ w[:, :3].T + w[:, 3]


def plan(points, w2b, lo, hi, band=0.0):
    """-> (action uint8 [n], offsets uint32 [n], count, near bool [n]): near = some local coordinate within band * (hi - lo) of a face"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = local(points, w2b)
    with np.errstate(invalid="ignore"):
        inside = ((c >= lo) & (c <= hi)).all(1)
        near = ((np.abs(c - lo) <= band * (hi - lo)) | (np.abs(c - hi) <= band * (hi - lo))).any(1)
    action = np.where(inside, KEEP, PRUNE).astype(np.uint8)
    kept = inside.astype(np.int64)
    return action, (np.cumsum(kept) - kept).astype(np.uint32), int(kept.sum()), near


def pixel_rays(proj, W, H):
    """world ray directions [H,W,3] (not normalised) of the pixel centres (ndc = (2 i + 1) / size - 1), from the camera's proj (element
    [c*4+r]): clip (x, y, w) = M d with M the rows 0, 1, 3 of proj's 3x3 part, so d = M^-1 (ndc_x, ndc_y, 1)"""
    p = np.asarray(proj, np.float64).reshape(4, 4)          # p[c][r]
    M = np.array([[p[c][r] for c in range(3)] for r in (0, 1, 3)])
    Minv = np.linalg.inv(M)
    nx = (2.0 * np.arange(W) + 1.0) / W - 1.0
    ny = (2.0 * np.arange(H) + 1.0) / H - 1.0
    ndc = np.stack([np.broadcast_to(nx[None, :], (H, W)), np.broadcast_to(ny[:, None], (H, W)), np.ones((H, W))], -1)
    return ndc @ Minv.T


def mask(cam, w2b, lo, hi, W, H, rel=1e-5):
    """-> (hit float32 [H,W] in {0, 1}, near bool [H,W]) of camera `cam` (fields proj, campos). near: the slab interval [tmin, tmax] is
    narrower than rel of its larger end (the ray grazes an edge or a corner), or a box the ray does cross ends within rel of the camera (tmax ~ 0)"""
    w = np.asarray(w2b, np.float64).reshape(3, 4)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = w[:, :3] @ np.asarray(list(cam.campos), np.float64) + w[:, 3]
    l = pixel_rays(list(cam.proj), W, H) @ w[:, :3].T       # [H,W,3]
    tmin, tmax = np.full((H, W), -np.inf), np.full((H, W), np.inf)
    ok = np.ones((H, W), bool)
    for k in range(3):
        zero = l[..., k] == 0.0
        ok &= ~zero | ((o[k] >= lo[k]) and (o[k] <= hi[k]))
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo[k] - o[k]) / l[..., k], (hi[k] - o[k]) / l[..., k]
        tmin = np.where(zero, tmin, np.maximum(tmin, np.minimum(t0, t1)))
        tmax = np.where(zero, tmax, np.minimum(tmax, np.maximum(t0, t1)))
    hit = ok & (tmin <= tmax) & (tmax >= 0.0)
    with np.errstate(invalid="ignore"):
        size = np.maximum(np.abs(tmin), np.abs(tmax))
        near = ok & np.isfinite(size) & ((np.abs(tmax - tmin) <= rel * size) | ((np.abs(tmax) <= rel * size) & (tmin <= tmax)))
    return hit.astype(np.float32), near
