"""dvs_undistort_view (csrc/undistort.hip, include/dvs_image.h) restated in numpy: the map of a pinhole target pixel into a distorted
COLMAP source image in float32, ONE rounded operation per statement in the order the header writes them, then the 1/32-pixel integer
bilinear blend. `undistort` is what the kernel must return byte for byte, mask float for float and count for count.

Beside it, independent of it: COLMAP's forward models (SIMPLE_RADIAL, RADIAL, OPENCV) in float64 as its documentation defines them
(`distort64`), a Newton inverse (`undistort_point64`) and a float64 bilinear resampler (`resample64`) for the cross-checks of
tests/test_undistort_format.py.

`python tests/undistort_ref.py` rewrites tests/golden/undistort_37x29.npz from `golden_case()`."""
import os
import numpy as np

F = np.float32
MODEL_IDS = {"SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}
FIELDS = ("fx", "fy", "cx", "cy", "ifx", "ify", "k1", "k2", "p1", "p2")


def split_params(model, params):
    """COLMAP's parameter list of model id 2, 3 or 4 -> (fx, fy, cx, cy, k1, k2, p1, p2) as Python floats (doubles)"""
    p = [float(v) for v in params]
    if model == 2:
        f, cx, cy, k = p
        return f, f, cx, cy, k, 0.0, 0.0, 0.0
    if model == 3:
        f, cx, cy, k1, k2 = p
        return f, f, cx, cy, k1, k2, 0.0, 0.0
    if model == 4:
        return tuple(p)
    raise ValueError(f"model {model} has no pinhole target here")


def descriptor(model, params, width, height):
    """the ten fp32 values of dvs_undistort_desc, each rounded once from the doubles (the reciprocals are taken in double)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = split_params(model, params)
    d = dict(width=int(width), height=int(height))
    for name, v in zip(FIELDS, (fx, fy, cx, cy, 1.0 / fx, 1.0 / fy, k1, k2, p1, p2)):
        d[name] = F(v)
    return d


def source_coordinates(desc):
    """-> (xs, ys, u + du, v + dv): float32 [H][W], every statement one rounded float32 operation"""
    W, H = desc["width"], desc["height"]
    fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2 = (F(desc[n]) for n in FIELDS)
    half, two = F(0.5), F(2.0)
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        u = x + half
        u = u - cx
        u = u * ifx
        v = y + half
        v = v - cy
        v = v * ify
        u2 = u * u
        v2 = v * v
        uv = u * v
        r2 = u2 + v2
        rad = k2 * r2
        rad = k1 + rad
        rad = rad * r2
        tp1 = two * p1
        tp2 = two * p2
        a = u * rad
        b = tp1 * uv
        a = a + b
        b = two * u2
        b = r2 + b
        b = p2 * b
        du = a + b
        a = v * rad
        b = tp2 * uv
        a = a + b
        b = two * v2
        b = r2 + b
        b = p1 * b
        dv = a + b
        ud = u + du
        vd = v + dv
        xs = fx * ud
        xs = xs + cx
        xs = xs - half
        ys = fy * vd
        ys = ys + cy
        ys = ys - half
    for t in (u, v, r2, rad, du, dv, ud, vd, xs, ys):
        assert t.dtype == F
    return xs, ys, ud, vd


def pixel_map(desc):
    """-> (valid bool [H][W], x0, x1, ax, y0, y1, ay as int64 [H][W]; 0 where invalid)"""
    W, H = desc["width"], desc["height"]
    xs, ys, _, _ = source_coordinates(desc)
    with np.errstate(all="ignore"):
        in_range = (xs > F(-1.0)) & (xs < F(W)) & (ys > F(-1.0)) & (ys < F(H))
        qxf = np.where(in_range, xs, F(0)) * F(32.0)
        qxf = np.floor(qxf + F(0.5))
        qyf = np.where(in_range, ys, F(0)) * F(32.0)
        qyf = np.floor(qyf + F(0.5))
    assert qxf.dtype == F and qyf.dtype == F
    qx, qy = qxf.astype(np.int64), qyf.astype(np.int64)
    valid = in_range & (qx >= 0) & (qx <= 32 * (W - 1)) & (qy >= 0) & (qy <= 32 * (H - 1))
    qx, qy = np.where(valid, qx, 0), np.where(valid, qy, 0)
    x0, ax, y0, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    return valid, x0, np.minimum(x0 + 1, W - 1), ax, y0, np.minimum(y0 + 1, H - 1), ay


def _blend(plane, m):
    _, x0, x1, ax, y0, y1, ay = m
    s = plane.astype(np.int64)
    return ((32 - ax) * (32 - ay) * s[y0, x0] + ax * (32 - ay) * s[y0, x1] + (32 - ax) * ay * s[y1, x0] + ax * ay * s[y1, x1] + 512) >> 10


def undistort(src, desc, mask=None):
    """src uint8 [planes][H][W], mask None or uint8 [H][W] in {0, 1} -> (dst uint8 [planes][H][W], mask float32 [H][W], invalid count)"""
    src = np.asarray(src, np.uint8)
    planes, H, W = src.shape
    assert (W, H) == (desc["width"], desc["height"])
    m = pixel_map(desc)
    valid = m[0]
    dst = np.zeros_like(src)
    for p in range(planes):
        dst[p] = np.where(valid, _blend(src[p], m), 0).astype(np.uint8)
    ok = valid
    if mask is not None:
        mask = np.asarray(mask, np.uint8)
        assert mask.shape == (H, W) and mask.max(initial=0) <= 1
        ok = valid & (_blend(mask.astype(np.int64) * 255, m) > 127)
    return dst, ok.astype(np.float32), int((~valid).sum())


# ---- the independent float64 side ----
def distort64(model, params, u, v):
    """COLMAP's forward model in normalised coordinates: (u, v) undistorted -> distorted, float64"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    r2 = u * u + v * v
    if model == 2:
        radial = params[3] * r2
        return u + u * radial, v + v * radial
    if model == 3:
        radial = params[3] * r2 + params[4] * r2 * r2
        return u + u * radial, v + v * radial
    if model == 4:
        k1, k2, p1, p2 = params[4:8]
        radial = k1 * r2 + k2 * r2 * r2
        du = u * radial + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u)
        dv = v * radial + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v)
        return u + du, v + dv
    raise ValueError(model)


def source_coordinates64(model, params, W, H):
    """-> (xs, ys) float64 [H][W]: where the centre of target pixel (x, y) falls in the source image, in index coordinates"""
    fx, fy, cx, cy = split_params(model, params)[:4]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ud, vd = distort64(model, params, (x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy)
    return fx * ud + cx - 0.5, fy * vd + cy - 0.5


def undistort_point64(model, params, ud, vd, iterations=50):
    """Newton's method on distort64 with a finite-difference Jacobian: distorted -> undistorted normalised coordinates"""
    ud, vd = np.asarray(ud, np.float64), np.asarray(vd, np.float64)
    u, v = ud.copy(), vd.copy()
    eps = 1e-7
    for _ in range(iterations):
        fu, fv = distort64(model, params, u, v)
        au, av = distort64(model, params, u + eps, v)
        bu, bv = distort64(model, params, u, v + eps)
        j00, j10, j01, j11 = (au - fu) / eps, (av - fv) / eps, (bu - fu) / eps, (bv - fv) / eps
        det = j00 * j11 - j01 * j10
        eu, ev = fu - ud, fv - vd
        u = u - (j11 * eu - j01 * ev) / det
        v = v - (j00 * ev - j10 * eu) / det
    return u, v


def resample64(plane, xs, ys):
    """float64 bilinear resampling of uint8 [H][W] at (xs, ys), rounded half up -> (uint8 [H][W], valid): valid iff the coordinate
    has a source, 0 <= xs <= W - 1 and 0 <= ys <= H - 1"""
    H, W = plane.shape
    with np.errstate(all="ignore"):
        valid = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
    sx, sy = np.where(valid, xs, 0.0), np.where(valid, ys, 0.0)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = sx - x0, sy - y0
    s = plane.astype(np.float64)
    val = (1 - ax) * (1 - ay) * s[y0, x0] + ax * (1 - ay) * s[y0, x1] + (1 - ax) * ay * s[y1, x0] + ax * ay * s[y1, x1]
    return np.where(valid, np.floor(val + 0.5), 0).astype(np.uint8), valid


def smooth_image(W, H, planes=3, seed=0):
    """uint8 [planes][H][W] of smooth random content: a sum of two low-frequency waves per plane; horizontally or vertically adjacent
    pixels differ by at most 16 levels (the slope is at most 60 * 0.12 + 50 * 0.1 = 12.2 levels per pixel, plus the two roundings)"""
    r = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    out = np.zeros((planes, H, W), np.uint8)
    for p in range(planes):
        a, b = r.uniform(0.04, 0.12, 2)
        c, d = r.uniform(-0.07, 0.07, 2)
        ph = r.uniform(0, 2 * np.pi, 3)
        img = 128 + 60 * np.sin(a * x + ph[0]) * np.cos(b * y + ph[1]) + 50 * np.sin(c * x + d * y + ph[2])
        out[p] = np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8)
    assert np.abs(np.diff(out.astype(int), axis=1)).max(initial=0) <= 16 and np.abs(np.diff(out.astype(int), axis=2)).max(initial=0) <= 16
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort_37x29.npz")
GOLDEN_MODEL, GOLDEN_PARAMS = 4, [31.5, 29.25, 20.75, 12.5, 0.21, -0.06, 0.013, -0.009]     # OPENCV, fx != fy, off-centre, all four coefficients


def golden_case():
    """-> the arrays of tests/golden/undistort_37x29.npz"""
    W, H = 37, 29
    desc = descriptor(GOLDEN_MODEL, GOLDEN_PARAMS, W, H)
    r = np.random.default_rng(2024)
    src = r.integers(0, 256, (3, H, W), dtype=np.uint8)
    src_mask = (r.random((H, W)) < 0.8).astype(np.uint8)
    dst, mask, invalid = undistort(src, desc)
    _, mask_m, _ = undistort(src, desc, src_mask)
    return dict(src=src, src_mask=src_mask, desc=np.array([desc[n] for n in FIELDS], np.float32), params=np.array(GOLDEN_PARAMS, np.float64),
                dst=dst, mask=mask, mask_with_source_mask=mask_m, invalid=np.array(invalid, np.int64))


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **golden_case())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
