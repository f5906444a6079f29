"""numpy restatement of the 3D smoothing filter (include/dvs_train.h, last section; divshot_amd/csrc/filter3d.hip): compute, apply, chain.

Every function takes `dtype`: float64 is the reference, float32 evaluates the SAME formulas in the kernels' precision (numpy rounds every
operation, there is no FMA), which is what the GPU tests measure their tolerance from."""
import numpy as np

NEAR = 0.2
MARGIN = 0.65
VARIANCE = 0.2


def pack_cameras(cameras):
    """[n_cams,16] float32 from objects with view (16 floats, view[c*4+r]), focal_x, width, height — dvs_filter3d_pack_cameras"""
    rows = np.zeros((len(cameras), 16), np.float32)
    for c, cam in enumerate(cameras):
        v = np.asarray(list(cam.view), np.float32).reshape(4, 4)               # v[c][r]
        rows[c, :12] = v.T[:3].reshape(12)
        rows[c, 12:15] = (cam.focal_x, cam.width, cam.height)
    return rows


def camera_space(pos, rows, dtype=np.float64):
    """-> x, y, z [n_cams, n] of every splat in every camera (rows: packed camera rows)"""
    p = np.asarray(pos, dtype).reshape(-1, 3)
    r = np.asarray(rows, dtype).reshape(-1, 16)
    out = []
    with np.errstate(all="ignore"):
        for k in range(3):
            m = r[:, 4 * k:4 * k + 4]
            out.append(((m[:, 0:1] * p[None, :, 0] + m[:, 1:2] * p[None, :, 1]) + m[:, 2:3] * p[None, :, 2]) + m[:, 3:4])
    return out


def visibility_terms(pos, rows, dtype=np.float64):
    """the three quantities the visibility rule compares and their bounds: (z, NEAR), (|x/z f|, MARGIN w), (|y/z f|, MARGIN h), each [n_cams, n]"""
    x, y, z = camera_space(pos, rows, dtype)
    r = np.asarray(rows, dtype).reshape(-1, 16)
    f, w, h = r[:, 12:13], r[:, 13:14], r[:, 14:15]
    with np.errstate(all="ignore"):
        return [(z, np.full_like(z, NEAR)), (np.abs(x / z * f), np.broadcast_to(dtype(MARGIN) * w, z.shape)),
                (np.abs(y / z * f), np.broadcast_to(dtype(MARGIN) * h, z.shape))]


def compute(pos, rows, dtype=np.float64):
    """-> (filter [n], seen [n] bool): filter = sqrt(0.2) min over the seeing cameras of z / focal_x; an unseen splat (a non-finite position
    always is) takes the maximum over the seen ones; all zeros when none is seen"""
    p = np.asarray(pos, dtype).reshape(-1, 3)
    (z, near), (ax, bx), (ay, by) = visibility_terms(p, rows, dtype)
    f = np.asarray(rows, dtype).reshape(-1, 16)[:, 12:13]
    with np.errstate(all="ignore"):
        sees = (z > near) & (ax <= bx) & (ay <= by) & np.isfinite(p).all(axis=1)[None, :]
        rate = np.where(sees, z / f, np.inf).min(axis=0)
    seen = sees.any(axis=0)
    filt = np.zeros(p.shape[0], dtype)
    if seen.any():
        filt[seen] = np.sqrt(dtype(VARIANCE)) * rate[seen]
        filt[~seen] = filt[seen].max()
    return filt, seen


def _terms(scale, opacity, filt, dtype):
    """r, q = 1 - r, d = s^2 + f^2 [n,3]; c, sp = sigmoid(a), sn = sigmoid(-a), u = 1 - o' [n] — the kernels' operations in their order"""
    s = np.asarray(scale, dtype).reshape(-1, 3)
    a = np.asarray(opacity, dtype).reshape(-1)
    f2 = (np.asarray(filt, dtype).reshape(-1) ** 2)[:, None]
    one, two = dtype(1), dtype(2)
    s2 = np.exp(two * s)
    d = s2 + f2
    r, q = s2 / d, f2 / d
    c = (np.sqrt(r[:, 0]) * np.sqrt(r[:, 1])) * np.sqrt(r[:, 2])
    one_minus_c = ((q[:, 0] + r[:, 0] * q[:, 1]) + (r[:, 0] * r[:, 1]) * q[:, 2]) / (one + c)
    sp = one / (one + np.exp(-a))
    sn = one / (one + np.exp(a))
    u = sn + sp * one_minus_c
    return r, q, d, c, sp, sn, u


def apply(scale, opacity, filt, dtype=np.float64):
    """-> (scale_eff [n,3], opacity_eff [n]); rows with filter 0 are the inputs"""
    s = np.asarray(scale, dtype).reshape(-1, 3)
    a = np.asarray(opacity, dtype).reshape(-1)
    r, q, d, c, sp, sn, u = _terms(s, a, filt, dtype)
    scale_eff = dtype(0.5) * np.log(d)
    opacity_eff = np.log(sp * c) - np.log(u)
    off = np.asarray(filt).reshape(-1) == 0
    scale_eff[off] = s[off]
    opacity_eff[off] = a[off]
    return scale_eff, opacity_eff


def chain(scale, opacity, filt, g_scale, g_opacity, dtype=np.float64):
    """-> (g_scale [n,3], g_opacity [n]) with respect to the trained values, from those with respect to the effective ones"""
    gs = np.asarray(g_scale, dtype).reshape(-1, 3).copy()
    go = np.asarray(g_opacity, dtype).reshape(-1).copy()
    r, q, d, c, sp, sn, u = _terms(scale, opacity, filt, dtype)
    out_s = gs * r + go[:, None] * q / u[:, None]
    out_o = go * sn / u
    off = np.asarray(filt).reshape(-1) == 0
    out_s[off] = gs[off]
    out_o[off] = go[off]
    return out_s, out_o
