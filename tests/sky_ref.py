"""fp64 restatement of the sky model (include/dvs_raster.h, dvs_sky_forward_views / dvs_sky_backward_views; csrc/sky.hip).

Ray of pixel (x, y): ndc = ((2 x + 1) / W - 1, (2 y + 1) / H - 1); a world direction d has clip coordinates (x, y, w) = M d with M the
rows 0, 1, 3 of proj's 3x3 part (proj[c * 4 + r] multiplies input c into output r), so d = normalize(M^-1 (ndc_x, ndc_y, 1)).
rays_centred() is the rule for a centred pinhole, normalize(R^T (ndc_x tan_fovx, ndc_y tan_fovy, 1)): the two agree when the principal
point is in the middle. Lookup: u = (atan2(d.x, d.z) / 2 pi + 0.5) Ws - 0.5, v = (asin(d.y) / pi + 0.5) Hs - 0.5, bilinear, u wraps, v is
clamped to [0, Hs - 1]. The row pass is importance_ref.importance's loop with six sums per splat and the same doubtful-band bookkeeping."""
import numpy as np
from depth_ref import TILE, S2D_X, S2D_Y, S2D_CONIC, S2D_OPACITY


def _ndc(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return (2.0 * xs + 1.0) / W - 1.0, (2.0 * ys + 1.0) / H - 1.0


def rays(proj, W, H):
    """proj: the 16 floats of dvs_camera.proj -> unit world directions [H,W,3]"""
    p = np.asarray(proj, np.float64).reshape(4, 4)                   # p[c, r]
    M = np.array([[p[k, r] for k in range(3)] for r in (0, 1, 3)])
    nx, ny = _ndc(W, H)
    d = np.stack([nx, ny, np.ones_like(nx)], -1) @ np.linalg.inv(M).T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def rays_centred(view, tan_fovx, tan_fovy, W, H):
    """the centred-pinhole rule: R^T (ndc_x tan_fovx, ndc_y tan_fovy, 1), R[r][c] = view[c * 4 + r]"""
    v = np.asarray(view, np.float64).reshape(4, 4)                   # v[c, r]
    R = v[:3, :3].T
    nx, ny = _ndc(W, H)
    d = np.stack([nx * tan_fovx, ny * tan_fovy, np.ones_like(nx)], -1) @ R            # (R^T d_cam)_c = sum_r R[r][c] d_cam_r
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def taps(d, Ws, Hs):
    """unit directions [...,3] -> texel indices [...,4] (y Ws + x; order 00, 01, 10, 11 = (y0,x0), (y0,x1), (y1,x0), (y1,x1)), weights [...,4]"""
    u = (np.arctan2(d[..., 0], d[..., 2]) / (2 * np.pi) + 0.5) * Ws - 0.5
    v = np.clip((np.arcsin(np.clip(d[..., 1], -1.0, 1.0)) / np.pi + 0.5) * Hs - 0.5, 0.0, Hs - 1.0)
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = u - u0, v - v0
    x0 = np.mod(u0.astype(np.int64), Ws); x1 = np.mod(x0 + 1, Ws)
    y0 = np.clip(v0.astype(np.int64), 0, Hs - 1); y1 = np.minimum(y0 + 1, Hs - 1)
    idx = np.stack([y0 * Ws + x0, y0 * Ws + x1, y1 * Ws + x0, y1 * Ws + x1], -1)
    w = np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], -1)
    return idx, w


def lookup(tex, d):
    """tex [Hs,Ws,3], directions [H,W,3] -> s [3,H,W]"""
    Hs, Ws, _ = tex.shape
    idx, w = taps(d, Ws, Hs)
    flat = np.asarray(tex, np.float64).reshape(-1, 3)
    return np.moveaxis((flat[idx] * w[..., None]).sum(-2), -1, 0)


def sky_forward(C, final_T, tex, d):
    """C [3,H,W] (the composite's image at bg = 0), final_T [H,W] -> (out = C + final_T s, s)"""
    s = lookup(tex, d)
    return np.asarray(C, np.float64) + np.asarray(final_T, np.float64)[None] * s, s


def sky_backward_tex(final_T, g, d, Ws, Hs, unit_weights=False):
    """g = dL/dout [3,H,W] -> dL/dtex [Hs,Ws,3]. unit_weights: every tap counts in full — with |g| for g this is, per texel, the sum of
    |T_final g| over the pixels that touch it (the size an error of the bilinear weights is measured against)"""
    idx, w = taps(d, Ws, Hs)
    if unit_weights:
        w = np.ones_like(w)
    tg = np.moveaxis(np.asarray(final_T, np.float64)[None] * np.asarray(g, np.float64), 0, -1)       # [H,W,3]
    out = np.zeros((Hs * Ws, 3))
    for k in range(4):
        np.add.at(out, idx[..., k].reshape(-1), (w[..., k, None] * tg).reshape(-1, 3))
    return out.reshape(Hs, Ws, 3)


def _walk(rec, ranges, sorted_splat, n_contrib, W, H):
    """per tile: (pixel grids, per-entry generator) — the forward's walk, shared by final_T() and sky_backward_rows()"""
    tiles_x = (W + TILE - 1) // TILE
    for tile, (start, end) in enumerate(np.asarray(ranges, np.int64)):
        x0, y0 = (tile % tiles_x) * TILE, (tile // tiles_x) * TILE
        ys, xs = np.mgrid[y0:min(y0 + TILE, H), x0:min(x0 + TILE, W)]
        if not xs.size:
            continue
        nc = n_contrib[ys, xs].astype(np.int64)
        assert (nc <= end - start).all()
        yield ys, xs, nc, [int(sorted_splat[start + j]) for j in range(int(nc.max()))]


def _entry(s, xs, ys):
    dx, dy = s[S2D_X] - xs, s[S2D_Y] - ys                               # d = mean - pixel
    power = -0.5 * (s[S2D_CONIC] * dx * dx + s[S2D_CONIC + 2] * dy * dy) - s[S2D_CONIC + 1] * dx * dy
    G = np.exp(power)
    return dx, dy, power, G, s[S2D_OPACITY] * G


def final_T(splat2d, ranges, sorted_splat, n_contrib, W, H):
    """T_final [H,W] = prod (1 - alpha) over the entries each pixel takes, from the records alone"""
    rec = np.asarray(splat2d, np.float64)
    out = np.ones((H, W))
    for ys, xs, nc, ids in _walk(rec, ranges, sorted_splat, n_contrib, W, H):
        T = np.ones(xs.shape)
        for j, rid in enumerate(ids):
            _, _, power, _, raw = _entry(rec[rid], xs, ys)
            a = np.minimum(0.99, raw)
            take = (j < nc) & ~(power > 0) & ~(a < 1.0 / 255.0)
            T = np.where(take, T * (1.0 - a), T)
        out[ys, xs] = T
    return out


def sky_backward_rows(splat2d, ranges, sorted_splat, n_contrib, T_final, g, s, W, H, n, view, lineage=False):
    """The gradient of sum_p T_final(p) (s(p) . g(p)) through T_final = prod (1 - alpha), as the six row values of
    dvs_get_bwd_intermediates: with h = s . g, every taken (pixel, entry) pair has dL/dalpha = -h T_final / (1 - alpha) and
    v5 = G dL/dalpha (zero where alpha hit the 0.99 cap unless lineage); rows[i] = (opacity sum v5 dx, opacity sum v5 dy,
    opacity sum v5 dx^2, opacity sum v5 dx dy, opacity sum v5 dy^2, sum v5), d = mean - pixel.
    splat2d [*,16] (the rows sorted_splat's values index; the splat is value - view * n), T_final [H,W], g and s [3,H,W]
    -> (rows [n,6], excluded [n] bool: in some pixel that walks it an entry at or before the splat's own falls into depth_ref's bands,
        mag [n,6]: the same sums over the absolute values of the pairs' terms — what a relative error per pair is measured against)"""
    rec = np.asarray(splat2d, np.float64)
    h = (np.asarray(s, np.float64) * np.asarray(g, np.float64)).sum(0)
    c5 = -h * np.asarray(T_final, np.float64)
    rows = np.zeros((n, 6)); excl = np.zeros(n, bool); mag = np.zeros((n, 6))
    for ys, xs, nc, ids in _walk(rec, ranges, sorted_splat, n_contrib, W, H):
        bad = np.zeros(xs.shape, bool)
        c = c5[ys, xs]
        for j, rid in enumerate(ids):
            i = rid - view * n
            assert 0 <= i < n
            dx, dy, power, G, raw = _entry(rec[rid], xs, ys)
            walk = j < nc
            bad |= walk & ((np.abs(raw * 255.0 - 1.0) < 1e-5) | (np.abs(raw / 0.99 - 1.0) < 1e-5) | (np.abs(power) < 1e-6))
            a = np.minimum(0.99, raw)
            take = walk & ~(power > 0) & ~(a < 1.0 / 255.0)
            gate = take if lineage else take & ~(raw > 0.99)
            v5 = np.where(gate, G * c / (1.0 - a), 0.0)
            op = rec[rid, S2D_OPACITY]
            terms = [op * v5 * dx, op * v5 * dy, op * v5 * dx * dx, op * v5 * dx * dy, op * v5 * dy * dy, v5]
            rows[i] += [t.sum() for t in terms]
            mag[i] += [np.abs(t).sum() for t in terms]
            if (walk & bad).any():
                excl[i] = True
    return rows, excl, mag


def rows_to_grads(rows, conic):
    """dvs_get_bwd_intermediates' relations: rows [n,6], conic [n,3] (a, b, c) -> dL/dmean2D [n,2], dL/dconic [n,3], dL/dopacity [n]"""
    a, b, c = conic[:, 0], conic[:, 1], conic[:, 2]
    dmean = np.stack([-(a * rows[:, 0] + b * rows[:, 1]), -(c * rows[:, 1] + b * rows[:, 0])], 1)
    dconic = np.stack([-0.5 * rows[:, 2], -rows[:, 3], -0.5 * rows[:, 4]], 1)
    return dmean, dconic, rows[:, 5]
