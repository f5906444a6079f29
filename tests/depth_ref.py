"""fp64 restatement of dvs_raster_depth_views (include/dvs_raster.h) from the exported forward state: per pixel the tile's list entries
[start, start + n_contrib) in order, skip when power > 0, skip when alpha < 1/255, alpha = min(0.99, opacity exp(power)),
w = alpha T, D += w z, T *= 1 - alpha; alpha_out = 1 - T, depth = D / alpha_out where alpha_out >= 1/255, else 0."""
import numpy as np

TILE = 16
S2D_X, S2D_Y, S2D_CONIC, S2D_OPACITY, S2D_DEPTH = 0, 1, 2, 5, 9


def depth_alpha(splat2d, ranges, sorted_splat, n_contrib, W, H):
    """splat2d [*,16] (the rows sorted_splat's values index), ranges [tiles,2], n_contrib [H,W] of ONE view
    -> (depth [H,W], alpha [H,W], excluded [H,W] bool: a walked entry within 1e-5 relative of a threshold, or |power| < 1e-6)"""
    rec = np.asarray(splat2d, np.float64)
    tiles_x = (W + TILE - 1) // TILE
    depth = np.zeros((H, W)); alpha_out = np.zeros((H, W)); excl = np.zeros((H, W), bool)
    for tile, (start, end) in enumerate(np.asarray(ranges, np.int64)):
        x0, y0 = (tile % tiles_x) * TILE, (tile // tiles_x) * TILE
        ys, xs = np.mgrid[y0:min(y0 + TILE, H), x0:min(x0 + TILE, W)]
        nc = n_contrib[ys, xs].astype(np.int64)
        assert (nc <= end - start).all()
        T = np.ones(xs.shape); D = np.zeros(xs.shape); bad = np.zeros(xs.shape, bool)
        for j in range(int(nc.max()) if nc.size else 0):
            s = rec[sorted_splat[start + j]]
            dx, dy = xs - s[S2D_X], ys - s[S2D_Y]
            power = -0.5 * (s[S2D_CONIC] * dx * dx + s[S2D_CONIC + 2] * dy * dy) - s[S2D_CONIC + 1] * dx * dy
            raw = s[S2D_OPACITY] * np.exp(power)
            walk = j < nc
            bad |= walk & ((np.abs(raw * 255.0 - 1.0) < 1e-5) | (np.abs(raw / 0.99 - 1.0) < 1e-5) | (np.abs(power) < 1e-6))
            a = np.minimum(0.99, raw)
            take = walk & ~(power > 0) & ~(a < 1.0 / 255.0)
            w = np.where(take, a * T, 0.0)
            D += w * s[S2D_DEPTH]
            T = np.where(take, T * (1.0 - a), T)
        al = 1.0 - T
        alpha_out[ys, xs] = al
        depth[ys, xs] = np.where(al >= 1.0 / 255.0, D / np.maximum(al, 1e-300), 0.0)
        excl[ys, xs] = bad
    return depth, alpha_out, excl
