"""fp64 restatement of dvs_raster_importance_views (include/dvs_raster.h) from the exported forward state: tests/depth_ref.py's loop,
accumulating per splat instead of per pixel. Per pixel the tile's list entries [start, start + n_contrib) in order, skip when power > 0,
skip when alpha < 1/255, alpha = min(0.99, opacity exp(power)); every taken entry gets w = alpha T, then T *= 1 - alpha."""
import numpy as np
from depth_ref import TILE, S2D_X, S2D_Y, S2D_CONIC, S2D_OPACITY


def importance(splat2d, ranges, sorted_splat, n_contrib, W, H, n, view, mask=None):
    """splat2d [*,16] (the rows sorted_splat's values index), ranges [tiles,2], n_contrib [H,W] of ONE view whose records start at row
    view * n; mask None or [H,W] (a pixel with value 0 contributes nothing)
    -> (sum [n] of w, max [n] of w, hits [n] int64, excluded [n] bool: in some pixel an entry at or before the splat's own falls into
    depth_ref's threshold bands — alpha within 1e-5 relative of 1/255 or 0.99, or |power| < 1e-6 — so its T or its own take is in doubt)"""
    rec = np.asarray(splat2d, np.float64)
    tiles_x = (W + TILE - 1) // TILE
    wsum = np.zeros(n); wmax = np.zeros(n); hits = np.zeros(n, np.int64); excl = np.zeros(n, bool)
    for tile, (start, end) in enumerate(np.asarray(ranges, np.int64)):
        x0, y0 = (tile % tiles_x) * TILE, (tile // tiles_x) * TILE
        ys, xs = np.mgrid[y0:min(y0 + TILE, H), x0:min(x0 + TILE, W)]
        nc = n_contrib[ys, xs].astype(np.int64)
        assert (nc <= end - start).all()
        if mask is not None:
            nc = np.where(mask[ys, xs] == 0, 0, nc)
        T = np.ones(xs.shape); bad = np.zeros(xs.shape, bool)
        for j in range(int(nc.max()) if nc.size else 0):
            rid = int(sorted_splat[start + j])
            s = rec[rid]
            i = rid - view * n
            assert 0 <= i < n
            dx, dy = xs - s[S2D_X], ys - s[S2D_Y]
            power = -0.5 * (s[S2D_CONIC] * dx * dx + s[S2D_CONIC + 2] * dy * dy) - s[S2D_CONIC + 1] * dx * dy
            raw = s[S2D_OPACITY] * np.exp(power)
            walk = j < nc
            bad |= walk & ((np.abs(raw * 255.0 - 1.0) < 1e-5) | (np.abs(raw / 0.99 - 1.0) < 1e-5) | (np.abs(power) < 1e-6))
            a = np.minimum(0.99, raw)
            take = walk & ~(power > 0) & ~(a < 1.0 / 255.0)
            w = np.where(take, a * T, 0.0)
            wsum[i] += w.sum(); wmax[i] = max(wmax[i], w.max()); hits[i] += int(take.sum())
            if (walk & bad).any():
                excl[i] = True
            T = np.where(take, T * (1.0 - a), T)
    return wsum, wmax, hits, excl


def oracle_records(mean2d, conic_opacity):
    """the record layout importance() reads, from the CPU oracle's own forward state (oracle.get("mean2d"), get("conic_opacity")): one
    [n,16] row per splat with the pixel centre at S2D_X / S2D_Y, the conic's (a, b, c) at S2D_CONIC .. + 2 and the opacity the composite
    multiplies exp(power) by at S2D_OPACITY -> float64 [n,16]; the list values of a single oracle view index these rows (view = 0)"""
    n = mean2d.shape[0]
    rec = np.zeros((n, 16))
    rec[:, S2D_X], rec[:, S2D_Y] = mean2d[:, 0], mean2d[:, 1]
    rec[:, S2D_CONIC:S2D_CONIC + 3] = conic_opacity[:, :3]
    rec[:, S2D_OPACITY] = conic_opacity[:, 3]
    return rec
