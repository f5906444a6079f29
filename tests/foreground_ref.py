"""fp64 restatement of dvs_raster_foreground_views (include/dvs_raster.h) and the rule of dvs_foreground_plan (include/dvs_train.h) in
Python integers. The votes are two calls of importance_ref.importance: one under the mask fg x valid, one under (1 - fg) x valid — a
pixel walks its list or not, and each pixel's walk is independent of every other's, so splitting the pixels splits the sums."""
import numpy as np
import importance_ref as IR

KEEP, PRUNE = 0, 3          # DVS_DENSIFY_KEEP, DVS_DENSIFY_PRUNE


def votes(splat2d, ranges, sorted_splat, n_contrib, W, H, n, view, fg=None, valid=None):
    """fg, valid: None or [H,W]; a pixel is foreground where fg is nonzero (everywhere without fg) and walks only where valid is nonzero
    -> (fg sum [n] of w, bg sum [n] of w, fg hits [n], bg hits [n], excluded [n]: the union of the two calls' exclusions)"""
    f = np.ones((H, W)) if fg is None else (np.asarray(fg) != 0).astype(np.float64)
    v = np.ones((H, W)) if valid is None else (np.asarray(valid) != 0).astype(np.float64)
    a = IR.importance(splat2d, ranges, sorted_splat, n_contrib, W, H, n, view, mask=f * v)
    b = IR.importance(splat2d, ranges, sorted_splat, n_contrib, W, H, n, view, mask=(1.0 - f) * v)
    return a[0], b[0], a[2], b[2], a[3] | b[3]


def keeps(fg, bg, percent):
    """the rule on Python integers (no wrap at any size)"""
    fg, bg, percent = int(fg), int(bg), int(percent)
    return fg > 0 and fg * (100 - percent) >= bg * percent


def plan(fg, bg, percent):
    """fg, bg: sequences of unsigned 64-bit values -> (action uint8 [n], offsets uint32 [n], new_count)"""
    assert 1 <= int(percent) <= 100
    kept = np.array([keeps(f, b, percent) for f, b in zip(fg, bg)], bool)
    action = np.where(kept, KEEP, PRUNE).astype(np.uint8)
    offsets = (np.cumsum(kept) - kept).astype(np.uint32)
    return action, offsets, int(kept.sum())
