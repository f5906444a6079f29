"""numpy restatement of dvs_knn_mean_dist2 (include/dvs_init.h): chunked all-pairs in float32, every operation rounded to float32 in the
order of the definition: d2(i, j) = ((dx dx + dy dy) + dz dz), dx = pos[j].x - pos[i].x; the m = min(3, n - 1) smallest over j != i in
ascending order; ((d0 + d1) + d2) / 3, (d0 + d1) / 2, d0 or 0. Also the inputs of tests/test_gpu_knn.py."""
import numpy as np

f32 = np.float32


def mean_dist2(pos, chunk=64):
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    out = np.zeros(n, f32)
    m = min(3, n - 1)
    if m <= 0:
        return out
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    for a in range(0, n, chunk):
        p = pos[a:a + chunk]
        d = x[None, :] - p[:, None, 0]                                      # dx, then dx dx (each operation rounds to float32 once)
        np.multiply(d, d, out=d)
        t = y[None, :] - p[:, None, 1]
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)                                                 # dx dx + dy dy
        np.subtract(z[None, :], p[:, None, 2], out=t)
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)                                                 # (dx dx + dy dy) + dz dz
        assert d.dtype == f32
        d[np.arange(len(p)), np.arange(a, a + len(p))] = np.inf           # j != i, by index: a duplicate stays a neighbour at 0
        rows = np.arange(len(p))
        best = np.empty((len(p), m), f32)
        for k in range(m):                                                  # the m smallest, ascending: m passes of argmin
            j = d.argmin(axis=1)
            best[:, k] = d[rows, j]
            d[rows, j] = np.inf
        if m == 3:
            out[a:a + chunk] = ((best[:, 0] + best[:, 1]) + best[:, 2]) / f32(3.0)
        elif m == 2:
            out[a:a + chunk] = (best[:, 0] + best[:, 1]) / f32(2.0)
        else:
            out[a:a + chunk] = best[:, 0]
    return out


def uniform(n, seed):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (n, 3)).astype(f32)


def clusters(n, seed, k=20):
    """k tight clusters far apart: whole boxes lie beyond a point's third-best distance, pruning decides"""
    r = np.random.default_rng(seed)
    centres = r.uniform(-500.0, 500.0, (k, 3))
    return (centres[r.integers(0, k, n)] + r.normal(0.0, 0.01, (n, 3))).astype(f32)


def line(n, seed):
    """all points on one line along x: zero extent on two Morton axes"""
    p = np.zeros((n, 3), f32)
    p[:, 0] = np.random.default_rng(seed).uniform(0.0, 100.0, n).astype(f32)
    p[:, 1] = f32(1.25)
    p[:, 2] = f32(-7.5)
    return p


def lattice(seed, side=27, dup=317):
    """a side^3 lattice plus exact duplicates: mass ties and zero distances"""
    g = np.arange(side, dtype=f32) * f32(0.5)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    r = np.random.default_rng(seed)
    p = np.concatenate([p, p[r.integers(0, len(p), dup)]])
    return np.ascontiguousarray(p[r.permutation(len(p))], f32)
