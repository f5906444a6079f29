"""tests/lod_ref.py as it stood before merge() recorded its branch census and took a `defect`, kept verbatim below this paragraph and never
edited: tests/test_lod_ref.py holds lod_ref.merge() to it byte for byte. (A digest of the outputs cannot do that: numpy's exp and log
differ in the last place between CPUs, so the bytes are only comparable within one process.)

numpy restatement of the level-of-detail merge (include/dvs_export.h, last section; csrc/lod.hip).

merge(params, origin, cell, dims, D, dtype): dtype float64 is the yardstick; float32 restates the device's arithmetic operation by
operation, in its order (the device's exp and log differ from numpy's by a few ulp, and nothing else). The cell of a splat and the
test for non-finite values are taken on the float32 inputs in both, so both see the same clusters.

The definition. Lattice: origin o[3], cell edge c > 0, dims[3] (1..1024 each).
  cell      per axis q = (p - o) / c in float32 (one subtraction, one division); 0 when !(q >= 0), dims - 1 when q >= dims, else int(q);
            key = (iz dims_y + iy) dims_x + ix
  dropped   a splat whose centre, opacity, scale or rotation holds a non-finite value
  weight    w = sigmoid(opacity) * exp(((s0 + s1) + s2) * (2/3))  =  alpha (sigma0 sigma1 sigma2)^(2/3)
  cluster   the surviving splats of one cell in ascending splat index; every sum is the serial sum in that order, from 0
  1 member  the six rows copied bit for bit
  else      W = sum w; !(W > 0): dropped with its members. mu = (sum w p) / W; then, second pass,
            Sigma' = (sum w (Sigma_i + (p - mu)(p - mu)^T)) / W, Sigma_i from the unit quaternion; sh0 and the shN elements of the bands
            <= D: (sum w c) / W, the bands above D: 0; cyclic Jacobi, at most SWEEPS sweeps; eigenvalues floored at 1e-7 of the largest;
            scale' = log(lambda) / 2; rot' = the unit quaternion, w >= 0, of the eigenvectors made a proper rotation;
            alpha' = min(0.99, W / (lambda0 lambda1 lambda2)^(1/3)), stored as its logit
  output    clusters in ascending key
"""
import numpy as np

SWEEPS = 12
LIMIT = (0, 9, 24, 45)          # shN elements of the bands <= D
KEYS = ("pos", "sh0", "shN", "opacity", "scale", "rot")


def cell_keys(pos, origin, cell, dims):
    """float32 [n,3] -> int64 [n], the rule of dec_axis per axis"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32)
    c = np.float32(cell)
    idx = []
    with np.errstate(all="ignore"):
        for a in range(3):
            q = (pos[:, a] - o[a]) / c
            i = np.zeros(len(pos), np.int64)
            inside = q >= 0                                  # (False for NaN)
            high = inside & (q >= np.float32(dims[a]))
            low = inside & ~high
            i[high] = dims[a] - 1
            i[low] = q[low].astype(np.int64)
            idx.append(i)
    return (idx[2] * int(dims[1]) + idx[1]) * int(dims[0]) + idx[0]


def finite_rows(p):
    """bool [n]: centre, opacity, scale and rotation hold finite values only"""
    ok = np.isfinite(np.asarray(p["pos"]).reshape(-1, 3)).all(1) & np.isfinite(np.asarray(p["opacity"]).reshape(-1))
    return ok & np.isfinite(np.asarray(p["scale"]).reshape(-1, 3)).all(1) & np.isfinite(np.asarray(p["rot"]).reshape(-1, 4)).all(1)


def unit_quat(rot, dt):
    """dvs_unit_quat: [n,4] (w, x, y, z) -> unit, (1, 0, 0, 0) for a squared norm of 0 or not finite"""
    r = np.asarray(rot, dt).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ss = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3]
        good = (ss > 0) & (ss < np.inf)
        q = r / np.sqrt(np.where(good, ss, dt(1)))[:, None]
    q[~good] = np.array([1, 0, 0, 0], dt)
    return q


def covariances(scale, rot, dt):
    """[n,6] = (xx, xy, xz, yy, yz, zz) of R diag(exp(scale)^2) R^T: dvs_quat_to_rot and dvs_cov3d in their order"""
    q = unit_quat(rot, dt)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two, one = dt(2), dt(1)
    R = [one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
         two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
         two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]
    with np.errstate(all="ignore"):
        s = np.exp(np.asarray(scale, dt).reshape(-1, 3))
        M = [R[3 * i + k] * s[:, k] for i in range(3) for k in range(3)]
        cov = [(M[0] * M[0] + M[1] * M[1]) + M[2] * M[2], (M[0] * M[3] + M[1] * M[4]) + M[2] * M[5], (M[0] * M[6] + M[1] * M[7]) + M[2] * M[8],
               (M[3] * M[3] + M[4] * M[4]) + M[5] * M[5], (M[3] * M[6] + M[4] * M[7]) + M[5] * M[8], (M[6] * M[6] + M[7] * M[7]) + M[8] * M[8]]
    return np.stack(cov, 1).astype(dt)


def weights(opacity, scale, dt):
    o = np.asarray(opacity, dt).reshape(-1)
    s = np.asarray(scale, dt).reshape(-1, 3)
    with np.errstate(all="ignore"):
        alpha = dt(1) / (dt(1) + np.exp(-o))
        return (alpha * np.exp(((s[:, 0] + s[:, 1]) + s[:, 2]) * dt(2.0 / 3.0))).astype(dt)


def sym3(c6):
    return np.array([[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]], c6.dtype)


def jacobi(A, dt):
    """cyclic Jacobi sweeps (0,1), (0,2), (1,2) -> (diagonal [3], V [3,3] with A = V diag V^T)"""
    A = np.array(A, dt)
    V = np.eye(3, dtype=dt)
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            if A[0, 1] == 0 and A[0, 2] == 0 and A[1, 2] == 0:
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[p, q]
                if apq == 0:
                    continue
                r = 3 - p - q
                theta = (A[q, q] - A[p, p]) / (two * apq)
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                A[p, p] = A[p, p] - t * apq
                A[q, q] = A[q, q] + t * apq
                A[p, q] = A[q, p] = 0
                arp, arq = A[r, p], A[r, q]
                A[r, p] = A[p, r] = c * arp - s * arq
                A[r, q] = A[q, r] = s * arp + c * arq
                for k in range(3):
                    vp, vq = V[k, p], V[k, q]
                    V[k, p] = c * vp - s * vq
                    V[k, q] = s * vp + c * vq
    return np.array([A[0, 0], A[1, 1], A[2, 2]], dt), V


def quat_of_rotation(V, dt):
    """the branch of the largest of trace, V00, V11, V22 (the first of equal ones), unit, w >= 0"""
    one, two, quarter = dt(1), dt(2), dt(0.25)
    tr = (V[0, 0] + V[1, 1]) + V[2, 2]
    if tr >= V[0, 0] and tr >= V[1, 1] and tr >= V[2, 2]:
        S = np.sqrt(tr + one) * two
        q = [quarter * S, (V[2, 1] - V[1, 2]) / S, (V[0, 2] - V[2, 0]) / S, (V[1, 0] - V[0, 1]) / S]
    elif V[0, 0] >= V[1, 1] and V[0, 0] >= V[2, 2]:
        S = np.sqrt(((one + V[0, 0]) - V[1, 1]) - V[2, 2]) * two
        q = [(V[2, 1] - V[1, 2]) / S, quarter * S, (V[0, 1] + V[1, 0]) / S, (V[0, 2] + V[2, 0]) / S]
    elif V[1, 1] >= V[2, 2]:
        S = np.sqrt(((one + V[1, 1]) - V[0, 0]) - V[2, 2]) * two
        q = [(V[0, 2] - V[2, 0]) / S, (V[0, 1] + V[1, 0]) / S, quarter * S, (V[1, 2] + V[2, 1]) / S]
    else:
        S = np.sqrt(((one + V[2, 2]) - V[0, 0]) - V[1, 1]) * two
        q = [(V[1, 0] - V[0, 1]) / S, (V[0, 2] + V[2, 0]) / S, (V[1, 2] + V[2, 1]) / S, quarter * S]
    q = np.array(q, dt)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return -q if q[0] < 0 else q


def merge(params, origin, cell, dims, D, dtype=np.float64):
    """params: float32 arrays pos [n,3], sh0 [n,3], shN [n,45], opacity [n], scale [n,3], rot [n,4].
    -> (out, info): out = the six arrays of m rows in `dtype` (rows of single-member clusters hold the float32 inputs exactly);
    info = {"m", "n_dropped", "keys" [m], "single" bool [m], "members" list of index arrays, "cov" [m,6] = Sigma' before the
    decomposition (NaN rows for single members), "W" [m]}"""
    dt = np.dtype(dtype).type
    p32 = {k: np.asarray(params[k], np.float32) for k in KEYS}
    p32 = {"pos": p32["pos"].reshape(-1, 3), "sh0": p32["sh0"].reshape(-1, 3), "shN": p32["shN"].reshape(-1, 45), "opacity": p32["opacity"].reshape(-1),
           "scale": p32["scale"].reshape(-1, 3), "rot": p32["rot"].reshape(-1, 4)}
    n = len(p32["opacity"])
    ok = finite_rows(p32)
    n_dropped = int((~ok).sum())
    keys = cell_keys(p32["pos"], origin, cell, dims)
    alive = np.nonzero(ok)[0]
    order = alive[np.argsort(keys[alive], kind="stable")]                    # by (key, splat index)
    skeys = keys[order]
    starts = np.nonzero(np.r_[True, skeys[1:] != skeys[:-1]])[0] if len(order) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(order)] if len(order) else starts
    P = {k: v.astype(dt) for k, v in p32.items()}
    w_all = weights(p32["opacity"], p32["scale"], dt)
    cov_all = np.zeros((n, 6), dt)
    cov_all[ok] = covariances(p32["scale"][ok], p32["rot"][ok], dt)
    rows = {k: [] for k in KEYS}
    info = {"keys": [], "single": [], "members": [], "cov": [], "W": []}
    zero = dt(0)
    with np.errstate(all="ignore"):
        for a, b in zip(starts, ends):
            mem = order[a:b]
            if len(mem) == 1:
                v = mem[0]
                for k in KEYS:
                    rows[k].append(P[k][v])
                info["cov"].append(np.full(6, np.nan, dt)); info["W"].append(w_all[v])
            else:
                W = zero
                s = np.zeros(3, dt)
                for v in mem:
                    W = W + w_all[v]
                    s = s + w_all[v] * P["pos"][v]
                if not W > 0:
                    n_dropped += len(mem)
                    continue
                mu = s / W
                c6 = np.zeros(6, dt)
                a0, aN = np.zeros(3, dt), np.zeros(45, dt)
                for v in mem:
                    d = P["pos"][v] - mu
                    dd = np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], dt)
                    c6 = c6 + w_all[v] * (cov_all[v] + dd)
                    a0 = a0 + w_all[v] * P["sh0"][v]
                    aN = aN + w_all[v] * P["shN"][v]
                c6 = c6 / W
                lam, V = jacobi(sym3(c6), dt)
                lmax = max(max(lam[0], lam[1]), lam[2])
                lam = np.maximum(lam, dt(np.float32(1e-7)) * lmax)
                l = np.log(lam)
                det = (V[0, 0] * (V[1, 1] * V[2, 2] - V[1, 2] * V[2, 1]) - V[0, 1] * (V[1, 0] * V[2, 2] - V[1, 2] * V[2, 0])) + \
                    V[0, 2] * (V[1, 0] * V[2, 1] - V[1, 1] * V[2, 0])
                if det < 0:
                    V[:, 2] = -V[:, 2]
                gm = np.exp(((l[0] + l[1]) + l[2]) / dt(3))
                alpha = min(dt(np.float32(0.99)), W / gm)
                shN = aN / W
                shN[LIMIT[D]:] = 0
                rows["pos"].append(mu); rows["sh0"].append(a0 / W); rows["shN"].append(shN)
                rows["opacity"].append(np.log(alpha / (dt(1) - alpha)))
                rows["scale"].append(dt(0.5) * l); rows["rot"].append(quat_of_rotation(V, dt))
                info["cov"].append(c6); info["W"].append(W)
            info["keys"].append(int(skeys[a])); info["single"].append(len(mem) == 1); info["members"].append(mem)
    m = len(info["keys"])
    width = {"pos": 3, "sh0": 3, "shN": 45, "opacity": 0, "scale": 3, "rot": 4}
    out = {k: (np.array(rows[k], dt).reshape((m, width[k]) if width[k] else (m,))) for k in KEYS}
    info = {"m": m, "n_dropped": n_dropped, "keys": np.array(info["keys"], np.int64), "single": np.array(info["single"], bool),
            "members": info["members"], "cov": np.array(info["cov"], dt).reshape(m, 6), "W": np.array(info["W"], dt)}
    return out, info


def written_covariances(scale, rot):
    """float64 [m,6] of R diag(e^{2 scale}) R^T for written rows: what a reader of the file reconstructs"""
    return covariances(np.asarray(scale, np.float64), np.asarray(rot, np.float64), np.float64)


def lattice_for(bounds, resolution):
    """dvs_lod_lattice_for: -> (origin float32 [3], cell float32, dims [3]) or None when it is refused"""
    b = np.asarray(bounds, np.float32).reshape(6)
    if not (4 <= resolution <= 1024) or not np.isfinite(b).all() or (b[3:] < b[:3]).any():
        return None
    side = b[3:].astype(np.float64) - b[:3].astype(np.float64)
    cell = np.float32(side.max() * (1.0 + 1e-5) / resolution)
    if not (cell > 0 and np.isfinite(cell)):
        return None
    dims = [int(min(1024.0, max(1.0, np.ceil(s / float(cell))))) for s in side]
    return b[:3].copy(), cell, dims
