"""fp64 numpy restatement of the ADC densifier's rule (include/dvs_train.h, dvs_densify_plan / dvs_densify_apply) — TEST INFRASTRUCTURE.

  actions          the per-splat decision with all three prune rules, the cap, the offsets and the new count, and for every splat the
                   relative distance of its inputs to the nearest threshold that could change its decision (`margin`)
  capped           the cap alone, on a given action array (what tests/test_gpu_train_ops_scale.py::test_densify_cap_max restates)
  split_moments    mean and covariance R diag(exp(2 s)) R^T of the Gaussian a SPLIT draws its two children from
  revised_opacity  the logit both results of a clone / split take with `revisedOpacity`
  plan_scene       the inputs of tests/test_gpu_densify_rules.py: every action, every prune cause alone and together with the growth
                   conditions, the integer radius at and one past its limit, never-seen splats; no splat nearer than MARGIN to a threshold

Nothing here looks at what a kernel computes."""
import numpy as np

KEEP, CLONE, SPLIT, PRUNE = 0, 1, 2, 3
MARGIN = 1e-3                     # __expf sigmoid / exp are good to ~1e-6 relative: at this distance the restatement alone decides
LOG_1P6 = float(np.log(1.6))
PRM_FIELDS = ("grad_threshold", "scale_threshold", "min_opacity", "max_world_scale", "max_screen_radius", "cap_max")


def params(prm):
    """the six fields of a dvs_densify_params the plan reads, as python numbers, from a ctypes struct (the float32 values the kernel
    receives) or a dict"""
    get = prm.get if isinstance(prm, dict) else lambda k, d=0: getattr(prm, k, d)
    p = {k: get(k, 0) for k in PRM_FIELDS}
    return {k: (int(v) if k in ("max_screen_radius", "cap_max") else float(v)) for k, v in p.items()}


def excl_cumsum(c):
    return np.concatenate([[0], np.cumsum(c, dtype=np.int64)[:-1]]) if len(c) else np.zeros(0, np.int64)


def capped(act0, cap):
    """the documented cap: the first max(0, cap - S) growth candidates in splat order keep CLONE / SPLIT, the rest become KEEP
    -> (action, S, number of candidates)"""
    S = int((act0 != PRUNE).sum())
    grow = np.nonzero((act0 == CLONE) | (act0 == SPLIT))[0]
    budget = len(grow) if cap <= 0 else min(len(grow), max(cap - S, 0))
    want = act0.copy()
    want[grow[budget:]] = KEEP
    return want, S, len(grow)


def _rel(x, thr):
    return np.abs(x - thr) / thr


def actions(opacity, scale, grad_accum, denom, max_radii, prm):
    """-> (action [n], cap-demoted action [n], offsets [n], new_count, margin [n]).

    PRUNE   opacity or a scale not finite; sigmoid(opacity) < min_opacity; max exp(scale) > max_world_scale (if > 0);
            max_radii > max_screen_radius (if > 0) — all before any growth decision
    SPLIT   avg = grad_accum / denom (0 where denom == 0) >= grad_threshold and max exp(scale) > scale_threshold
    CLONE   avg >= grad_threshold otherwise;   KEEP the rest
    offsets = exclusive scan of the output counts (0 / 1 / 2 / 2) of the cap-demoted actions, new_count their sum.

    margin: the relative distance |x - t| / t of the splat's quantities to the nearest threshold whose crossing would change the
    decision. A pruned splat changes only when EVERY prune cause that fires stops firing: the farthest of them counts. A splat that is
    not pruned changes when any prune rule starts to fire, when avg crosses grad_threshold or, if it grows, when the scale crosses
    scale_threshold. The radius comparison is between integers and cannot be misjudged: it contributes inf, except at max_radii ==
    max_screen_radius exactly, where the decision hangs on `>` against `>=` and one pixel, 1 / max_screen_radius, is the distance.
    Non-finite splats have margin inf."""
    p = params(prm)
    o = np.asarray(opacity, np.float64).reshape(-1)
    s = np.asarray(scale, np.float64).reshape(-1, 3)
    ga, de = np.asarray(grad_accum, np.float64).reshape(-1), np.asarray(denom, np.float64).reshape(-1)
    mr = np.asarray(max_radii).astype(np.int64).reshape(-1)
    n = o.size
    bad = ~(np.isfinite(o) & np.isfinite(s).all(1))
    with np.errstate(all="ignore"):
        op = 1.0 / (1.0 + np.exp(-np.where(bad, 0.0, o)))
        smax = np.exp(np.where(bad[:, None], 0.0, s).max(1)) if n else np.zeros(0)
        avg = np.where(de > 0, ga / np.where(de > 0, de, 1.0), 0.0)
    inf = np.full(n, np.inf)
    c_op = op < p["min_opacity"]
    m_op = _rel(op, p["min_opacity"])
    ws_on, r_on = p["max_world_scale"] > 0, p["max_screen_radius"] > 0
    c_ws = (smax > p["max_world_scale"]) if ws_on else np.zeros(n, bool)
    m_ws = _rel(smax, p["max_world_scale"]) if ws_on else inf
    c_r = (mr > p["max_screen_radius"]) if r_on else np.zeros(n, bool)
    m_r = np.where(mr == p["max_screen_radius"], 1.0 / p["max_screen_radius"], np.inf) if r_on else inf
    pruned = c_op | c_ws | c_r
    with np.errstate(invalid="ignore"):
        grows = avg >= p["grad_threshold"]                  # (a NaN statistic does not grow, as !(avg >= t) in the kernel)
    big = smax > p["scale_threshold"]
    act = np.where(bad | pruned, PRUNE, np.where(grows, np.where(big, SPLIT, CLONE), KEEP)).astype(np.uint8)
    m_pruned = np.maximum.reduce([np.where(c_op, m_op, 0.0), np.where(c_ws, m_ws, 0.0), np.where(c_r, m_r, 0.0)])
    m_alive = np.minimum.reduce([m_op, m_ws, m_r, _rel(avg, p["grad_threshold"]), np.where(grows, _rel(smax, p["scale_threshold"]), np.inf)])
    margin = np.where(bad, np.inf, np.where(pruned, m_pruned, m_alive))
    act_cap, _, _ = capped(act, p["cap_max"])
    cnt = np.where(act_cap == PRUNE, 0, np.where(act_cap == KEEP, 1, 2))
    return act, act_cap, excl_cumsum(cnt), int(cnt.sum()), margin


def actions_literal(opacity, scale, grad_accum, denom, max_radii, prm):
    """the same rule and cap as one loop over the splats, written from the header's sentences — what `actions` is checked against
    -> (cap-demoted action, offsets, new_count)"""
    p = params(prm)
    n = len(opacity)
    act = []
    for i in range(n):
        o, s = float(opacity[i]), [float(x) for x in np.asarray(scale).reshape(-1, 3)[i]]
        if not all(np.isfinite(x) for x in [o] + s):
            act.append(PRUNE); continue
        op, smax = 1.0 / (1.0 + np.exp(-o)), np.exp(max(s))
        if op < p["min_opacity"] or (p["max_world_scale"] > 0 and smax > p["max_world_scale"]) \
                or (p["max_screen_radius"] > 0 and int(max_radii[i]) > p["max_screen_radius"]):
            act.append(PRUNE); continue
        avg = float(grad_accum[i]) / float(denom[i]) if denom[i] > 0 else 0.0
        act.append((SPLIT if smax > p["scale_threshold"] else CLONE) if avg >= p["grad_threshold"] else KEEP)
    S = sum(a != PRUNE for a in act)
    left = max(0, p["cap_max"] - S) if p["cap_max"] > 0 else n
    offs, o = [], 0
    for i in range(n):
        if act[i] in (CLONE, SPLIT):
            if left > 0:
                left -= 1
            else:
                act[i] = KEEP
        offs.append(o)
        o += {KEEP: 1, CLONE: 2, SPLIT: 2, PRUNE: 0}[act[i]]
    return np.array(act, np.uint8), np.array(offs, np.int64), o


def quat_to_rot(q):
    """R of the (w, x, y, z) quaternion q [4], normalised first, entry by entry as dvs_quat_to_rot lays it out (row-major R[r][c]);
    the zero quaternion gives the identity, as k_densify_apply's 1 / |q| = 0 does"""
    q = np.asarray(q, np.float64)
    nq = np.sqrt((q * q).sum())
    w, x, y, z = q / nq if nq > 0 else np.zeros(4)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def split_moments(pos, scale, rot):
    """-> (mean [3], Sigma [3, 3]) of pos + R diag(exp s) z, z ~ N(0, I): Sigma = R diag(exp(2 s)) R^T, the covariance dvs_cov3d renders"""
    R = quat_to_rot(rot)
    return np.asarray(pos, np.float64).copy(), R @ np.diag(np.exp(2.0 * np.asarray(scale, np.float64))) @ R.T


def revised_opacity(logit):
    """logit of o' = clip(1 - sqrt(1 - o), 1e-6, 1 - 1e-6), o = sigmoid(logit): the pair composites to o, 1 - (1 - o')^2 = o"""
    o = 1.0 / (1.0 + np.exp(-np.asarray(logit, np.float64)))
    no = np.clip(1.0 - np.sqrt(1.0 - o), 1e-6, 1.0 - 1e-6)
    return np.log(no / (1.0 - no))


# ---- inputs of the plan tests ----------------------------------------------------------------------------------------------------------
_f32 = lambda x: float(np.float32(x))                  # the thresholds as the kernel receives them
PLAN_PRM = dict(grad_threshold=_f32(2e-4), scale_threshold=_f32(0.05), min_opacity=_f32(0.005), max_world_scale=_f32(0.5), max_screen_radius=30)
# constructed splats, at i % 32 == key: (logit, three scales, avg, denom, max_radii)
_BIG, _MID, _SMALL, _HUGE = np.log(0.2), np.log(0.03), np.log(0.01), np.log(0.8)
CONSTRUCTED = {
    3: ("opacity prune over a SPLIT", -9.0, (_BIG, _SMALL, _SMALL), 1e-3, 2, 5),
    5: ("opacity prune over a CLONE", -9.0, (_MID, _SMALL, _SMALL), 1e-3, 1, 5),
    7: ("world-scale prune over a SPLIT", 2.0, (_SMALL, _HUGE, _SMALL), 1e-3, 3, 5),
    11: ("radius prune over a SPLIT", 2.0, (_BIG, _BIG, _SMALL), 1e-3, 2, 31),
    12: ("radius prune over a CLONE", 2.0, (_MID, _MID, _SMALL), 1e-3, 2, 31),
    13: ("radius at the limit: kept", 2.0, (_MID, _SMALL, _SMALL), 0.0, 4, 30),
    14: ("radius at the limit: SPLIT", 2.0, (_SMALL, _SMALL, _BIG), 1e-3, 4, 30),
    17: ("radius one past the limit alone", 2.0, (_MID, _SMALL, _SMALL), 1e-5, 4, 31),
    19: ("opacity alone", -9.0, (_SMALL, _SMALL, _SMALL), 1e-5, 2, 3),
    23: ("world scale alone", 2.0, (_HUGE, _SMALL, _SMALL), 0.0, 2, 3),
    29: ("never seen: kept", 2.0, (_SMALL, _SMALL, _SMALL), 0.0, 0, 0),
    30: ("never seen, middling scale: kept", 0.5, (_MID, _SMALL, _MID), 0.0, 0, 0),
}
CONSTRUCTED_WANT = {3: PRUNE, 5: PRUNE, 7: PRUNE, 11: PRUNE, 12: PRUNE, 13: KEEP, 14: SPLIT, 17: PRUNE, 19: PRUNE, 23: PRUNE, 29: KEEP, 30: KEEP}


def _draw(rng, n):
    de = rng.integers(0, 6, n).astype(np.float32)
    avg = np.abs(rng.normal(0, 2.5e-4, n))
    mr = np.where(de > 0, rng.integers(1, 41, n), 0).astype(np.int32)       # a splat that was never visible has no radius
    return (rng.normal(0, 3, n).astype(np.float32), rng.normal(-3, 1, (n, 3)).astype(np.float32), (avg * de).astype(np.float32), de, mr)


def plan_scene(n, seed):
    """-> (A, grad_accum, denom, max_radii): splat arrays (rot[:, 3] = the splat id, copied verbatim by every action) and interval
    statistics for PLAN_PRM. Random draws (opacity logit N(0, 3), log-scales N(-3, 1), avg |N(0, 2.5e-4)|, radii 1 .. 40) with the
    CONSTRUCTED splats at i % 32 and a run of dead splats over the first block boundary; every random splat whose margin under
    PLAN_PRM, or under the same rule with both limits off, is below MARGIN is drawn again."""
    rng = np.random.default_rng(seed)
    A = {"pos": rng.normal(size=(n, 3)), "sh0": rng.normal(size=(n, 3)), "shN": rng.normal(size=(n, 15, 3)), "rot": rng.normal(size=(n, 4))}
    A = {k: v.astype(np.float32) for k, v in A.items()}
    A["rot"][:, 3] = np.arange(n, dtype=np.float32)                          # exact below 2^24
    op, sc, ga, de, mr = _draw(rng, n)
    op[200:300] = -9.0
    fixed = np.zeros(n, bool)
    for k, (_, o, s, avg, d, r) in CONSTRUCTED.items():
        idx = np.arange(k, n, 32)
        op[idx], sc[idx], de[idx], mr[idx] = o, np.array(s, np.float32), d, r
        ga[idx] = np.float32(avg * d)
        fixed[idx] = True
    off = dict(PLAN_PRM, max_world_scale=0.0, max_screen_radius=0)
    for _ in range(64):
        near = np.minimum(actions(op, sc, ga, de, mr, PLAN_PRM)[4], actions(op, sc, ga, de, mr, off)[4]) < MARGIN
        if not near.any():
            break
        assert not (near & fixed).any()
        idx = np.nonzero(near)[0]
        o2, s2, g2, d2, r2 = _draw(rng, idx.size)
        op[idx], sc[idx], ga[idx], de[idx], mr[idx] = o2, s2, g2, d2, r2     # (the dead run is 97 % from its threshold: never drawn again)
    A["opacity"], A["scale"] = op, sc
    return A, ga, de, mr
