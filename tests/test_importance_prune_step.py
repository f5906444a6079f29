"""The importance prune at step level: WHICH splats `gaussian_train --importancePrune 30` removes at a prune occasion, and what state it
leaves for the next Adam step. tests/test_gpu_importance.py pins the score kernel, tests/test_gpu_importance_plan.py the selection, and
tests/test_gpu_importance_train.py only how many splats go; this file pins how GaussianTrainerScene::Impl::prune_importance
(gstrain/trainer_refine.cpp) wires them: which cameras are scored (the training ones, every pass of them, each with its own mask), from
which state (after the step's Adam update and after the light prune has compacted the arrays), with which options (the model's full SH
degree, the run's anti-alias setting), that the WORST go, and that parameters and both Adam moments travel together. The structure is
that of tests/test_train_step_options.py, whose helpers and bars (RTOL 1e-4 with floor 1e-2, update bar 1e-2, SHARE_L1 0.90, decision
margin 5 % with a firm share of at least 0.9) are imported, not restated:

CPU part (not marked gpu), per GPU case: the share of decisions with a 5 % margin (float32 and float64 restatement agree on them), the
pinned share of the survivors, and discrimination — every wiring mistake listed below decides differently from the rule on at least 1 %
of the splats, and at least 10, whose decision is firm under the rule AND under the mistake (so that a product making the mistake
would certainly fail the GPU test).
GPU part: `gaussian_train` resumed from a model written here (--load_itr 0), `--densifyStrategy 0 --refineStopIter 1 --pruneStrategy 1
--pruneEvery K --importancePrune 30`, the survivors decoded from the saved model.

The scenes. The light prune does not leave `_start_model` alone at 96x64, small as these runs must be: the synthetic scene's splats
are 1.5 pixels wide whatever the image size, so at this focal length nearly all of them exceed pruneScale3d x extent = 0.055 (the
reason for `_prune_start_model`'s compression), and some 0.5 % start below the 0.005 opacity threshold. Splats that large also make
the exclusion rule of tests/importance_ref.py (one pixel within 1e-5 of a threshold excludes every splat behind it) take 0 .. 36 % of
the model depending on the seed (12 seeds at 1500 splats: firm share 0.63 .. 0.95, below 0.9 for 7 of them) — a firm share the GPU
test, whose trajectory comes from other targets, could not rely on. So every case starts from `_start_model` with
`_prune_start_model`'s compression of the log-scales (largest 0.045, 18 % under the light prune's limit) and, where the light prune is
to take nothing, the opacity logits floored at -3.5 (0.029; logit(0.005) is -5.3, and the twins assert the light prune's margin at the
prune step): lists of a few entries per pixel, firm share 0.95 .. 0.985 over six seeds."""
import copy
import re
import numpy as np
import pytest
from oracle.oracle import Oracle
from train_step_ref import TrainStepRef, KEYS, importance_decisions
from test_train_step import _scene, _hip_targets, _decode_actions
from test_train_step_options import (RTOL, SHARE_L1, _flags, _start_model, _prune_start_model, _oracle_targets, _pair, _r64, _pinned,
                                     _median_difference, _product, _bars, _dump)

PERCENT = 30
FIRM = 0.05                                    # decision margin, FIRM_SHARE of the splats must have it (tests/test_train_step_options.py: the light prune)
FIRM_SHARE = 0.9
# scene and step count of each GPU case, chosen on the CPU (the test_*_case_* tests below measure them)
CASES = {
    "plain": dict(n=1500, W=96, H=64, cams=4, sh=1, seed=52, K=24, more=2),
    "composed": dict(n=2000, W=96, H=64, cams=7, sh=1, seed=58, K=8, holdout=3, eval_views=3),
    "order": dict(n=1000, W=96, H=64, cams=4, sh=1, seed=54, K=4, culled=0.4),
}


def _case(name):
    c = CASES[name]
    spec, cams = _scene(c["n"], c["W"], c["H"], c["cams"], c["sh"], c["seed"])
    return c, spec, cams


def _kept(n):
    return n - n * PERCENT // 100               # prune_importance: new_n = n - n P / 100


def _plain_start_model(spec, seed):
    """`_start_model` with the log-scales compressed as `_prune_start_model` compresses them (x 0.35 towards the largest, which becomes
    0.045) and the opacity logits floored at -3.5: the light prune takes nothing (the module docstring says why neither holds for
    `_start_model` itself at this image size)"""
    A = _start_model(spec, seed)
    A["scale"] = (np.log(0.045) + 0.35 * (A["scale"] - A["scale"].max())).astype(np.float32)
    A["opacity"] = np.maximum(A["opacity"], np.float32(-3.5))
    return A


def _order_start_model(spec, seed, culled):
    """case D: `_plain_start_model` whose last `culled` share of rows is mirrored behind the cameras (z -> -z: every camera of the rig
    sits in the plane z = 0 and looks towards +z) — ordinary opacity, scale, colour and rotation, listed by no camera"""
    A = _plain_start_model(spec, seed)
    first = spec.n - int(spec.n * culled)
    A["pos"][first:, 2] = -A["pos"][first:, 2]
    return A, first


def _splits(c):
    """(training cameras, test cameras) of --evalHoldout h: camera i is held out iff i % h == 0 (gstrain/trainer_load.cpp setup_split)"""
    h = c.get("holdout", 0)
    cams = list(range(c["cams"]))
    return ([i for i in cams if i % h] if h else cams), ([i for i in cams if i % h == 0] if h else [])


def _scores_of(r, rows, cam_indices, mask=False, sh_degree=None):
    """importance_scores of the restatement's state restricted to `rows` (what the product's arrays hold after a compaction), the state
    itself left alone"""
    q = copy.copy(r)
    q.P = {k: r.P[k][rows] for k in KEYS}
    if sh_degree is not None:
        q.deg = sh_degree
    return q.importance_scores(cam_indices, mask=mask)


def _swapped(scores, keep):
    """the best removed instead of the worst: the n - keep LARGEST scores go"""
    prune = np.zeros(scores.shape[0], bool)
    prune[np.argsort(-scores, kind="stable")[:scores.shape[0] - keep]] = True
    return prune


def _differ(rule, firm, alt, alt_firm=None):
    """on how many splats a wiring mistake certainly shows: firm under the rule (the GPU test asserts there), decided otherwise by the
    mistake, and firm under the mistake too where it has a margin of its own -> (count, share of the rule's firm splats)"""
    sure = firm & (rule != alt) & (True if alt_firm is None else alt_firm)
    return int(sure.sum()), float(sure.sum() / max(1, firm.sum()))


def _assert_discriminates(found):
    for name, (count, share) in found.items():
        assert count >= 10 and share >= 0.01, (name, count, share, found)


# ---- the restated selection rule ----------------------------------------------------------------------------------------------------
def test_importance_decisions_on_explicit_scores():
    """the total order (score, then larger index first), the cut and the margins, on values small enough to check by hand"""
    s = np.array([5.0, 0.0, 2.0, 2.0, 0.0, 9.0, 2.0, 1.0])
    none = np.zeros(8, bool)
    # ascending in the order: 4 (0, larger index first), 1, 7 (1), then the three 2s from the largest index: 6, 3, 2, then 0, 5
    for keep, gone in ((8, []), (7, [4]), (6, [4, 1]), (5, [4, 1, 7]), (4, [4, 1, 7, 6]), (3, [4, 1, 7, 6, 3]), (2, [4, 1, 7, 6, 3, 2]), (1, [4, 1, 7, 6, 3, 2, 0])):
        prune, margin = importance_decisions(s, none, keep)
        assert sorted(np.flatnonzero(prune)) == sorted(gone), (keep, np.flatnonzero(prune))
        assert prune.sum() == 8 - keep
    prune, margin = importance_decisions(s, none, 4)                  # cut = 2 (the last kept is index 3): the 2s have no margin
    assert np.array_equal(margin, np.abs(s - 2.0) / 2.0) and (margin[[2, 3, 6]] == 0).all() and margin[5] == 3.5 and margin[1] == 1.0
    excl = none.copy(); excl[5] = True
    assert importance_decisions(s, excl, 4)[1][5] == 0 and np.array_equal(importance_decisions(s, excl, 4)[0], prune)
    prune, margin = importance_decisions(s, none, 7)                  # cut = 0 (the last kept is index 1): zero scores have no margin,
    assert margin[1] == 0 and margin[4] == 0 and (margin[[0, 2, 3, 5, 6, 7]] > 1e300).all()      # every other splat is infinitely far
    assert importance_decisions(s, none, 100)[0].sum() == 0


# ---- the cases on the CPU -----------------------------------------------------------------------------------------------------------
def _plain_rule(r):
    """-> (prune, firm, scores, excluded) of case A / B from the restated state at the prune step"""
    c = CASES["plain"]
    scores, excl = r.importance_scores(range(c["cams"]))
    prune, margin = importance_decisions(scores, excl, _kept(c["n"]))
    return prune, margin > FIRM, scores, excl


def test_plain_case_is_pinned_and_discriminates():
    """measured (oracle targets, 1500 splats, 96x64, 4 cameras, 24 steps): the rule removes 450; 98.2 % of the decisions have a 5 % margin
    (float32 and float64 agree on all of them), no splat is excluded, 41 splats score exactly 0; the light prune's nearest decision has
    a margin of 9.9 %. Firm under the rule and under the mistake, decided differently: camera 0 only 55 splats (3.7 %), best removed 886
    (60 %), scored from the start model 40 (2.7 % — the reason for 24 steps: 5 splats after 6 steps, 9 after 10, 20 after 16). Scored
    at SH degree 0: every score is bit-identical (the score does not read colour), so that mistake cannot be seen and is not a case.
    Pinned share of the survivors (pos sh0 shN opacity scale rot): 1 1 1 .9819 1 .9998."""
    c, spec, cams = _case("plain")
    n, K, more = c["n"], c["K"], c["more"]
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _plain_start_model(spec, c["seed"])
    r32, r64 = _pair(cams, tg, init, c["sh"], K + more, K)
    light, lmargin = r64.prune_decisions()
    assert not light.any() and lmargin.min() > FIRM, (light.sum(), lmargin.min())             # the light prune firmly takes nothing
    prune, firm, scores, excl = _plain_rule(r64)
    p32, f32, s32, _ = _plain_rule(r32)
    keep = _kept(n)
    assert prune.sum() == n - keep == n * PERCENT // 100
    assert firm.mean() >= FIRM_SHARE and np.array_equal(prune[firm], p32[firm]), (firm.mean(), (prune != p32)[firm].sum())
    zero = scores == 0
    assert 10 <= zero.sum() < prune.sum() and (s32 == 0).sum() == zero.sum()                      # never-taken splats exist, the cut is above them
    found = {}
    s_cam0, e_cam0 = r64.importance_scores([0])
    p, m = importance_decisions(s_cam0, e_cam0, keep)
    found["camera 0 only"] = _differ(prune, firm, p, m > FIRM)
    s_deg0, _ = _scores_of(r64, slice(None), range(c["cams"]), sh_degree=0)
    assert np.array_equal(s_deg0, scores)                 # the score does not read colour: the SH degree cannot be seen here (dropped)
    found["best removed"] = _differ(prune, firm, _swapped(scores, keep))
    r0 = TrainStepRef(Oracle, cams, tg, init, c["sh"], K + more, np.float64)
    s_start, e_start = r0.importance_scores(range(c["cams"]))
    p, m = importance_decisions(s_start, e_start, keep)
    found["scored from the start model"] = _differ(prune, firm, p, m > FIRM)
    shares = _pinned(*_after_prune(r32, r64, ~prune), {k: init[k][~prune] for k in KEYS}, SHARE_L1)
    print(dict(firm=float(firm.mean()), excluded=int(excl.sum()), zero=int(zero.sum()), pruned=int(prune.sum())), found, shares)
    _assert_discriminates(found)


def _after_prune(r32, r64, keep):
    """copies of the pair with `keep` applied (the pair itself stays at the prune step)"""
    a, b = _clone(r32), _clone(r64)
    a.apply_prune(keep); b.apply_prune(keep)
    return a, b


def _clone(r):
    """a restatement that shares the oracle and the views and owns its parameters, moments and statistics"""
    q = copy.copy(r)
    q.P, q.M, q.V = ({k: v.copy() for k, v in D.items()} for D in (r.P, r.M, r.V))
    q.grad_accum, q.grad_accum_mean2d, q.denom, q.max_radii = r.grad_accum.copy(), r.grad_accum_mean2d.copy(), r.denom.copy(), r.max_radii.copy()
    q.losses = list(r.losses)
    return q


def test_moments_case_is_pinned_and_discriminates():
    """measured (oracle targets; the plain case two steps past its prune at 24): pinned share (pos sh0 shN opacity scale rot)
    1 1 1 .9838 1 .9998; median difference on the moved elements two steps on, moments zeroed instead of carried sh0 3.2e-3, opacity
    4.1e-2; moments carried one row off sh0 1.0e-3, opacity 1.4e-2 (the bar: 10 x RTOL = 1e-3)."""
    c, spec, cams = _case("plain")
    K, more = c["K"], c["more"]
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _plain_start_model(spec, c["seed"])
    r32, r64 = _pair(cams, tg, init, c["sh"], K + more, K)
    keep = ~_plain_rule(r64)[0]
    at_prune = {k: r64.P[k][keep].copy() for k in KEYS}
    variants = {}
    for name in ("carried", "zeroed", "shifted"):
        r = _clone(r64)
        r.apply_prune(keep)
        assert r.P["pos"].shape[0] == keep.sum() and r.M["shN"].shape == (keep.sum(), 15, 3)
        for k in KEYS:
            if name == "zeroed":
                r.M[k][:] = 0; r.V[k][:] = 0
            if name == "shifted":
                r.M[k], r.V[k] = np.roll(r.M[k], 1, axis=0), np.roll(r.V[k], 1, axis=0)
        for _ in range(more):
            r.train_step()
        variants[name] = r
    r32.apply_prune(keep); r64.apply_prune(keep)
    for _ in range(more):
        r32.train_step(); r64.train_step()
    for k in KEYS:
        assert np.array_equal(r64.P[k], variants["carried"].P[k])
    shares = _pinned(r32, r64, {k: init[k][keep] for k in KEYS}, SHARE_L1)
    moved = {}
    for name in ("zeroed", "shifted"):
        for k in ("sh0", "opacity"):
            moved[name, k] = _median_difference(r64, variants[name], at_prune, k)
    print(shares, moved)
    for key, d in moved.items():
        assert d > 10 * RTOL, (key, d)


def _composed_rule(r, c, cam_indices=None, mask=True, before_light=False):
    """the pruned set of case C over the n splats of the restated state at the prune step: the light prune's, and of its survivors the
    30 % with the smallest score over the training cameras, masked -> (pruned [n], firm [n], light [n], report). The alternatives of
    the discrimination test: other cameras, no mask, or the importance prune planned over all n splats (scored before the light prune
    compacted them, 30 % of n)."""
    n = r.P["pos"].shape[0]
    train, _ = _splits(c)
    light, lmargin = r.prune_decisions()
    rows = np.arange(n) if before_light else np.flatnonzero(~light)
    scores, excl = _scores_of(r, rows, train if cam_indices is None else cam_indices, mask=mask)
    p, m = importance_decisions(scores, excl, _kept(rows.size))
    pruned, firm = light.copy(), lmargin > FIRM
    pruned[rows] |= p
    firm[rows] &= (m > FIRM) | light[rows]                # a light-pruned splat goes whatever it scores
    return pruned, firm, light, dict(light=int(light.sum()), light_firm=float((lmargin > FIRM).mean()), importance=int(p.sum()),
                                     excluded=int(excl.sum()), zero=int((scores == 0).sum()), firm=float(firm.mean()))


def test_composed_case_is_pinned_and_discriminates():
    """measured (oracle targets, 2000 splats, 96x64, 7 cameras of which 0, 3, 6 are held out, mask, 8 steps): the light prune takes 316
    (99.75 % of its decisions firm), the importance prune 505 of the 1684 survivors, of which 349 score 0 under the mask; 99.3 % of the
    2000 decisions are firm, none excluded. Firm under the rule and under the mistake, decided differently: all seven cameras 24
    splats (1.2 %), first pass only (cameras 1, 2, 4) 23 (1.2 %), no mask 323 (16 %), scored before the light prune 147 (7.4 %). The
    cameras of the rig sit 0.5 apart and look at one point, so a camera more or less moves few ranks across the cut: 2000 splats and
    this seed are what put both camera mistakes over 1 % (1500 splats: 5 .. 14 for six seeds). Pinned share of the survivors: opacity
    .9975, every other group 1."""
    c, spec, cams = _case("composed")
    n, K = c["n"], c["K"]
    train, test = _splits(c)
    assert train == [1, 2, 4, 5] and test == [0, 3, 6] and c["eval_views"] == min(len(test), 8)    # ensure_eval_ctx: min(n_test, 8) views per pass
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _prune_start_model(spec, cams, c["seed"])
    r32, r64 = _pair(cams, tg, init, c["sh"], K, K, mask=True, train_cams=train)
    assert set(r64.order[:K]) <= set(train) and len(set(r64.order[:K])) > 1
    pruned, firm, light, rep = _composed_rule(r64, c)
    p32, _, l32, _ = _composed_rule(r32, c)
    assert firm.mean() >= FIRM_SHARE and np.array_equal(pruned[firm], p32[firm]), (rep, (pruned != p32)[firm].sum())
    assert 0.12 * n < light.sum() < 0.2 * n and rep["light_firm"] > 0.95 and np.array_equal(light, l32), rep      # a firm, non-empty light prune first
    assert rep["importance"] == (n - light.sum()) * PERCENT // 100
    found = {}
    for name, kw in (("all seven cameras", dict(cam_indices=range(c["cams"]))),
                     ("first pass only", dict(cam_indices=train[:c["eval_views"]])),
                     ("no mask", dict(mask=False)),
                     ("scored before the light prune", dict(before_light=True))):
        alt, alt_firm, _, _ = _composed_rule(r64, c, **kw)
        found[name] = _differ(pruned, firm, alt, alt_firm)
    assert train[:c["eval_views"]] == [1, 2, 4]
    keep = ~pruned
    shares = _pinned(*_after_prune(r32, r64, keep), {k: init[k][keep] for k in KEYS}, SHARE_L1)
    print(rep, found, shares)
    _assert_discriminates(found)


def test_order_case_culls_its_tail_in_every_camera():
    """case D on the CPU: the last 40 % of the start model is culled by the oracle in every camera (radii == 0, float32 and float64),
    keeps ordinary opacities and scales that the light prune firmly leaves alone, scores exactly 0 — so the restated selection from the
    START model already removes exactly the last n 30 // 100 indices (zero scores tie, the larger index goes first), whatever the
    visible splats score (measured: 600 visible rows of which 18 score 0 too, 400 culled, 300 removed)."""
    c, spec, cams = _case("order")
    n = c["n"]
    init, first = _order_start_model(spec, c["seed"], c["culled"])
    assert first == n - int(0.4 * n) and n - first > n * PERCENT // 100
    for dt in (np.float32, np.float64):
        o = Oracle(dt)
        for cam in cams:
            o.forward(init, cam, sh_degree=c["sh"])
            radii = o.get("radii")
            assert (radii[first:] == 0).all() and (radii[:first] > 0).mean() > 0.5
    r = TrainStepRef(Oracle, cams, _oracle_targets(spec, cams, c["sh"]), init, c["sh"], c["K"], np.float64)
    light, lmargin = r.prune_decisions()
    assert not light.any() and lmargin.min() > FIRM
    scores, excl = r.importance_scores(range(c["cams"]))
    assert (scores[first:] == 0).all() and not excl[first:].any()
    prune, _ = importance_decisions(scores, excl, _kept(n))
    assert np.array_equal(np.flatnonzero(prune), np.arange(n - n * PERCENT // 100, n))
    G = r.train_step()
    for k in KEYS:                                               # no gradient, no step: the culled rows never move
        assert not G[k][first:].any() and np.array_equal(r.P[k][first:], init[k].reshape(r.P[k].shape)[first:])
    print(dict(first=first, culled=n - first, removed=int(prune.sum()), visible_zero=int((scores[:first] == 0).sum())))


# ---- the product ------------------------------------------------------------------------------------------------------------------------
LIGHT_LINE = r"light prune @(\d+): (\d+) -> (\d+) splats"
IMPORTANCE_LINE = r"importance prune @(\d+): (\d+) -> (\d+) splats, (\d+) views, (\d+) never taken"


def _prune_flags(K, **over):
    return _flags(refineStopIter=1, pruneStrategy=1, pruneEvery=K, importancePrune=PERCENT, **over)


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """cases A and B share their runs: the product to the prune step K and to K + 2, the training views, and the restated pair at K"""
    c, spec, cams = _case("plain")
    K, more = c["K"], c["more"]
    tmp = tmp_path_factory.mktemp("plain")
    init = _plain_start_model(spec, c["seed"])
    tg = _hip_targets(spec, cams, c["sh"])
    pa, gotA = _product(tmp, "a", c, init, _prune_flags(K), 0, K)
    pb, gotB = _product(tmp, "b", c, init, _prune_flags(K), 0, K + more)
    return dict(init=init, tg=tg, pa=pa, gotA=gotA, pb=pb, gotB=gotB)


def _decode_kept(r64, got):
    act = _decode_actions({k: r64.P[k].astype(np.float32) for k in KEYS}, got)
    assert set(act.tolist()) <= {0, 3}, np.bincount(act, minlength=4)
    return act == 3


@pytest.mark.gpu
def test_plugin_importance_prune_removes_the_restated_set(plain_runs):
    """case A: four cameras, no mask, no hold-out, the run ends at the prune step 6; the light prune takes nothing. The rows missing from
    the saved model are importance_decisions() of the restated state after six steps, scored on all four cameras, wherever the decision
    has a 5 % margin; the survivors carry — in order, all six groups — the trajectory under the L1 bars; the logged `never taken` is
    the restated count of zero scores to within the excluded splats. On the CPU (oracle targets): firm share .982, 41 zero
    scores, pinned share opacity .9819, rot .9998, others 1. On the GPU the same firm share and counts (450 removed, never taken 41, no
    splat differing on the firm set); worst pinned element 2.8e-5 (an opacity)."""
    c, spec, cams = _case("plain")
    n, K = c["n"], c["K"]
    init, tg, pa, gotA = (plain_runs[k] for k in ("init", "tg", "pa", "gotA"))
    report = {}
    try:
        assert not re.findall(LIGHT_LINE, pa.stderr), pa.stderr[-1500:]
        m = re.findall(IMPORTANCE_LINE, pa.stderr)
        assert len(m) == 1, pa.stderr[-1500:]
        it, a, b, views, never = (int(v) for v in m[0])
        assert (it, a, b, views) == (K, n, _kept(n), c["cams"]) and gotA["pos"].shape[0] == b, (m, gotA["pos"].shape)
        r32, r64 = _pair(cams, tg, init, c["sh"], K, K)
        want, firm, scores, excl = _plain_rule(r64)
        pruned = _decode_kept(r64, gotA)
        report.update(firm=float(firm.mean()), pruned=int(pruned.sum()), want=int(want.sum()), excluded=int(excl.sum()),
                      zero=int((scores == 0).sum()), never_taken=never, differ_on_firm=int((pruned != want)[firm].sum()))
        print(report)
        assert firm.mean() >= FIRM_SHARE, report
        assert np.array_equal(pruned[firm], want[firm]), (np.flatnonzero(pruned[firm] != want[firm])[:10], report)
        assert abs(never - int((scores == 0).sum())) <= int(excl.sum()), report
        keep = ~pruned
        r32.apply_prune(keep); r64.apply_prune(keep)
        report["a"] = {}
        _bars(gotA, r32, r64, {k: init[k][keep] for k in KEYS}, report["a"], ssim=False)
        print(report["a"])
    finally:
        _dump("importance_plain", report)


@pytest.mark.gpu
def test_plugin_importance_prune_carries_the_moments(plain_runs):
    """case B: the same run continued two steps past the prune, against the restatement with the PRODUCT's kept set applied at step 6
    and two more steps, under the L1 bars: the two Adam steps use the moments that travelled with their rows (zeroed or misplaced
    moments move the median sh0 / opacity element by more than 10x the tolerance: test_moments_case_is_pinned_and_discriminates). Measured on the GPU: pinned share opacity .9838, rot .9998, others 1; worst pinned
    element 2.6e-5."""
    c, spec, cams = _case("plain")
    n, K, more = c["n"], c["K"], c["more"]
    init, tg, gotA, pb, gotB = (plain_runs[k] for k in ("init", "tg", "gotA", "pb", "gotB"))
    report = {}
    try:
        m = re.findall(IMPORTANCE_LINE, pb.stderr)
        assert [tuple(int(v) for v in x[:4]) for x in m] == [(K, n, _kept(n), c["cams"])] and gotB["pos"].shape[0] == _kept(n), (m, gotB["pos"].shape)
        r32, r64 = _pair(cams, tg, init, c["sh"], K + more, K)
        keep = ~_decode_kept(_r64(cams, tg, init, c["sh"], K, K), gotA)            # (run A's own schedule: maxIteration K)
        assert keep.sum() == _kept(n)
        r32.apply_prune(keep); r64.apply_prune(keep)
        for _ in range(more):
            r32.train_step(); r64.train_step()
        report["b"] = {}
        _bars(gotB, r32, r64, {k: init[k][keep] for k in KEYS}, report["b"], ssim=False)
        print(report["b"])
    finally:
        _dump("importance_moments", report)


@pytest.mark.gpu
def test_plugin_importance_prune_after_the_light_prune_on_masked_training_cameras(tmp_path):
    """case C: seven cameras with --evalHoldout 3 (0, 3, 6 held out; 1, 2, 4, 5 train; eval_views = 3, so the scoring runs as one pass
    of three cameras and a partial pass of one) and --useMask 1, from the light-prune test's start model. At step 6 the log carries the
    light prune's line, then the importance prune's, whose `a` is the light prune's result, on 4 views; the rows missing from the saved
    model are prune_decisions() united with importance_decisions() over the light prune's survivors, scored on the four training
    cameras under the mask, wherever both decisions have a 5 % margin; the survivors carry the masked, training-cameras-only trajectory
    under the L1 bars. On the CPU (oracle targets): light 316, importance 505, firm share .993. On the GPU the same counts, no splat
    differing on the firm set; worst pinned element 2.4e-5 (an opacity)."""
    c, spec, cams = _case("composed")
    n, K = c["n"], c["K"]
    train, _ = _splits(c)
    init = _prune_start_model(spec, cams, c["seed"])
    tg = _hip_targets(spec, cams, c["sh"])
    report = {}
    try:
        p, got = _product(tmp_path, "c", c, init, _prune_flags(K, evalHoldout=c["holdout"], useMask=1), 0, K)
        both = re.findall(LIGHT_LINE + "|" + IMPORTANCE_LINE, p.stderr)
        assert len(both) == 2 and both[0][0] == str(K) and both[1][3] == str(K), p.stderr[-2500:]          # the light line first, both at step K
        light_n = int(both[0][2])
        a, b, views = (int(v) for v in both[1][4:7])
        assert int(both[0][1]) == n and a == light_n and b == _kept(a) and views == len(train) == 4, both
        assert got["pos"].shape[0] == b
        r32, r64 = _pair(cams, tg, init, c["sh"], K, K, mask=True, train_cams=train)
        want, firm, light, rep = _composed_rule(r64, c)
        pruned = _decode_kept(r64, got)
        report.update(rep, product_light=n - light_n, pruned=int(pruned.sum()), want=int(want.sum()), differ_on_firm=int((pruned != want)[firm].sum()))
        print(report)
        assert firm.mean() >= FIRM_SHARE and 0.12 * n < light.sum() < 0.2 * n, report
        assert np.array_equal(pruned[firm], want[firm]), (np.flatnonzero(pruned[firm] != want[firm])[:10], report)
        keep = ~pruned
        r32.apply_prune(keep); r64.apply_prune(keep)
        report["c"] = {}
        _bars(got, r32, r64, {k: init[k][keep] for k in KEYS}, report["c"], ssim=False)
        print(report["c"])
    finally:
        _dump("importance_composed", report)


@pytest.mark.gpu
def test_plugin_importance_prune_takes_zero_scores_from_the_largest_index(tmp_path):
    """case D, exact and independent of the trajectory: the last 40 % of the model lies behind every camera — never listed, score exactly
    0, gradient exactly 0 — with ordinary opacities and scales, so the light prune keeps them. --importancePrune 30 removes exactly the
    last n 30 // 100 indices (zero scores tie; the larger index goes first), and every surviving culled row of the saved model is bit
    for bit the row written four steps earlier. Measured on the GPU: 418 never taken (the 400 culled and 18 visible ones), rows 600 .. 699
    identical in all six groups."""
    c, spec, cams = _case("order")
    n, K = c["n"], c["K"]
    init, first = _order_start_model(spec, c["seed"], c["culled"])
    p, got = _product(tmp_path, "d", c, init, _prune_flags(K), 0, K)
    assert not re.findall(LIGHT_LINE, p.stderr)
    m = re.findall(IMPORTANCE_LINE, p.stderr)
    assert len(m) == 1 and tuple(int(v) for v in m[0][:4]) == (K, n, _kept(n), c["cams"]), p.stderr[-1500:]
    assert int(m[0][4]) >= n - first                                             # the culled splats at least were never taken
    last = _kept(n)
    assert first < last < n and got["pos"].shape[0] == last
    report = dict(first_culled=first, kept=last, never_taken=int(m[0][4]), rows_differing={})
    for k in KEYS:
        a, b = got[k][first:last], np.ascontiguousarray(init[k][first:last], np.float32)
        report["rows_differing"][k] = int((a.view(np.uint32) != b.view(np.uint32)).reshape(last - first, -1).any(1).sum())
    # the visible rows moved (they were trained) and stayed in place: rotations identify a row (tests/test_train_step.py _decode_actions)
    report["visible_rows_in_place"] = float((np.abs(got["rot"][:first] - init["rot"][:first]).max(1) < 2e-2).mean())   # (four steps at rate 1e-3; rows differ by O(1))
    _dump("importance_order", report)
    print(report)
    assert not any(report["rows_differing"].values()) and report["visible_rows_in_place"] == 1.0, report
    assert (got["sh0"][:first] != init["sh0"][:first]).mean() > 0.5
