"""The ADC densifier (csrc/densify.hip) on the branches a real run takes after its first opacity reset, against the fp64 restatement
tests/densify_ref.py: the plan with the world-scale and screen-radius limits on (prune before grow, both comparisons strict, a
never-seen splat kept, the prunes counted out of the cap's budget), the same inputs under a cap and with the limits off, splats with
non-finite parameters, the distribution of the split samples (mean, covariance R S^2 R^T, independence of the two children, kurtosis,
tail), and the revised opacity at both ends of the logit range.

Every bar is exact, taken from the existing test it names, or derived from the sample count and the restated covariance; the inputs
are drawn (on the CPU, before any launch) so that no decision is within densify_ref.MARGIN of a threshold: there is no exclusion list."""
import functools
import numpy as np
import pytest
import densify_ref as D
from densify_ref import KEEP, CLONE, SPLIT, PRUNE
from test_gpu_train_ops_scale import _Adc, _check_apply

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 10_007, 65_537]              # 65 537 = one splat past a 256-block chunk of k_densify_scan_blocks


def _prm(**over):
    from divshot_amd._lib import DensifyParams
    kw = dict(D.PLAN_PRM, cap_max=0, seed=91, shn_layout=0, revised_opacity=0)
    kw.update(over)
    return DensifyParams(**kw)


@functools.lru_cache(maxsize=None)
def _scene(n):
    """the inputs of one size and their restated plan under PLAN_PRM and with both limits off, computed once and left unchanged"""
    A, ga, de, mr = D.plan_scene(n, seed=1000 + n % 1000)
    ref_on = D.actions(A["opacity"], A["scale"], ga, de, mr, _prm())
    ref_off = D.actions(A["opacity"], A["scale"], ga, de, mr, _prm(max_world_scale=0.0, max_screen_radius=0))
    for x in list(A.values()) + [ga, de, mr] + [r for ref in (ref_on, ref_off) for r in ref if isinstance(r, np.ndarray)]:
        x.setflags(write=False)
    return A, ga, de, mr, ref_on, ref_off


def _quantities(A, ga, de):
    op = 1.0 / (1.0 + np.exp(-A["opacity"].astype(np.float64)))
    smax = np.exp(A["scale"].max(1).astype(np.float64))
    avg = np.where(de > 0, ga.astype(np.float64) / np.maximum(de, 1), 0.0)
    return op, smax, avg


def _assert_plan(got, want_act, want_offs, want_n, tag):
    act, offs, new_n = got
    assert np.array_equal(act, want_act), (tag, int((act != want_act).sum()), np.flatnonzero(act != want_act)[:8])
    assert np.array_equal(offs, want_offs), (tag, np.flatnonzero(offs != want_offs)[:8])
    assert new_n == want_n, (tag, new_n, want_n)


@pytest.mark.parametrize("n", SIZES)
def test_plan_with_both_limits_on(gpu_device, n):
    """dvs_densify_plan with max_world_scale = 0.5 and max_screen_radius = 30: action, offsets and new count exactly the restatement's
    on every splat. From 255 splats on the inputs hold all four actions; each prune cause (opacity, world scale, screen radius) alone;
    each together with avg >= grad_threshold and a scale over scale_threshold (PRUNE, not SPLIT / CLONE); max_radii == 30 (not pruned:
    KEEP and SPLIT) and == 31 (pruned); denom == 0 with max_radii == 0 (kept). A single splat is one plain draw. Up to 10 007 splats
    apply is checked row by row as well."""
    A, ga, de, mr, ref, _ = _scene(n)
    act0, act, offs, new_n, margin = ref
    assert margin.min() >= D.MARGIN, margin.min()
    p = D.params(_prm())
    op, smax, avg = _quantities(A, ga, de)
    c_op, c_ws, c_r = op < p["min_opacity"], smax > p["max_world_scale"], mr > p["max_screen_radius"]
    grows, big = avg >= p["grad_threshold"], smax > p["scale_threshold"]
    if n >= 255:
        assert set(act.tolist()) == {KEEP, CLONE, SPLIT, PRUNE}
        for name, alone in (("opacity", c_op & ~c_ws & ~c_r), ("world", c_ws & ~c_op & ~c_r), ("screen", c_r & ~c_op & ~c_ws)):
            assert alone.sum() >= 5 and (act[alone] == PRUNE).all(), name
            assert (alone & grows & big).sum() >= 5, name                              # prune before grow
        assert (act[(mr == 30) & ~c_op & ~c_ws] != PRUNE).all() and ((mr == 30) & (act == KEEP)).any() and ((mr == 30) & (act == SPLIT)).any()
        assert (act[mr == 31] == PRUNE).all() and ((mr == 31) & ~c_op & ~c_ws).any()
        assert ((de == 0) & (mr == 0) & (act == KEEP)).sum() >= 5
        for k, want in D.CONSTRUCTED_WANT.items():
            assert (act[k::32] == want).all(), D.CONSTRUCTED[k][0]
    d = _Adc(A, ga, de, mr, False, gpu_device)
    prm = _prm()
    _assert_plan(d.plan(prm), act, offs, new_n, "limits on")
    if n <= 10_007 and new_n:
        _check_apply(A, act, offs, new_n, d.apply(prm, 0, new_n), 0)


@pytest.mark.parametrize("n", SIZES)
def test_plan_under_a_cap_counts_every_prune_out_of_the_budget(gpu_device, n):
    """The same inputs and limits with cap_max cutting inside a block, exactly at S, below S and <= 0. S counts the survivors of ALL
    THREE prune rules (with the limits off it would be larger, and the budget cap_max - S smaller: asserted below), demoted candidates
    read KEEP, PRUNE is untouched, new_count = min(uncapped, max(cap_max, S))."""
    A, ga, de, mr, ref, ref_off = _scene(n)
    act0, _, _, uncapped, margin = ref
    assert margin.min() >= D.MARGIN
    S = int((act0 != PRUNE).sum())
    grow = np.flatnonzero((act0 == CLONE) | (act0 == SPLIT))
    if n >= 255:
        assert int((ref_off[0] != PRUNE).sum()) > S + 5                                # the two limits do change S
    caps = {"no cap (0)": 0, "no cap (negative)": -7}
    inside = [k for k in range(max(1, len(grow) // 2), len(grow)) if grow[k - 1] // 256 == grow[k] // 256]
    if inside:
        caps["inside a block"] = S + inside[0]
    if S > 0:
        caps["exactly S"] = S
    if S > 1:
        caps["below S"] = S - 1
    if S > 40:
        caps["far below S"] = S // 3
    d = _Adc(A, ga, de, mr, False, gpu_device)
    for name, cap in caps.items():
        prm = _prm(cap_max=cap)
        a0, act, offs, new_n, _ = D.actions(A["opacity"], A["scale"], ga, de, mr, prm)
        assert np.array_equal(a0, act0)
        demoted = act != act0
        assert (act[demoted] == KEEP).all() and np.isin(act0[demoted], (CLONE, SPLIT)).all() and np.array_equal(act == PRUNE, act0 == PRUNE)
        assert new_n == (uncapped if cap <= 0 else min(uncapped, max(cap, S))), name
        if name == "inside a block":
            assert 0 < demoted.sum() < len(grow)
        if name in ("exactly S", "below S", "far below S"):
            assert demoted.sum() == len(grow) and new_n == S
        _assert_plan(d.plan(prm), act, offs, new_n, name)


@pytest.mark.parametrize("n", SIZES)
def test_plan_with_the_limits_off_is_the_opacity_only_rule(gpu_device, n):
    """max_world_scale = 0 and max_screen_radius = 0 on the same inputs: the rule the older tests took, written out once more here."""
    A, ga, de, mr, _, ref = _scene(n)
    _, act, offs, new_n, margin = ref
    assert margin.min() >= D.MARGIN
    op, smax, avg = _quantities(A, ga, de)
    p = D.params(_prm())
    plain = np.where(op < p["min_opacity"], PRUNE, np.where(avg >= p["grad_threshold"], np.where(smax > p["scale_threshold"], SPLIT, CLONE), KEEP))
    assert np.array_equal(act, plain)
    d = _Adc(A, ga, de, mr, False, gpu_device)
    _assert_plan(d.plan(_prm(max_world_scale=0.0, max_screen_radius=0)), act, offs, new_n, "limits off")


def test_non_finite_parameters_are_pruned(gpu_device):
    """A splat whose opacity or any one scale is NaN, +inf or -inf is PRUNE whatever the limits and the cap (twelve kinds, each at a
    block start, a block end, mid-array and among the last splats; with growth statistics, and never seen). It is not counted in S
    (new_count under a cap that cuts), its neighbours' offsets are the restatement's, and apply writes nothing from it: every output
    row is a finite survivor's."""
    n = 10_007
    A0, ga0, de0, mr0, _, _ = _scene(n)
    A = {k: v.copy() for k, v in A0.items()}
    ga, de, mr = ga0.copy(), de0.copy(), mr0.copy()
    kinds = [("opacity", None, v) for v in (np.nan, np.inf, -np.inf)] + [("scale", k, v) for k in range(3) for v in (np.nan, np.inf, -np.inf)]
    poison = []
    for j, (key, axis, v) in enumerate(kinds):
        for base in (256 * (j + 1), 256 * (j + 20) - 1, 5000 + 37 * j, n - 1 - j):
            poison.append(base)
            A["opacity"][base], A["scale"][base] = 2.0, np.log(np.float32(0.03))       # alive and a CLONE but for the poisoned value
            if key == "opacity":
                A["opacity"][base] = v
            else:
                A["scale"][base, axis] = v
            seen = (base % 2) == 0
            ga[base], de[base], mr[base] = (1e-2, 2, 7) if seen else (0, 0, 0)
    poison = np.array(poison)
    assert len(set(poison.tolist())) == len(kinds) * 4
    d = _Adc(A, ga, de, mr, True, gpu_device)
    for limits in (dict(), dict(max_world_scale=0.0, max_screen_radius=0)):
        a0, _, _, uncapped, margin = D.actions(A["opacity"], A["scale"], ga, de, mr, _prm(**limits))
        assert margin.min() >= D.MARGIN and (a0[poison] == PRUNE).all()
        S = int((a0 != PRUNE).sum())
        G = int(np.isin(a0, (CLONE, SPLIT)).sum())
        for cap in (0, S + G // 2, S):
            prm = _prm(cap_max=cap, shn_layout=1, **limits)
            _, act, offs, new_n, _ = D.actions(A["opacity"], A["scale"], ga, de, mr, prm)
            assert new_n == (uncapped if cap == 0 else min(uncapped, max(cap, S)))
            got = d.plan(prm)
            assert (got[0][poison] == PRUNE).all(), (limits, cap, got[0][poison])
            _assert_plan(got, act, offs, new_n, (limits, cap))
            if cap != S:
                out = d.apply(prm, 0, new_n)
                assert all(np.isfinite(v).all() for v in out.values())
                assert not np.isin(out["rot"][:, 3].astype(np.int64), poison).any()
                _check_apply(A, act, offs, new_n, out, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the split samples
# ---------------------------------------------------------------------------------------------------------------------------
N_SPLIT = 8192
SPLIT_POS, SPLIT_SCALE, SPLIT_ROT = (0.3, -1.1, 2.0), np.log((0.05, 0.2, 0.1)), (0.3, -0.5, 0.7, 0.2)
Z_MAX = float(np.sqrt(-2.0 * np.log(0.5 / 2 ** 24)))     # Box-Muller on d_uniform's smallest value (0 + 0.5) / 2^24: 5.887


def _cov_bar(Sigma, M):
    """6 standard errors of every entry of the sample covariance of M draws from N(0, Sigma): Var = (S_ii S_jj + S_ij^2) / M"""
    dg = np.diag(Sigma)
    return 6.0 * np.sqrt((np.outer(dg, dg) + Sigma ** 2) / M)


def _split_children(dev, rot, seed, tiled=False):
    """N_SPLIT identical splats, every one planned SPLIT -> (pos [N, 2, 3], scale [N, 2, 3], all outputs) of the children"""
    n = N_SPLIT
    rng = np.random.default_rng(5)
    f = np.float32
    A = {"pos": np.tile(f(SPLIT_POS), (n, 1)), "sh0": rng.normal(size=(n, 3)).astype(f), "shN": rng.normal(size=(n, 15, 3)).astype(f),
         "opacity": np.full(n, 2.0, f), "scale": np.tile(SPLIT_SCALE.astype(f), (n, 1)), "rot": np.tile(f(rot), (n, 1))}
    d = _Adc(A, np.ones(n, f), np.ones(n, f), np.ones(n, np.int32), tiled, dev)
    prm = _prm(seed=seed, shn_layout=int(tiled))
    act, offs, new_n = d.plan(prm)
    assert (act == SPLIT).all() and new_n == 2 * n and np.array_equal(offs, 2 * np.arange(n))
    out = d.apply(prm, 0, new_n)
    return out["pos"].reshape(n, 2, 3), out["scale"].reshape(n, 2, 3), out, A


def _check_moments(pos, rot):
    """the children [N, 2, 3] against split_moments of the splat, per child slot and for both together"""
    f = np.float32
    mean, Sigma = D.split_moments(f(SPLIT_POS), SPLIT_SCALE.astype(f), f(rot))
    R = D.quat_to_rot(f(rot))
    sig = np.exp(SPLIT_SCALE.astype(f).astype(np.float64))
    assert np.isfinite(pos).all()
    dev = pos.astype(np.float64) - mean
    for name, d in (("child 0", dev[:, 0]), ("child 1", dev[:, 1]), ("both", dev.reshape(-1, 3))):
        M = d.shape[0]
        m = d.mean(0)
        print(name, "mean / bar", np.abs(m) / (6 * np.sqrt(np.diag(Sigma) / M)))
        assert (np.abs(m) <= 6.0 * np.sqrt(np.diag(Sigma) / M)).all(), (name, m)
        cov = (d - m).T @ (d - m) / M
        print(name, "cov / bar", (np.abs(cov - Sigma) / _cov_bar(Sigma, M)).max())
        assert (np.abs(cov - Sigma) <= _cov_bar(Sigma, M)).all(), (name, cov, Sigma)
        z = (d @ R) / sig                                            # coordinates along the principal axes, in standard deviations
        zc = z - z.mean(0)
        kurt = (zc ** 4).mean(0) / (zc ** 2).mean(0) ** 2 - 3.0
        print(name, "excess kurtosis / bar", np.abs(kurt) / (6 * np.sqrt(24.0 / M)), "max |z|", np.abs(z).max(0))
        assert (np.abs(kurt) <= 6.0 * np.sqrt(24.0 / M)).all(), (name, kurt)
        assert (np.abs(z).max(0) <= Z_MAX).all(), (name, np.abs(z).max(0))
    d0, d1 = dev[:, 0] - dev[:, 0].mean(0), dev[:, 1] - dev[:, 1].mean(0)
    cross = d0.T @ d1 / N_SPLIT
    print("cross / bar", (np.abs(cross) / _cov_bar(Sigma, N_SPLIT)).max())
    assert (np.abs(cross) <= _cov_bar(Sigma, N_SPLIT)).all(), cross
    return Sigma


def test_split_samples_have_the_splats_own_covariance(gpu_device):
    """8192 identical splats (pos (0.3, -1.1, 2), scales (0.05, 0.2, 0.1), the unnormalised quaternion (0.3, -0.5, 0.7, 0.2)), all SPLIT:
    the RNG is keyed on the splat index, so the children are 2 x 8192 independent draws of pos + R diag(exp s) z. Per child slot
    (M = 8192) and for both (M = 16 384): mean within 6 sqrt(S_ii / M); every covariance entry within 6 sqrt((S_ii S_jj + S_ij^2) / M)
    of S = R diag(exp 2s) R^T; child 0 against child 1 uncorrelated within that bar; excess kurtosis along each principal axis within
    6 sqrt(24 / M); |z| <= sqrt(-2 ln(0.5 / 2^24)) = 5.887, the generator's own tail. The bars are sampling theory at 6 sigma with a
    fixed seed. Power, asserted first on the CPU: S built with R^T, and S with two scale axes swapped, each miss some entry by more
    than 3 bars at M = 8192."""
    f = np.float32
    _, Sigma = D.split_moments(f(SPLIT_POS), SPLIT_SCALE.astype(f), f(SPLIT_ROT))
    R = D.quat_to_rot(f(SPLIT_ROT))
    S2 = np.diag(np.exp(2.0 * SPLIT_SCALE.astype(f).astype(np.float64)))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0)
    transposed = R.T @ S2 @ R
    _, swapped = D.split_moments(f(SPLIT_POS), SPLIT_SCALE.astype(f)[[1, 0, 2]], f(SPLIT_ROT))
    for name, wrong in (("R^T", transposed), ("scale axes swapped", swapped)):
        power = (np.abs(wrong - Sigma) / _cov_bar(Sigma, N_SPLIT)).max()
        print("power", name, power)
        assert power > 3.0, (name, power)
    pos, scale, out, A = _split_children(gpu_device, SPLIT_ROT, seed=91)
    _check_moments(pos, SPLIT_ROT)
    # children's scales: s - log 1.6 to one float32 ulp; everything else is the parent's
    want = (A["scale"].astype(np.float64) - D.LOG_1P6).astype(f)
    for c in (0, 1):
        assert (np.abs(scale[:, c] - want) <= np.spacing(np.abs(want))).all(), np.abs(scale[:, c] - want).max()
        for k in ("sh0", "shN", "opacity", "rot"):
            assert np.array_equal(out[k].reshape((N_SPLIT, 2) + out[k].shape[1:])[:, c], A[k]), k


def test_split_samples_are_a_function_of_seed_and_index_only(gpu_device):
    """Two calls with one seed are bit-identical and another seed is not; DVS_SHN_ROWS and DVS_SHN_TILED give bit-identical positions
    and scales."""
    p0, s0, _, _ = _split_children(gpu_device, SPLIT_ROT, seed=91)
    p1, s1, _, _ = _split_children(gpu_device, SPLIT_ROT, seed=91)
    p2, s2, _, _ = _split_children(gpu_device, SPLIT_ROT, seed=92)
    pt, st, _, _ = _split_children(gpu_device, SPLIT_ROT, seed=91, tiled=True)
    u = lambda a: a.view(np.uint32)
    assert np.array_equal(u(p0), u(p1)) and np.array_equal(u(s0), u(s1))
    assert np.array_equal(u(p0), u(pt)) and np.array_equal(u(s0), u(st))
    assert (p0 != p2).any(2).mean() > 0.999 and np.array_equal(u(s0), u(s2))
    assert (p0[:, 0] != p0[:, 1]).any(1).all()                      # the two children of a splat are different draws


def test_split_of_a_zero_quaternion_is_axis_aligned(gpu_device):
    """rot = 0: k_densify_apply's 1 / |q| is taken as 0 and R = I. Finite output, and the same moment bars against S = diag(exp 2s)."""
    pos, _, out, _ = _split_children(gpu_device, (0.0, 0.0, 0.0, 0.0), seed=17)
    Sigma = _check_moments(pos, (0.0, 0.0, 0.0, 0.0))
    assert np.array_equal(Sigma, np.diag(np.diag(Sigma))) and all(np.isfinite(v).all() for v in out.values())


# ---------------------------------------------------------------------------------------------------------------------------
# revised opacity
# ---------------------------------------------------------------------------------------------------------------------------
def test_revised_opacity_over_the_logit_range(gpu_device):
    """revisedOpacity on clones and splits for logits -12 .. 12 (2001 values) and at +-20, +-88, where the fp32 sigmoid saturates and
    exp overflows. In -12 .. 12: sigmoid(output) against the fp64 restatement at the bar of test_densify_plan_and_apply (rtol 2e-4,
    atol 1e-7), and the pair composites to o (that test's rtol 5e-4, atol 2e-6). At the four ends: finite, and inside
    [logit(1e-6), logit(1 - 1e-6)] to 1e-3. Both results are bit-identical; kept splats keep their logit."""
    f = np.float32
    logits = np.concatenate([np.linspace(-12, 12, 2001), [-20, 20, -88, 88]]).astype(f)
    m = logits.size
    n = 3 * m                                                       # one CLONE, one SPLIT, one KEEP per logit
    rng = np.random.default_rng(3)
    A = {"pos": rng.normal(size=(n, 3)).astype(f), "sh0": rng.normal(size=(n, 3)).astype(f), "shN": rng.normal(size=(n, 15, 3)).astype(f),
         "opacity": np.tile(logits, 3), "scale": np.full((n, 3), np.log(0.01), f), "rot": rng.normal(size=(n, 4)).astype(f)}
    A["scale"][m:2 * m, 1] = np.log(0.2)
    ga = np.ones(n, f); ga[2 * m:] = 0
    d = _Adc(A, ga, np.ones(n, f), np.ones(n, np.int32), False, gpu_device)
    prm = _prm(min_opacity=0.0, revised_opacity=1)                  # nothing is pruned for its opacity
    act, offs, new_n = d.plan(prm)
    want_act = np.repeat([CLONE, SPLIT, KEEP], m)
    assert np.array_equal(act, want_act) and new_n == 5 * m
    got = d.apply(prm, 0, new_n)["opacity"]
    assert np.array_equal(got[offs[2 * m:]], A["opacity"][2 * m:])
    first, second = got[offs[:2 * m]], got[offs[:2 * m] + 1]
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert np.array_equal(first[:m].view(np.uint32), first[m:].view(np.uint32))      # clone and split revise alike
    sig = lambda x: 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
    mid = np.abs(logits) <= 12
    assert mid.sum() == 2001
    o, o_new, o_want = sig(logits[mid]), sig(first[:m][mid]), sig(D.revised_opacity(logits[mid]))
    print("revised opacity: worst |err| / (2e-4 want + 1e-7)", (np.abs(o_new - o_want) / (2e-4 * o_want + 1e-7)).max())
    np.testing.assert_allclose(o_new, o_want, rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(1.0 - (1.0 - o_new) ** 2, o, rtol=5e-4, atol=2e-6)
    ends = first[:m][~mid].astype(np.float64)
    lo, hi = np.log(1e-6 / (1 - 1e-6)), np.log((1 - 1e-6) / 1e-6)
    print("revised opacity at -20, 20, -88, 88:", ends)
    assert np.isfinite(ends).all() and (ends >= lo - 1e-3).all() and (ends <= hi + 1e-3).all(), ends
    assert (ends[[0, 2]] < 0).all() and (ends[[1, 3]] > 0).all()
