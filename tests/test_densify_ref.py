"""The restatement tests/densify_ref.py itself, on the CPU: the vectorised rule against one literal loop over the splats, the generated
inputs of tests/test_gpu_densify_rules.py (margins, what they cover), and the power of its covariance bars."""
import numpy as np
import pytest
import densify_ref as D
from densify_ref import KEEP, CLONE, SPLIT, PRUNE


@pytest.mark.parametrize("limits", [True, False])
def test_vectorised_rule_equals_the_literal_loop(limits):
    n = 1031
    A, ga, de, mr = D.plan_scene(n, seed=4)
    op, sc = A["opacity"].copy(), A["scale"].copy()
    op[[5, 600]], sc[40, 1], sc[41, 0], sc[900, 2] = (np.nan, np.inf), np.nan, -np.inf, np.inf
    base = dict(D.PLAN_PRM) if limits else dict(D.PLAN_PRM, max_world_scale=0.0, max_screen_radius=0)
    a0, _, _, uncapped, _ = D.actions(op, sc, ga, de, mr, base)
    S, G = int((a0 != PRUNE).sum()), int(np.isin(a0, (CLONE, SPLIT)).sum())
    assert (a0[[5, 600, 40, 41, 900]] == PRUNE).all() and G > 50
    for cap in (0, -3, 1, S - 1, S, S + 1, S + G // 2, S + G - 1, S + G, S + G + 9):
        prm = dict(base, cap_max=cap)
        _, act, offs, new_n, _ = D.actions(op, sc, ga, de, mr, prm)
        lit = D.actions_literal(op, sc, ga, de, mr, prm)
        assert np.array_equal(act, lit[0]) and np.array_equal(offs, lit[1]) and new_n == lit[2], cap
        assert new_n == (uncapped if cap <= 0 else min(uncapped, max(cap, S))), cap


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10_007, 65_537])
def test_generated_inputs_keep_their_distance_from_every_threshold(n):
    A, ga, de, mr = D.plan_scene(n, seed=1000 + n % 1000)
    off = dict(D.PLAN_PRM, max_world_scale=0.0, max_screen_radius=0)
    for prm in (D.PLAN_PRM, off):
        act, _, _, _, margin = D.actions(A["opacity"], A["scale"], ga, de, mr, prm)
        assert margin.min() >= D.MARGIN, margin.min()
        if n >= 255:
            assert set(act.tolist()) == {KEEP, CLONE, SPLIT, PRUNE}
    assert (mr[de == 0] == 0).all()


def test_margin_of_the_integer_radius_and_of_a_doubly_pruned_splat():
    z = np.zeros(1, np.float32)
    prm = dict(D.PLAN_PRM)
    one = lambda logit, s, r: D.actions(np.float32([logit]), np.float32([[s, s, s]]), z, z + 1, np.int32([r]), prm)
    assert one(2.0, np.log(0.01), 29)[4][0] > 0.9 and one(2.0, np.log(0.01), 30)[4][0] == pytest.approx(1 / 30) and one(2.0, np.log(0.01), 30)[0][0] == KEEP
    assert one(2.0, np.log(0.01), 31)[4][0] == np.inf and one(2.0, np.log(0.01), 31)[0][0] == PRUNE
    # pruned by the world scale with 60 % to spare: an opacity a hair under its threshold does not make the decision doubtful
    hair = float(np.log(0.005 / 0.995)) - 1e-6
    act, _, _, _, margin = one(hair, np.log(0.8), 5)
    assert act[0] == PRUNE and margin[0] == pytest.approx(0.6, rel=1e-3)
    assert one(hair, np.log(0.01), 5)[4][0] < 1e-5


def test_split_moments_and_revised_opacity():
    mean, S = D.split_moments((1, 2, 3), np.log((0.5, 1.0, 2.0)), (0, 0, 0, 0))
    assert np.array_equal(S, np.diag([0.25, 1.0, 4.0])) and mean.tolist() == [1, 2, 3]
    # a quarter turn about z, q = (cos 45, 0, 0, sin 45) scaled by 3: x -> y, so the x scale shows up on the y axis
    _, S = D.split_moments((0, 0, 0), np.log((0.5, 1.0, 2.0)), (3 * np.sqrt(0.5), 0, 0, 3 * np.sqrt(0.5)))
    assert np.allclose(S, np.diag([1.0, 0.25, 4.0]), atol=1e-15)
    R = D.quat_to_rot((0.3, -0.5, 0.7, 0.2))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    x = np.linspace(-12, 12, 101)
    o, o2 = 1 / (1 + np.exp(-x)), 1 / (1 + np.exp(-D.revised_opacity(x)))
    assert np.allclose(1 - (1 - o2) ** 2, o, rtol=1e-9, atol=0) and (o2 < o).all()
    assert D.revised_opacity(np.array([-88.0, 88.0])).tolist() == pytest.approx([np.log(1e-6 / (1 - 1e-6)), np.log((1 - 1e-6) / 1e-6)])
