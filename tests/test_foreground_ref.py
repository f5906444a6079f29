"""The restatement tests/foreground_ref.py pinned without a GPU: the plan rule on hand cases (the ones a 64-bit product would get wrong
among them) and the votes on a hand-made forward state."""
import numpy as np
import foreground_ref as FR
import importance_ref as IR
from depth_ref import S2D_X, S2D_Y, S2D_CONIC, S2D_OPACITY


def test_rule_on_hand_cases():
    assert not FR.keeps(0, 0, 50)                       # never taken by a valid pixel: in no training view
    assert not FR.keeps(0, 7, 1) and not FR.keeps(0, 7, 100)
    assert FR.keeps(1, 0, 1) and FR.keeps(1, 0, 50) and FR.keeps(1, 0, 100)          # bg = 0 stays at every threshold
    assert FR.keeps(5, 5, 50) and not FR.keeps(5, 6, 50) and FR.keeps(6, 5, 50)      # equality at T = 50 stays
    assert not FR.keeps(10 ** 9, 1, 100) and FR.keeps(1, 0, 100)                     # T = 100: one background unit removes
    assert FR.keeps(99, 1, 99) and not FR.keeps(98, 1, 99) and FR.keeps(1, 99, 1) and not FR.keeps(1, 100, 1)


def test_rule_does_not_wrap_at_two_to_the_62():
    big = 1 << 62
    assert big * 50 >= 1 << 64                          # both products wrap in 64 bits
    assert FR.keeps(big, big, 50)
    assert (big * 20) % (1 << 64) == (big * 80) % (1 << 64) == 0 and not FR.keeps(big, big, 80)      # a wrapped rule compares 0 >= 0 and keeps
    assert (big * 50) % (1 << 64) > (2 * big * 50) % (1 << 64) and not FR.keeps(big, 2 * big, 50)    # ... and keeps here too
    assert not FR.keeps(big, big + 1, 50) and FR.keeps(big + 1, big, 50)
    assert not FR.keeps(big, big, 51) and FR.keeps(big, big, 49)
    m = (1 << 64) - 1
    assert FR.keeps(m, m, 50) and not FR.keeps(m - 1, m, 50) and FR.keeps(m, 0, 100) and not FR.keeps(m, 1, 100)


def test_plan_is_the_scan_of_the_kept():
    fg = [0, 4, 3, 1 << 62, 9, 0]
    bg = [0, 4, 5, 1 << 62, 0, 2]
    action, offsets, count = FR.plan(fg, bg, 50)
    assert action.tolist() == [3, 0, 3, 0, 0, 3] and offsets.tolist() == [0, 0, 1, 1, 2, 3] and count == 3
    action, offsets, count = FR.plan(fg, bg, 100)
    assert action.tolist() == [3, 3, 3, 3, 0, 3] and offsets.tolist() == [0, 0, 0, 0, 0, 1] and count == 1
    assert FR.plan([0, 0], [1, 0], 1)[2] == 0


def test_votes_split_the_importance_sum():
    """a 20x18 image (2x2 tiles, the same two-entry list in each), two splats; the left columns background, a blank border: fg + bg = the sum under `valid`, a
    splat over background pixels alone votes background alone"""
    W, H, n = 20, 18, 2
    rec = np.zeros((n, 16))
    for i, (x, y, op) in enumerate([(3.3, 8.4, 0.8), (12.3, 8.4, 0.6)]):
        rec[i, S2D_X], rec[i, S2D_Y], rec[i, S2D_OPACITY] = x, y, op
        rec[i, S2D_CONIC], rec[i, S2D_CONIC + 2] = 0.5, 0.5
    ranges = np.array([[0, 2], [2, 4], [4, 6], [6, 8]], np.uint32)
    sorted_splat = np.array([0, 1] * 4, np.uint32)
    n_contrib = np.full((H, W), 2, np.uint32)
    fg = np.ones((H, W), np.float32); fg[:, :7] = 0
    valid = np.ones((H, W), np.float32); valid[:2] = 0; valid[:, -3:] = 0
    f, b, fh, bh, excl = FR.votes(rec, ranges, sorted_splat, n_contrib, W, H, n, 0, fg, valid)
    full = IR.importance(rec, ranges, sorted_splat, n_contrib, W, H, n, 0, mask=valid)
    assert np.allclose(f + b, full[0], rtol=0, atol=1e-12) and np.array_equal(fh + bh, full[2]) and not excl.any()
    assert b[0] > 10 * f[0] > 0 and f[1] > 10 * b[1] >= 0
    none = FR.votes(rec, ranges, sorted_splat, n_contrib, W, H, n, 0)
    unmasked = IR.importance(rec, ranges, sorted_splat, n_contrib, W, H, n, 0)
    assert np.array_equal(none[0], unmasked[0]) and not none[1].any() and not none[3].any()
