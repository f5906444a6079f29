"""dvs_foreground_plan against the Python-integer rule of tests/foreground_ref.py (no tolerance): action, offsets (the exclusive scan of
the kept) and new_count. Sizes 1, 255, 256, 257 and 70001 (a single splat, a block less one, a full block, a block and one, and 274
blocks: more than one 256-block chunk of the block-sum scan, so its running carry is exercised); thresholds 1, 50, 100. The votes
are random 64-bit values over the whole range with a share of zeros (fg alone, bg alone, both), exact ties fg (100 - T) == bg T —
some of them with products far beyond 64 bits — their neighbours one unit to either side, and values near 2^62, where both products
wrap in 64 bits. A plan that keeps nothing returns new_count = 0."""
import numpy as np
import pytest
import torch
from divshot_amd import prune
import foreground_ref as FR

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def votes(n, T):
    r = np.random.default_rng(1000 * T + n)
    fg = [int(v) for v in r.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)]
    bg = [int(v) for v in r.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)]
    kind = r.integers(0, 10, n)
    for i in range(n):
        k = int(kind[i])
        if k == 0: fg[i] = 0
        elif k == 1: bg[i] = 0
        elif k == 2: fg[i] = bg[i] = 0
        elif k in (3, 4, 5):            # a tie fg (100 - T) == bg T (fg = m T, bg = m (100 - T)), and at 4 / 5 one unit to either side of it
            m = int(r.integers(1, M64 // 100)) if i % 2 else int(r.integers(1, 1000))
            fg[i], bg[i] = m * T, m * (100 - T)
            if k == 4: fg[i] = max(fg[i] - 1, 0)
            if k == 5: bg[i] = max(bg[i] - 1, 0)
        elif k == 6:                    # near 2^62: both products wrap in 64 bits
            fg[i] = (1 << 62) + int(r.integers(-3, 4)); bg[i] = ((1 << 62) if i % 2 else (1 << 63)) + int(r.integers(-3, 4))
    return fg, bg


def run(gpu_device, fg, bg, T):
    as_dev = lambda v: torch.from_numpy(np.array(v, np.uint64).view(np.int64)).to(gpu_device)
    action, offsets, count = prune.foreground_plan(as_dev(fg), as_dev(bg), T)
    return action.cpu().numpy(), offsets.cpu().numpy().view(np.uint32), count


@pytest.mark.parametrize("T", [1, 50, 100])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_plan_equals_the_integer_rule(gpu_device, n, T):
    fg, bg = votes(n, T)
    want_action, want_offsets, want_count = FR.plan(fg, bg, T)
    got_action, got_offsets, got_count = run(gpu_device, fg, bg, T)
    assert got_count == want_count
    assert np.array_equal(got_action, want_action)
    assert np.array_equal(got_offsets, want_offsets)
    if n >= 255:
        assert 0 < want_count < n                                           # both outcomes occur


def test_hand_cases_on_the_device(gpu_device):
    big = 1 << 62
    cases = [(0, 0, 50), (0, 7, 1), (1, 0, 100), (5, 5, 50), (5, 6, 50), (10 ** 9, 1, 100), (big, big, 50), (big, big + 1, 50), (big, 2 * big, 50),
             (big, big, 80), (big, big, 20), (M64, M64, 50), (M64 - 1, M64, 50), (M64, 1, 100), (M64, 0, 100)]
    for T in sorted({c[2] for c in cases}):
        fg = [c[0] for c in cases if c[2] == T]; bg = [c[1] for c in cases if c[2] == T]
        want = FR.plan(fg, bg, T)
        got = run(gpu_device, fg, bg, T)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], T


@pytest.mark.parametrize("n", [1, 70001])
def test_a_plan_that_keeps_nothing(gpu_device, n):
    r = np.random.default_rng(n)
    fg = [0] * n if n == 1 else [int(v) for v in r.integers(0, 100, n)]
    bg = [int(v) for v in r.integers(1 << 40, 1 << 41, n)]
    action, offsets, count = run(gpu_device, fg, bg, 50)
    assert count == 0 and (action == FR.PRUNE).all() and not offsets.any()
