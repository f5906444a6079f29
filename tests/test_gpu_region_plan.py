"""dvs_region_plan against tests/region_ref.py.

Exact case: centres and an axis-aligned box on a 1/64 grid with the identity transform, so every fused multiply-add is exact: points on
faces, edges and corners stay, points one grid step outside go; n = 1, 63, 64, 65, 257 and 70001 (a partial block, one block, more than
one, and more than one 256-block chunk of the block scan: 70001 / 256 = 274 blocks), the array 16-byte aligned (16-byte loads for the
full blocks) and shifted by one float (the scalar path). action, offsets and new_count equal the reference exactly.
Rotated case: the box and the 70001 uniform centres of tests/test_region_abi.py (which shows on the reference alone that at most 1 % of
them lie within 1e-5 (hi - lo) of a face); those are left out, the action of every other splat matches exactly, and offsets and new_count
are the exclusive scan and the sum of the action the device itself wrote. All inside, all outside (new_count 0), NaN and
+-inf centres. The plan applied through dvs_densify_apply (modes 0 and 1, tiled shN) equals numpy's boolean compaction of all six arrays."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, region
import region_ref as RR
from test_region_abi import ROTATED, rotated_points

pytestmark = pytest.mark.gpu
KEEP, PRUNE = RR.KEEP, RR.PRUNE
LO, HI = (-0.5, -0.25, 0.0), (0.5, 0.75, 1.0)                               # multiples of 1/64


def identity_region(lo=LO, hi=HI):
    return region.region_from_trs((0, 0, 0), (0, 0, 0), (1, 1, 1), lo, hi)[0]


def grid_points(n):
    """n points on the 1/64 grid: the 27 face / edge / corner / centre combinations of the box first, each followed by its copy one grid
    step outside along every axis it touches, then random grid points around the box"""
    lo, hi, mid = np.array(LO), np.array(HI), (np.array(LO) + np.array(HI)) / 2
    special = []
    for ix in range(3):
        for iy in range(3):
            for iz in range(3):
                p = np.array([(lo, mid, hi)[i][k] for k, i in enumerate((ix, iy, iz))])
                special.append(p)
                for k, i in enumerate((ix, iy, iz)):
                    if i != 1:
                        q = p.copy(); q[k] += (-1 if i == 0 else 1) / 64.0
                        special.append(q)
    r = np.random.default_rng(n)
    rand = r.integers(-64, 97, (max(n, len(special)), 3)) / 64.0
    pts = np.concatenate([np.array(special), rand])[:n] if n >= len(special) else np.array(special)[r.permutation(len(special))[:n]]
    return np.ascontiguousarray(pts, np.float32)


def run_plan(dev, pts, reg, shift=0):
    buf = torch.zeros(pts.size + 8, dtype=torch.float32, device=dev)
    view = buf[shift:shift + pts.size]
    view.copy_(torch.from_numpy(pts.reshape(-1)))
    assert (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    action, offsets, count = region.region_plan(view, reg)
    return action.cpu().numpy(), offsets.cpu().numpy().view(np.uint32), count


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 70001])
def test_exact_case_equals_the_reference(gpu_device, n, shift):
    pts, reg = grid_points(n), identity_region()
    want_action, want_offsets, want_count, _ = RR.plan(pts, list(reg.w2b), LO, HI)
    got_action, got_offsets, got_count = run_plan(gpu_device, pts, reg, shift)
    assert np.array_equal(got_action, want_action)
    assert np.array_equal(got_offsets, want_offsets) and got_count == want_count
    if n >= 257:
        assert 0 < want_count < n
        on_face = ((pts == np.array(LO, np.float32)) | (pts == np.array(HI, np.float32))).any(1) & (want_action == KEEP)
        assert on_face.sum() >= 26                              # the faces, edges and corners themselves are kept


def test_rotated_case_matches_outside_the_band(gpu_device):
    pts = rotated_points()
    reg, _ = region.region_from_trs(ROTATED["pos"], ROTATED["rot"], ROTATED["scale"], ROTATED["lo"], ROTATED["hi"])
    want_action, _, _, near = RR.plan(pts, list(reg.w2b), ROTATED["lo"], ROTATED["hi"], ROTATED["band"])
    got_action, got_offsets, got_count = run_plan(gpu_device, pts, reg)
    assert near.mean() <= 0.01
    assert np.array_equal(got_action[~near], want_action[~near])
    kept = (got_action == KEEP).astype(np.int64)                # offsets and count: the scan of the action the device itself wrote
    assert np.array_equal(got_offsets, (np.cumsum(kept) - kept).astype(np.uint32)) and got_count == kept.sum()
    assert set(np.unique(got_action)) == {KEEP, PRUNE}


def test_edge_cases(gpu_device):
    n = 70001
    pts = np.random.default_rng(1).uniform(-1, 1, (n, 3)).astype(np.float32)
    a, o, c = run_plan(gpu_device, pts, identity_region((-2, -2, -2), (2, 2, 2)))                  # all inside
    assert c == n and (a == KEEP).all() and np.array_equal(o, np.arange(n, dtype=np.uint32))
    a, o, c = run_plan(gpu_device, pts, identity_region((5, 5, 5), (6, 6, 6)))                     # all outside
    assert c == 0 and (a == PRUNE).all() and (o == 0).all()
    bad = pts.copy()
    rows = np.arange(0, n, 97)
    for j, i in enumerate(rows):
        bad[i, (j // 3) % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    reg, _ = region.region_from_trs((0.1, 0, 0), (0.3, 0.2, 0.1), (1, 1, 1), (-2, -2, -2), (2, 2, 2))     # rotated: a bad coordinate reaches every row
    a, o, c = run_plan(gpu_device, bad, reg)
    assert (a[rows] == PRUNE).all()
    good = np.ones(n, bool); good[rows] = False
    assert (a[good] == KEEP).all() and c == good.sum()


def test_apply_compacts_all_six_arrays(gpu_device):
    """modes 0 and 1 of dvs_densify_apply from the region's plan, shN in the tiled layout: the kept rows, in order"""
    n = 70001
    r = np.random.default_rng(11)
    widths = (3, 3, 45, 1, 3, 4)
    A = [np.ascontiguousarray(r.normal(size=(n, w)), np.float32) for w in widths]
    A[0] = np.ascontiguousarray(r.uniform(-1, 1, (n, 3)), np.float32)
    reg = identity_region((-0.5, -0.75, -1.0), (0.5, 0.25, 0.9))
    want_action, _, want_count, _ = RR.plan(A[0], list(reg.w2b), (-0.5, -0.75, -1.0), (0.5, 0.25, 0.9))
    keep = want_action == KEEP

    def tiled(rows, count):                                     # [count,45] -> DVS_SHN_TILED [ceil(count/64)][12][64][4]
        t = np.zeros(((count + 63) // 64, 12, 64, 4), np.float32)
        i = np.arange(count)
        for e in range(45):
            t[i >> 6, e >> 2, i & 63, e & 3] = rows[:, e]
        return t
    dev = gpu_device
    src = [torch.from_numpy(tiled(a, n) if k == 2 else a).to(dev).contiguous() for k, a in enumerate(A)]
    action, offsets, count = region.region_plan(src[0].reshape(-1), reg)
    assert count == want_count and 0 < count < n
    prm = _lib.DensifyParams(shn_layout=1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in (0, 1):
        dst = [torch.zeros(((count + 63) // 64) * 64 * 48 if k == 2 else count * w, dtype=torch.float32, device=dev) for k, w in enumerate(widths)]
        sp = (C.c_void_p * 6)(*[t.data_ptr() for t in src]); dp = (C.c_void_p * 6)(*[t.data_ptr() for t in dst])
        _lib.check(dv.lib.dvs_densify_apply(st, n, action.data_ptr(), offsets.data_ptr(), C.byref(prm), mode, sp, dp, count), "dvs_densify_apply")
        torch.cuda.synchronize()
        for k, w in enumerate(widths):
            got = dst[k].cpu().numpy()
            want = tiled(A[k][keep], count).reshape(-1) if k == 2 else A[k][keep].reshape(-1)
            assert np.array_equal(got, want), (mode, k)


def test_invalid_arguments_are_refused(gpu_device):
    reg = identity_region()
    pos = torch.zeros(30, dtype=torch.float32, device=gpu_device)
    a = torch.zeros(16, dtype=torch.uint8, device=gpu_device); o = torch.zeros(16, dtype=torch.int32, device=gpu_device)
    s = torch.zeros(16, dtype=torch.int32, device=gpu_device); c = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    f = dv.lib.dvs_region_plan
    assert f(None, 0, pos.data_ptr(), C.byref(reg), a.data_ptr(), o.data_ptr(), s.data_ptr(), c.data_ptr()) == 1
    assert f(None, 10, None, C.byref(reg), a.data_ptr(), o.data_ptr(), s.data_ptr(), c.data_ptr()) == 1
    assert f(None, 10, pos.data_ptr(), None, a.data_ptr(), o.data_ptr(), s.data_ptr(), c.data_ptr()) == 1
    assert f(None, 10, pos.data_ptr(), C.byref(reg), a.data_ptr(), o.data_ptr(), s.data_ptr(), c.data_ptr() + 4) == 1
