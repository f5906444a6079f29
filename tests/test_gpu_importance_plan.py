"""dvs_importance_plan against numpy on integer keys (no tolerance): the pruned splats are the n - min(keep, n) first of
np.lexsort((-index, score)) — smallest score, among equal scores the larger index first. Sizes 1, 255, 257 and 70001 (no multiple of 256,
more than one histogram block, more than one chunk of the block scan: 70001 / 256 = 274 blocks); scores all zero, all equal, differing
only in the high or only in the low 32 bits, heavy ties straddling the cut; keep = n, 1 and > n. action, offsets (exclusive scan of the
kept) and new_count are checked, and dvs_densify_apply mode 0 on them yields the kept rows in order.

The hidden-splat test is what the feature exists for: an opaque wall and, strictly behind it in both views, a cluster of opaque splats.
Their hits are 0; planning with keep = the number of splats with a non-zero score, applying and rendering again gives bit-identical
views — while their activated opacity is far above pruneOpacity, so the opacity-threshold prune would have kept them."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, prune
from divshot_amd.raster import Rasterizer, params_to_device

pytestmark = pytest.mark.gpu
KEEP, PRUNE = 0, 3


def scores(kind, n):
    r = np.random.default_rng(n + len(kind))
    if kind == "random":
        return r.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)      # all 64 bits in use
    if kind == "zero":
        return np.zeros(n, np.uint64)
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if kind == "high":
        return r.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32) | np.uint64(0x9E3779B1)
    if kind == "low":
        return np.uint64(0x7F4A7C15) << np.uint64(32) | r.integers(0, 1 << 32, n, dtype=np.uint64)
    if kind == "ties":                    # four values, about a quarter of the splats each: every cut but a few falls inside a tie group
        return np.array([0, 5, 5 << 40, (5 << 40) + 1], np.uint64)[r.integers(0, 4, n)]
    raise ValueError(kind)


def expected(score, keep):
    n = score.size
    order = np.lexsort((-np.arange(n, dtype=np.int64), score))
    action = np.full(n, KEEP, np.uint8)
    action[order[:n - min(keep, n)]] = PRUNE
    kept = (action == KEEP).astype(np.int64)
    return action, (np.cumsum(kept) - kept).astype(np.uint32), min(keep, n)


CASES = [("random", 1, 1), ("random", 255, 100), ("random", 257, 129), ("random", 70001, 49001), ("zero", 70001, 30000), ("zero", 257, 1),
         ("equal", 70001, 256), ("equal", 255, 254), ("high", 70001, 35000), ("low", 70001, 35000), ("ties", 70001, 26000), ("ties", 70001, 61000),
         ("ties", 257, 100), ("random", 70001, 70001), ("ties", 70001, 1), ("random", 257, 1), ("ties", 255, 1000), ("random", 70001, 1 << 31)]


@pytest.mark.parametrize("kind,n,keep", CASES)
def test_plan_equals_numpy(gpu_device, kind, n, keep):
    sc = scores(kind, n)
    want_action, want_offsets, want_count = expected(sc, keep)
    d = torch.from_numpy(sc.view(np.int64)).to(gpu_device)
    action, offsets, count = prune.importance_plan(d, keep)
    got_action, got_offsets = action.cpu().numpy(), offsets.cpu().numpy().view(np.uint32)
    assert count == want_count and int((got_action == KEEP).sum()) == want_count
    assert np.array_equal(got_action, want_action)
    assert np.array_equal(got_offsets[got_action == KEEP], want_offsets[want_action == KEEP])
    assert np.array_equal(got_offsets, want_offsets)
    if kind == "ties" and 1 < keep < n:
        cut_value = np.sort(sc)[n - keep]
        group = got_action[sc == cut_value]
        assert (group == KEEP).any() and (group == PRUNE).any(), "the cut does not straddle a tie group"
        assert (np.diff((group == PRUNE).astype(np.int8)) >= 0).all()           # inside the group: the kept ones first, the larger indices go


def apply_rows(dev, P, action, offsets, n, new_n):
    """dvs_densify_apply mode 0 (row layout) of the six arrays -> dict of new device tensors"""
    keys, width = ("pos", "sh0", "shN", "opacity", "scale", "rot"), (3, 3, 45, 1, 3, 4)
    dst = {k: torch.full((new_n * w,), 9.0, device=dev) for k, w in zip(keys, width)}
    prm = _lib.DensifyParams(shn_layout=0)
    sp = (C.c_void_p * 6)(*[P[k].data_ptr() for k in keys]); dp = (C.c_void_p * 6)(*[dst[k].data_ptr() for k in keys])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(dv.lib.dvs_densify_apply(st, n, action.data_ptr(), offsets.data_ptr(), C.byref(prm), 0, sp, dp, new_n), "dvs_densify_apply")
    torch.cuda.synchronize()
    return dst


def test_apply_compacts_the_kept_rows_in_order(gpu_device):
    n, keep = 70001, 41234
    r = np.random.default_rng(5)
    A = {"pos": r.normal(size=(n, 3)), "sh0": r.normal(size=(n, 3)), "shN": r.normal(size=(n, 15, 3)), "opacity": r.normal(size=(n,)),
         "scale": r.normal(size=(n, 3)), "rot": r.normal(size=(n, 4))}
    A = {k: np.ascontiguousarray(v, np.float32) for k, v in A.items()}
    P = params_to_device(A, gpu_device)
    sc = scores("ties", n)
    action, offsets, count = prune.importance_plan(torch.from_numpy(sc.view(np.int64)).to(gpu_device), keep)
    assert count == keep
    out = apply_rows(gpu_device, P, action, offsets, n, keep)
    rows = np.where(expected(sc, keep)[0] == KEEP)[0]
    for k, v in A.items():
        assert np.array_equal(out[k].cpu().numpy().reshape((keep,) + v.shape[1:]), v[rows]), k


# ---- hidden splats -----------------------------------------------------------------------------------------------------------------
HW, HH = 50, 37
PRUNE_OPACITY = 0.005          # GaussianTrainConfig::pruneOpacity


def hidden_scene():
    """four layers of an opaque wall at z = 3.0 .. 3.15 (centres every 4 pixels, sigma 0.3 = 4.3 pixels, reaching 8 pixels past the image),
    then 40 opaque splats around the optical axis at z = 6 .. 7 — behind the wall for both cameras"""
    fx = HW / (2 * np.tan(np.radians(30.0)))
    gx, gy = np.meshgrid(np.arange(-8.0, HW + 8.5, 4.0), np.arange(-8.0, HH + 8.5, 4.0))
    wall = []
    for z in (3.0, 3.05, 3.1, 3.15):
        wall.append(np.stack([(gx.ravel() - (HW - 1) / 2) * z / fx, (gy.ravel() - (HH - 1) / 2) * z / fx, np.full(gx.size, z)], 1))
    wall = np.concatenate(wall)
    r = np.random.default_rng(3)
    cluster = np.stack([r.uniform(-0.8, 0.8, 40), r.uniform(-0.5, 0.5, 40), r.uniform(6.0, 7.0, 40)], 1)
    nw, n = len(wall), len(wall) + 40
    rot = np.zeros((n, 4)); rot[:, 0] = 1
    P = {"pos": np.concatenate([wall, cluster]), "sh0": r.normal(0, 1, (n, 3)), "shN": np.zeros((n, 15, 3)),
         "opacity": np.concatenate([np.full(nw, 8.0), np.full(40, 3.0)]),
         "scale": np.log(np.concatenate([np.full((nw, 3), 0.3), np.full((40, 3), 0.15)])), "rot": rot}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}, nw


def hidden_cameras():
    cams = []
    for tx in (0.0, 0.08):
        cam = dv.Camera()
        R = np.eye(3, dtype=np.float32); t = np.array([tx, -0.02 * (tx > 0), 0.0], np.float32)
        _lib.check(dv.lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, 60.0, HW, HH, C.byref(cam)), "dvs_make_camera")
        cams.append(cam)
    return cams


def test_splats_hidden_behind_a_wall_go_and_the_views_do_not_change(gpu_device):
    A, nw = hidden_scene()
    n = A["pos"].shape[0]
    P = params_to_device(A, gpu_device)
    cams = hidden_cameras()
    r = Rasterizer(0, max_splats=2048, max_w=HW, max_h=HH, max_views=2)
    before = r.forward_views(P, cams, sh_degree=0).clone()
    s, m, h = prune.importance_scores(r)
    s_np, h_np = s.cpu().numpy(), h.cpu().numpy()
    assert (h_np[nw:] == 0).all() and (s_np[nw:] == 0).all(), "a pixel took a splat of the hidden cluster"
    assert ((s_np == 0) == (h_np == 0)).all()
    assert (1.0 / (1.0 + np.exp(-A["opacity"][nw:].astype(np.float64))) > PRUNE_OPACITY).all()      # the light prune's rule keeps every one of them
    keep = int((s_np != 0).sum())
    assert 0 < keep <= nw
    action, offsets, count = prune.importance_plan(s, keep)
    assert count == keep and (action.cpu().numpy()[nw:] == PRUNE).all()
    assert np.array_equal(action.cpu().numpy() == KEEP, s_np != 0)
    Q = apply_rows(gpu_device, P, action, offsets, n, keep)
    Q = {k: v.reshape((keep,) + tuple(P[k].shape[1:])) for k, v in Q.items()}
    after = r.forward_views(Q, cams, sh_degree=0)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert float(before.std()) > 0.05                           # pictures, not flat fields
    r.close()
