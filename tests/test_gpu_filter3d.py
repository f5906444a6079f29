"""The 3D smoothing filter's kernels (divshot_amd/csrc/filter3d.hip) through the C-ABI against tests/filter3d_ref.py in float64.

compute: 1000 splats (a multiple of neither 64 nor 256: four workgroups, the last one partial) under 1, 3, 64, 65 and 130 cameras — below,
at and across the seam of the 64-camera LDS batch. The rig: cameras in lanes 10 apart along x looking down +z with a little yaw and roll,
several per lane at different depths and focal lengths (so the minimum over the seeing cameras is a real choice), the LAST camera alone in
a lane of its own at x = -50 (when there is more than one) and, past 64 cameras, camera 63 (the last of the first batch) alone at x = -100. The splats: random ones in
front of the rig, plus splats behind every camera, outside every frustum, in each of the two lonely lanes, and one NaN position. They are
drawn by rejection so that no (splat, camera) pair lies within a relative 1e-3 of any of the three visibility bounds, which the test
asserts before it compares anything: seen / unseen must then agree exactly and no case is left out.

apply / chain: log-scales in [-8, 2], logits in [-12, 12], filters 0, far below (1e-3 x), comparable to and far above (100 x) the largest
scale; the whole array and the range (256, 300) over sentinel-filled outputs; rows with a zero filter bit for bit.

Tolerance: not a constant. Every comparison is e = |x - ref64| / max(|ref64|, 1) and the bar is 4 x the largest e of the SAME formulas
evaluated in numpy float32 (filter3d_ref with dtype float32) on the same inputs: numpy rounds every operation, the device's exp / log
are a few ulp looser. Printed by each test. Measured on an MI355X (device / float32 restatement, the bar being 4 x the latter):
  compute, 1 / 3 / 64 / 65 / 130 cameras   7.1e-9 / 8.4e-9 / 6.9e-9 / 7.9e-9 / 8.9e-9, the device's figure and the restatement's alike
                                             (the filters are ~0.01 .. 0.07: one float32 ulp)
  apply    scale_eff   1.53e-7 / 1.09e-7     opacity_eff  3.27e-7 / 2.52e-7
  chain    g_scale     2.83e-7 / 2.83e-7     g_opacity    1.21e-7 / 1.21e-7
"""
import ctypes as C
import numpy as np
import pytest
import filter3d_ref as F

pytestmark = pytest.mark.gpu
N = 1000
BATCH = 64


def _camera(pos, yaw, roll, focal, w=64, h=48):
    from divshot_amd._lib import Camera
    cy, sy, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    R = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])      # world -> camera
    t = -R @ np.asarray(pos, np.float64)
    cam = Camera()
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    cam.view[:] = [float(np.float32(v)) for v in M.T.reshape(16)]              # view[c*4+r]
    cam.focal_x, cam.focal_y, cam.width, cam.height = float(focal), float(focal), w, h
    return cam


def _rig(n_cams):
    cams = []
    for c in range(n_cams):
        lane, depth = c % 8, c // 8
        cams.append(_camera((10.0 * lane, 0.0, -0.3 * depth), 0.04 * ((c % 5) - 2), 0.1 * ((c % 3) - 1), 80.0 + 3.0 * c))
    if n_cams > 1:
        cams[-1] = _camera((-50.0, 0.0, 0.0), 0.03, -0.2, 90.0)
    if n_cams > BATCH:
        cams[BATCH - 1] = _camera((-100.0, 0.0, 0.0), -0.03, 0.2, 70.0)
    return cams


def _splats(rows, seed):
    """-> pos [N,3] float32 with the special splats at known rows, the margin asserted"""
    rng = np.random.default_rng(seed)
    m = 6 * N
    cand = np.stack([rng.uniform(-5, 75, m), rng.uniform(-4, 4, m), rng.uniform(-2, 12, m)], 1)
    special = np.array([[20, 0, -30], [35, 1.5, -9],                           # behind every camera
                        [20, 300, 3], [-300, 0, 2],                            # outside every frustum
                        [-50.2, 0.1, 3], [-49.5, -0.3, 6],                     # the last camera's lane
                        [-100.3, 0.2, 2.5], [-99.8, -0.1, 5]])                 # camera 63's lane (past 64 cameras; seen by nobody below)
    allp = np.concatenate([special, cand]).astype(np.float32)
    ok = np.ones(allp.shape[0], bool)
    for q, b in F.visibility_terms(allp, rows):
        with np.errstate(all="ignore"):
            ok &= ~(np.abs(q - b) <= 1e-3 * np.abs(b)).any(axis=0)
    assert ok[:special.shape[0]].all(), "a special splat sits on a visibility bound: move it"
    pos = allp[ok][:N - 1]
    assert pos.shape[0] == N - 1
    pos = np.concatenate([pos[:500], np.array([[np.nan, 0, 3]], np.float32), pos[500:]])      # the NaN position in the second workgroup
    for q, b in F.visibility_terms(pos, rows):                                # the margin itself, on what is compared: no pair is left out
        with np.errstate(all="ignore"):
            rel = np.abs(q - b) / np.abs(b)
        assert not (rel[:, np.isfinite(pos).all(1)] <= 1e-3).any()
    return np.ascontiguousarray(pos)


def _scaled(x, ref):
    return float((np.abs(np.asarray(x, np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max())


@pytest.mark.parametrize("n_cams", [1, 3, 64, 65, 130])
def test_compute_matches_the_reference(gpu_device, n_cams):
    import torch
    from divshot_amd import filter3d
    cams = _rig(n_cams)
    rows = filter3d.pack_cameras(cams)
    assert np.array_equal(rows, F.pack_cameras(cams)), "dvs_filter3d_pack_cameras differs from the restatement"
    pos = _splats(rows, 100 + n_cams)
    ref, seen = F.compute(pos, rows)
    ref32, seen32 = F.compute(pos, rows, np.float32)
    assert np.array_equal(seen, seen32) and 40 < seen.sum() < N - 8
    # what the set holds: behind, outside, the lonely lanes (with the cameras that sit in them), the NaN
    assert not seen[:4].any() and not seen[500] and seen[4:6].all() == (n_cams > 1) and seen[6:8].all() == (n_cams > BATCH)
    assert seen[4:6].any() == seen[4:6].all() and seen[6:8].any() == seen[6:8].all()
    if n_cams > 1:
        last_only = F.compute(pos, rows[:-1])[1]
        assert not last_only[4:6].any(), "the last camera's lane is seen by another camera"
    got, info = filter3d.compute(torch.from_numpy(pos).to(gpu_device), cams)
    got = got.cpu().numpy()
    assert info["n_seen"] == int(seen.sum())
    gmax = np.float32(info["max"])
    assert gmax == got[seen].max() and np.array_equal(got[~seen], np.full(int((~seen).sum()), gmax)), "an unseen splat does not carry the maximum"
    assert np.all(got[seen] <= gmax) and (got[seen] < gmax).sum() >= seen.sum() - 1     # (a wrongly unseen splat would carry the maximum)
    e_dev, e_32 = _scaled(got, ref), _scaled(ref32, ref)
    print(f"compute {n_cams} cameras: device {e_dev:.3g}, float32 restatement {e_32:.3g}, bar {4 * e_32:.3g}")
    assert e_dev <= 4 * e_32


def test_compute_when_no_camera_sees_anything(gpu_device):
    import torch
    from divshot_amd import filter3d
    cams = _rig(65)
    rng = np.random.default_rng(5)
    pos = np.stack([rng.uniform(-5, 75, N), rng.uniform(-4, 4, N), rng.uniform(-30, -5, N)], 1).astype(np.float32)      # behind every camera
    assert not F.compute(pos, F.pack_cameras(cams))[1].any()
    got, info = filter3d.compute(torch.from_numpy(pos).to(gpu_device), cams)
    assert info == {"max": 0.0, "n_seen": 0} and np.array_equal(got.cpu().numpy().view(np.uint32), np.zeros(N, np.uint32))


def _apply_inputs():
    rng = np.random.default_rng(11)
    scale = rng.uniform(-8, 2, (N, 3)).astype(np.float32)
    opacity = rng.uniform(-12, 12, N).astype(np.float32)
    s = np.exp(scale.max(1).astype(np.float64))
    kind = rng.integers(0, 4, N)                                                # every kind in every workgroup and in the range
    filt = np.where(kind == 0, 0.0, np.where(kind == 1, 1e-3 * s, np.where(kind == 2, s * rng.uniform(0.5, 2, N), 1e2 * s))).astype(np.float32)
    assert all((kind[256:556] == k).sum() > 40 for k in range(4))
    return scale, opacity, filt, rng


def test_apply_whole_and_range(gpu_device):
    import torch
    from divshot_amd import filter3d
    scale, opacity, filt, _ = _apply_inputs()
    d = lambda a: torch.from_numpy(a).to(gpu_device)
    rs, ro = F.apply(scale, opacity, filt)
    rs32, ro32 = F.apply(scale, opacity, filt, np.float32)
    se, oe = filter3d.apply(d(scale), d(opacity), d(filt))
    se, oe = se.cpu().numpy(), oe.cpu().numpy()
    off = filt == 0
    assert np.array_equal(se[off].view(np.uint32), scale[off].view(np.uint32)) and np.array_equal(oe[off].view(np.uint32), opacity[off].view(np.uint32))
    assert np.all(np.isfinite(se)) and np.all(np.isfinite(oe)) and np.all(oe[~off] < opacity[~off]) and np.all(se[~off] >= scale[~off])
    for name, got, ref, r32 in (("scale_eff", se, rs, rs32), ("opacity_eff", oe, ro, ro32)):
        e_dev, e_32 = _scaled(got, ref), _scaled(r32, ref)
        print(f"apply {name}: device {e_dev:.3g}, float32 restatement {e_32:.3g}, bar {4 * e_32:.3g}")
        assert e_dev <= 4 * e_32, name
    # the range form: rows 256 .. 555 as in the whole-array call, every other row's sentinel untouched
    out = (torch.full((N, 3), -777.0, device=gpu_device), torch.full((N,), -777.0, device=gpu_device))
    filter3d.apply(d(scale), d(opacity), d(filt), first=256, count=300, out=out)
    ps, po = out[0].cpu().numpy(), out[1].cpu().numpy()
    inside = np.zeros(N, bool); inside[256:556] = True
    assert np.array_equal(ps[inside].view(np.uint32), se[inside].view(np.uint32)) and np.array_equal(po[inside].view(np.uint32), oe[inside].view(np.uint32))
    assert np.all(ps[~inside] == -777.0) and np.all(po[~inside] == -777.0)


def test_chain_whole_and_range(gpu_device):
    import torch
    from divshot_amd import filter3d
    scale, opacity, filt, rng = _apply_inputs()
    gs, go = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    d = lambda a: torch.from_numpy(a.copy()).to(gpu_device)
    rs, ro = F.chain(scale, opacity, filt, gs, go)
    rs32, ro32 = F.chain(scale, opacity, filt, gs, go, np.float32)
    cs, co = filter3d.chain(d(scale), d(opacity), d(filt), d(gs), d(go))
    cs, co = cs.cpu().numpy(), co.cpu().numpy()
    off = filt == 0
    assert np.array_equal(cs[off].view(np.uint32), gs[off].view(np.uint32)) and np.array_equal(co[off].view(np.uint32), go[off].view(np.uint32))
    for name, got, ref, r32 in (("g_scale", cs, rs, rs32), ("g_opacity", co, ro, ro32)):
        e_dev, e_32 = _scaled(got, ref), _scaled(r32, ref)
        print(f"chain {name}: device {e_dev:.3g}, float32 restatement {e_32:.3g}, bar {4 * e_32:.3g}")
        assert e_dev <= 4 * e_32, name
    ps, po = filter3d.chain(d(scale), d(opacity), d(filt), d(gs), d(go), first=256, count=300)
    ps, po = ps.cpu().numpy(), po.cpu().numpy()
    inside = np.zeros(N, bool); inside[256:556] = True
    assert np.array_equal(ps[inside].view(np.uint32), cs[inside].view(np.uint32)) and np.array_equal(po[inside].view(np.uint32), co[inside].view(np.uint32))
    assert np.array_equal(ps[~inside].view(np.uint32), gs[~inside].view(np.uint32)) and np.array_equal(po[~inside].view(np.uint32), go[~inside].view(np.uint32))


def test_bad_arguments_are_refused(gpu_device):
    import torch
    from divshot_amd._lib import lib
    t = torch.zeros(64, device=gpu_device)
    p = t.data_ptr()
    assert lib.dvs_filter3d_apply_range(None, 16, 8, 9, p, p, p, p, p) == 1      # a range past n
    assert lib.dvs_filter3d_apply_range(None, 16, 0, 16, p, p + 4, p, p, p) == 1  # a misaligned array
    assert lib.dvs_filter3d_chain_range(None, 16, -1, 4, p, p, p, p, p) == 1 and lib.dvs_filter3d_chain(None, 16, p, p, None, p, p) == 1
    assert lib.dvs_filter3d_compute(None, 16, p, p, 0, p, p) == 1 and lib.dvs_filter3d_compute(None, 16, p, None, 1, p, p) == 1
    assert lib.dvs_filter3d_pack_cameras(None, 1, p) == 1
