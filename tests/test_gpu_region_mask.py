"""dvs_region_mask_views against tests/region_ref.py: out = in * hit, exactly, for every pixel whose float64 slab interval is not narrower
than a relative 1e-5 (rays that graze an edge or a corner; at most 2 % of a view, asserted on the reference).

Sizes 16x16, 64x48 (16-byte path) and 33x17 (odd: the scalar path), and 64x48 with the arrays shifted by one float (the scalar path by
alignment); 1, 3 and 16 views of a ring of cameras with different yaws; with and without an input mask of random values in [0, 1].
Geometries: a rotated, scaled box in front of the cameras that covers part of the image; the cameras inside the box (all ones); the box
behind them (all zeros); a slab that every ray crosses (all ones); and at 33x17, whose centre column has ndc_x = 0 exactly, one camera
with the identity pose looking down the z axis of an axis-aligned box, so that the centre column's local x direction is exactly 0: with
the origin inside the x slab (the column hits), outside it (the column misses while its neighbour hits) and exactly ON its face (lo - o
= 0 over l = 0 would be NaN: the column hits). A view's result does not depend on which other views share the call."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib, region
import region_ref as RR

pytestmark = pytest.mark.gpu
FOV = 60.0
GEOMETRIES = {
    #            pos, rot, scale, lo, hi
    "front": ((0.1, 0.0, 0.2), (0.2, -0.3, 0.1), (1.0, 1.2, 0.8), (-0.3, -0.2, 2.5), (0.6, 0.4, 3.5)),
    "inside": ((0, 0, 0), (0.3, 0.2, -0.4), (1, 1, 1), (-5, -5, -5), (5, 5, 5)),
    "behind": ((0, 0, 0), (0, 0, 0), (1, 1, 1), (-1, -1, -3), (1, 1, -2)),
    "covers": ((0, 0, 0), (0, 0, 0), (1, 1, 1), (-100, -100, 1), (100, 100, 2)),
}
AXIS = {
    "axis_inside": ((-0.25, -0.3, 2.0), (0.5, 0.3, 3.0)),
    "axis_outside": ((0.25, -0.3, 2.0), (0.75, 0.3, 3.0)),
    "axis_on_face": ((0.0, -0.3, 2.0), (0.5, 0.3, 3.0)),
}


def make_camera(k, W, H):
    """camera k of the ring: centre on a circle of radius 0.3 in the z = 0 plane, yaw between -0.3 and 0.3 rad; camera 0 has the identity pose"""
    yaw = 0.0 if k == 0 else 0.3 * np.sin(1.7 * k)
    centre = np.zeros(3) if k == 0 else np.array([0.3 * np.cos(0.9 * k), 0.3 * np.sin(0.9 * k), 0.0])
    R = np.array([[np.cos(yaw), 0, -np.sin(yaw)], [0, 1, 0], [np.sin(yaw), 0, np.cos(yaw)]], np.float32)
    t = (-R.astype(np.float64) @ centre).astype(np.float32)
    cam = dv.Camera()
    _lib.check(dv.lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, FOV, W, H, C.byref(cam)), "dvs_make_camera")
    return cam


def make_region(name):
    if name in AXIS:
        lo, hi = AXIS[name]
        return region.region_from_trs((0, 0, 0), (0, 0, 0), (1, 1, 1), lo, hi)[0]
    pos, rot, scale, lo, hi = GEOMETRIES[name]
    return region.region_from_trs(pos, rot, scale, lo, hi)[0]


@functools.lru_cache(maxsize=None)
def reference(name, k, W, H):
    reg = make_region(name)
    hit, near = RR.mask(make_camera(k, W, H), list(reg.w2b), list(reg.lo), list(reg.hi), W, H)
    hit.setflags(write=False); near.setflags(write=False)
    return hit, near


def run(dev, name, ks, W, H, with_mask, shift=0):
    P = W * H
    cams = [make_camera(k, W, H) for k in ks]
    r = np.random.default_rng(W * 1000 + H + len(ks))
    ins = [r.uniform(0, 1, P).astype(np.float32) for _ in ks] if with_mask else None
    bufs = [torch.full((P + 8,), -7.0, dtype=torch.float32, device=dev) for _ in ks]
    outs = [b[shift:shift + P] for b in bufs]
    d_in = None
    if with_mask:
        d_in = []
        for m in ins:
            b = torch.zeros(P + 8, dtype=torch.float32, device=dev)
            b[shift:shift + P].copy_(torch.from_numpy(m))
            d_in.append(b[shift:shift + P])
    region.region_mask_views(cams, make_region(name), outs, d_in)
    torch.cuda.synchronize()
    for b in bufs:                                              # nothing outside the image was written
        assert (b[:shift].cpu().numpy() == -7.0).all() and (b[shift + P:].cpu().numpy() == -7.0).all()
    return [o.cpu().numpy().reshape(H, W) for o in outs], [m.reshape(H, W) for m in ins] if with_mask else None


def check(name, ks, W, H, got, ins):
    for j, k in enumerate(ks):
        hit, near = reference(name, k, W, H)
        assert near.mean() <= 0.02, (name, k, near.mean())
        want = hit if ins is None else ins[j] * hit
        assert np.array_equal(got[j][~near], want[~near]), (name, k, int((got[j] != want)[~near].sum()))
        assert set(np.unique(got[j])) <= {0.0, 1.0} or ins is not None


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("W,H,n_views,shift", [(16, 16, 1, 0), (16, 16, 3, 0), (33, 17, 3, 0), (33, 17, 16, 0), (64, 48, 1, 0), (64, 48, 16, 0), (64, 48, 3, 1)])
def test_mask_equals_the_reference(gpu_device, W, H, n_views, shift, with_mask):
    ks = list(range(n_views))
    for name in GEOMETRIES:
        got, ins = run(gpu_device, name, ks, W, H, with_mask, shift)
        check(name, ks, W, H, got, ins)
    # the geometries are what their names say, on the reference
    for k in ks:
        assert reference("inside", k, W, H)[0].all() and reference("covers", k, W, H)[0].all() and not reference("behind", k, W, H)[0].any()
        front = reference("front", k, W, H)[0]
        assert 0.02 < front.mean() < 0.98, (k, front.mean())


@pytest.mark.parametrize("with_mask", [False, True])
def test_a_direction_component_that_is_exactly_zero(gpu_device, with_mask):
    W, H = 33, 17
    for name in AXIS:
        got, ins = run(gpu_device, name, [0], W, H, with_mask)
        check(name, [0], W, H, got, ins)
    col = W // 2
    inside, outside, on_face = (reference(n, 0, W, H)[0] for n in ("axis_inside", "axis_outside", "axis_on_face"))
    assert inside[:, col].sum() >= 3 and on_face[:, col].sum() >= 3
    assert not outside[:, col].any() and outside[:, col + 3].sum() >= 3
    assert not any(reference(n, 0, W, H)[1][:, col].any() for n in AXIS)            # the centre column is compared, not left out
    g = run(gpu_device, "axis_on_face", [0], W, H, False)[0][0]
    assert np.array_equal(g[:, col], on_face[:, col]) and np.array_equal(run(gpu_device, "axis_outside", [0], W, H, False)[0][0][:, col], outside[:, col])


def test_a_view_does_not_depend_on_its_neighbours(gpu_device):
    W, H = 64, 48
    all16, _ = run(gpu_device, "front", list(range(16)), W, H, False)
    for k in (0, 5, 15):
        alone, _ = run(gpu_device, "front", [k], W, H, False)
        assert np.array_equal(alone[0], all16[k])
    some, _ = run(gpu_device, "front", [15, 2, 9], W, H, False)
    assert np.array_equal(some[0], all16[15]) and np.array_equal(some[1], all16[2]) and np.array_equal(some[2], all16[9])


def test_invalid_arguments_are_refused(gpu_device):
    reg = make_region("front")
    out = torch.zeros(16 * 16, dtype=torch.float32, device=gpu_device)
    views = (_lib.RegionMaskView * 1)()
    views[0].cam = make_camera(0, 16, 16); views[0].out = out.data_ptr()
    f = dv.lib.dvs_region_mask_views
    assert f(None, views, 1, 16, 16, C.byref(reg)) == 0
    assert f(None, views, 1, 16, 0, C.byref(reg)) == 1 and f(None, views, 0, 16, 16, C.byref(reg)) == 1 and f(None, views, 17, 16, 16, C.byref(reg)) == 1
    assert f(None, None, 1, 16, 16, C.byref(reg)) == 1 and f(None, views, 1, 16, 16, None) == 1
    views[0].out = None
    assert f(None, views, 1, 16, 16, C.byref(reg)) == 1
    torch.cuda.synchronize()
