"""dvs_raster_depth_views against the fp64 restatement tests/depth_ref.py on the exported forward state.

Scene (tests/replay_scene.py, seed 11): two views of 50x37 (4x3 tiles, neither size a multiple of 16), 700 splats: 370 small ones spread over pixels x < 40, y < 28 (so
tile (3, 2) stays empty), 300 faint ones (opacity about 0.03) crowded into tile (1, 0) — more than one 256-entry staging batch, and faint
enough that its pixels walk past entry 256 — and a stack of 30 opaque ones over pixel (10, 20), which saturates the pixels under it (the forward ends such a pixel before the entry that would take T below 1e-4, so its
final_T stays at about 1e-4 and n_contrib stops short of the list end).
Excluded pixels (computed by the reference alone): a walked entry's alpha within 1e-5 relative of 1/255 or 0.99, or |power| < 1e-6. The
bands are 1e-5 wide in a quantity spread over orders of magnitude, so a seed needs no search: the expected count is far below one
pixel; the test asserts <= 1 %."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import mesh
from divshot_amd.raster import Rasterizer, params_to_device
import depth_ref as DR
from replay_scene import W, H, cameras, scene_params, export_view

pytestmark = pytest.mark.gpu
SEED = 11


@pytest.fixture(scope="module")
def runs(gpu_device):
    """the two-view forward's maps, exported state and reference (computed once); the single-view maps"""
    P = params_to_device(scene_params(SEED), gpu_device)
    cams = cameras()
    r2 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H, max_views=2)
    assert dv.lib.dvs_raster_depth_views(r2.ctx, None, C.byref(dv.Opts()), 1, 1) == 4          # DVS_ERR_STATE before any forward
    r2.forward_views(P, cams, sh_degree=0)
    depth, alpha = (t.cpu().numpy() for t in mesh.depth_maps(r2))
    views = [export_view(r2, v, 2) for v in range(2)]
    refs = [DR.depth_alpha(e["splat2d"], e["ranges"], e["sorted_splat"], e["n_contrib"], W, H) for e in views]
    singles = []
    r1 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    for cam in cams:
        r1.forward(P, cam, sh_degree=0)
        singles.append(tuple(t.cpu().numpy()[0] for t in mesh.depth_maps(r1)))
    r1.close(); r2.close()
    return depth, alpha, views, refs, singles


def test_scene_has_the_cases(runs):
    _, _, views, _, _ = runs
    for e in views:
        length = e["ranges"][:, 1].astype(np.int64) - e["ranges"][:, 0]
        assert (length == 0).any(), "no empty tile"
        assert length.max() > 256 and e["n_contrib"].max() > 256, (length.max(), e["n_contrib"].max())
        tile_len = length[(np.arange(H)[:, None] // 16) * 4 + np.arange(W)[None, :] // 16]
        sat = e["final_T"] < 1e-3           # (the forward stops a pixel BEFORE the entry that would take T below 1e-4: T ends at about 1e-4)
        assert sat.any() and (e["n_contrib"][sat] < tile_len[sat]).any(), "no saturated pixel that stops short of its list"


@pytest.mark.parametrize("view", [0, 1])
def test_depth_and_alpha_match_the_reference(runs, view):
    depth, alpha, views, refs, _ = runs
    d_ref, a_ref, excl = refs[view]
    print(f"view {view}: excluded {int(excl.sum())} of {excl.size} pixels")
    assert excl.mean() <= 0.01
    keep = ~excl
    a_err = np.abs(alpha[view] - a_ref)[keep].max()
    d_err = (np.abs(depth[view] - d_ref) / np.maximum(np.abs(d_ref), 1e-30))[keep & (d_ref != 0)].max()
    t_err = np.abs(alpha[view] - (1.0 - views[view]["final_T"].astype(np.float64))).max()
    print(f"view {view}: alpha abs err {a_err:.3e}, depth rel err {d_err:.3e}, |alpha - (1 - final_T)| {t_err:.3e}")
    assert a_err <= 1e-4
    assert d_err <= 1e-4
    assert (depth[view][keep & (d_ref == 0)] == 0).all()
    assert t_err <= 1e-4
    assert (a_ref > 0.5).any() and (d_ref > 2.0).any()


def test_two_view_slices_equal_single_view_runs_bit_for_bit(runs):
    depth, alpha, _, _, singles = runs
    for v in range(2):
        assert np.array_equal(depth[v].view(np.uint32), singles[v][0].view(np.uint32))
        assert np.array_equal(alpha[v].view(np.uint32), singles[v][1].view(np.uint32))


def test_async_and_tight_tiles(gpu_device):
    """asynchronous mode and DVS_TILES_TIGHT: the same maps to 1e-4 (the lists differ, the contributing entries do not)"""
    P = params_to_device(scene_params(SEED), gpu_device)
    cam = cameras()[0]
    r = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    r.forward(P, cam, sh_degree=0)
    base = [t.cpu().numpy() for t in mesh.depth_maps(r)]
    r.forward(P, cam, sh_degree=0, tight_tiles=True)
    tight = [t.cpu().numpy() for t in mesh.depth_maps(r)]
    r.set_async(True)
    r.forward(P, cam, sh_degree=0)
    asy = [t.cpu().numpy() for t in mesh.depth_maps(r)]
    r.close()
    for other in (tight, asy):
        assert np.abs(other[1] - base[1]).max() <= 1e-4
        assert (np.abs(other[0] - base[0]) <= 1e-4 * np.abs(base[0])).all()
    assert np.array_equal(asy[0], base[0]) and np.array_equal(asy[1], base[1])
