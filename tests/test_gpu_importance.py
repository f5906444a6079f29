"""dvs_raster_importance_views against the fp64 restatement tests/importance_ref.py on the exported forward state.

The scene is tests/replay_scene.py's, as in tests/test_gpu_depth.py but for the seed: two views of 50x37 (neither size a multiple of 16), 700 splats, an empty tile, a tile with more than 256 faint entries
(its pixels walk past one staging batch) and a saturating opaque stack (n_contrib stops short of the list) — the shapes at which this
kernel can go wrong; test_scene_has_the_cases asserts them.
A splat is excluded when, in some pixel, an entry at or before its own falls into depth_ref's threshold bands (1e-5 wide; the reference
alone computes this); the cap is 1 % of the splats. The seed: one banded pixel excludes every splat behind it in that pixel's list, and
with the depth test's seed 11 view 0 has one such pixel inside the crowded tile — 1 of 1850 pixels there, 121 of 700 splats here — so
this file uses SEED, the first seed after 11 for which the reference finds no banded pixel in either view. On the others:
  hits exact;  |sum / 2^24 - ref| <= hits (1e-4 + 2^-24): the project's per-pixel 1e-4 bar on T (which the depth test pins) times
  alpha <= 1, plus the quantisation step, per taken pixel;  |max - ref| <= 1e-4;
  conservation: the sum over the splats of a view's sum / 2^24 = the sum over its pixels of dvs_raster_depth_views' alpha (sum of
  w = 1 - final_T), within pixels x 1e-4.
Bit for bit: the same call twice; the two-view pass against the two single-view passes accumulated into one array; asynchronous against
synchronous mode; DVS_TILES_TIGHT against the canonical rectangles (dropped instances never contribute)."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import mesh, prune
from divshot_amd.raster import Rasterizer, params_to_device
import importance_ref as IR
from replay_scene import W, H, N, cameras, scene_params, export_view

pytestmark = pytest.mark.gpu
Q = 16777216.0
SEED = 12


def to_np(triple):
    s, m, h = triple
    return s.cpu().numpy().astype(np.uint64), m.cpu().numpy(), h.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def runs(gpu_device):
    """the two-view pass (scores, depth pass alpha, exported state, reference, masked variant); per-view single passes"""
    P = params_to_device(scene_params(SEED), gpu_device)
    cams = cameras()
    r2 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H, max_views=2)
    z = torch.zeros(N, dtype=torch.int64, device=gpu_device)
    assert dv.lib.dvs_raster_importance_views(r2.ctx, None, C.byref(dv.Opts()), None, z.data_ptr(), None, None) == 4   # DVS_ERR_STATE before any forward
    r2.forward_views(P, cams, sh_degree=0)
    both = to_np(prune.importance_scores(r2))
    again = to_np(prune.importance_scores(r2))
    alpha = mesh.depth_maps(r2)[1].cpu().numpy()
    mask = np.ones((H, W), np.float32); mask[:, :W // 2] = 0
    masked = to_np(prune.importance_scores(r2, masks=[torch.from_numpy(mask).to(gpu_device), None]))
    only = torch.zeros(N, dtype=torch.int64, device=gpu_device)                                                       # max and hits may be NULL
    assert dv.lib.dvs_raster_importance_views(r2.ctx, None, C.byref(r2._opts), None, only.data_ptr(), None, None) == 0
    sum_only = only.cpu().numpy().astype(np.uint64)
    views = [export_view(r2, v, 2) for v in range(2)]
    refs = [IR.importance(e["splat2d"], e["ranges"], e["sorted_splat"], e["n_contrib"], W, H, N, v) for v, e in enumerate(views)]
    ref_masked = IR.importance(views[0]["splat2d"], views[0]["ranges"], views[0]["sorted_splat"], views[0]["n_contrib"], W, H, N, 0, mask=mask)
    r1 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    singles, acc = [], None
    for cam in cams:
        r1.forward(P, cam, sh_degree=0)
        singles.append(to_np(prune.importance_scores(r1)))
        acc = prune.importance_scores(r1, out=acc)
    acc = to_np(acc)
    r1.close(); r2.close()
    return dict(both=both, again=again, alpha=alpha, masked=masked, sum_only=sum_only, views=views, refs=refs, ref_masked=ref_masked,
                singles=singles, acc=acc)


def test_scene_has_the_cases(runs):
    for e in runs["views"]:
        length = e["ranges"][:, 1].astype(np.int64) - e["ranges"][:, 0]
        assert (length == 0).any(), "no empty tile"
        assert length.max() > 256 and e["n_contrib"].max() > 256, (length.max(), e["n_contrib"].max())
        tile_len = length[(np.arange(H)[:, None] // 16) * 4 + np.arange(W)[None, :] // 16]
        sat = e["final_T"] < 1e-3
        assert sat.any() and (e["n_contrib"][sat] < tile_len[sat]).any(), "no saturated pixel that stops short of its list"


def check_against(got, ref, what, min_taken=100, min_wmax=0.5):
    """min_taken, min_wmax: what the scene must exercise (this file's scene by default; tests/test_gpu_list_seams.py gives its scenes' own)"""
    s, m, h = got
    wsum, wmax, hits, excl = ref
    print(f"{what}: excluded {int(excl.sum())} of {excl.size} splats; taken splats {int((hits > 0).sum())}, hits {int(hits.sum())}")
    assert excl.mean() <= 0.01
    k = ~excl
    assert np.array_equal(h[k], hits[k])
    s_err = np.abs(s.astype(np.float64) / Q - wsum)
    bound = hits * (1e-4 + 2.0 ** -24)
    m_err = np.abs(m.astype(np.float64) - wmax)
    print(f"{what}: sum err max {s_err[k].max():.3e} (worst ratio to its bound {np.max(s_err[k] / np.maximum(bound[k], 1e-300)):.3e}), max err {m_err[k].max():.3e}")
    assert (s_err[k] <= bound[k]).all()
    assert (m_err[k] <= 1e-4).all()
    assert (hits[k] > 0).sum() > min_taken and wmax[k].max() > min_wmax


@pytest.mark.parametrize("view", [0, 1])
def test_single_view_scores_match_the_reference(runs, view):
    check_against(runs["singles"][view], runs["refs"][view], f"view {view}")


def test_two_view_scores_match_the_summed_reference(runs):
    a, b = runs["refs"]
    check_against(runs["both"], (a[0] + b[0], np.maximum(a[1], b[1]), a[2] + b[2], a[3] | b[3]), "both views")


@pytest.mark.parametrize("view", [0, 1])
def test_weights_sum_to_the_alpha_of_the_depth_pass(runs, view):
    total = float(runs["singles"][view][0].astype(np.float64).sum() / Q)
    want = float(runs["alpha"][view].astype(np.float64).sum())
    print(f"view {view}: sum of w {total:.6f}, sum of alpha {want:.6f}, bound {W * H * 1e-4:.4f}")
    assert abs(total - want) <= W * H * 1e-4 and want > 50


def test_repeatable_and_additive_bit_for_bit(runs):
    for a, b in zip(runs["both"], runs["again"]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    s, m, h = runs["both"]
    assert np.array_equal(s, runs["acc"][0]) and np.array_equal(h, runs["acc"][2]) and np.array_equal(m.view(np.uint32), runs["acc"][1].view(np.uint32))
    assert np.array_equal(s, runs["singles"][0][0] + runs["singles"][1][0])
    assert np.array_equal(m, np.maximum(runs["singles"][0][1], runs["singles"][1][1]))
    assert np.array_equal(s, runs["sum_only"])
    assert s.max() > 0


def test_mask_zeroes_the_left_half_of_view_0(runs):
    a, b = runs["ref_masked"], runs["refs"][1]
    check_against(runs["masked"], (a[0] + b[0], np.maximum(a[1], b[1]), a[2] + b[2], a[3] | b[3]), "view 0 masked + view 1")
    assert (runs["masked"][2] < runs["both"][2]).any()


def test_async_and_tight_tiles_bit_for_bit(gpu_device):
    P = params_to_device(scene_params(SEED), gpu_device)
    cam = cameras()[0]
    r = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    r.forward(P, cam, sh_degree=0)
    base = to_np(prune.importance_scores(r))
    r.forward(P, cam, sh_degree=0, tight_tiles=True)
    tight = to_np(prune.importance_scores(r))
    r.set_async(True)
    r.forward(P, cam, sh_degree=0)
    asy = to_np(prune.importance_scores(r))
    r.close()
    for other in (tight, asy):
        for a, b in zip(base, other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert base[0].max() > 0
