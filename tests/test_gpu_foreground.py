"""dvs_raster_foreground_views against the fp64 restatement tests/foreground_ref.py on the exported forward state.

The scene is tests/replay_scene.py's with the seed of tests/test_gpu_importance.py, exactly as there: two views of 50x37, 700 splats, an
empty tile, a tile with more than 256 faint entries and a saturating opaque stack; test_scene_has_the_cases asserts them again. That
file documents that for SEED the reference finds no banded pixel in either view, and every valid pixel here walks what it walks there,
so the 1 % exclusion cap is met by the reference alone (asserted).
Masks: view 0's left half is background; view 1's pixels with (x + y) % 3 == 0 are background, so every wave holds both labels; a
valid plane for view 1 blanks a 5-pixel border.
On the non-excluded splats fg and bg are each within hits (1e-4 + 2^-24) of the reference, hits the reference's own count for that
label: the project's per-pixel 1e-4 bar on T times alpha <= 1, plus the quantisation step, per taken pixel.
Bit for bit: fg + bg = importance_scores(masks=valid)' sum; no masks at all gives fg = the importance sum and bg = 0; all-zero fg
planes give the reverse; the same call twice; the two-view pass against the two single-view passes accumulated; asynchronous mode
and DVS_TILES_TIGHT against the base run."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import prune
from divshot_amd.raster import Rasterizer, params_to_device
import foreground_ref as FR
from replay_scene import W, H, N, cameras, scene_params, export_view

pytestmark = pytest.mark.gpu
Q = 16777216.0
SEED = 12


def masks_np():
    ys, xs = np.mgrid[0:H, 0:W]
    fg0 = np.ones((H, W), np.float32); fg0[:, :W // 2] = 0
    fg1 = ((xs + ys) % 3 != 0).astype(np.float32)
    valid1 = np.zeros((H, W), np.float32); valid1[5:H - 5, 5:W - 5] = 1
    return fg0, fg1, valid1


def to_np(pair):
    return tuple(t.cpu().numpy().astype(np.uint64) for t in pair)


@pytest.fixture(scope="module")
def runs(gpu_device):
    P = params_to_device(scene_params(SEED), gpu_device)
    cams = cameras()
    fg0, fg1, valid1 = masks_np()
    dev = lambda a: torch.from_numpy(a).to(gpu_device)
    d_fg, d_valid = [dev(fg0), dev(fg1)], [None, dev(valid1)]
    r2 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H, max_views=2)
    z = torch.zeros(2 * N, dtype=torch.int64, device=gpu_device)
    state_err = dv.lib.dvs_raster_foreground_views(r2.ctx, None, C.byref(dv.Opts()), None, None, z.data_ptr(), z.data_ptr() + 8 * N)
    r2.forward_views(P, cams, sh_degree=0)
    both = to_np(prune.foreground_votes(r2, d_fg, d_valid))
    again = to_np(prune.foreground_votes(r2, d_fg, d_valid))
    imp_valid = prune.importance_scores(r2, masks=d_valid)[0].cpu().numpy().astype(np.uint64)
    imp_all = prune.importance_scores(r2)[0].cpu().numpy().astype(np.uint64)
    no_masks = to_np(prune.foreground_votes(r2))
    zero = torch.zeros(H, W, dtype=torch.float32, device=gpu_device)
    all_bg = to_np(prune.foreground_votes(r2, [zero, zero]))
    views = [export_view(r2, v, 2) for v in range(2)]
    refs = [FR.votes(e["splat2d"], e["ranges"], e["sorted_splat"], e["n_contrib"], W, H, N, v, fg, valid)
            for v, (e, fg, valid) in enumerate(zip(views, (fg0, fg1), (None, valid1)))]
    r1 = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    singles, acc = [], None
    for v, cam in enumerate(cams):
        r1.forward(P, cam, sh_degree=0)
        singles.append(to_np(prune.foreground_votes(r1, [d_fg[v]], [d_valid[v]])))
        acc = prune.foreground_votes(r1, [d_fg[v]], [d_valid[v]], out=acc)
    acc = to_np(acc)
    r1.close(); r2.close()
    return dict(state_err=state_err, both=both, again=again, imp_valid=imp_valid, imp_all=imp_all, no_masks=no_masks, all_bg=all_bg, views=views,
                refs=refs, singles=singles, acc=acc)


def test_state_error_before_any_forward(runs):
    assert runs["state_err"] == 4               # DVS_ERR_STATE


def test_scene_has_the_cases(runs):
    for e in runs["views"]:
        length = e["ranges"][:, 1].astype(np.int64) - e["ranges"][:, 0]
        assert (length == 0).any(), "no empty tile"
        assert length.max() > 256 and e["n_contrib"].max() > 256, (length.max(), e["n_contrib"].max())
        tile_len = length[(np.arange(H)[:, None] // 16) * 4 + np.arange(W)[None, :] // 16]
        sat = e["final_T"] < 1e-3
        assert sat.any() and (e["n_contrib"][sat] < tile_len[sat]).any(), "no saturated pixel that stops short of its list"


def check_against(got, ref, what):
    fg, bg = got
    wf, wb, hf, hb, excl = ref
    print(f"{what}: excluded {int(excl.sum())} of {excl.size} splats; fg hits {int(hf.sum())}, bg hits {int(hb.sum())}")
    assert excl.mean() <= 0.01
    k = ~excl
    for name, s, w, h in (("fg", fg, wf, hf), ("bg", bg, wb, hb)):
        err = np.abs(s.astype(np.float64) / Q - w)
        bound = h * (1e-4 + 2.0 ** -24)
        print(f"{what} {name}: err max {err[k].max():.3e} (worst ratio to its bound {np.max(err[k] / np.maximum(bound[k], 1e-300)):.3e})")
        assert (err[k] <= bound[k]).all()


@pytest.mark.parametrize("view", [0, 1])
def test_single_view_votes_match_the_reference(runs, view):
    check_against(runs["singles"][view], runs["refs"][view], f"view {view}")


def test_two_view_votes_match_the_summed_reference(runs):
    a, b = runs["refs"]
    check_against(runs["both"], (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], a[4] | b[4]), "both views")


def test_both_labels_are_exercised(runs):
    fg, bg = runs["both"]
    assert fg.sum() > 0 and bg.sum() > 0
    assert ((fg > 0) & (bg > 0)).sum() > 100


def test_votes_split_the_importance_sum_bit_for_bit(runs):
    fg, bg = runs["both"]
    assert np.array_equal(fg + bg, runs["imp_valid"]) and runs["imp_valid"].max() > 0
    assert (runs["imp_valid"] < runs["imp_all"]).any()                        # the blank border took weight away


def test_no_masks_and_all_background_bit_for_bit(runs):
    fg, bg = runs["no_masks"]
    assert np.array_equal(fg, runs["imp_all"]) and not bg.any() and fg.max() > 0
    fg, bg = runs["all_bg"]
    assert np.array_equal(bg, runs["imp_all"]) and not fg.any()


def test_repeatable_and_additive_bit_for_bit(runs):
    for a, b in zip(runs["both"], runs["again"]):
        assert np.array_equal(a, b)
    for k in range(2):
        assert np.array_equal(runs["both"][k], runs["acc"][k])
        assert np.array_equal(runs["both"][k], runs["singles"][0][k] + runs["singles"][1][k])
    assert runs["both"][0].max() > 0


def test_async_and_tight_tiles_bit_for_bit(gpu_device):
    P = params_to_device(scene_params(SEED), gpu_device)
    cam = cameras()[1]
    _, fg1, valid1 = masks_np()
    fg, valid = [torch.from_numpy(fg1).to(gpu_device)], [torch.from_numpy(valid1).to(gpu_device)]
    r = Rasterizer(0, max_splats=1024, max_w=W, max_h=H)
    r.forward(P, cam, sh_degree=0)
    base = to_np(prune.foreground_votes(r, fg, valid))
    r.forward(P, cam, sh_degree=0, tight_tiles=True)
    tight = to_np(prune.foreground_votes(r, fg, valid))
    r.set_async(True)
    r.forward(P, cam, sh_degree=0)
    asy = to_np(prune.foreground_votes(r, fg, valid))
    r.close()
    for other in (tight, asy):
        for a, b in zip(base, other):
            assert np.array_equal(a, b)
    assert base[0].max() > 0 and base[1].max() > 0
