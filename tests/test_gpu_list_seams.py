"""Every kernel that walks a tile's sorted list, on tests/seam_scene.py's scenes: lists of exactly 63, 64, 65, 255, 256, 257, 511, 512,
513 and 769 entries (both sides of each 64-entry word and 256-entry LDS batch seam), every pixel's walk ending exactly on list position
256 and 257, and a 3x2-tile scene with an empty tile, a view that sees nothing, short lists and a list above 512. Every scene has three
views, so a batch launches 3 or 18 tiles in a grid of 8 or 24 workgroups: some have no tile, and view index 2 is reached.
tests/test_seam_scene.py pins on the CPU that the scenes are what they claim and that the references' exclusions stay under the caps.

Composite forward and both backwards (render.hip, render_tr.hip with and without the live lists, render_blocks.hip) against the CPU
oracle with the comparator and bars of test_gpu_parity.py::test_edge_cases; the three-view batch against the single-view runs as
test_multi_view_batch_equals_single_views does; live lists on against off as test_live_lists_give_the_same_gradients does.
The replay passes (depth.hip, importance.hip, foreground.hip, sky.hip's rows; replay_walk.h) on the batch's exported state against
the fp64 restatements at the bars of test_gpu_depth.py, test_gpu_importance.py, test_gpu_foreground.py and test_gpu_sky.py. No
tolerance here is new.

The sky rows are summed with fp32 atomics, one per (tile, batch, splat, column): bit-identical between runs only where a splat sits in
one tile per view, so that comparison is made on the single-tile scenes and not on `tiles`."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import mesh, prune
from divshot_amd.raster import Rasterizer, params_to_device
from util import KEYS, rel_close
import depth_ref as DR
import importance_ref as IR
import foreground_ref as FR
import seam_scene as SS
from replay_scene import export_view
from test_seam_scene import vote_planes
import test_gpu_importance as TI
import test_gpu_foreground as TF
import test_gpu_sky as TS

pytestmark = pytest.mark.gpu
Q = 16777216.0
V = SS.V
DEG = 1
_cache = {}


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene(name):
    return memo(("scene", name), lambda: SS.scene(name))


def rasterizer(sc, views=1):
    return Rasterizer(0, max_splats=1024, max_w=sc["W"], max_h=sc["H"], max_views=views)


# ---- the replay passes' runs: once per scene --------------------------------------------------------------------------------------
def imp_np(triple):
    s, m, h = triple
    return s.cpu().numpy().astype(np.uint64), m.cpu().numpy(), h.cpu().numpy().astype(np.int64)


def replay(gpu_device, name):
    """the three-view batch's exported state and pass outputs (each pass twice), the single-view passes, alone and accumulated"""
    def make():
        sc = scene(name)
        W, H = sc["W"], sc["H"]
        P = params_to_device(sc["P"], gpu_device)
        fg, valid = vote_planes(W, H)
        dev = lambda a: torch.from_numpy(a).to(gpu_device)
        d_fg, d_valid = [dev(fg), None, dev(fg)], [dev(valid), None, dev(valid)]          # NULL and non-NULL plane pointers around view 1
        rb = rasterizer(sc, V)
        rb.forward_views(P, sc["cams"], sh_degree=DEG)
        out = dict(views=[export_view(rb, v, V) for v in range(V)], num_rendered=int(rb.num_rendered))
        out["depth"] = [tuple(t.cpu().numpy() for t in mesh.depth_maps(rb)) for _ in range(2)]
        out["imp"] = [imp_np(prune.importance_scores(rb)) for _ in range(2)]
        out["imp_valid"] = prune.importance_scores(rb, masks=d_valid)[0].cpu().numpy().astype(np.uint64)
        out["votes"] = [TF.to_np(prune.foreground_votes(rb, d_fg, d_valid)) for _ in range(2)]
        rb.close()
        r1 = rasterizer(sc)
        out["depth1"], out["imp1"], out["votes1"], imp_acc, votes_acc = [], [], [], None, None
        for v, cam in enumerate(sc["cams"]):
            r1.forward(P, cam, sh_degree=DEG)
            out["depth1"].append(tuple(t.cpu().numpy()[0] for t in mesh.depth_maps(r1)))
            out["imp1"].append(imp_np(prune.importance_scores(r1)))
            imp_acc = prune.importance_scores(r1, out=imp_acc)
            out["votes1"].append(TF.to_np(prune.foreground_votes(r1, [d_fg[v]], [d_valid[v]])))
            votes_acc = prune.foreground_votes(r1, [d_fg[v]], [d_valid[v]], out=votes_acc)
        out["imp_acc"], out["votes_acc"] = imp_np(imp_acc), TF.to_np(votes_acc)
        r1.close()
        out["planes"] = [(fg, valid), (None, None), (fg, valid)]
        return out
    return memo(("replay", name), make)


def ref_args(sc, e):
    return e["splat2d"], e["ranges"], e["sorted_splat"], e["n_contrib"], sc["W"], sc["H"]


def exercised(sc, v=None):
    """(min_taken, min_wmax) for test_gpu_importance.check_against: what this scene must exercise in view v (None: all views together)"""
    if sc["name"] == "tiles":
        return (-1, -1.0) if v == 1 else (100, 0.5)
    if sc["stop"]:
        return (sc["stop"] - 60, 0.1)                               # most of the entries before the stop; the opaque entry's weight
    return (int(0.9 * sc["n"]), 1e-3)


@pytest.mark.parametrize("name", SS.NAMES)
def test_scenes_have_the_cases(gpu_device, name):
    """first, and from the device's own exported ranges, n_contrib and final_T: a forward that is wrong on a seam fails here"""
    sc, run = scene(name), replay(gpu_device, name)
    facts = SS.check_cases(sc, run["views"])
    for v, (length, nc_max) in enumerate(facts):
        print(f"{name} view {v}: list lengths {length}, largest n_contrib {nc_max}, smallest final_T {float(run['views'][v]['final_T'].min()):.3e}")
    assert run["num_rendered"] == sum(sum(f[0]) for f in facts)
    tiles = V * ((sc["W"] + 15) // 16) * ((sc["H"] + 15) // 16)
    assert tiles % 8 != 0, "every workgroup of the batch launch has a tile"


# ---- the composite kernels against the oracle -------------------------------------------------------------------------------------
def oracle_view(oracle_mod, name, v):
    """the fp32 oracle's forward and backward of one view (computed once, left unchanged)"""
    def make():
        sc = scene(name)
        o = oracle_mod.Oracle(np.float32)
        ref = o.forward(sc["P"], sc["cams"][v], sh_degree=DEG)
        dL = np.random.default_rng(v).standard_normal(ref.shape).astype(np.float32)
        out = {k: o.get(k) for k in ("radii", "vals", "keys", "ranges", "n_contrib")}
        out.update(img=ref, ok=~o.get("fragile").astype(bool), dL=dL, grads=o.backward(dL))
        return out
    return memo(("oracle", name, v), make)


VARIANTS = {"tr": ("tr", False), "blocks": ("blocks", None), "tr_live": ("tr", True)}


def composite(gpu_device, oracle_mod, name, variant):
    """single-view contexts and the three-view batch under one backward variant, everything test_edge_cases.run compares compared with
    the oracle on the way -> the gradients, for the live-list comparison"""
    def make():
        sc = scene(name)
        bwd, live = VARIANTS[variant]
        P = params_to_device(sc["P"], gpu_device)
        r1, rb = rasterizer(sc), rasterizer(sc, V)
        for r in (r1, rb):
            r.set_backward_variant(bwd)
            if live is not None:
                r.set_live_lists(live)
        imgs1, saved1, grads1 = [], [], []
        for v, cam in enumerate(sc["cams"]):
            o = oracle_view(oracle_mod, name, v)
            img = r1.forward(P, cam, sh_degree=DEG, absgrad=True)
            torch.cuda.synchronize()
            saved = r1.saved()
            np.testing.assert_array_equal(saved["radii"], o["radii"])
            np.testing.assert_array_equal(saved["vals"], o["vals"])
            np.testing.assert_array_equal(r1.sorted_keys(), o["keys"])
            np.testing.assert_array_equal(saved["ranges"], o["ranges"])
            ok = o["ok"]
            m, worst = rel_close(img.cpu().numpy()[:, ok], o["img"][:, ok], 1e-4, 1e-6)
            print(f"{name} {variant} view {v}: fragile pixels {int((~ok).sum())}; image worst error / tolerance {worst:.3f}")
            assert m.all(), (v, worst)
            assert np.array_equal(saved["n_contrib"][ok], o["n_contrib"][ok]), v
            g = r1.backward(torch.from_numpy(o["dL"]).to(gpu_device))
            torch.cuda.synchronize()
            for k in KEYS:
                m, worst = rel_close(g[k].cpu().numpy(), o["grads"][k], 2e-4, 1e-5)
                print(f"    {k}: worst error / tolerance {worst:.3f}")
                assert m.all(), (v, k, worst)
            imgs1.append(img.clone()); saved1.append(saved); grads1.append({k: t.clone() for k, t in g.items()})
        imgs = rb.forward_views(P, sc["cams"], sh_degree=DEG, absgrad=True)
        torch.cuda.synchronize()
        assert rb.num_rendered == sum(s["vals"].size for s in saved1)
        for v in range(V):
            assert torch.equal(imgs[v], imgs1[v]), f"image of view {v}"
            sv = rb.view_saved(v)
            for k in ("radii", "flags", "tiles_touched", "vals", "sorted_tile", "ranges", "n_contrib"):
                np.testing.assert_array_equal(sv[k], saved1[v][k], err_msg=f"view {v} {k}")
            for k in ("mean2d", "depth", "conic_opacity", "rgb", "final_T"):
                assert np.array_equal(sv[k].view(np.uint32), saved1[v][k].view(np.uint32)), f"view {v} {k}"
        dL_all = torch.from_numpy(np.stack([oracle_view(oracle_mod, name, v)["dL"] for v in range(V)])).to(gpu_device)
        gb = rb.backward_views(dL_all)
        torch.cuda.synchronize()
        for k in KEYS:
            want = sum(oracle_view(oracle_mod, name, v)["grads"][k].astype(np.float64) for v in range(V))
            m, worst = rel_close(gb[k].cpu().numpy(), want, 2e-4, 1e-5)
            print(f"{name} {variant} batch {k}: worst error / tolerance {worst:.3f}")
            assert m.all(), (k, worst)
            assert np.abs(want).max() > 0
        out = dict(single=grads1, batch={k: t.clone() for k, t in gb.items()})
        r1.close(); rb.close()
        return out
    return memo(("composite", name, variant), make)


@pytest.mark.parametrize("variant", ["tr", "blocks"])
@pytest.mark.parametrize("name", SS.NAMES)
def test_composite_matches_the_oracle(gpu_device, oracle_mod, name, variant):
    composite(gpu_device, oracle_mod, name, variant)


@pytest.mark.parametrize("name", SS.NAMES)
def test_composite_with_live_lists(gpu_device, oracle_mod, name):
    """"tr" over the forward's compacted lists: against the oracle as above, and against the same kernel over the full lists"""
    on, off = composite(gpu_device, oracle_mod, name, "tr_live"), composite(gpu_device, oracle_mod, name, "tr")
    for ga, gb in list(zip(off["single"], on["single"])) + [(off["batch"], on["batch"])]:
        for k in ("pos", "sh0", "shN", "opacity", "scale", "rot", "absgrad2d"):
            x, y = ga[k].double(), gb[k].double()
            assert float((x - y).norm()) <= 2e-6 * float(x.norm()) + 1e-30, k


# ---- depth and alpha --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SS.NAMES)
def test_depth_and_alpha(gpu_device, name):
    sc, run = scene(name), replay(gpu_device, name)
    depth, alpha = run["depth"][0]
    for v, e in enumerate(run["views"]):
        d_ref, a_ref, excl = DR.depth_alpha(*ref_args(sc, e))
        assert excl.mean() <= 0.01
        keep = ~excl
        a_err = np.abs(alpha[v] - a_ref)[keep].max()
        nz = keep & (d_ref != 0)
        d_err = (np.abs(depth[v] - d_ref) / np.maximum(np.abs(d_ref), 1e-30))[nz].max() if nz.any() else 0.0
        t_err = np.abs(alpha[v] - (1.0 - e["final_T"].astype(np.float64))).max()
        print(f"{name} view {v}: excluded {int(excl.sum())} pixels; alpha abs err {a_err:.3e}, depth rel err {d_err:.3e}, |alpha - (1 - final_T)| {t_err:.3e}")
        assert a_err <= 1e-4
        assert d_err <= 1e-4
        assert (depth[v][keep & (d_ref == 0)] == 0).all()
        assert t_err <= 1e-4
        assert nz.any() == (SS.tile_lengths(e["ranges"]).sum() > 0)
        assert np.array_equal(depth[v].view(np.uint32), run["depth1"][v][0].view(np.uint32))      # the batch's slice = the single-view run
        assert np.array_equal(alpha[v].view(np.uint32), run["depth1"][v][1].view(np.uint32))
    for a, b in zip(run["depth"][0], run["depth"][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))                                # the same call twice


# ---- importance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SS.NAMES)
def test_importance(gpu_device, name):
    sc, run = scene(name), replay(gpu_device, name)
    n, W, H = sc["n"], sc["W"], sc["H"]
    refs = [IR.importance(*ref_args(sc, e), n, v) for v, e in enumerate(run["views"])]
    for v in range(V):
        TI.check_against(run["imp1"][v], refs[v], f"{name} view {v}", *exercised(sc, v))
        total, want = float(run["imp1"][v][0].astype(np.float64).sum() / Q), float(run["depth"][0][1][v].astype(np.float64).sum())
        print(f"{name} view {v}: sum of w {total:.6f}, sum of the depth pass's alpha {want:.6f}, bound {W * H * 1e-4:.4f}")
        assert abs(total - want) <= W * H * 1e-4                                                   # conservation
        assert (want > 1.0) == (SS.tile_lengths(run["views"][v]["ranges"]).sum() > 0)
    summed = (sum(r[0] for r in refs), np.maximum.reduce([r[1] for r in refs]), sum(r[2] for r in refs), np.logical_or.reduce([r[3] for r in refs]))
    TI.check_against(run["imp"][0], summed, f"{name} three views", *exercised(sc))
    s, m, h = run["imp"][0]
    for a, b in zip(run["imp"][0], run["imp"][1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    acc, one = run["imp_acc"], run["imp1"]
    assert np.array_equal(s, acc[0]) and np.array_equal(h, acc[2]) and np.array_equal(m.view(np.uint32), acc[1].view(np.uint32))
    assert np.array_equal(s, one[0][0] + one[1][0] + one[2][0]) and np.array_equal(h, one[0][2] + one[1][2] + one[2][2])
    assert np.array_equal(m, np.maximum.reduce([o[1] for o in one]))
    assert s.max() > 0
    if name == "tiles":
        assert not one[1][0].any() and not one[1][2].any() and not one[1][1].any()                 # the view that sees nothing


# ---- foreground votes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SS.NAMES)
def test_votes(gpu_device, name):
    sc, run = scene(name), replay(gpu_device, name)
    n = sc["n"]
    refs = [FR.votes(*ref_args(sc, e), n, v, *run["planes"][v]) for v, e in enumerate(run["views"])]
    for v in range(V):
        TF.check_against(run["votes1"][v], refs[v], f"{name} view {v}")
    TF.check_against(run["votes"][0], tuple(sum(r[i] for r in refs) for i in range(4)) + (np.logical_or.reduce([r[4] for r in refs]),), f"{name} three views")
    fg, bg = run["votes"][0]
    assert fg.sum() > 0 and bg.sum() > 0
    assert np.array_equal(fg + bg, run["imp_valid"])                                               # bit for bit
    assert (run["imp_valid"] <= run["imp"][0][0]).all() and (run["imp_valid"] < run["imp"][0][0]).any()   # the blank column took weight away
    for a, b in zip(run["votes"][0], run["votes"][1]):
        assert np.array_equal(a, b)
    for k in range(2):
        assert np.array_equal(run["votes"][0][k], run["votes_acc"][k])
        assert np.array_equal(run["votes"][0][k], run["votes1"][0][k] + run["votes1"][1][k] + run["votes1"][2][k])


# ---- the sky pass's rows ----------------------------------------------------------------------------------------------------------
def sky_rows(gpu_device, P, cams, tex, dL):
    """the device side of test_gpu_sky.run_against_reference alone -> rows [V,n,12]"""
    n, W, H = P["pos"].shape[0], cams[0].width, cams[0].height
    r = Rasterizer(0, max_splats=max(n, 256), max_w=W, max_h=H, max_views=len(cams))
    r.keep_intermediates(True)
    texd = torch.from_numpy(tex).to(gpu_device)
    imgs = r.forward_views(params_to_device(P, gpu_device), cams, sh_degree=0)
    s = r.sky_forward(texd, imgs, want_sky_rgb=True)
    r.backward_composite(dL)
    r.sky_backward(texd, dL, sky_rgb=s)
    torch.cuda.synchronize()
    rows = TS.all_rows(r, len(cams), n)
    r.close()
    return rows


@pytest.mark.parametrize("name", SS.NAMES)
def test_sky_rows(gpu_device, name):
    sc = SS.scene(name, bg=(0.0, 0.0, 0.0))                          # the sky replaces the background colour
    P = SS.colourless(sc["P"])
    tex = np.random.default_rng(22).uniform(0, 1, (TS.HS, TS.WS, 3)).astype(np.float32)
    facts, _, _ = TS.run_against_reference(gpu_device, P, sc["cams"], tex, what=f"{name}:")
    for v, f in enumerate(facts):
        assert (f["took"] > 0) == (SS.tile_lengths(f["e"]["ranges"]).sum() > 0)
        for k in ("ranges", "n_contrib", "final_T"):                 # the colourless scene walks what the coloured one walks
            a, b = f["e"][k], replay(gpu_device, name)["views"][v][k]
            assert np.array_equal(a, b), (v, k)
    if name == "tiles":
        return
    dL = torch.from_numpy(np.random.default_rng(99).normal(0, 1, (V, 3, sc["H"], sc["W"])).astype(np.float32)).to(gpu_device)     # run_against_reference's
    rows = sky_rows(gpu_device, P, sc["cams"], tex, dL)
    for v in range(V):
        assert np.array_equal(rows[v, :, :6], facts[v]["rows"][:, :6]), f"view {v}: a second run gives other rows"      # (columns 0..5 are the sky pass's)
        one = sky_rows(gpu_device, P, [sc["cams"][v]], tex, dL[v:v + 1].contiguous())
        assert np.array_equal(rows[v, :, :6], one[0, :, :6]), f"view {v}: the three-view pass differs from the single-view pass"
