"""tests/seam_scene.py without a GPU: each scene is what it claims, on the CPU oracle's fp32 forward (the specification the device
matches bit for bit in its lists and, off the fragile pixels, in n_contrib), and the references the GPU tests compare with leave out
no more than the existing tests' caps allow — the counts come from the references alone, on the oracle's state (its lists,
n_contrib, final_T and records through importance_ref.oracle_records), the way SEED_C of tests/test_gpu_sky.py was chosen.

Caps (conditions on the seed, never raised): fragile pixels <= 1 % (the composite comparator's exclusion); doubtful pixels <= 1 %
(tests/test_gpu_depth.py); doubtful splats <= 1 % (tests/test_gpu_importance.py, tests/test_gpu_foreground.py: the votes' exclusion is
the union of two masked importance walks, each a subset of the unmasked walk counted here, and it is counted as the GPU test masks it
too); doubtful splats <= 2 % of those that took a pixel (tests/test_gpu_sky.py). seam_scene.SEEDS holds, per scene, the first seed
from 1 that meets all of them in all three views."""
import numpy as np
import pytest
import depth_ref as DR
import importance_ref as IR
import foreground_ref as FR
import sky_ref as SR
import seam_scene as SS


def vote_planes(W, H):
    """the planes tests/test_gpu_list_seams.py gives the votes pass: a checkerboard fg, a valid plane that blanks the last column"""
    ys, xs = np.mgrid[0:H, 0:W]
    fg = ((xs + ys) % 2).astype(np.float32)
    valid = np.ones((H, W), np.float32); valid[:, W - 1] = 0
    return fg, valid


def oracle_views(oracle_mod, sc, P=None):
    """the fp32 oracle's forward state of each view, in the form the references read"""
    views = []
    for cam in sc["cams"]:
        o = oracle_mod.Oracle(np.float32)
        o.forward(sc["P"] if P is None else P, cam, sh_degree=1)
        views.append(dict(rec=IR.oracle_records(o.get("mean2d"), o.get("conic_opacity")), ranges=o.get("ranges"), vals=o.get("vals"),
                          n_contrib=o.get("n_contrib"), final_T=o.get("final_T"), fragile=o.get("fragile").astype(bool)))
    return views


def excluded_shares(sc, views):
    """per view: the shares the four comparisons leave out, each counted by its reference alone -> list of dicts"""
    W, H, n = sc["W"], sc["H"], sc["n"]
    fg, valid = vote_planes(W, H)
    r = np.random.default_rng(99)
    out = []
    for v, e in enumerate(views):
        a = (e["rec"], e["ranges"], e["vals"], e["n_contrib"], W, H)
        depth_excl = DR.depth_alpha(*a)[2]
        _, _, hits, imp_excl = IR.importance(*a, n, 0)
        vote_excl = FR.votes(*a, n, 0, fg if v != 1 else None, valid if v != 1 else None)[4]
        g, s = r.normal(0, 1, (3, H, W)), r.uniform(0, 1, (3, H, W))
        _, sky_excl, mag = SR.sky_backward_rows(*a[:4], e["final_T"], g, s, W, H, n, 0)
        took = mag[:, 5] > 0
        out.append(dict(fragile=float(e["fragile"].mean()), depth=float(depth_excl.mean()), importance=float(imp_excl.mean()), votes=float(vote_excl.mean()),
                        sky=float((sky_excl & took).sum()) / max(int(took.sum()), 1), hits=hits))
    return out


def within_caps(shares):
    return all(s["fragile"] <= 0.01 and s["depth"] <= 0.01 and s["importance"] <= 0.01 and s["votes"] <= 0.01 and s["sky"] <= 0.02 for s in shares)


@pytest.mark.parametrize("name", SS.NAMES)
def test_scene_is_what_it_claims_and_the_references_keep_it(oracle_mod, name):
    sc = SS.scene(name)
    views = oracle_views(oracle_mod, sc)
    facts = SS.check_cases(sc, views)
    shares = excluded_shares(sc, views)
    for v, ((length, nc_max), s) in enumerate(zip(facts, shares)):
        print(f"{name} (seed {SS.SEEDS[name]}) view {v}: list lengths {length}, largest n_contrib {nc_max}, smallest final_T {float(views[v]['final_T'].min()):.3e}; "
              f"left out: fragile pixels {s['fragile']:.4f}, depth pixels {s['depth']:.4f}, importance splats {s['importance']:.4f}, "
              f"vote splats {s['votes']:.4f}, sky splats (of those that took a pixel) {s['sky']:.4f}")
    for v, s in enumerate(shares):
        assert s["fragile"] <= 0.01 and s["depth"] <= 0.01, (v, s["fragile"], s["depth"])
        assert s["importance"] <= 0.01 and s["votes"] <= 0.01, (v, s["importance"], s["votes"])
        assert s["sky"] <= 0.02, (v, s["sky"])
    if sc["length"] and not sc["stop"]:
        for v, s in enumerate(shares):                               # every entry: taken by some pixels, skipped by others
            assert (s["hits"] > 0).all() and (s["hits"] < sc["W"] * sc["H"]).all(), (v, int(s["hits"].min()), int(s["hits"].max()))
    if name == "tiles":
        assert int(views[1]["vals"].size) == 0                       # the view's share of num_rendered
        assert views[0]["vals"].size > 512 and views[2]["vals"].size > 512


def test_the_colourless_scenes_have_the_same_lists(oracle_mod):
    """the sky rows run on seam_scene.colourless(): the colour does not reach the lists, n_contrib or final_T the caps were counted on"""
    for name in ("len257", "stop256", "tiles"):
        sc = SS.scene(name)
        a, b = oracle_views(oracle_mod, sc), oracle_views(oracle_mod, sc, SS.colourless(sc["P"]))
        for x, y in zip(a, b):
            for k in ("ranges", "vals", "n_contrib", "final_T", "rec"):
                assert np.array_equal(x[k], y[k]), (name, k)
