"""The level-of-detail merge's restatement (tests/lod_ref.py) against what merging must do, without a GPU: a single member is the
identity, two coincident copies merge to themselves with twice the weight, Sigma' is symmetric positive semi-definite, mu is the
weighted centroid, and the written quaternion and scale reproduce Sigma'."""
import functools
import numpy as np
import pytest
import lod_ref as L
import lod_ref_frozen as F
import test_gpu_lod as G

ORIGIN, CELL, DIMS = np.zeros(3, np.float32), np.float32(1.0), [4, 4, 4]


def splats(n, seed, lo=0.0, hi=4.0):
    r = np.random.default_rng(seed)
    return {"pos": r.uniform(lo, hi, (n, 3)).astype(np.float32), "sh0": r.normal(0, 0.5, (n, 3)).astype(np.float32),
            "shN": r.normal(0, 0.2, (n, 45)).astype(np.float32), "opacity": r.normal(0, 2, n).astype(np.float32),
            "scale": r.normal(-2.5, 0.5, (n, 3)).astype(np.float32), "rot": r.normal(0, 1, (n, 4)).astype(np.float32)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_single_member_is_the_identity(dtype):
    p = splats(1, 1)
    out, info = L.merge(p, ORIGIN, CELL, DIMS, 3, dtype)
    assert info["m"] == 1 and info["n_dropped"] == 0 and info["single"].tolist() == [True]
    for k in L.KEYS:
        assert np.array_equal(out[k].astype(np.float32).reshape(-1).view(np.uint32), p[k].reshape(-1).view(np.uint32)), k


def test_every_splat_alone_comes_out_in_key_order():
    i, j, k = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    p = splats(64, 2)
    perm = np.random.default_rng(3).permutation(64)
    p["pos"] = (np.stack([i, j, k], -1).reshape(64, 3)[perm] + 0.5).astype(np.float32)
    out, info = L.merge(p, ORIGIN, CELL, DIMS, 0, np.float32)
    want = np.argsort(L.cell_keys(p["pos"], ORIGIN, CELL, DIMS), kind="stable")
    assert info["m"] == 64 and info["single"].all() and (np.diff(info["keys"]) > 0).all()
    for key in L.KEYS:
        assert np.array_equal(out[key], p[key][want]), key


def test_two_coincident_copies_merge_to_themselves_with_twice_the_weight():
    p = splats(1, 4)
    p["opacity"][:] = -1.0                                               # alpha = 0.269: 2 alpha < 0.99
    two = {k: np.concatenate([v, v]) for k, v in p.items()}
    out, info = L.merge(two, ORIGIN, CELL, DIMS, 3, np.float64)
    assert info["m"] == 1 and not info["single"][0]
    want = L.written_covariances(p["scale"], p["rot"])[0]
    assert np.abs(info["cov"][0] - want).max() <= 1e-12 * np.abs(want).max()             # the same Sigma'
    assert np.abs(out["pos"][0] - p["pos"][0]).max() <= 1e-12                            # the same mean
    assert np.abs(out["sh0"][0] - p["sh0"][0]).max() <= 1e-12 and np.abs(out["shN"][0] - p["shN"][0]).max() <= 1e-12
    alpha = 1.0 / (1.0 + np.exp(1.0))
    assert abs(1.0 / (1.0 + np.exp(-out["opacity"][0])) - min(0.99, 2 * alpha)) <= 1e-12
    two["opacity"][:] = 3.0                                              # 2 alpha > 0.99: clamped
    out, _ = L.merge(two, ORIGIN, CELL, DIMS, 3, np.float64)
    assert abs(1.0 / (1.0 + np.exp(-out["opacity"][0])) - float(np.float32(0.99))) <= 1e-12


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-4)])
def test_moments_and_the_written_rows(dtype, tol):
    """n = 400 on 4^3 cells: every multi-member cluster's mu is the weighted centroid and its Sigma' the weighted second moment, both
    recomputed here with numpy's own sums in float64; Sigma' is symmetric positive semi-definite; quaternion (unit, w >= 0) and scale
    reproduce it. tol: float64 to its roundoff; float32 to 2e-4 of |Sigma'| (a few hundred ulp over sums of up to ~15 members and the
    Jacobi sweeps)."""
    p = splats(400, 5)
    out, info = L.merge(p, ORIGIN, CELL, DIMS, 2, dtype)
    w = L.weights(p["opacity"], p["scale"], np.float64)
    cov = L.covariances(p["scale"], p["rot"], np.float64)
    multi = np.nonzero(~info["single"])[0]
    assert len(multi) >= 50 and info["n_dropped"] == 0
    back = L.written_covariances(out["scale"], out["rot"])
    for o in multi:
        mem = info["members"][o]
        W = w[mem].sum()
        mu = (w[mem, None] * p["pos"][mem].astype(np.float64)).sum(0) / W
        d = p["pos"][mem].astype(np.float64) - mu
        dd = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        S = (w[mem, None] * (cov[mem] + dd)).sum(0) / W
        norm = np.linalg.norm(L.sym3(S))
        assert np.abs(out["pos"][o] - mu).max() <= tol
        assert np.linalg.norm(L.sym3(info["cov"][o].astype(np.float64)) - L.sym3(S)) <= tol * norm
        assert np.linalg.eigvalsh(L.sym3(info["cov"][o].astype(np.float64))).min() >= -tol * norm
        assert np.linalg.norm(L.sym3(back[o]) - L.sym3(S)) <= tol * norm, o
        q = out["rot"][o].astype(np.float64)
        assert abs(np.linalg.norm(q) - 1.0) <= max(tol, 1e-6) and q[0] >= 0
        assert (out["shN"][o][L.LIMIT[2]:] == 0).all() and np.abs(out["shN"][o][:L.LIMIT[2]]).max() > 0
        assert np.abs(out["sh0"][o] - (w[mem, None] * p["sh0"][mem]).sum(0) / W).max() <= tol


def test_dropped_splats_and_weightless_clusters():
    p = splats(12, 6, 0.0, 1.0)                                            # all in cell 0
    p["pos"][0, 1] = np.nan; p["opacity"][1] = -np.inf; p["scale"][2, 0] = np.inf; p["rot"][3, 2] = np.nan
    out, info = L.merge(p, ORIGIN, CELL, DIMS, 3, np.float32)
    assert info["m"] == 1 and info["n_dropped"] == 4 and sorted(info["members"][0].tolist()) == list(range(4, 12))
    p["scale"][4:] = -1000.0                                               # exp underflows to 0 in both precisions: W = 0
    for dtype in (np.float32, np.float64):
        out, info = L.merge(p, ORIGIN, CELL, DIMS, 3, dtype)
        assert info["m"] == 0 and info["n_dropped"] == 12


def test_the_census_changes_no_byte_of_the_earlier_cases():
    for name in G.CASES:
        p, (o, c, d) = G.case(name)
        for D in (0, 3):
            for dtype in (np.float32, np.float64):
                (a, ia), (b, ib) = L.merge(p, o, c, d, D, dtype), F.merge(p, o, c, d, D, dtype)
                for k in L.KEYS:
                    assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (name, D, dtype, k)
                for k in ("keys", "single", "cov", "W"):
                    assert ia[k].tobytes() == ib[k].tobytes(), (name, D, dtype, k)
                assert (ia["m"], ia["n_dropped"]) == (ib["m"], ib["n_dropped"])
                assert len(ia["census"]) == int((~ia["single"]).sum()) and np.array_equal(ia["census_row"], np.nonzero(~ia["single"])[0])


@functools.lru_cache(maxsize=None)
def restated(name, D, defect):
    """the float32 restatement of a case of tests/test_gpu_lod.py as the device's result would arrive: float32 rows and the two counts"""
    p, (o, c, d) = G.case(name)
    out, info = L.merge(p, o, c, d, D, np.float32, defect)
    return {k: v.astype(np.float32) for k, v in out.items()}, {"m": info["m"], "n_dropped": info["n_dropped"]}


def rejected(runs, defect):
    """the (name, D) of `runs` at which test_gpu_lod.compare() refuses the float32 restatement with `defect`"""
    bad = []
    for name, D in sorted({(name, D) for name, D, _, _ in runs}):
        try:
            G.compare(name, D, *restated(name, D, defect))
        except AssertionError:
            bad.append((name, D))
    return bad


def test_the_float32_restatement_passes_every_comparison_of_the_gpu_test():
    """(this is also where the bounds of test_gpu_lod come from: run with -s for the figures)"""
    assert rejected(G.OLD_RUNS + G.NEW_RUNS, None) == []


# the defects the earlier cases already refused, and one case that did (the one-pass moment: every earlier case with a merged cluster but
# `thin`, whose cluster lies near the origin; the missing cap: the four with a capped cluster, n2049, one_cell, mix and thin)
ALREADY_REJECTED = {"one_pass_moment": ("n2049", 3), "no_alpha_cap": ("one_cell", 3)}


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_a_defect_is_rejected_by_a_new_case_and_was_not_before(defect):
    """The gap the new cases close: each of lod_ref.DEFECTS went through every comparison of the earlier cases (but for the ones
    ALREADY_REJECTED records), and is refused by at least one of the cases added with the census."""
    assert rejected(G.NEW_RUNS, defect), defect
    before = rejected(G.OLD_RUNS, defect)
    assert ALREADY_REJECTED[defect] in before if defect in ALREADY_REJECTED else before == [], before


def test_lattice_for():
    o, c, d = L.lattice_for([0, 0, 0, 8, 4, 0], 8)
    assert o.tolist() == [0, 0, 0] and c == np.float32(8 * (1 + 1e-5) / 8) and d == [8, 4, 1]
    assert L.cell_keys(np.array([[8, 4, 0]], np.float32), o, c, d)[0] == (0 * 4 + 3) * 8 + 7          # the maximum lands in the last cells
    for bad in ([0, 0, 0, 8, 4, 0], 3), ([0, 0, 0, 8, 4, 0], 1025), ([1, 1, 1, 1, 1, 1], 8), ([0, 0, 0, np.nan, 1, 1], 8), ([0, 0, 0, -1, 1, 1], 8):
        assert L.lattice_for(*bad) is None
