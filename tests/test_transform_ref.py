"""The export transform on the CPU: tests/transform_ref.py (the numpy restatement of dvs_transform_splats) and the host helpers of
include/dvs_export.h (dvs_similarity_from_trs, dvs_similarity_inverse, dvs_sh_rotation), judged by properties — a colour must not change
when coefficients and direction are rotated together — with the CPU oracle's SH evaluator (oracle/dvs_oracle.hpp sh_basis, float64) as
the independent basis; the camera-derived orientation (libgsplyio.so); the CLI's refusals, which happen before the plugin is loaded.

tests/golden/sh_rotation_ref.npz holds data recorded from the reference's SHRotation (diverse_base/source/utility/sh_utils.cpp, compiled
stand-alone against its bundled glm): 8 rotation matrices, 8 x 45 coefficients, its outputs. The property tests remain the definition."""
import os
import subprocess
import numpy as np
import pytest
import transform_ref as T
from divshot_amd import transform as X
from divshot_amd._lib import DvsError
from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
f32, f64 = np.float32, np.float64


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _axis_turns():
    out = [np.eye(3)]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for sgn in (1.0, -1.0):
            R = np.zeros((3, 3)); R[a, a] = 1.0; R[b, c] = -sgn; R[c, b] = sgn      # a quarter turn about axis a
            out.append(R)
    return out


@pytest.fixture(scope="module")
def rotations():
    rng = np.random.default_rng(7)
    return [_random_rotation(rng) for _ in range(16)] + _axis_turns()


@pytest.fixture(scope="module")
def oracle_basis():
    o = Oracle(f64)
    return lambda d: np.stack([np.asarray(o.sh_basis(3, v), f64)[1:16] for v in np.asarray(d, f64).reshape(-1, 3)])


@pytest.fixture(scope="module")
def directions():
    d = np.random.default_rng(11).normal(size=(200, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def test_restatement_basis_is_the_oracles(oracle_basis, directions):
    assert np.abs(T.basis15(directions) - oracle_basis(directions)).max() <= 1e-15


def test_sh_invariance_fp64(rotations, oracle_basis, directions):
    """colour from D c at R d == colour from c at d, to 1e-12 |c|_1, with the float64 band matrices"""
    rng = np.random.default_rng(3)
    y0 = oracle_basis(directions)
    worst = 0.0
    for R in rotations:
        c = rng.normal(size=(1, 45))
        c2 = T.rotate_sh(T.sh_rotation64(R), c, 3, f64).reshape(15, 3)
        y1 = oracle_basis(directions @ R.T)
        err = np.abs(y1 @ c2 - y0 @ c.reshape(15, 3)).max()
        worst = max(worst, err / np.abs(c).sum())
        assert err <= 1e-12 * np.abs(c).sum()
    print(f"fp64 invariance: worst {worst:.3e} of |c|_1")


def test_sh_invariance_fp32_matrices(rotations, oracle_basis, directions):
    """the fp32 D[83] of dvs_sh_rotation, applied by the fp32 restatement: per band within 2^-20 |c_band|_1"""
    rng = np.random.default_rng(4)
    y0 = oracle_basis(directions)
    worst = 0.0
    for R in rotations:
        D = X.sh_rotation(R.astype(f32))
        c = rng.normal(size=(1, 45)).astype(f32)
        c2 = T.rotate_sh(D, c, 3, f32).astype(f64).reshape(15, 3)
        c0 = c.astype(f64).reshape(15, 3)
        y1 = oracle_basis(directions @ R.T)
        for first, m, _ in T.BANDS:
            for ch in range(3):
                err = np.abs(y1[:, first:first + m] @ c2[first:first + m, ch] - y0[:, first:first + m] @ c0[first:first + m, ch]).max()
                norm = np.abs(c0[first:first + m, ch]).sum()
                worst = max(worst, err / norm)
                assert err <= 2.0 ** -20 * norm, (first, err, norm)
    print(f"fp32 invariance: worst {worst:.3e} of |c_band|_1 (bound {2.0 ** -20:.3e})")


def test_matrices_equal_an_independent_least_squares_solve(rotations, oracle_basis):
    d = np.random.default_rng(5).normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    y0 = oracle_basis(d)
    for R in rotations:
        D = X.sh_rotation(R.astype(f32)).astype(f64)
        y1 = oracle_basis(d @ R.T)
        for first, m, off in T.BANDS:
            want = np.linalg.lstsq(y1[:, first:first + m], y0[:, first:first + m], rcond=None)[0]
            assert np.abs(D[off:off + m * m].reshape(m, m) - want).max() <= 1e-6
        assert np.abs(D - T.sh_rotation64(R.astype(f32))).max() <= 1e-6


def test_matrices_compose_and_are_orthogonal(rotations):
    for R1, R2 in zip(rotations[:8], rotations[8:16]):
        D1, D2, D12 = (X.sh_rotation(R.astype(f32)).astype(f64) for R in (R1, R2, R1 @ R2))
        for _, m, off in T.BANDS:
            a, b, ab = (D[off:off + m * m].reshape(m, m) for D in (D1, D2, D12))
            assert np.abs(a @ b - ab).max() <= 1e-5
            assert np.abs(a @ a.T - np.eye(m)).max() <= 1e-5


def test_axis_turns_and_identity_give_exact_matrices():
    """the identity gives identity matrices exactly; a quarter turn gives a band-1 matrix that is exactly a signed permutation, and in bands
    2 and 3 (whose true entries are 0, +-1/4, +-1/2, +-sqrt(3)/2, +-sqrt(3/8), +-sqrt(5/8), +-sqrt(15)/4, +-1) no entry lies strictly between 0
    and 0.24 in magnitude: the solve leaves no 1e-17 remainders where the true entry is 0"""
    D = X.sh_rotation(np.eye(3, dtype=f32))
    want = np.concatenate([np.eye(m).reshape(-1) for _, m, _ in T.BANDS]).astype(f32)
    assert np.array_equal(D, want)
    for R in _axis_turns()[1:]:
        D = X.sh_rotation(R.astype(f32))
        M1 = D[0:9].reshape(3, 3)
        assert np.isin(M1, (-1.0, 0.0, 1.0)).all() and (np.abs(M1).sum(axis=0) == 1).all() and (np.abs(M1).sum(axis=1) == 1).all()
        nz = D[D != 0]
        assert (np.abs(nz) >= 0.24).all(), nz[np.abs(nz) < 0.24]                 # nothing between 0 and the smallest true entry, 1/4


def test_reference_fixture_agrees():
    """tests/golden/sh_rotation_ref.npz: R [8,3,3] (row-major; handed to the reference as the glm::mat3 with m[col][row] = R[row][col], i.e. the
    matrix R itself), coeffs [8,45] in this repository's element order j * 3 + c (the recorder regrouped them into the reference's three
    15-float channel vectors and back), rotated = what SHRotation(R).apply returned. Convention mapping needed: NONE — the reference's
    band-1 matrix {{R11, -R12, R10}, {-R21, R22, -R20}, {R01, -R02, R00}} is this basis's (-y, z, -x) order and signs, and bands 2 and 3 follow
    the same real basis; coefficient order and signs agree in all three bands. Compared to 1e-5 (measured: 4.8e-7 at most, the reference's
    fp32 recurrence)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "sh_rotation_ref.npz"))
    assert g["R"].shape == (8, 3, 3) and g["coeffs"].shape == (8, 45) and g["rotated"].shape == (8, 45)
    worst = 0.0
    for R, c, want in zip(g["R"], g["coeffs"], g["rotated"]):
        got32 = T.rotate_sh(X.sh_rotation(R), c[None], 3, f32)[0]
        got64 = T.rotate_sh(T.sh_rotation64(R), c[None], 3, f64)[0]
        worst = max(worst, np.abs(got32 - want).max(), np.abs(got64 - want).max())
        assert np.abs(got32 - want).max() <= 1e-5 and np.abs(got64 - want).max() <= 1e-5
    print(f"reference fixture: worst difference {worst:.3e}")


def _model(rng, n):
    return {"pos": rng.normal(size=(n, 3)).astype(f32) * 3, "shN": rng.normal(size=(n, 45)).astype(f32), "scale": rng.normal(size=(n, 3)).astype(f32) - 2,
            "rot": rng.normal(size=(n, 4)).astype(f32)}


def _apply(sim, model, degree=3):
    return T.transform_splats(sim.R, sim.t, sim.s, X.sh_rotation(sim.R), model["pos"], model["shN"], model["scale"], model["rot"], degree)


def test_identity_returns_every_array_bit_identical():
    m = _model(np.random.default_rng(1), 300)
    out = _apply(X.similarity_from_trs([0, 0, 0], [0, 0, 0], 1.0), m)
    for k in m:
        assert np.array_equal(out[k].view(np.uint32), m[k].view(np.uint32)), k


def test_covariance_identity_fixes_the_quaternion_order():
    """R(q') diag(e^(2 scale')) R(q')^T == s^2 R Sigma R^T, float64 from the fp32 outputs, to 1e-5 relative; the opposite product order fails it"""
    m = _model(np.random.default_rng(2), 200)
    sim = X.similarity_from_trs([0.5, -1, 2], [0.3, -0.7, 1.1], 2.5)
    out = _apply(sim, m)
    R, s = np.array(sim.R, f64).reshape(3, 3), float(sim.s)

    def cov(rot, scale):
        Q = T.quat_to_matrix(rot)
        return np.einsum("nij,nj,nkj->nik", Q, np.exp(2.0 * np.asarray(scale, f64)), Q)

    want = s * s * np.einsum("ij,njk,lk->nil", R, cov(m["rot"], m["scale"]), R)
    got = cov(out["rot"], out["scale"])
    rel = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"covariance identity: worst relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-5
    a = T.quat_of_rotation(sim.R).astype(f32)
    q = m["rot"]
    wrong = np.stack([q[:, 0] * a[0] - q[:, 1] * a[1] - q[:, 2] * a[2] - q[:, 3] * a[3], q[:, 0] * a[1] + q[:, 1] * a[0] + q[:, 2] * a[3] - q[:, 3] * a[2],
                      q[:, 0] * a[2] - q[:, 1] * a[3] + q[:, 2] * a[0] + q[:, 3] * a[1], q[:, 0] * a[3] + q[:, 1] * a[2] - q[:, 2] * a[1] + q[:, 3] * a[0]], axis=1)
    bad = cov(wrong, out["scale"])
    assert (np.abs(bad - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max() > 1e-2
    assert np.allclose(np.linalg.norm(out["rot"], axis=1), np.linalg.norm(q, axis=1), rtol=1e-6)       # the norm survives


def test_inverse_round_trip():
    m = _model(np.random.default_rng(6), 500)
    sim = X.similarity_from_trs([0.5, -1, 2], [0.3, -0.7, 1.1], 2.5)
    inv = X.similarity_inverse(sim)
    Ri, ti, si = T.similarity_inverse(sim.R, sim.t, sim.s)
    assert np.array_equal(np.array(inv.R, f32), Ri.reshape(-1)) and np.array_equal(np.array(inv.t, f32), ti) and f32(inv.s) == si
    fwd = _apply(sim, m)
    back = _apply(inv, fwd)
    # |p|, |t|: the vectors' largest components (a rotation mixes the components, so a small component carries the error of a large one)
    ulp = np.spacing(np.maximum(np.abs(m["pos"]).max(axis=1), np.abs(np.array(sim.t, f32)).max()).astype(f32))[:, None]
    d = np.abs(back["pos"].astype(f64) - m["pos"]) / ulp
    print(f"round trip: pos worst {d.max():.2f} ulp of max(|p|, |t|)")
    assert (d <= 4).all()
    c0, c1 = m["shN"].astype(f64).reshape(-1, 15, 3), back["shN"].astype(f64).reshape(-1, 15, 3)
    for first, k, _ in T.BANDS:
        err = np.abs(c1[:, first:first + k] - c0[:, first:first + k]).max(axis=1)
        assert (err <= 2.0 ** -19 * np.abs(c0[:, first:first + k]).sum(axis=1)).all()


def test_helpers_refuse_what_is_not_a_similarity():
    for t, e, s in (([0, 0, np.nan], [0, 0, 0], 1), ([0, 0, 0], [np.inf, 0, 0], 1), ([0, 0, 0], [0, 0, 0], 0), ([0, 0, 0], [0, 0, 0], -2)):
        with pytest.raises(DvsError):
            X.similarity_from_trs(t, e, s)
    for R in (np.diag([1, 1, -1]), np.diag([1, 1, 1.001]), np.full((3, 3), np.nan)):
        with pytest.raises(DvsError):
            X.sh_rotation(R)
        with pytest.raises(DvsError):
            X.similarity_inverse(X.make_similarity(R, [0, 0, 0], 1.0))
    with pytest.raises(DvsError):
        X.similarity_inverse(X.make_similarity(np.eye(3), [0, 0, 0], 0.0))


def test_euler_convention_is_the_focus_regions():
    from divshot_amd.region import region_from_trs
    rot = [0.3, -0.7, 1.1]
    sim = X.similarity_from_trs([0, 0, 0], rot, 1.0)
    _, b2w = region_from_trs([0, 0, 0], rot, [1, 1, 1], [-1, -1, -1], [1, 1, 1])
    assert np.array_equal(np.array(sim.R, f32).reshape(3, 3), b2w[:3, :3])


# ---- the orientation derived from the cameras ------------------------------------------------------------------------------------------
def _ring(Q, n=12, radius=4.0, height=1.0, offset=(0.0, 0.0, 0.0)):
    """n cameras on a ring about the y axis, y-up world, looking at the origin (camera: x right, y DOWN, z forward), then the whole rig
    turned by Q and moved by offset. -> (views [n,16] as dvs_camera.view (view[c*4+r]), centres [n,3])"""
    views, centres = [], []
    for k in range(n):
        a = 2 * np.pi * k / n
        c = np.array([radius * np.cos(a), height, radius * np.sin(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, np.array([0.0, 1.0, 0.0])); x /= np.linalg.norm(x)      # right
        y = np.cross(z, x)                                                       # down
        c2w = Q @ np.stack([x, y, z], axis=1)
        cw = Q @ c + np.asarray(offset)
        w2c = c2w.T
        V = np.eye(4); V[:3, :3] = w2c; V[:3, 3] = -w2c @ cw
        views.append(V.T.reshape(-1))                                            # view[c*4+r]
        centres.append(cw)
    return np.array(views, f32), np.array(centres, f32)


def test_tilted_ring_comes_back_upright():
    Q = _random_rotation(np.random.default_rng(9))
    views, centres = _ring(Q, offset=(3.0, -2.0, 5.0))
    R, t = X.export_orientation(views, centres, "+y")
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
    assert np.abs(R @ (Q @ np.array([0.0, 1.0, 0.0])) - np.array([0.0, 1.0, 0.0])).max() <= 1e-6
    assert np.abs(R @ centres.astype(f64).mean(axis=0) + t).max() <= 1e-6
    R2, _ = X.export_orientation(views, centres, "-z")
    assert np.abs(R2 @ (Q @ np.array([0.0, 1.0, 0.0])) - np.array([0.0, 0.0, -1.0])).max() <= 1e-6


def test_antiparallel_takes_the_stated_axis_and_zero_mean_is_refused():
    views, centres = _ring(np.eye(3))                                            # mean up = +y exactly opposite to -y
    R, _ = X.export_orientation(views, centres, "-y")                            # (nearly) opposite: still a rotation onto -y
    assert np.abs(R @ np.array([0.0, 1.0, 0.0]) - np.array([0.0, -1.0, 0.0])).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-9
    one = np.zeros((1, 16), f32); one[0, [0, 5, 10, 15]] = 1.0                   # a single identity camera: up = -y exactly
    R, _ = X.export_orientation(one, np.zeros((1, 3), f32), "+y")
    assert np.array_equal(R, np.diag([-1.0, -1.0, 1.0]))
    R, _ = X.export_orientation(one, np.zeros((1, 3), f32), "-y")
    assert np.array_equal(R, np.eye(3))
    two = np.concatenate([one, one]); two[1, 0] = two[1, 5] = -1.0               # the second camera rolled by pi: the ups cancel
    with pytest.raises(DvsError, match="cancel"):
        X.export_orientation(two, np.zeros((2, 3), f32), "+y")
    with pytest.raises(DvsError, match="axis"):
        X.export_orientation(one, np.zeros((1, 3), f32), "up")


# ---- the CLI refuses before the plugin is loaded ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--exportTransform", "0,0,0,0,0,0"], "--exportTransform takes"),
    (["--exportTransform", "0,0,0,0,0,0,0"], "--exportTransform takes"),
    (["--exportTransform", "0,0,0,0,0,0,1,5"], "--exportTransform takes"),
    (["--exportTransform", "0,0,0,0,0,0,1x"], "--exportTransform takes"),
    (["--exportOrient", "up"], "--exportOrient takes"),
    (["--exportTransform", "0,0,0,0,0,0,1", "--exportOrient", "+y"], "exclude each other"),
    (["--exportFormat", "transformed"], "needs --exportTransform or --exportOrient"),
])
def test_cli_refusals(args, word):
    p = subprocess.run([DRIVER] + args, capture_output=True, text=True)
    assert p.returncode == 1 and "Command Line Error:" in p.stdout and word in p.stdout
    assert "gstrain" not in p.stderr                                             # nothing was loaded
