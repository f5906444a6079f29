"""The sky model without a GPU: tests/sky_ref.py (the fp64 restatement the GPU tests compare against) is itself pinned — its ray rule
against the projection the loaders build, its texture gradient and its row sums against finite differences, its constant-texture case
against the CPU oracle's constant-bg backward — and the two C-ABI entry points refuse bad arguments before they touch a device.

Scene: 180 synthetic splats at 32x32 (2x2 tiles), the fp64 oracle's own forward state (its lists, n_contrib and records through
importance_ref.oracle_records). L = sum_p w(p) . out(p) with random w; the sky's share of it is sum_p T_final(p) (s(p) . w(p))."""
import ctypes as C
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import _lib
import importance_ref as IR
import sky_ref as SR
from depth_ref import S2D_X, S2D_Y, S2D_CONIC, S2D_OPACITY

W = H = 32
N = 180
WS, HS = 16, 8
INVALID = 1


def intrinsics_camera(R, t, fx, fy, cx, cy, w, h):
    cam = dv.Camera()
    R = np.ascontiguousarray(R, np.float32); t = np.ascontiguousarray(t, np.float32)
    _lib.check(dv.lib.dvs_make_camera_intrinsics(R.ctypes.data, t.ctypes.data, C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), w, h,
                                                 C.byref(cam)), "dvs_make_camera_intrinsics")
    return cam


def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def project(cam, p):
    """world point -> pixel coordinates by `proj` and the rule of A2: mean2D = ((ndc + 1) size - 1) / 2"""
    m = np.asarray(cam.proj[:], np.float64).reshape(4, 4)
    clip = np.append(p, 1.0) @ m
    assert clip[3] > 0
    return ((clip[0] / clip[3] + 1) * cam.width - 1) / 2, ((clip[1] / clip[3] + 1) * cam.height - 1) / 2


@pytest.fixture(scope="module")
def scene(oracle_mod):
    spec = dv.make_spec(N, W, H, sh_degree=1, seed=3)
    P = dv.synth_splats(spec)
    cam = dv.synth_camera(spec, 0)
    cam.bg[0] = cam.bg[1] = cam.bg[2] = 0.0
    o = oracle_mod.Oracle(np.float64)
    o.forward(P, cam, sh_degree=1)
    rec = IR.oracle_records(o.get("mean2d"), o.get("conic_opacity"))
    st = dict(rec=rec, ranges=o.get("ranges"), vals=o.get("vals"), n_contrib=o.get("n_contrib"), final_T=o.get("final_T").astype(np.float64))
    r = np.random.default_rng(7)
    return dict(P=P, cam=cam, st=st, w=r.normal(0, 1, (3, H, W)), tex=r.uniform(0, 1, (HS, WS, 3)), d=SR.rays(cam.proj[:], W, H))


def test_ray_rule_agrees_with_the_projection():
    """a point 50 units along the ray of a pixel projects onto that pixel, for a centred camera and for the loaders' forms (COLMAP intrinsics with
    an off-centre principal point, a cropped downscaled level); for the centred camera the tan_fov rule gives the same rays"""
    R = rot_xyz(0.3, -0.7, 0.2); t = np.array([0.4, -0.2, 1.5])
    centred = dv.Camera()
    _lib.check(dv.lib.dvs_make_camera(np.ascontiguousarray(R, np.float32).ctypes.data, np.ascontiguousarray(t, np.float32).ctypes.data, C.c_float(55.0), 40, 24,
                                      C.byref(centred)), "dvs_make_camera")
    off = intrinsics_camera(R, t, 31.0, 29.5, 23.7, 9.2, 40, 24)
    big = intrinsics_camera(R, t, 62.0, 59.0, 40.3, 26.1, 83, 51)             # 83 x 51 halves to 41 x 25 with a cropped column and row
    half = dv.camera_downscale(big, 2)
    assert np.abs(SR.rays(centred.proj[:], 40, 24) - SR.rays_centred(centred.view[:], centred.tan_fovx, centred.tan_fovy, 40, 24)).max() < 1e-6
    assert np.abs(SR.rays(off.proj[:], 40, 24) - SR.rays_centred(off.view[:], off.tan_fovx, off.tan_fovy, 40, 24)).max() > 1e-2
    for cam in (centred, off, half):
        d = SR.rays(cam.proj[:], cam.width, cam.height)
        pos = np.asarray(cam.campos[:], np.float64)
        for x, y in ((0, 0), (cam.width - 1, cam.height - 1), (cam.width // 3, cam.height // 2)):
            px, py = project(cam, pos + 50.0 * d[y, x])
            assert abs(px - x) < 1e-3 and abs(py - y) < 1e-3, (x, y, px, py)


def test_lookup_wraps_in_u_and_clamps_in_v():
    tex = np.random.default_rng(1).uniform(0, 1, (HS, WS, 3))
    back = np.array([[[1e-9, 0.0, -1.0]], [[-1e-9, 0.0, -1.0]]])               # either side of the seam: both halfway between columns Ws - 1 and 0
    s = SR.lookup(tex, back)
    mid = 0.5 * (tex[:, WS - 1] + tex[:, 0])
    row = 0.5 * (mid[HS // 2 - 1] + mid[HS // 2])
    assert np.abs(s[:, 0, 0] - row).max() < 1e-6 and np.abs(s[:, 1, 0] - row).max() < 1e-6
    up = SR.lookup(tex, np.array([[[0.0, 1.0, 0.0]], [[0.0, -1.0, 0.0]]]))      # (atan2(0, 0) = 0: u = Ws / 2 - 0.5)
    for k, y in ((0, HS - 1), (1, 0)):
        assert np.abs(up[:, k, 0] - 0.5 * (tex[y, WS // 2 - 1] + tex[y, WS // 2])).max() < 1e-12


def test_texture_gradient_is_the_derivative(scene):
    """out is linear in the texture: one forward difference per texel value is exact"""
    st, d, w = scene["st"], scene["d"], scene["w"]
    g_tex = SR.sky_backward_tex(st["final_T"], w, d, WS, HS)
    base = (SR.sky_forward(np.zeros((3, H, W)), st["final_T"], scene["tex"], d)[0] * w).sum()
    worst = 0.0
    for k in range(HS * WS * 3):
        tex = scene["tex"].copy(); tex.reshape(-1)[k] += 1.0
        fd = (SR.sky_forward(np.zeros((3, H, W)), st["final_T"], tex, d)[0] * w).sum() - base
        worst = max(worst, abs(fd - g_tex.reshape(-1)[k]))
    assert worst < 1e-10 and np.abs(g_tex).max() > 0.1, worst


def test_reference_final_T_is_the_oracles(scene):
    st = scene["st"]
    T = SR.final_T(st["rec"], st["ranges"], st["vals"], st["n_contrib"], W, H)
    assert np.abs(T - st["final_T"]).max() < 1e-12 and T.min() < 0.5


def test_row_sums_match_finite_differences(scene):
    """the six row values, pushed through the relations of dvs_get_bwd_intermediates, are dL/d(mean2D, conic, opacity) of sum_p T_final (s . w)"""
    st, w = scene["st"], scene["w"]
    s = SR.lookup(scene["tex"], scene["d"])
    h = (s * w).sum(0)
    rows, excl, _ = SR.sky_backward_rows(st["rec"], st["ranges"], st["vals"], st["n_contrib"], st["final_T"], w, s, W, H, N, 0)
    dmean, dconic, dop = SR.rows_to_grads(rows, st["rec"][:, S2D_CONIC:S2D_CONIC + 3])
    ana = np.concatenate([dmean, dconic, dop[:, None]], 1)                      # columns as `cols` below
    cols = [S2D_X, S2D_Y, S2D_CONIC, S2D_CONIC + 1, S2D_CONIC + 2, S2D_OPACITY]

    def L(rec):
        return (SR.final_T(rec, st["ranges"], st["vals"], st["n_contrib"], W, H) * h).sum()
    took = np.flatnonzero((np.abs(rows).sum(1) > 0) & ~excl)
    assert took.size >= 40 and excl.mean() <= 0.02, (took.size, excl.sum())
    pick = np.random.default_rng(5).choice(took, 12, replace=False)
    fd = np.zeros((12, 6))
    for a, i in enumerate(pick):
        for b, col in enumerate(cols):
            eps = 1e-6 * max(1.0, abs(st["rec"][i, col]))
            hi, lo = st["rec"].copy(), st["rec"].copy()
            hi[i, col] += eps; lo[i, col] -= eps
            fd[a, b] = (L(hi) - L(lo)) / (2 * eps)
    for b in range(6):
        err = np.abs(fd[:, b] - ana[pick, b]).max() / np.abs(ana[pick, b]).max()
        print(f"column {b}: max |fd - analytic| / max |analytic| = {err:.2e}")
        assert err < 1e-6, (b, err)


@pytest.mark.parametrize("mode", [0, 1])
def test_constant_texture_gives_the_rows_of_the_bg_path(scene, oracle_mod, mode):
    """texels all b: the rows equal what the oracle's composite backward adds when it starts from bg_dot = b . g instead of 0"""
    b = np.array([0.2, 0.7, 0.4], np.float32).astype(np.float64)               # (dvs_camera.bg is fp32: the oracle reads these values)
    P, cam, st, w = scene["P"], scene["cam"], scene["st"], scene["w"]
    got = {}
    for name, bg in (("zero", (0.0, 0.0, 0.0)), ("b", b)):
        c = dv.Camera.from_buffer_copy(cam)
        c.bg[0], c.bg[1], c.bg[2] = bg
        o = oracle_mod.Oracle(np.float64)
        o.forward(P, c, sh_degree=1)
        o.backward(w, grad_mode=mode)
        got[name] = (o.get("dL_dmean2d").copy(), o.get("dL_dconic_opacity").copy())
    want = np.concatenate([got["b"][0] - got["zero"][0], got["b"][1] - got["zero"][1]], 1)
    tex = np.broadcast_to(b, (HS, WS, 3))
    s = SR.lookup(tex, scene["d"])
    assert np.abs(s - b[:, None, None]).max() < 1e-15
    rows, _, _ = SR.sky_backward_rows(st["rec"], st["ranges"], st["vals"], st["n_contrib"], st["final_T"], w, s, W, H, N, 0, lineage=bool(mode))
    dmean, dconic, dop = SR.rows_to_grads(rows, st["rec"][:, S2D_CONIC:S2D_CONIC + 3])
    have = np.concatenate([dmean, dconic, dop[:, None]], 1)
    for k in range(6):
        err = np.abs(have[:, k] - want[:, k]).max() / np.abs(want[:, k]).max()
        assert err < 1e-9, (k, err)


def _sky(tex=256, width=16, height=8):
    return _lib.Sky(tex, width, height)


def test_symbols_are_exported_and_bound():
    for name in ("dvs_sky_forward_views", "dvs_sky_backward_views"):
        assert hasattr(dv.lib, name) and name in _lib._PROTOS, name


def test_entry_points_refuse_bad_arguments(scene):
    fwd, bwd = dv.lib.dvs_sky_forward_views, dv.lib.dvs_sky_backward_views
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))                  # never dereferenced: the argument checks come first
    cams = (dv.Camera * 1)(scene["cam"])
    with_bg = (dv.Camera * 1)(scene["cam"]); with_bg[0].bg[1] = 0.25
    flat = (dv.Camera * 1)(dv.Camera())                                         # proj all zero: no ray per pixel
    opts = dv.Opts()
    bad_mode = dv.Opts(); bad_mode.grad_mode = 2
    sky = _sky()

    def f(ctx=fake, cams=cams, V=1, sky=sky, out=512, s=None):
        return fwd(ctx, None, cams, V, C.byref(sky) if sky is not None else None, out, s)

    def g(ctx=fake, cams=cams, V=1, opts=opts, sky=sky, dL=512, s=None, g_tex=1024):
        return bwd(ctx, None, cams, V, C.byref(opts) if opts is not None else None, C.byref(sky) if sky is not None else None, dL, s, g_tex)
    for call in (f, g):
        assert call(ctx=None) == INVALID
        assert call(cams=None) == INVALID
        assert call(sky=None) == INVALID
        assert call(sky=_sky(tex=None)) == INVALID
        assert call(sky=_sky(tex=260)) == INVALID                               # misaligned texture
        assert call(sky=_sky(width=15)) == INVALID and call(sky=_sky(width=8, height=8)) == INVALID
        assert call(sky=_sky(width=2, height=1)) == INVALID
        assert call(V=0) == INVALID and call(V=17) == INVALID
        assert call(cams=with_bg) == INVALID
        assert call(cams=flat) == INVALID
        assert call(s=520) == INVALID                                           # misaligned sky_rgb
    assert f(out=None) == INVALID and f(out=516) == INVALID
    assert b"dvs_sky_forward_views" in dv.lib.dvs_last_error()
    assert g(opts=None) == INVALID and g(opts=bad_mode) == INVALID
    assert g(dL=None) == INVALID and g(dL=516) == INVALID
    assert g(g_tex=None) == INVALID and g(g_tex=1028) == INVALID
    assert b"dvs_sky_backward_views" in dv.lib.dvs_last_error()
