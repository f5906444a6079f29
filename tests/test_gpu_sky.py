"""dvs_sky_forward_views / dvs_sky_backward_views (csrc/sky.hip) on the device.

(a) the ray rule against A2: a splat 50 units along the reference's ray of a pixel projects onto that pixel, for a centred camera and
    for the loaders' forms (off-centre COLMAP intrinsics, a cropped downscaled level).
(b) a texture whose texels all hold b against the existing cam.bg = b path: images to 1e-6, all six gradient groups at the suite's
    1e-4 bar (util.rel_close(1e-4, 2e-6), the comparator test_gpu_parity.py holds two fp32-atomic summation orders to). This is the
    test that fails without the feature, and it holds the new row pass to the oracle-pinned composite backward.
(c) a 16x8 random texture seen by six 110-degree off-centre cameras along +-Z, +-X and straight up and down (the u wrap and both v clamps
    are hit: asserted) against tests/sky_ref.py on the exported state.
(d) edge tiles: tests/test_gpu_depth.py's scene (a tile with more than 256 entries, an empty tile, a saturating stack), a view whose
    pixels all saturate and a view that sees no splat.
(e) state and argument errors.
In (c) and (d) every splat's colour is clamped to zero (sh0 = -10), so the composite backward leaves columns 0..5 of the rows at zero and
what is read there is the sky pass alone. Bars: image and lookup 1e-4 absolute (a few ulp of atan2f times Ws / 2 pi texels times a texel
contrast <= 1); g_tex per texel 1e-4 of the sum of |T_final g| over the pixels that touch it (the same weight error); rows per splat and
column 1e-4 of the sum of the pairs' absolute terms + 2e-6 of the column's largest value (the importance test's per-pair 1e-4 with the
parity comparator's floor). Splats the reference marks doubtful are excluded; their share of the splats that took a pixel is capped at 2 %."""
import ctypes as C
import numpy as np
import pytest
import torch
import divshot_amd as dv
from divshot_amd import _lib
from divshot_amd.raster import Rasterizer, params_to_device
from util import KEYS, rel_close
import sky_ref as SR
import replay_scene as RS
from test_sky_ref import intrinsics_camera, rot_xyz

pytestmark = pytest.mark.gpu
WS, HS = 16, 8
SEED_C = 2            # chosen on the CPU with the reference (fp32 oracle state): no doubtful splat in any of the six views; seeds 3 and 6 each put one banded pixel in front of a third of a view's splats


def look(f, right):
    """rows = the camera's axes in the world: right, down = forward x right, forward"""
    f, right = np.asarray(f, float), np.asarray(right, float)
    return np.stack([right, np.cross(f, right), f])


def export(r, v, V, W, H):
    st, st0 = _lib.FwdState(), _lib.FwdState()
    _lib.check(dv.lib.dvs_get_view_state(r.ctx, v, C.byref(st)), "dvs_get_view_state")
    _lib.check(dv.lib.dvs_get_view_state(r.ctx, 0, C.byref(st0)), "dvs_get_view_state")
    tiles = st.tiles_x * st.tiles_y
    return dict(splat2d=r._d2h(st0.splat2d, (V * st.n, 16), np.float32), ranges=r._d2h(st.ranges, (tiles, 2), np.uint32),
                sorted_splat=r._d2h(st0.sorted_splat, (int(r.num_rendered),), np.uint32), n_contrib=r._d2h(st.n_contrib, (H, W), np.uint32),
                final_T=r._d2h(st.final_T, (H, W), np.float32))


def all_rows(r, V, n):
    rows, width = C.c_void_p(), C.c_int(0)
    _lib.check(dv.lib.dvs_get_bwd_intermediates(r.ctx, C.byref(rows), C.byref(width)))
    assert width.value == 12
    return r._d2h(rows.value, (V, n, 12), np.float32).astype(np.float64)


def colourless(P):
    P = {k: v.copy() for k, v in P.items()}
    P["sh0"][:] = -10.0; P["shN"][:] = 0.0                       # colour = max(0, C0 sh0 + 0.5) = 0 for every splat
    return P


def run_against_reference(gpu_device, P, cams, tex, mode=0, sky_rgb_kept=True, what=""):
    """forward_views + sky forward, composite backward + sky backward on the device; everything compared with sky_ref. Returns per-view facts."""
    n, V, W, H = P["pos"].shape[0], len(cams), cams[0].width, cams[0].height
    r = Rasterizer(0, max_splats=max(n, 256), max_w=W, max_h=H, max_views=V)
    r.keep_intermediates(True)
    Pd = params_to_device(P, gpu_device)
    texd = torch.from_numpy(tex).to(gpu_device)
    imgs = r.forward_views(Pd, cams, sh_degree=0, grad_mode=mode)
    C0 = imgs.cpu().numpy().astype(np.float64)
    s_dev = r.sky_forward(texd, imgs, want_sky_rgb=True)
    out, s_gpu = imgs.cpu().numpy(), s_dev.cpu().numpy()
    dL = torch.from_numpy(np.random.default_rng(99).normal(0, 1, (V, 3, H, W)).astype(np.float32)).to(gpu_device)
    r.backward_composite(dL)
    torch.cuda.synchronize()
    before = all_rows(r, V, n)
    g_tex = r.sky_backward(texd, dL, sky_rgb=s_dev if sky_rgb_kept else None).cpu().numpy()
    torch.cuda.synchronize()
    rows = all_rows(r, V, n)
    assert (before[:, :, :6] == 0).all()                                      # colourless splats: the composite backward leaves the geometry columns at zero
    assert np.array_equal(before[:, :, 6:], rows[:, :, 6:])                   # the sky pass writes columns 0..5 only: colour and abs-grad columns as they were
    g = dL.cpu().numpy()
    g_ref, g_mag, facts = np.zeros((HS, WS, 3)), np.zeros((HS, WS, 3)), []
    for v in range(V):
        e = export(r, v, V, W, H)
        d = SR.rays(cams[v].proj[:], W, H)
        out_ref, s_ref = SR.sky_forward(C0[v], e["final_T"], tex, d)
        img_err, s_err = np.abs(out[v] - out_ref).max(), np.abs(s_gpu[v] - s_ref).max()
        g_ref += SR.sky_backward_tex(e["final_T"], g[v], d, WS, HS)
        g_mag += SR.sky_backward_tex(e["final_T"], np.abs(g[v]), d, WS, HS, unit_weights=True)
        ref, excl, mag = SR.sky_backward_rows(e["splat2d"], e["ranges"], e["sorted_splat"], e["n_contrib"], e["final_T"], g[v], s_gpu[v], W, H, n, v,
                                              lineage=bool(mode))
        took = mag[:, 5] > 0
        share = float((excl & took).sum()) / max(int(took.sum()), 1)
        k = ~excl
        tol = 1e-4 * mag + 2e-6 * np.abs(ref).max(0)[None]
        ratio = float((np.abs(rows[v, :, :6] - ref)[k] / np.maximum(tol[k], 1e-300)).max()) if k.any() else 0.0
        print(f"{what} view {v}: image err {img_err:.2e}, lookup err {s_err:.2e}; splats that took a pixel {int(took.sum())}, excluded {int((excl & took).sum())}; "
              f"rows worst error / bound {ratio:.3f} (largest |row| {np.abs(ref).max():.3e})")
        assert img_err <= 1e-4 and s_err <= 1e-4
        assert share <= 0.02, share
        assert (np.abs(rows[v, :, :6] - ref)[k] <= tol[k]).all(), ratio
        assert (rows[v][~took & k][:, :6] == 0).all()                         # splats no pixel took
        facts.append(dict(e=e, d=d, took=int(took.sum()), out=out[v], s=s_gpu[v], C0=C0[v], rows=rows[v], ref=ref, g=g[v]))
    g_err = np.abs(g_tex - g_ref)
    print(f"{what} g_tex: worst error / bound {float((g_err / np.maximum(1e-4 * g_mag, 1e-300)).max()):.3f} (largest |g_tex| {np.abs(g_ref).max():.3e})")
    assert (g_err <= 1e-4 * g_mag).all()
    r.close()
    return facts, g_tex, g_ref


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def test_ray_rule_agrees_with_the_projection_of_the_rasterizer(gpu_device):
    R = rot_xyz(0.3, -0.7, 0.2); t = np.array([0.4, -0.2, 1.5])
    centred = dv.Camera()
    _lib.check(dv.lib.dvs_make_camera(np.ascontiguousarray(R, np.float32).ctypes.data, np.ascontiguousarray(t, np.float32).ctypes.data, C.c_float(55.0), 40, 24,
                                      C.byref(centred)), "dvs_make_camera")
    off = intrinsics_camera(R, t, 31.0, 29.5, 23.7, 9.2, 40, 24)
    half = dv.camera_downscale(intrinsics_camera(R, t, 62.0, 59.0, 40.3, 26.1, 83, 51), 2)      # 41 x 25, a cropped column and row
    for name, cam in (("centred", centred), ("off-centre intrinsics", off), ("cropped level", half)):
        W, H = cam.width, cam.height
        d = SR.rays(cam.proj[:], W, H)
        pix = [(0, 0), (W - 1, H - 1), (W // 3, H // 2)]
        pos = np.stack([np.asarray(cam.campos[:], np.float64) + 50.0 * d[y, x] for x, y in pix])
        P = {"pos": pos, "sh0": np.zeros((3, 3)), "shN": np.zeros((3, 15, 3)), "opacity": np.full(3, 5.0), "scale": np.zeros((3, 3)),
             "rot": np.tile([1.0, 0, 0, 0], (3, 1))}
        P = {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}
        r = Rasterizer(0, max_splats=256, max_w=W, max_h=H)
        r.forward(params_to_device(P, gpu_device), cam, sh_degree=0)
        m = r.saved()["mean2d"]
        r.close()
        err = np.abs(m - np.array(pix, np.float64)).max()
        print(f"{name}: splat2d X/Y off the pixel by at most {err:.2e} px")
        assert err < 1e-3, (name, m)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_b(gpu_device):
    n, W, H = 1500, 40, 24
    spec = dv.make_spec(n, W, H, sh_degree=1, n_cams=3, seed=17)
    return dict(n=n, W=W, H=H, spec=spec, P=params_to_device(dv.synth_splats(spec), gpu_device),
                dL=torch.from_numpy(np.random.default_rng(5).normal(0, 1, (2, 3, H, W)).astype(np.float32)).to(gpu_device))


@pytest.mark.parametrize("mode,tight", [(0, False), (1, False), (0, True), (1, True)])
def test_constant_texture_equals_the_bg_path(gpu_device, scene_b, mode, tight):
    b = (0.2, 0.7, 0.4)
    n, W, H, P, dL = scene_b["n"], scene_b["W"], scene_b["H"], scene_b["P"], scene_b["dL"]
    cams_b, cams_0 = [], []
    for i in (1, 2):
        for lst, bg in ((cams_b, b), (cams_0, (0.0, 0.0, 0.0))):
            c = dv.synth_camera(scene_b["spec"], i)
            c.bg[0], c.bg[1], c.bg[2] = bg
            lst.append(c)
    r = Rasterizer(0, max_splats=n, max_w=W, max_h=H, max_views=2)
    if mode == 1 and tight:
        r.set_async(True)                                        # one combination runs both paths in asynchronous mode
    want_img = r.forward_views(P, cams_b, sh_degree=1, grad_mode=mode, tight_tiles=tight).clone()
    want = {k: t.clone() for k, t in r.backward_views(dL, want_mean2d=True).items()}
    tex = torch.tensor(b, dtype=torch.float32, device=gpu_device).repeat(HS, WS, 1).contiguous()
    img = r.forward_views(P, cams_0, sh_degree=1, grad_mode=mode, tight_tiles=tight)
    keep = mode == 0 and not tight                               # one combination repeats the lookup inside the backward instead
    s = r.sky_forward(tex, img, want_sky_rgb=True)
    r.backward_composite(dL)
    g_tex = r.sky_backward(tex, dL, sky_rgb=None if keep else s)
    got = r.backward_project(want_mean2d=True)
    torch.cuda.synchronize()
    r.close()
    err = float((img - want_img).abs().max())
    print(f"mode {mode} tight {tight}: image differs from the bg path by {err:.2e}")
    assert err <= 1e-6
    for k in list(KEYS) + ["mean2d"]:
        m, worst = rel_close(got[k].cpu().numpy(), want[k].cpu().numpy(), 1e-4, 2e-6)
        print(f"  {k}: worst error / tolerance {worst:.3f}")
        assert m.all(), (k, worst)
        assert float(want[k].abs().max()) > 0
    assert np.isfinite(g_tex.cpu().numpy()).all() and float(g_tex.abs().max()) > 0


def test_the_sky_term_reaches_the_gradients(gpu_device, scene_b):
    """without dvs_sky_backward_views the bg = 0 gradients are NOT those of the bg path: the comparison above has teeth"""
    n, W, H, P, dL = scene_b["n"], scene_b["W"], scene_b["H"], scene_b["P"], scene_b["dL"]
    cam_b, cam_0 = dv.synth_camera(scene_b["spec"], 1), dv.synth_camera(scene_b["spec"], 1)
    cam_b.bg[0], cam_b.bg[1], cam_b.bg[2] = 0.2, 0.7, 0.4
    cam_0.bg[0] = cam_0.bg[1] = cam_0.bg[2] = 0.0
    r = Rasterizer(0, max_splats=n, max_w=W, max_h=H)
    r.forward(P, cam_b, sh_degree=1)
    want = r.backward(dL[0].contiguous())["opacity"].clone()
    r.forward(P, cam_0, sh_degree=1)
    got = r.backward(dL[0].contiguous())["opacity"]
    r.close()
    m, _ = rel_close(got.cpu().numpy(), want.cpu().numpy(), 1e-4, 2e-6)
    assert not m.all()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def cameras_c(W=40, H=24):
    """six off-centre 110-degree cameras at the origin: along +Z, -Z, +X, -X, straight up (+Y) and straight down"""
    X, Y, Z = np.eye(3)
    axes = [(Z, X), (-Z, -X), (X, -Z), (-X, Z), (Y, X), (-Y, X)]
    return [intrinsics_camera(look(f, rt), np.zeros(3), 14.0, 13.0, 0.5 * W + 2.3, 0.5 * H - 1.7, W, H) for f, rt in axes]


def scene_c(seed=SEED_C, n=600):
    r = np.random.default_rng(seed)
    dirs = r.normal(0, 1, (n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    P = {"pos": dirs * r.uniform(3, 6, (n, 1)), "sh0": np.full((n, 3), -10.0), "shN": np.zeros((n, 15, 3)), "opacity": r.normal(0, 1.5, n),
         "scale": np.log(r.uniform(0.15, 0.5, (n, 1))) + r.normal(0, 0.15, (n, 3)), "rot": r.normal(0, 1, (n, 4))}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}


@pytest.mark.parametrize("mode", [0, 1])
def test_varying_texture_matches_the_reference(gpu_device, mode):
    tex = np.random.default_rng(21).uniform(0, 1, (HS, WS, 3)).astype(np.float32)
    cams = cameras_c()
    facts, g_tex, g_ref = run_against_reference(gpu_device, scene_c(), cams, tex, mode=mode, what=f"varying texture, mode {mode}:")
    idx = np.concatenate([SR.taps(f["d"], WS, HS)[0].reshape(-1, 4) for f in facts])
    x0, x1 = idx[:, 0] % WS, idx[:, 1] % WS
    assert ((x0 == WS - 1) & (x1 == 0)).any(), "no pixel across the u wrap"
    ylat = np.concatenate([np.arcsin(np.clip(f["d"][..., 1], -1, 1)).reshape(-1) for f in facts]) / np.pi + 0.5
    assert (ylat * HS - 0.5 < 0).any() and (ylat * HS - 0.5 > HS - 1).any(), "a v clamp is not hit"
    assert all(f["took"] >= 30 for f in facts), [f["took"] for f in facts]
    assert np.abs(g_ref).max() > 1.0 and max(np.abs(f["ref"]).max() for f in facts) > 0.1


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def test_long_lists_empty_tiles_and_saturated_pixels(gpu_device):
    """tests/test_gpu_depth.py's scene with the importance test's seed: a tile with more than 256 walked entries (a second LDS batch), an empty tile, a saturating stack"""
    tex = np.random.default_rng(22).uniform(0, 1, (HS, WS, 3)).astype(np.float32)
    facts, _, _ = run_against_reference(gpu_device, colourless(RS.scene_params(12)), RS.cameras(), tex, what="depth-test scene:")
    for f in facts:
        e = f["e"]
        length = e["ranges"][:, 1].astype(np.int64) - e["ranges"][:, 0]
        assert (length == 0).any() and length.max() > 256 and e["n_contrib"].max() > 256
        assert (e["final_T"] < 1e-3).any()


def test_a_saturated_view_and_a_view_that_sees_nothing(gpu_device):
    W, H = 40, 24
    X, Y, Z = np.eye(3)
    cams = [intrinsics_camera(look(Z, X), np.zeros(3), 30.0, 30.0, 0.5 * W, 0.5 * H, W, H), intrinsics_camera(look(-Z, -X), np.zeros(3), 30.0, 30.0, 0.5 * W, 0.5 * H, W, H)]
    r = np.random.default_rng(4)
    n = 1000                                                     # a wall of large opaque splats in front of view 0, behind view 1
    P = {"pos": np.stack([r.uniform(-4, 4, n), r.uniform(-3, 3, n), r.uniform(3.5, 4.5, n)], 1), "sh0": np.full((n, 3), -10.0), "shN": np.zeros((n, 15, 3)),
         "opacity": np.full(n, 4.0), "scale": np.full((n, 3), np.log(0.6)), "rot": np.tile([1.0, 0, 0, 0], (n, 1))}
    P = {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}
    tex = np.random.default_rng(23).uniform(0, 1, (HS, WS, 3)).astype(np.float32)
    facts, g_tex, g_ref = run_against_reference(gpu_device, P, cams, tex, what="wall:")
    sat, none = facts
    # the forward ends a pixel BEFORE the entry that would take T below 1e-4, and an entry takes at most 0.99 of T: a saturated pixel's
    # final_T stays between 1e-4 and 1e-4 / (1 - 0.99) = 1e-2 — it cannot get below 1e-4 — and its n_contrib stops short of the tile's list
    length = sat["e"]["ranges"][:, 1].astype(np.int64) - sat["e"]["ranges"][:, 0]
    tile_len = length[(np.arange(H)[:, None] // 16) * ((W + 15) // 16) + np.arange(W)[None, :] // 16]
    assert (sat["e"]["final_T"] < 1e-2).all() and (sat["e"]["n_contrib"] < tile_len).all(), sat["e"]["final_T"].max()
    assert np.abs(sat["out"] - sat["C0"]).max() <= 1e-2                       # the sky term vanishes behind the wall
    assert (none["e"]["final_T"] == 1).all() and (none["e"]["n_contrib"] == 0).all() and none["took"] == 0
    assert np.array_equal(none["out"], none["s"]) and (none["rows"] == 0).all()   # out = 0 + 1 s, bit for bit; nothing for the rows


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors(gpu_device, scene_b):
    n, W, H, P, dL = scene_b["n"], scene_b["W"], scene_b["H"], scene_b["P"], scene_b["dL"]
    cam = dv.synth_camera(scene_b["spec"], 1)
    cam.bg[0] = cam.bg[1] = cam.bg[2] = 0.0
    r = Rasterizer(0, max_splats=n, max_w=W, max_h=H)
    tex = torch.zeros((HS, WS, 3), device=gpu_device)
    img = torch.zeros((3, H, W), device=gpu_device)
    g_tex = torch.zeros_like(tex)
    sky = _lib.Sky(tex.data_ptr(), WS, HS)
    cams = (dv.Camera * 1)(cam)
    opts = dv.Opts()
    STATE, INVALID = 4, 1
    assert dv.lib.dvs_sky_forward_views(r.ctx, None, cams, 1, C.byref(sky), img.data_ptr(), None) == STATE          # before any forward
    assert dv.lib.dvs_sky_backward_views(r.ctx, None, cams, 1, C.byref(opts), C.byref(sky), dL.data_ptr(), None, g_tex.data_ptr()) == STATE
    out = r.forward(P, cam, sh_degree=1)
    assert dv.lib.dvs_sky_backward_views(r.ctx, None, cams, 1, C.byref(opts), C.byref(sky), dL.data_ptr(), None, g_tex.data_ptr()) == STATE   # no composite backward pending
    assert b"composite backward" in dv.lib.dvs_last_error()
    two = (dv.Camera * 2)(cam, cam)
    assert dv.lib.dvs_sky_forward_views(r.ctx, None, two, 2, C.byref(sky), out.data_ptr(), None) == STATE           # not the forward's n_views
    with_bg = (dv.Camera * 1)(cam); with_bg[0].bg[2] = 0.5
    assert dv.lib.dvs_sky_forward_views(r.ctx, None, with_bg, 1, C.byref(sky), out.data_ptr(), None) == INVALID
    r.backward_composite(dL[0].contiguous())
    assert dv.lib.dvs_sky_backward_views(r.ctx, None, with_bg, 1, C.byref(opts), C.byref(sky), dL.data_ptr(), None, g_tex.data_ptr()) == INVALID
    before = out.clone()
    r.sky_forward(tex, out)                                                   # a fresh (all-zero) sky: the image over a black background
    r.sky_backward(tex, dL[0].contiguous(), g_tex=g_tex)
    r.backward_project()
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    assert dv.lib.dvs_sky_backward_views(r.ctx, None, cams, 1, C.byref(opts), C.byref(sky), dL.data_ptr(), None, g_tex.data_ptr()) == STATE   # the rows were consumed
    r.close()
