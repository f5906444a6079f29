"""`train_step` at step level with the sky model on (--enableBg 1): K iterations of the product against tests/train_step_ref.py with
`sky=` — oracle gradients at cam.bg = 0, the per-pixel background out = C + final_T s restated by linearity of the oracle's backward in
dL and bg, tests/sky_ref.py's rays / lookup / texel gradient, numpy Adam on the texture. tests/test_gpu_sky.py pins the kernels of
csrc/sky.hip one by one and tests/test_gpu_sky_train.py runs the product where no splat covers a pixel; these pin how
gstrain/trainer_step.cpp wires the sky into the step where final_T is neither 0 nor 1.

One scene for every case, chosen on the CPU against the oracle alone (test_the_scene_has_the_case): synthetic 64x64, 1500 splats, six
cameras, seed 41, the start model of tests/test_train_step_options.py, log-scales as they are (scale_offset 0: at N = 1500 the model is
translucent — final_T in (0.05, 0.95) on 0.69 .. 0.71 of every camera's pixels, and the final_T part is 0.43 of the opacities' and 0.62
of the scales' gradient; at N = 2000 the share is 0.36, with the scales 0.4 larger it is 0). Six cameras, because with them the first
sixteen draws of the camera stream never hand both ranks the same view. The model is written as iteration START = 1 together with a
seeded random 32x16 texture in [0, 1] and resumed through --load_itr: the sky term is large from the first step, and the resumed step
number is what the bias corrections must use (a resume at 0 could not tell s.it from a counter that starts with the process). START is
1 and not later because a resume skips the fast start of the position-rate schedule: float32 storage of the coordinates alone costs
the float32 restatement 4.7e-3 .. 5.2e-3 of the positions' update against float64 at START = 1 (2.7e-3 at 0, 1.1e-2 at 3), and the
bar on the product stays the 1e-2 of the other trajectory tests.

What each GPU case guards (render_backward / step_sky of gstrain/trainer_step.cpp):
  l1           the loss on d_out AFTER dvs_sky_forward_views (C + final_T s, not C); composite backward -> dvs_sky_backward_views ->
               backward_project, so that the final_T term is in the rows A9 consumes; step_sky's dvs_adam_step: SKY_LR, betas, eps, s.it.
  ssim_views4  the multi-view pass: one dvs_sky_forward_views / dvs_sky_backward_views over pass_views = 4, d_sky_grad zeroed once per
               step and summed over the step's views; the SSIM mix formed from the composited image.
  sequential   DVS_VIEWS_MODE=sequential: the `+ v * img` offsets of d_out, d_dL and d_sky_rgb, opts.accumulate on the rows, d_sky_grad
               NOT zeroed between the passes. Same restatement as ssim_views4: both view modes land on the same numbers.
  two_ranks    step_sky's all-reduce of d_sky_grad (the ranks hold different views in every step); after the sky pass has modified the
               rows: the factorised exchange with A9 whole, the same with the chunked A9 (DVS_A9_CHUNKS=4:
               dvs_raster_backward_project_chunk per 512 splats), and the all-reduce exchange; both ranks save byte-identical textures.
  level        a coarser level of the resolution schedule: s.Wd x s.Hd = 32x32 and the level cameras in both sky calls, img = 3 Wd Hd
               while d_sky_rgb is sized for 64x64.
  mask         k_mask_mul in loss_of_view multiplies d_dL BEFORE dvs_sky_backward_views reads it (texel gradient and rows).

Texture pinned share (the share of the moved, firmly supported texel values on which the float32 and the float64 restatement agree to a
quarter of the bar; measured on the CPU with oracle targets, test_sky_case_is_pinned_on_the_cpu asserts it): l1, ssim_views4 (and
sequential), two_ranks, level 1.0; mask 0.9885 (TEX_SHARE below). The GPU cases assert that share minus 0.05. The six cameras see an
eighth of the sphere: 64 of the 512 texels (58 under the mask) are firmly supported, 448 are untouched, at most 2 in between.

A texel value is compared when the bilinear weight the step's pixels put on its texel sums to more than 1e-3, and asserted bit-equal to
the file that was written when no pixel reaches its texel even with every ray turned by 1e-5 rad (Adam's eps = 1e-15 turns ANY non-zero
gradient into a full-size step, so a texel that a float32 ray touches with weight 1e-6 and the float64 ray misses is not comparable
between any two implementations); the texels in between are counted and bounded (<= 2 %).

CPU part (not marked gpu): the restatement against fp64 finite differences of its own loss, the scene's final_T and G_T shares, the
pinned shares, and five WRONG restatements that must each end >= 10x the bar away from the right one."""
import json
import os
import re
import types
import numpy as np
import pytest
import divshot_amd as dv
from oracle.oracle import Oracle
import sky_ref as SR
from train_step_ref import TrainStepRef, KEYS, LR, camera_stream, ellipse_mask
from test_gpu_parity import REPORT as _PARITY_REPORT
from test_train_step import _run, _read_ply, _write_ply, _scene, _hip_targets, _compare, COMMON
from test_train_step_options import _start_model, _oracle_targets, _pinned, RTOL, SHARE_L1, SHARE_SSIM

SCENE = dict(n=1500, W=64, H=64, cams=6, sh=1, seed=41, scale_offset=0.0)
HS, TEX_SEED, SKY_LR, START = 16, 5, 0.02, 1
CASES = {
    "l1": dict(K=8),
    "ssim_views4": dict(K=6, views=4, ssim=0.2),
    "sequential": dict(K=6, views=4, ssim=0.2),
    "two_ranks": dict(K=8, world=2),
    "level": dict(K=8, level=1),
    "mask": dict(K=8, mask=True),
}
# measured on the CPU (oracle targets): test_sky_case_is_pinned_on_the_cpu prints and asserts them
TEX_SHARE = {"l1": 1.0, "ssim_views4": 1.0, "sequential": 1.0, "two_ranks": 1.0, "level": 1.0, "mask": 0.988}
SRC = "synthetic:N={n},W={W},H={H},cams={cams},sh={sh},seed={seed}".format(**SCENE)


def _scene_and_start():
    c = SCENE
    spec, cams = _scene(c["n"], c["W"], c["H"], c["cams"], c["sh"], c["seed"])
    init = _start_model(spec, c["seed"])
    init["scale"] = init["scale"] + np.float32(c["scale_offset"])
    return spec, cams, init


def _start_texture(hs=HS, seed=TEX_SEED):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (hs, 2 * hs, 3)).astype(np.float32)


def _level_of(c, cams, targets):
    """the cameras and fp32 targets the case's steps run on: the full-size ones, or level 1 of the resolution schedule"""
    if not c.get("level"):
        return cams, targets
    from test_resolution_schedule import _level_inputs
    lc, lt, _ = _level_inputs(cams, targets, c["level"], False, False)[c["level"]]
    return lc, lt


def _restate(c, cams, targets, init, dtype, cls=TrainStepRef, sky_lr=SKY_LR):
    """the restatement of a case (a CASES entry or a dict of its form) after the case's K steps"""
    r = cls(Oracle, cams, targets, init, SCENE["sh"], START + c["K"], dtype, views_per_step=c.get("views", 1), world=c.get("world", 1),
            ssim_weight=c.get("ssim", 0.0), start_step=START, mask=c.get("mask", False), sky=dict(tex=_start_texture(), lr=sky_lr))
    lc, lt = _level_of(c, cams, targets)
    r.cams, r.targets = lc, [np.asarray(t, r.dt) for t in lt]
    for _ in range(c["K"]):
        r.train_step()
    return r


def _draws(name):
    c = CASES[name]
    return camera_stream(SCENE["cams"], c["K"] * c.get("views", 1) * c.get("world", 1))


def _texel_support(name, cams):
    """-> (wsum [Hs,Ws]: the bilinear weight the pixels of the case's views put on each texel, every view of every step counted once per
    use, pixels outside the case's mask not at all; reach [Hs,Ws] bool: some such pixel reaches the texel when its ray is turned by up to
    1e-5 rad about any axis — about 5e-5 texels, ten times what float32 trigonometry moves a tap by)"""
    ws, hs = 2 * HS, HS
    wsum, reach = np.zeros(hs * ws), np.zeros(hs * ws, bool)
    lc = [dv.camera_downscale(c, 1 << CASES[name].get("level", 0)) for c in cams]        # (what _level_inputs hands the restatement)
    for ci in sorted(set(_draws(name))):
        cam = lc[ci]
        pw = ellipse_mask(cam.width, cam.height).astype(np.float64) if CASES[name].get("mask") else np.ones((cam.height, cam.width))
        d = SR.rays(cam.proj[:], cam.width, cam.height)
        idx, w = SR.taps(d, ws, hs)
        np.add.at(wsum, idx.reshape(-1), (w * pw[..., None]).reshape(-1) * _draws(name).count(ci))
        for axis in range(3):
            for sign in (-1e-5, 1e-5):
                e = d.copy()
                e[..., axis] += sign
                e /= np.linalg.norm(e, axis=-1, keepdims=True)
                reach[SR.taps(e, ws, hs)[0][pw > 0].reshape(-1)] = True
        reach[idx[pw > 0].reshape(-1)] = True
    return wsum.reshape(hs, ws), reach.reshape(hs, ws)


def _compare_texture(got_tex, r32, r64, tex0, support, min_fraction, report, ssim):
    """the texture under `_compare` itself (imported, not copied): its metric, its `comparable` rule and its bars, over the moved values
    of firmly supported texels; untouched texels bit-equal to the start texture"""
    wsum, reach = support
    t64 = r64.sky["tex"]
    untouched, firm = ~reach, wsum > 1e-3
    doubtful = ~untouched & ~firm
    sel = firm[..., None] & (t64 != tex0)
    report["texture_support"] = dict(untouched=float(untouched.mean()), firm=float(firm.mean()), doubtful=float(doubtful.mean()), moved=float(sel.mean()))
    assert untouched.mean() > 0.1 and firm.mean() > 0.08 and doubtful.mean() <= 0.02, report["texture_support"]
    assert np.array_equal(t64[untouched], tex0[untouched].astype(np.float64))                  # zero gradient: no Adam movement
    assert np.array_equal(got_tex[untouched].view(np.uint32), tex0[untouched].view(np.uint32)), "a texel no pixel touches has moved"
    assert sel[firm].mean() > 0.9, report["texture_support"]
    # `_compare` walks the six splat groups of objects with a .P dict: every group is handed the same texel values, so it compares the
    # texture six times over and the six reports are identical — only one of them (filed under "pos") is kept
    shim = lambda a: types.SimpleNamespace(P=dict.fromkeys(KEYS, a[sel]))
    rep = {}
    kw = dict(worst_rtol=1e-3, quantile=0.995) if ssim else {}
    try:
        _compare(dict.fromkeys(KEYS, got_tex[sel]), shim(r32.sky["tex"]), shim(t64), dict.fromkeys(KEYS, tex0[sel]), RTOL, min_fraction, rep, **kw)
    finally:
        report["texture"] = rep.get("pos")
    assert report["texture"]["rel_l2_of_update"] < 1e-2, report["texture"]
    return report["texture"]["comparable"]


# ---- wrong restatements: each differs from TrainStepRef in the one place its name says -------------------------------------------------------
class _NoFinalT(TrainStepRef):
    def final_T_gradient(self, cam, dL, s):
        return {k: np.zeros_like(self.P[k]) for k in KEYS}


class _LossOnC(TrainStepRef):
    def loss_image(self, C, T, s):
        return C


class _LastViewTexture(TrainStepRef):
    def tex_gradient(self):
        return self.tex_grads[-1]


class _BiasFromZero(TrainStepRef):
    def sky_step_number(self):
        return self.step - self.start + 1


class _Recording(TrainStepRef):
    """keeps the final_T part of the step's gradient beside the sum"""
    def gradients(self):
        self.GT = {k: np.zeros_like(v) for k, v in self.P.items()}
        return super().gradients()

    def final_T_gradient(self, cam, dL, s):
        g = super().final_T_gradient(cam, dL, s)
        for k in KEYS:
            self.GT[k] += g[k].reshape(self.GT[k].shape)
        return g


@pytest.fixture(scope="module")
def cpu_scene():
    spec, cams, init = _scene_and_start()
    return spec, cams, init, _oracle_targets(spec, cams, SCENE["sh"])


# ---- CPU: the restatement itself ---------------------------------------------------------------------------------------------------------
def test_restated_pieces_are_sky_refs_in_float64(cpu_scene):
    """in float64 the restatement's lookup and texel gradient ARE tests/sky_ref.py's (same sums, same order: bit for bit)"""
    spec, cams, init, tg = cpu_scene
    r = TrainStepRef(Oracle, cams, tg, init, SCENE["sh"], 10, np.float64, sky=dict(tex=_start_texture(), lr=SKY_LR))
    cam = cams[1]
    d = SR.rays(cam.proj[:], cam.width, cam.height)
    assert np.array_equal(r.sky_lookup(cam), SR.lookup(r.sky["tex"], d))
    rng = np.random.default_rng(0)
    T, g = rng.uniform(0, 1, (64, 64)), rng.standard_normal((3, 64, 64))
    assert np.array_equal(r.sky_tex_gradient(cam, T, g), SR.sky_backward_tex(T, g, d, 2 * HS, HS))
    C = rng.uniform(0, 1, (3, 64, 64))
    assert np.array_equal(r.loss_image(C, T, r.sky_lookup(cam)), SR.sky_forward(C, T, r.sky["tex"], d)[0])
    assert r.sky_step_number() == 1
    r.step = r.start = 7
    assert r.sky_step_number() == 8                    # Step::it = step + 1 (trainer_step.cpp plan_step), what step_sky passes on


@pytest.mark.parametrize("w", [0.0, 0.2])
def test_restated_gradient_against_finite_differences(w):
    """fp64 central differences of the restated loss (1 - w) mean|out - t| + w (1 - SSIM(out, t)), out = C + final_T s, on the 48-splat
    32x32 scene of tests/test_oracle_fd.py with a random 32x16 texture: 60 splat parameters over the six groups against G_colour + G_T,
    40 touched texels against the texture gradient; the two-step-size discontinuity filter and the bars of test_oracle_fd.py."""
    spec = dv.make_spec(48, 32, 32, sh_degree=1, seed=1)
    P = {k: v.astype(np.float64) for k, v in dv.synth_splats(spec).items()}
    P["scale"] += 0.7
    cam = dv.synth_camera(spec, 0)
    tgt = dv.synth_target(spec, 0).astype(np.float64)
    tex = np.random.default_rng(2).uniform(0, 1, (16, 32, 3))
    r = _Recording(Oracle, [cam], [tgt], P, 1, 10, np.float64, ssim_weight=w, sky=dict(tex=tex, lr=SKY_LR))
    G = r.gradients()
    g_tex = r.tex_gradient()
    T = r.orc.get("final_T")
    assert ((T > 0.05) & (T < 0.95)).mean() > 0.25
    for k in ("opacity", "scale", "pos"):
        assert np.linalg.norm(r.GT[k]) > 0.05 * np.linalg.norm(G[k]), k       # the final_T part is in what is differentiated

    def loss():
        r.gradients()
        return r.losses[-1]

    rng = np.random.default_rng(3)
    total = bad = 0
    touched = np.flatnonzero(np.abs(g_tex).reshape(-1) > 0)
    assert touched.size >= 40
    pick = {k: rng.choice(r.P[k].size, 10, replace=False) for k in KEYS}
    pick["shN"] = rng.choice(48, 10, replace=False) * 45 + rng.integers(0, 9, 10)       # the nine coefficients of degree 1 (the rest has no gradient)
    groups = [(r.P[k].reshape(-1), G[k].reshape(-1), pick[k]) for k in KEYS]            # (views: a write lands in the restatement's parameters)
    groups.append((r.sky["tex"].reshape(-1), g_tex.reshape(-1), rng.choice(touched, 40, replace=False)))
    for flat, gk, idxs in groups:
        scale = np.abs(gk).max() + 1e-30
        for i in idxs:
            old = flat[i]
            fds = []
            for eps in (1e-5, 2.5e-6):
                flat[i] = old + eps; Lp = loss()
                flat[i] = old - eps; Lm = loss()
                fds.append((Lp - Lm) / (2 * eps))
            flat[i] = old
            total += 1
            if abs(fds[0] - fds[1]) > 1e-3 * scale + 1e-2 * abs(fds[1]):
                bad += 1
                continue
            assert abs(fds[1] - gk[i]) <= 1e-3 * abs(gk[i]) + 2e-5 * scale, (int(i), fds, float(gk[i]))
    assert total == 100 and bad <= 0.02 * total, (bad, total)


def test_the_scene_has_the_case(cpu_scene):
    """the start model under every training camera: final_T in (0.05, 0.95) on at least a quarter of the pixels; in the first step of
    the four-view case the final_T part is at least 5 % of the gradient of the opacities and of the scales; in every step of the
    two-rank case the ranks hold different cameras"""
    spec, cams, init, tg = cpu_scene
    o = Oracle(np.float64)
    shares = []
    for cam in cams:
        o.forward(init, cam, sh_degree=SCENE["sh"])
        T = o.get("final_T")
        shares.append(float(((T > 0.05) & (T < 0.95)).mean()))
    r = _Recording(Oracle, cams, tg, init, SCENE["sh"], START + 6, np.float64, views_per_step=4, start_step=START, sky=dict(tex=_start_texture(), lr=SKY_LR))
    G = r.gradients()
    part = {k: float(np.linalg.norm(r.GT[k]) / np.linalg.norm(G[k])) for k in KEYS}
    print("final_T in (0.05, 0.95):", shares, "|G_T| / |G|:", part)
    assert min(shares) >= 0.25, shares
    assert part["opacity"] >= 0.05 and part["scale"] >= 0.05, part
    d = _draws("two_ranks")
    assert all(a != b for a, b in zip(d[0::2], d[1::2])), d
    assert len(set(_draws("ssim_views4"))) == SCENE["cams"]


def _texture_share(r32, r64, tex0, support):
    firm = support[0] > 1e-3
    sel = firm[..., None] & (r64.sky["tex"] != tex0)
    t64, t32 = r64.sky["tex"][sel], r32.sky["tex"][sel].astype(np.float64)
    return float((np.abs(t32 - t64) <= 0.25 * RTOL * np.maximum(np.abs(t64), 1e-2)).mean())


@pytest.mark.parametrize("name", ["l1", "ssim_views4", "two_ranks", "level", "mask"])
def test_sky_case_is_pinned_on_the_cpu(cpu_scene, name):
    """float32 against float64 of the restatement alone (oracle targets): every splat group pins the share the GPU case asserts and uses
    at most half of the update bar (`_pinned`; three quarters for the positions, see the module docstring: measured 4.7e-3 .. 5.2e-3),
    and the texture pins TEX_SHARE[name] >= 0.5 (`sequential` is ssim_views4's restatement). Measured, worst group (opacity): l1 .9993,
    ssim_views4 .996, two_ranks .9953, level .9973, mask .986."""
    spec, cams, init, tg = cpu_scene
    r32, r64 = (_restate(CASES[name], cams, tg, init, dt) for dt in (np.float32, np.float64))
    shares = _pinned(r32, r64, init, SHARE_SSIM if CASES[name].get("ssim") else SHARE_L1, pos_update=0.0075)
    tex = _texture_share(r32, r64, _start_texture(), _texel_support(name, cams))
    print(name, shares, "texture:", tex)
    assert tex >= TEX_SHARE[name] - 1e-9 and TEX_SHARE[name] >= 0.5, (tex, TEX_SHARE[name])
    np.testing.assert_allclose(r32.losses, r64.losses, rtol=2e-4)


def _distance(a, b, a0, k):
    """median over the values that moved in either trajectory of |a - b| / max(|a|, 1e-2): `_compare`'s metric"""
    moved = (a != a0.reshape(a.shape)) | (b != a0.reshape(a.shape))
    assert moved.mean() > 0.05, (k, moved.mean())          # (the six cameras see an eighth of the sphere)
    return float(np.median((np.abs(a - b) / np.maximum(np.abs(a), 1e-2))[moved]))


def test_sky_case_discriminates(cpu_scene):
    """Five wrong restatements of the four-view L1 step (K = 6, resumed at START), each against the right float64 trajectory: the median
    moved value of the named group, or of the texture, ends more than 10x the bar of 1e-4 away (the assertion: > 1e-3). Measured: final_T term omitted 2.8e-2
    (opacity), loss on C 1.2e-2 (sh0), last view's texture gradient only 4.7e-2, bias correction from 0 2.0e-2, feature rate 1.6e-1."""
    spec, cams, init, tg = cpu_scene
    case = dict(K=6, views=4)
    f64 = lambda **kw: _restate(case, cams, tg, init, np.float64, **kw)
    right = f64()
    wrong = {
        "final_T term omitted": (f64(cls=_NoFinalT), "opacity"),
        "loss on C": (f64(cls=_LossOnC), "sh0"),
        "texture gradient of the last view only": (f64(cls=_LastViewTexture), "texture"),
        "texture bias correction from 0": (f64(cls=_BiasFromZero), "texture"),
        "feature rate for the texture": (f64(sky_lr=LR["featurelr"]), "texture"),
    }
    tex0 = _start_texture().astype(np.float64)
    out = {}
    for what, (r, k) in wrong.items():
        if k == "texture":
            out[what] = _distance(right.sky["tex"], r.sky["tex"], tex0, k)
        else:
            out[what] = _distance(right.P[k], r.P[k], np.asarray(init[k], np.float64), k)
    print(out)
    for what, d in out.items():
        assert d > 10 * RTOL, (what, d)


# ---- GPU: the product ------------------------------------------------------------------------------------------------------------------
def _write_sky(path, tex):
    tex = np.ascontiguousarray(tex, "<f4")
    with open(path, "wb") as f:
        f.write(b"DVSSKY1\0" + np.array([tex.shape[1], tex.shape[0]], "<u4").tobytes() + tex.tobytes())


def _sky_args(K):
    return ["--inputPath", SRC, "--maxIteration", str(START + K), "--load_itr", str(START), "--enableBg", "1", "--skyResolution", str(HS)]


def _sky_env(extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("DVS_SKY_RESOLUTION", "DVS_SKY_LR", "DVS_VIEWS_MODE", "DVS_EXCHANGE", "DVS_A9_CHUNKS", "DVS_EXCHANGE_PIPELINE",
                                                             "DVS_FORCE_COMM", "DVS_TIGHT_TILES")}
    env.update(DVS_SKY_LR=repr(SKY_LR))
    env.update(extra or {})
    return env


def _seed_run(out, init):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    _write_ply(f"{out}_{START}.ply", init)
    _write_sky(f"{out}_{START}.sky", _start_texture())


def _check_log(log, rank=0):
    assert "(resumed)" in log and "densify @" not in log, log[-3000:]
    assert re.search(rf"sky: read the {2 * HS}x{HS} texture from .*_{START}\.sky", log), log[-3000:]
    if rank == 0:                                                           # (the configuration lines are rank 0's)
        assert re.search(rf"config: skyModel {2 * HS}x{HS}: .*lr {SKY_LR:g}\)", log), log[-3000:]


def _product(tmp_path, name, init, flags, env=None):
    from test_gpu_sky_train import read_sky
    K = CASES[name]["K"]
    out = str(tmp_path / name / "it")
    _seed_run(out, init)
    p = _run(_sky_args(K) + ["--outputPath", out] + flags, timeout=300, env=_sky_env(env))
    _check_log(p.stderr)
    return p, _read_ply(f"{out}_{START + K}.ply"), read_sky(f"{out}_{START + K}.sky")


@pytest.fixture(scope="module")
def gpu_scene():
    spec, cams, init = _scene_and_start()
    return spec, cams, init, _hip_targets(spec, cams, SCENE["sh"])


@pytest.fixture(scope="module")
def restated(gpu_scene):
    """float32 and float64 restatement per case, computed once (ssim_views4 and sequential share one)"""
    spec, cams, init, tg = gpu_scene
    cache = {}

    def get(name):
        key = "ssim_views4" if name == "sequential" else name
        if key not in cache:
            cache[key] = tuple(_restate(CASES[key], cams, tg, init, dt) for dt in (np.float32, np.float64))
        return cache[key]
    return get


def _bars_and_report(name, tag, got, got_tex, r32, r64, init, cams, report):
    ssim = bool(CASES[name].get("ssim"))
    try:
        if ssim:
            _compare(got, r32, r64, init, RTOL, SHARE_SSIM, report, worst_rtol=1e-3, quantile=0.995)
        else:
            _compare(got, r32, r64, init, RTOL, SHARE_L1, report)
        for k in KEYS:
            assert report[k]["rel_l2_of_update"] < 1e-2, (k, report[k])
        _compare_texture(got_tex, r32, r64, _start_texture(), _texel_support(name, cams), TEX_SHARE[name] - 0.05, report, ssim)
    finally:
        out_dir = os.path.dirname(_PARITY_REPORT)             # the run-report directory of the parity suites, beside their reports
        os.makedirs(out_dir, exist_ok=True)
        json.dump(report, open(os.path.join(out_dir, f"train_step_parity_sky_{tag}.json"), "w"), indent=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["l1", "ssim_views4", "sequential", "level", "mask"])
def test_plugin_trajectory_with_the_sky(tmp_path, gpu_scene, restated, name):
    """K steps of the product with --enableBg 1 from the written model and texture against the restatement (see the module docstring for
    what each case guards): the six splat groups under the bars of the matching trajectory test of tests/test_train_step.py (L1: every
    pinned element within 1e-4, >= 0.90 pinned; SSIM: 0.995 quantile 1e-4, worst 1e-3, >= 0.85 pinned; update within 1e-2 in relative L2),
    the texture under the same bars on the values of firmly supported texels that moved (pinned share TEX_SHARE - 0.05), untouched texels
    bit-equal to the file that was written."""
    spec, cams, init, tg = gpu_scene
    c = CASES[name]
    flags = list(COMMON) + ["--warmupLength", "100000"]
    if c.get("ssim"):
        flags[flags.index("--ssim") + 1] = str(c["ssim"])
    if c.get("views", 1) > 1:
        flags += ["--viewsPerIter", str(c["views"])]
    if c.get("level"):
        flags += ["--resolutionSchedule", "100", "--numDownscales", str(c["level"])]
    if c.get("mask"):
        flags += ["--useMask", "1"]
    p, got, got_tex = _product(tmp_path, name, init, flags, {"DVS_VIEWS_MODE": "sequential"} if name == "sequential" else None)
    if name == "sequential":
        assert "one pass per view, gradients accumulated (DVS_VIEWS_MODE=sequential)" in p.stderr
    if c.get("level"):
        assert re.findall(r"resolution @(\d+): (\d+x\d+)", p.stderr) == [(str(START + 1), "32x32")], p.stderr[-3000:]      # every step at level 1
    if c.get("mask"):
        assert "useMask 1" in p.stderr
    assert got["pos"].shape[0] == SCENE["n"]
    r32, r64 = restated(name)
    _bars_and_report(name, name, got, got_tex, r32, r64, init, cams, {})


# the gradient exchanges of the two-rank case: DVS_EXCHANGE, DVS_A9_CHUNKS (1: one dvs_raster_backward_project over all splats; 4: the
# chunked branch of render_backward — n = 1500 >= 256 x 4, chunks of 512 splats, so dvs_raster_backward_project_chunk runs three times
# after dvs_sky_backward_views and each chunk's geometry all-reduce leaves behind it)
EXCHANGES = {"factorised": ("factorised", 1), "factorised_chunks4": ("factorised", 4), "allreduce": ("allreduce", 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", list(EXCHANGES))
def test_plugin_two_ranks_with_the_sky(tmp_path, gpu_scene, restated, exchange):
    """two ranks, one view each per step and never the same one (test_the_scene_has_the_case), against the restatement with world = 2:
    the texture gradient is summed over the ranks, the splat gradients go through the factorised exchange (all-gather of the colour
    gradients; A9 whole, or in splat chunks with DVS_A9_CHUNKS=4 — the log says which) or the plain all-reduce after the sky pass has
    added to the rows; both ranks save the same bytes. Every variable that selects a path of the step is set here, whatever the caller's
    environment holds (`_plugin_run` passes that on)."""
    from test_gpu_multirank import _plugin_run
    from test_gpu_sky_train import read_sky
    spec, cams, init, tg = gpu_scene
    K = CASES["two_ranks"]["K"]
    mode, chunks = EXCHANGES[exchange]
    tag = "two_ranks_" + exchange
    _seed_run(os.path.join(str(tmp_path), tag, "it"), init)
    env = {"DVS_SKY_LR": repr(SKY_LR), "DVS_EXCHANGE": mode, "DVS_A9_CHUNKS": str(chunks), "DVS_EXCHANGE_PIPELINE": "0", "DVS_VIEWS_MODE": "multi"}
    out, res = _plugin_run(tmp_path, tag, _sky_args(K) + list(COMMON) + ["--warmupLength", "100000"], 2, extra_env=env, timeout=300)
    for rank, (_, _, log) in enumerate(res):
        _check_log(log, rank)
    log0 = res[0][2]
    assert ("factorised (all-gather" in log0) == (mode == "factorised"), log0[-3000:]
    assert (f"gradient exchange: A9 in {chunks} splat chunks" in log0) == (chunks > 1) and ("splat chunks" in log0) == (chunks > 1), log0[-3000:]
    assert "one pass per view" not in log0
    stop = START + K
    a, b = open(f"{out}_{stop}.sky", "rb").read(), open(f"{out}_{stop}.sky.rank1", "rb").read()
    assert a == b and len(a) == 16 + 2 * HS * HS * 12
    assert open(f"{out}_{stop}.ply", "rb").read() == open(f"{out}_{stop}.ply.rank1", "rb").read()
    r32, r64 = restated("two_ranks")
    _bars_and_report("two_ranks", tag, _read_ply(f"{out}_{stop}.ply"), read_sky(f"{out}_{stop}.sky"), r32, r64, init, cams, {})
