"""CPU restatement of one `train_step` of the gstrain plugin (A10) — TEST INFRASTRUCTURE, not product code.

What the reference's host calls per iteration is one opaque symbol, `train_step(scene)` (application/diverseshot-cli/source/
gs_train.cpp:156; flags main.cpp:24-25,46-48); the trainer behind it is closed source (README.md:46), so this file restates the step
this build's plugin defines (divshot_amd/gstrain/gstrain.cpp trainStep) from independent parts:

  camera draw (xorshift64, one stream) -> oracle forward (oracle/dvs_oracle.hpp) -> photometric gradient of (1 - w) L1 + w (1 - SSIM)
  ((1 - w) sign(out - target) / (3 W H) - w dSSIM/dout; w = --ssim, 0 = L1 only; the SSIM and its gradient restated analytically below)
  -> oracle backward in DVS_GRAD_LINEAGE -> per-group Adam in numpy (beta 0.9 / 0.999, eps 1e-15, bias-corrected) with the learning
  rates of gaussian_trainer_scene.hpp (position: extent x exponential decay) -> abs-grad densification statistics
  (sqrt((|gx| W/2)^2 + (|gy| H/2)^2) per visible splat, denominator + 1), and the statistic of `--absgrad 0`, the same expression on the
  signed dL/dmean2D.

Options of the step, each off by default (the host flags of gstrain/trainer_step.cpp plan_step / loss_of_view and gstrain.cpp trainStep): start_step (a resume
through --load_itr), progressive (SH degree min(sh, step // 1000)), antialias, pack_u8 (8-bit training views), mask (the synthetic
inscribed-ellipse mask on the photometric gradient), reset_alpha_every (the opacity reset inside the step), train_cams (the training
cameras of a hold-out), the light prune (prune_decisions / apply_prune), the importance prune (importance_scores /
importance_decisions) and sky (--enableBg 1: the learned texture behind the splats, its own section of TrainStepRef).

dtype float32 mirrors the arithmetic the plugin performs; float64 is the ground truth of the same recurrences. The parity test compares
the plugin with the float64 trajectory on every element where the float32 restatement itself stays within tolerance of it: Adam with
eps = 1e-15 turns a gradient that is pure rounding noise into a full-size step of either sign, and such elements are not comparable
between ANY two float32 implementations. The comparable fraction is bounded in the test.
"""
import numpy as np

KEYS = ("pos", "sh0", "shN", "opacity", "scale", "rot")
# gaussian_trainer_scene.hpp (defaults of GaussianTrainConfig; names gs_train.cpp:52-57)
LR = dict(poslrInit=0.00016, poslrFinal=0.0000016, featurelr=0.0025, opacitylr=0.05, scalinglr=0.005, rotationlr=0.001)


def _gauss_window(dt):
    x = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-x * x / (2 * 1.5 ** 2))
    return (g / g.sum()).astype(dt)


def _conv_same(img, g):
    """separable 11-tap convolution with zero padding (its own adjoint: the window is symmetric), img [H, W]"""
    H, W = img.shape
    p = np.pad(img, 5)
    t = sum(g[k] * p[:, k:k + W] for k in range(11))
    return sum(g[k] * t[k:k + H, :] for k in range(11))


def ssim_and_grad(x, y):
    """mean SSIM of x against y ([3, H, W]; 11x11 Gaussian window sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2 — the definition of
    include/dvs_train.h / csrc/ssim.hip, the standard one of the lineage) and its gradient d(mean SSIM)/dx, analytically, in x's dtype.
    With mu1 = g*x, E2 = g*x^2, E12 = g*xy the map is m = A B / (C D), A = 2 mu1 mu2 + C1, B = 2 (E12 - mu1 mu2) + C2,
    C = mu1^2 + mu2^2 + C1, D = (E2 - mu1^2) + sigma2 + C2, and d mean/dx = [ g*(dm/dmu1) + 2 x g*(dm/dE2) + y g*(dm/dE12) ] / N."""
    dt = x.dtype
    g = _gauss_window(dt)
    C1, C2 = dt.type(0.01 ** 2), dt.type(0.03 ** 2)
    two = dt.type(2.0)
    grad = np.zeros_like(x)
    tot = 0.0
    for c in range(3):
        xc, yc = x[c], y[c]
        mu1, mu2 = _conv_same(xc, g), _conv_same(yc, g)
        e2, e12 = _conv_same(xc * xc, g), _conv_same(xc * yc, g)
        s1, s2, s12 = e2 - mu1 * mu1, _conv_same(yc * yc, g) - mu2 * mu2, e12 - mu1 * mu2
        A, B = two * mu1 * mu2 + C1, two * s12 + C2
        Cc, D = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
        m = (A * B) / (Cc * D)
        tot += float(m.sum(dtype=np.float64))
        dm_dE12 = two * A / (Cc * D)
        dm_dE2 = -m / D
        # total derivative w.r.t. mu1 at fixed E2, E12: A and C directly, B and D through sigma12 = E12 - mu1 mu2, sigma1 = E2 - mu1^2
        dm_dmu1 = two * mu2 * B / (Cc * D) - two * mu2 * A / (Cc * D) - two * mu1 * m / Cc + two * mu1 * m / D
        grad[c] = _conv_same(dm_dmu1, g) + two * xc * _conv_same(dm_dE2, g) + yc * _conv_same(dm_dE12, g)
    n = x.size
    return tot / n, (grad / dt.type(n)).astype(dt)


def camera_stream(n_cams, count, single_camera=False):
    """The plugin's camera draw: ONE xorshift64 stream shared by all ranks (gstrain.cpp trainStep)."""
    s = 88172645463325252
    out = []
    for _ in range(count):
        s ^= (s << 13) & 0xFFFFFFFFFFFFFFFF
        s ^= s >> 7
        s ^= (s << 17) & 0xFFFFFFFFFFFFFFFF
        out.append(0 if single_camera else s % n_cams)
    return out


def pack_unpack_u8(t):
    """--packLevel 1 (k_pack_u8 then k_unpack_u8): a view stored as 8 bits per channel and expanded again, in the kernels' float32
    operation order — float32(rint(clip(t * 255, 0, 255))) * float32(1 / 255); rint rounds half to even."""
    q = np.rint(np.clip(np.asarray(t, np.float32) * np.float32(255.0), np.float32(0.0), np.float32(255.0))).astype(np.float32)
    return q * np.float32(1.0 / 255.0)


def ellipse_mask(W, H):
    """--useMask on a synthetic scene (gstrain/trainer_load.cpp load_synthetic): 1 inside the ellipse inscribed in the image, 0 outside; pixel
    centres u = (x + 0.5) / W * 2 - 1, v likewise, u^2 + v^2 <= 1, evaluated in float32 as the plugin does. -> [H, W] float32"""
    f = np.float32
    u = (np.arange(W, dtype=np.float32) + f(0.5)) / f(W) * f(2.0) - f(1.0)
    v = (np.arange(H, dtype=np.float32) + f(0.5)) / f(H) * f(2.0) - f(1.0)
    return (u[None, :] * u[None, :] + v[:, None] * v[:, None] <= f(1.0)).astype(np.float32)


def sh_degree_at(step, sh_degree, progressive=True):
    """the SH degree a step trains at: one more band every 1000 steps with --progressTrain 1 (gstrain/trainer.hpp sh_degree_at)"""
    return min(sh_degree, step // 1000) if progressive else sh_degree


def shn_active_chunks(deg):
    """float4 chunks of a splat's 45 (+3 pad) higher-order SH floats that hold the bands up to `deg`: ceil(3 ((deg + 1)^2 - 1) / 4)
    (what plan_step hands the Adam kernel; at degree 3 the product passes 0 = all twelve)"""
    return -(-3 * ((deg + 1) ** 2 - 1) // 4)


def scene_extent(cams):
    """1.1 x the largest distance of a camera centre from their mean; tiny rigs fall back to 5 (gstrain/trainer_load.cpp finish_load)."""
    c = np.array([[cam.campos[0], cam.campos[1], cam.campos[2]] for cam in cams], np.float64)
    far = np.sqrt(((c - c.mean(0)) ** 2).sum(1)).max()
    return float(np.float32(1.1 * far)) if far > 1e-3 else 5.0


class TrainStepRef:
    def __init__(self, oracle_cls, cams, targets, init, sh_degree, num_iters, dtype=np.float32, views_per_step=1, world=1, lr=None,
                 ssim_weight=0.0, mcmc_reg=None, start_step=0, progressive=False, antialias=False, pack_u8=False, mask=False,
                 reset_alpha_every=0, train_cams=None, sky=None):
        """ssim_weight: w of L = (1 - w) mean|x - y| + w (1 - mean SSIM) (--ssim, main.cpp:24: 0.2; 0 = L1 only).
        mcmc_reg: (opacity_reg, scale_reg) of densifyStrategy 1 (gstrain/trainer_step.cpp finish_range: 0.01, 0.01), added to the summed gradients once per step.
        start_step: a resume through --load_itr — the step number (Adam bias correction, position-rate schedule, SH degree) starts there,
        the moments at zero and the camera stream at its seed. progressive: --progressTrain 1. antialias: --mipAntiliased 1.
        pack_u8: --packLevel 1, the targets go through 8 bits. mask: --useMask 1, the photometric gradient (not the reported loss) is
        multiplied by ellipse_mask. reset_alpha_every: --resetAlphaEvery, applied after the Adam step of iterations it % r == 0.
        train_cams: --evalHoldout h, the indices i with i % h != 0 in order — a draw is train_cams[xorshift % len(train_cams)] (gstrain/
        trainer.hpp draw_cameras: held-out cameras are never trained on); None = every camera, cams[xorshift % len(cams)]. The extent
        stays that of ALL cameras (trainer_load.cpp finish_load).
        sky: --enableBg 1, dict(tex=[Hs, 2 Hs, 3], lr=DVS_SKY_LR) — the texture a resume reads from <model>_<it>.sky (see the sky
        section below); None = no sky, nothing of it runs."""
        self.w_ssim, self.mcmc_reg = float(ssim_weight), mcmc_reg
        self.dt = np.dtype(dtype)
        self.sky = None
        if sky is not None:
            tex = np.array(sky["tex"], self.dt)
            assert tex.ndim == 3 and tex.shape[1] == 2 * tex.shape[0] and tex.shape[2] == 3, tex.shape
            self.sky = dict(tex=tex, m=np.zeros_like(tex), v=np.zeros_like(tex), lr=float(sky["lr"]))
            self._taps = {}
        self.orc = oracle_cls(self.dt)
        self.progressive, self.antialias, self.reset_every = bool(progressive), bool(antialias), int(reset_alpha_every)
        self.cams, self.targets = cams, [np.asarray(pack_unpack_u8(t) if pack_u8 else t, self.dt) for t in targets]
        self.mask = [np.asarray(ellipse_mask(c.width, c.height), self.dt) for c in cams] if mask else None
        self.P = {k: np.array(init[k], self.dt) for k in KEYS}
        self.P["shN"] = self.P["shN"].reshape(-1, 15, 3)
        self.M = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.V = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.deg, self.num_iters = sh_degree, num_iters
        self.views, self.world = views_per_step, world
        self.extent = scene_extent(cams)
        self.lr = dict(LR, **(lr or {}))
        self.step = self.start = int(start_step)
        n = self.P["pos"].shape[0]
        self.train_cams = list(range(len(cams))) if train_cams is None else [int(c) for c in train_cams]
        self.order = [self.train_cams[d] for d in camera_stream(len(self.train_cams), 4096 * views_per_step * world)]
        self.grad_accum, self.denom, self.max_radii = np.zeros(n, self.dt), np.zeros(n, self.dt), np.zeros(n, np.int32)
        self.grad_accum_mean2d = np.zeros(n, self.dt)         # the statistic of --absgrad 0
        self.losses = []

    def degree(self):
        return sh_degree_at(self.step, self.deg, self.progressive)

    def learning_rates(self):
        f = self.dt.type
        t = min(f(1.0), f(self.step) / f(max(1, self.num_iters)))
        lr_pos = f(self.extent) * np.exp((f(1.0) - t) * np.log(f(self.lr["poslrInit"])) + t * np.log(f(self.lr["poslrFinal"])))
        return {"pos": f(lr_pos), "sh0": f(self.lr["featurelr"]), "shN": f(self.lr["featurelr"]) / f(20.0), "opacity": f(self.lr["opacitylr"]),
                "scale": f(self.lr["scalinglr"]), "rot": f(self.lr["rotationlr"])}

    def gradients(self):
        """Sum over the step's views (all ranks' views: the exchange sums them) of the L1 loss gradient; also the statistics."""
        f = self.dt.type
        n_views = self.views * self.world
        k = self.step - self.start                              # the camera stream restarts with the process
        draws = self.order[k * n_views:(k + 1) * n_views]
        G = {k: np.zeros_like(v) for k, v in self.P.items()}
        loss = 0.0
        self.tex_grads = []                                    # per view of the step, all ranks' (sky only)
        for ci in draws:
            cam, tgt = self.cams[ci], self.targets[ci]
            out = self.orc.forward(self.P, cam, sh_degree=self.degree(), antialias=self.antialias, absgrad=True, grad_mode=1)
            if self.sky is not None:                           # out = C + final_T s; the loss below is taken on it
                C, T = out, self.orc.get("final_T").copy()
                s = self.sky_lookup(cam)
                out = self.loss_image(C, T, s)
            d = out - tgt
            scale = f(1.0) / f(d.size)
            w = f(self.w_ssim)
            dL = (np.sign(d) * (scale * (f(1.0) - w))).astype(self.dt)
            loss += float(np.abs(d).sum() * scale) * (1.0 - self.w_ssim)
            if self.w_ssim > 0:
                val, gs = ssim_and_grad(np.ascontiguousarray(out, self.dt), tgt)
                dL = (dL - w * gs).astype(self.dt)
                loss += self.w_ssim * (1.0 - val)
            if self.mask is not None:                       # after the L1 / SSIM mix; the loss above stays unmasked (k_mask_mul: dL only)
                dL = (dL * self.mask[ci][None]).astype(self.dt)
            g = self.orc.backward(dL, grad_mode=1)
            for k in KEYS:
                G[k] += g[k].reshape(G[k].shape)
            radii = self.orc.get("radii")
            ag, gm = self.orc.get("absgrad"), self.orc.get("dL_dmean2d")
            vis = radii > 0
            W, H = cam.width, cam.height
            self.grad_accum += np.where(vis, np.hypot(ag[:, 0] * f(0.5 * W), ag[:, 1] * f(0.5 * H)), 0).astype(self.dt)
            self.grad_accum_mean2d += np.where(vis, np.hypot(gm[:, 0] * f(0.5 * W), gm[:, 1] * f(0.5 * H)), 0).astype(self.dt)
            self.denom += vis.astype(self.dt)
            self.max_radii = np.maximum(self.max_radii, np.where(vis, radii, 0))
            if self.sky is not None:                       # (after the statistics: they are the colour path's, sky.hip leaves columns 9, 10 alone)
                self.tex_grads.append(self.sky_tex_gradient(cam, T, dL))
                gT = self.final_T_gradient(cam, dL, s)
                for k in KEYS:
                    G[k] += gT[k].reshape(G[k].shape)
        self.losses.append(loss / len(draws))
        if self.mcmc_reg is not None:            # dvs_mcmc_regularize: d/dlogit of wo mean(sigmoid), d/dlog s of ws mean(exp(log s))
            wo, ws = self.mcmc_reg
            n = self.P["opacity"].shape[0]
            sg = f(1.0) / (f(1.0) + np.exp(-self.P["opacity"]))
            G["opacity"] += (f(wo) / f(n)) * sg * (f(1.0) - sg)
            G["scale"] += (f(ws) / f(3 * n)) * np.exp(self.P["scale"])
        return G

    def adam(self, G):
        f = self.dt.type
        it = self.step + 1
        b1, b2, eps = f(0.9), f(0.999), f(1e-15)
        bc1, bc2 = f(1.0) / (f(1.0) - b1 ** f(it)), f(1.0) / (f(1.0) - b2 ** f(it))
        lr = self.learning_rates()
        deg = self.degree()
        for k in KEYS:
            g = G[k]
            if k == "shN":                                   # only the float4 chunks of the active SH bands are stepped (zero gradient above them anyway)
                if deg == 0:                                 # no shN step at all at degree 0 (plan_step: count = 0)
                    continue
                g = g.copy()
                g[:, (deg + 1) ** 2 - 1:, :] = 0
            self.M[k] = b1 * self.M[k] + (f(1.0) - b1) * g
            self.V[k] = b2 * self.V[k] + (f(1.0) - b2) * g * g
            self.P[k] = (self.P[k] - lr[k] * (self.M[k] * bc1) / (np.sqrt(self.V[k] * bc2) + eps)).astype(self.dt)

    def train_step(self):
        G = self.gradients()
        self.adam(G)
        if self.sky is not None:
            self.sky_adam(self.tex_gradient())
        self.step += 1
        if self.reset_every > 0 and self.step % self.reset_every == 0:      # trainStep reset_now -> dvs_reset_opacity(0.01)
            f = self.dt.type
            self.P["opacity"] = np.minimum(self.P["opacity"], np.log(f(0.01) / (f(1.0) - f(0.01)))).astype(self.dt)
            self.M["opacity"][:] = 0
            self.V["opacity"][:] = 0
        return G

    # ---- sky model (--enableBg 1; gstrain/trainer_step.cpp render_backward / step_sky, csrc/sky.hip) -----------------------------------------
    # The oracle knows a constant cam.bg only. A background that varies per pixel, out = C + final_T s, is restated from it by linearity:
    # the oracle's backward is linear in dL and, through the one term bg . dL it hands to dL/dalpha, in bg — so the gradient through
    # final_T of sum_p final_T(p) h(p), h = s . dL, is backward(dL' = (h, 0, 0); bg = (1, 0, 0)) - backward(dL'; bg = 0): the colour
    # path of dL' is in both and cancels. Each piece is its own method so that a test can restate the step WRONGLY in one place.
    def _sky_taps(self, cam):
        """-> (texel indices [H,W,4], bilinear weights [H,W,4] in the run's dtype) of the camera's pixels: tests/sky_ref.py's rays and taps"""
        import sky_ref as SR
        key = (cam.width, cam.height, tuple(cam.proj))
        if key not in self._taps:
            Hs, Ws, _ = self.sky["tex"].shape
            idx, w = SR.taps(SR.rays(cam.proj[:], cam.width, cam.height), Ws, Hs)
            self._taps[key] = (idx, w.astype(self.dt))
        return self._taps[key]

    def sky_lookup(self, cam):
        """s [3,H,W]: sky_ref.lookup in the run's dtype"""
        idx, w = self._sky_taps(cam)
        flat = self.sky["tex"].reshape(-1, 3)
        return np.ascontiguousarray(np.moveaxis((flat[idx] * w[..., None]).sum(-2), -1, 0), self.dt)

    def loss_image(self, C, T, s):
        """the image the loss and its gradient are formed from"""
        return (C + T[None] * s).astype(self.dt)

    def sky_tex_gradient(self, cam, T, dL):
        """dL/dtex [Hs,Ws,3] of one view: sky_ref.sky_backward_tex (the same sums in the same order) in the run's dtype"""
        idx, w = self._sky_taps(cam)
        Hs, Ws, _ = self.sky["tex"].shape
        tg = np.moveaxis(T[None] * dL, 0, -1)
        out = np.zeros((Hs * Ws, 3), self.dt)
        for k in range(4):
            np.add.at(out, idx[..., k].reshape(-1), (w[..., k, None] * tg).reshape(-1, 3))
        return out.reshape(Hs, Ws, 3)

    def final_T_gradient(self, cam, dL, s):
        """the gradient of sum_p final_T(p) (s(p) . dL(p)) in the six groups (DVS_GRAD_LINEAGE, like the colour path). Leaves the oracle
        in the state of another forward: read what the step needs of the colour-path state before."""
        assert cam.bg[0] == 0 and cam.bg[1] == 0 and cam.bg[2] == 0, "the sky texture is the background (never both)"
        dLh = np.zeros_like(dL)
        dLh[0] = (s * dL).sum(0)
        kw = dict(sh_degree=self.degree(), antialias=self.antialias, absgrad=True, grad_mode=1)
        g = []
        for b in (1.0, 0.0):
            cam.bg[0] = b
            try:
                self.orc.forward(self.P, cam, **kw)
                g.append(self.orc.backward(dLh, grad_mode=1))
            finally:
                cam.bg[0] = 0.0
        return {k: g[0][k] - g[1][k] for k in KEYS}

    def tex_gradient(self):
        """the step's texture gradient: the sum over its views, all ranks' (step_sky's all-reduce)"""
        return sum(self.tex_grads[1:], self.tex_grads[0])

    def sky_step_number(self):
        """what step_sky hands dvs_adam_step for the bias correction: Step::it = step + 1, the resumed step number included"""
        return self.step + 1

    def sky_adam(self, g):
        """plain Adam on every texel, betas and eps of the other groups, rate DVS_SKY_LR; the moments start from zero"""
        f = self.dt.type
        it = self.sky_step_number()
        b1, b2, eps = f(0.9), f(0.999), f(1e-15)
        bc1, bc2 = f(1.0) / (f(1.0) - b1 ** f(it)), f(1.0) / (f(1.0) - b2 ** f(it))
        S = self.sky
        S["m"] = b1 * S["m"] + (f(1.0) - b1) * g
        S["v"] = b2 * S["v"] + (f(1.0) - b2) * g * g
        S["tex"] = (S["tex"] - f(S["lr"]) * (S["m"] * bc1) / (np.sqrt(S["v"] * bc2) + eps)).astype(self.dt)

    # ---- light prune of gstrain/trainer_refine.cpp prune_light() (pruneStrategy > 0, after refinement has stopped) ----------------------------------
    def prune_decisions(self, prune_opacity=0.005, min_opacity=0.005, prune_scale3d=0.1):
        """-> (prune [n] bool, margin [n]): a splat goes when sigmoid(opacity) < max(pruneOpacity, min_opacity) or max exp(scale) >
        pruneScale3d x extent; margin = relative distance to the nearer threshold."""
        op = 1.0 / (1.0 + np.exp(-self.P["opacity"].astype(np.float64)))
        smax = np.exp(self.P["scale"].max(1).astype(np.float64))
        thr_o, thr_s = max(prune_opacity, min_opacity), prune_scale3d * self.extent
        return (op < thr_o) | (smax > thr_s), np.minimum(np.abs(op - thr_o) / thr_o, np.abs(smax - thr_s) / thr_s)

    def apply_prune(self, keep):
        """compacts the parameters and both Adam moments of all six groups in order (apply_plan with zero_moments = false)"""
        keep = np.asarray(keep, bool)
        for D in (self.P, self.M, self.V):
            for k in KEYS:
                D[k] = np.ascontiguousarray(D[k][keep])
        self.grad_accum, self.denom, self.max_radii = (np.zeros(int(keep.sum()), a.dtype) for a in (self.grad_accum, self.denom, self.max_radii))
        self.grad_accum_mean2d = np.zeros(int(keep.sum()), self.dt)

    # ---- importance prune of gstrain/trainer_refine.cpp prune_importance() (--importancePrune P, after the light prune) ---------------------------------
    def importance_scores(self, cam_indices, mask=False):
        """-> (score [n] float64, excluded [n] bool): the blend weight alpha T of every splat summed over the pixels of the listed cameras
        (include/dvs_raster.h dvs_raster_importance_views), from the current parameters: per camera the oracle forward at the model's
        FULL SH degree and the run's anti-alias setting (the evaluation's options, whatever degree the step trains at), its own state
        (mean2d, conic_opacity, vals, ranges, n_contrib) through tests/importance_ref.py; mask: ellipse_mask(W, H), a pixel outside it
        contributes nothing. excluded: the OR over the cameras of importance_ref's threshold bands. The product sums rintf(w 2^24) in a
        uint64; this stays in float64."""
        import importance_ref as IR
        n = self.P["pos"].shape[0]
        score, excluded = np.zeros(n), np.zeros(n, bool)
        for ci in cam_indices:
            cam = self.cams[ci]
            self.orc.forward(self.P, cam, sh_degree=self.deg, antialias=self.antialias)
            rec = IR.oracle_records(self.orc.get("mean2d"), self.orc.get("conic_opacity"))
            m = ellipse_mask(cam.width, cam.height) if mask else None
            wsum, _, _, excl = IR.importance(rec, self.orc.get("ranges"), self.orc.get("vals"), self.orc.get("n_contrib"), cam.width, cam.height, n, 0, mask=m)
            score += wsum
            excluded |= excl
        return score, excluded

    # ---- ADC refinement decision of gstrain/trainer_refine.cpp densify() / densify.hip d_action --------------------------------------------------------
    def adc_actions(self, grow_grad2d, min_opacity=0.005, stat="absgrad", max_world_scale=0.0, max_screen_radius=0):
        """0 keep, 1 clone, 2 split, 3 prune — and the margin of each decision (relative distance to its nearest threshold).
        stat: "absgrad" (--absgrad 1) or "mean2d" (--absgrad 0: hypot(gx W/2, gy H/2) of the signed dL/dmean2D).
        max_world_scale / max_screen_radius: the two limits a refinement after the first opacity reset also prunes by (densify():
        pruneScale3d x extent, and max(1, int(pruneScale2d x max(W, H))) pixels below refineScale2dStopIter), both strict, both decided
        before any growth; 0 = off, the rule before any reset. The radius is an integer, but the plugin's and the restatement's may differ
        by a pixel: its margin is the distance to limit + 1/2, so that the radii limit and limit + 1 are never firm at a limit >= 10."""
        accum = {"absgrad": self.grad_accum, "mean2d": self.grad_accum_mean2d}[stat]
        op = 1.0 / (1.0 + np.exp(-self.P["opacity"].astype(np.float64)))
        smax = np.exp(self.P["scale"].max(1).astype(np.float64))
        avg = np.where(self.denom > 0, accum.astype(np.float64) / np.maximum(self.denom, 1), 0.0)
        thr_s = 0.01 * self.extent
        act = np.where(op < min_opacity, 3, np.where(avg >= grow_grad2d, np.where(smax > thr_s, 2, 1), 0))
        margin = np.minimum(np.abs(op - min_opacity) / min_opacity, np.abs(avg - grow_grad2d) / grow_grad2d)
        margin = np.where(avg >= grow_grad2d, np.minimum(margin, np.abs(smax - thr_s) / thr_s), margin)
        if max_world_scale > 0:
            act = np.where(smax > max_world_scale, 3, act)
            margin = np.minimum(margin, np.abs(smax - max_world_scale) / max_world_scale)
        if max_screen_radius > 0:
            act = np.where(self.max_radii > max_screen_radius, 3, act)
            margin = np.minimum(margin, np.abs(self.max_radii - (max_screen_radius + 0.5)) / (max_screen_radius + 0.5))
        return act, margin


def importance_decisions(scores, excluded, keep):
    """-> (prune [n] bool, margin [n]): the n - keep smallest go, in the total order (score, then larger index first) that include/
    dvs_train.h documents for dvs_importance_plan; margin = |score - cut| / max(cut, tiny), cut = the score of the last kept splat (the
    smallest score that survives) — 0 for an excluded splat, and for a zero-score splat when the cut is itself 0 (ties decided by the
    index alone: whether a splat scores exactly 0 is not something a restatement in another precision can promise)."""
    s = np.asarray(scores, np.float64)
    n = s.shape[0]
    keep = min(int(keep), n)
    order = np.lexsort((-np.arange(n), s))                  # ascending score; among equals the larger index first
    prune = np.zeros(n, bool)
    prune[order[:n - keep]] = True
    cut = s[order[n - keep]] if keep > 0 else np.inf
    with np.errstate(over="ignore"):                        # (a cut of 0: every positive score is infinitely far from it)
        margin = np.abs(s - cut) / max(cut, np.finfo(np.float64).tiny)
    margin[np.asarray(excluded, bool)] = 0.0
    if cut == 0:
        margin[s == 0] = 0.0
    return prune, margin
