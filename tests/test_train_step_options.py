"""`train_step` at step level with the options the reference CLI turns on by default, and the other host flags of the step: progressive
SH (--progressTrain 1), 8-bit training views (--packLevel 1), --useMask, --mipAntiliased, the opacity reset inside the step, the light
prune, ADC on the statistic of --absgrad 0, and the ADC refinement after an opacity reset (both size limits on). The kernel-level suites pin the ops; these pin how the trainer (gstrain/trainer_step.cpp, trainer_refine.cpp) wires them: on which step
they run, with which arguments, and what state they leave for the next Adam step.

CPU part (not marked gpu): the restatement's own pieces (pack formula, mask, degree schedule), and for every GPU case below
  * discrimination — the float64 restatement with the option on and off, oracle-rendered targets, same scene and step count: the two
    trajectories differ by more than 10x the GPU test's element tolerance on the median moved element of the group the option acts on
    (otherwise the GPU test could not see the option being ignored), and
  * pinned fraction — float32 against float64 of the restatement alone pins at least the share of each group the GPU test asserts
    (`_compare`'s `comparable` rule, unchanged).
GPU part: `gaussian_train` from a start model written by this file (through the host's own resume path, --load_itr) against the
restatement, under the bars of tests/test_train_step.py: rtol 1e-4 with floor 1e-2 (worst 1e-3 at quantile 0.995 with SSIM), relative
L2 of the update < 1e-2, pinned share >= 0.90 with L1 only, >= 0.85 with SSIM.

Out of scope here: MCMC exploration noise (noiselr > 0) is a hash RNG and is covered at kernel level (tests/test_gpu_train_ops*.py);
visibleAdam has no CLI flag and is covered at kernel level; ADC's randomly sampled split children beyond what
tests/test_train_step.py::test_plugin_adc_refinement_matches_the_restated_rule checks."""
import ctypes as C
import json
import os
import re
import numpy as np
import pytest
import divshot_amd as dv
from oracle.oracle import Oracle
from train_step_ref import TrainStepRef, KEYS, LR, pack_unpack_u8, ellipse_mask, sh_degree_at, shn_active_chunks
from test_gpu_parity import REPORT as _PARITY_REPORT
from test_train_step import _run, _read_ply, _write_ply, _scene, _hip_targets, _compare, _decode_actions

RTOL = 1e-4                                    # the element tolerance of every trajectory test here (floor 1e-2)
SHARE_L1, SHARE_SSIM = 0.90, 0.85              # pinned share asserted with L1 only / with SSIM (tests/test_train_step.py)
# scene and step count of each GPU case, chosen on the CPU (the test_*_case_* tests below measure them)
CASES = {
    "progressive": dict(n=1500, W=48, H=48, cams=2, sh=3, seed=7),
    "loss_path": dict(n=2000, W=72, H=52, cams=4, sh=1, seed=32, K=12),          # non-square, neither side a multiple of 16
    "antialias": dict(n=2000, W=64, H=64, cams=4, sh=1, seed=33, K=8),
    "reset": dict(n=2000, W=64, H=64, cams=4, sh=1, seed=34, every=6),
    "prune": dict(n=1500, W=256, H=256, cams=4, sh=2, seed=35, K=10, more=2),      # n is not a multiple of 64: the last shN tile is partial
    "adc": dict(n=3000, W=96, H=48, cams=4, sh=1, seed=12, K=10),                # clearly non-square
    "adc_limits": dict(n=3000, W=96, H=48, cams=4, sh=1, seed=12, K=10, every=4),  # resets at 4 and 8, ONE refinement at 10 > 4
}
BASE = ["--ssim", "0", "--packLevel", "0", "--densifyStrategy", "0", "--progressTrain", "0", "--absgrad", "1", "--warmupLength", "100000"]


def _flags(**over):
    f = dict(zip(BASE[0::2], BASE[1::2]))
    f.update({"--" + k: str(v) for k, v in over.items()})
    return [x for kv in f.items() for x in kv]


def _case(name):
    c = CASES[name]
    spec, cams = _scene(c["n"], c["W"], c["H"], c["cams"], c["sh"], c["seed"])
    return c, spec, cams


def _start_model(spec, seed, shn_amp=0.0):
    """the start model of every case: the generating scene perturbed the way load_synthetic perturbs it (positions 0.2 % of the depth,
    sh0 +-0.5, opacity - 1, scale +-0.15), shN zero or small noise in all bands"""
    gt = dv.synth_splats(spec)
    rng = np.random.default_rng(seed)
    u = lambda shape: rng.uniform(-1, 1, shape).astype(np.float32)
    A = {k: v.copy() for k, v in gt.items()}
    A["pos"] = A["pos"] + np.float32(0.002) * A["pos"][:, 2:3] * u(A["pos"].shape)
    A["sh0"] = A["sh0"] + np.float32(0.5) * u(A["sh0"].shape)
    A["shN"] = (shn_amp * rng.standard_normal(A["shN"].shape)).astype(np.float32)
    A["opacity"] = A["opacity"] - np.float32(1.0)
    A["scale"] = A["scale"] + np.float32(0.15) * u(A["scale"].shape)
    return A


def _prune_start_model(spec, cams, seed):
    """start of the light-prune case: the log-scales compressed towards their maximum (x 0.35, which keeps every splat's anisotropy) and
    shifted so that the largest is 0.045 — the rig's extent is 0.55, so the rule's 0.1 x extent = 0.055 would otherwise take nearly every
    splat of the synthetic scene (hence also the 256 x 256 image: the small splats still cover a pixel or more); then a tenth of the
    splats at logit -8, 3 % with an activated opacity drawn around the 0.005 threshold (0.002 .. 0.009), and 4 % with one scale axis at
    1.2 .. 2 x (0.1 x extent)."""
    from train_step_ref import scene_extent
    A = _start_model(spec, seed)
    n = spec.n
    A["scale"] = (np.log(0.045) + 0.35 * (A["scale"] - A["scale"].max())).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    r = rng.random(n)
    A["opacity"][r < 0.10] = -8.0
    near = (r >= 0.10) & (r < 0.13)
    o = rng.uniform(0.002, 0.009, n)
    A["opacity"][near] = np.log(o / (1 - o))[near].astype(np.float32)
    big = (r >= 0.13) & (r < 0.17)
    A["scale"][big, rng.integers(0, 3, n)[big]] = np.log(0.1 * scene_extent(cams) * rng.uniform(1.2, 2.0, n))[big].astype(np.float32)
    return A


def _oracle_targets(spec, cams, sh, antialias=False):
    o = Oracle(np.float32)
    gt = dv.synth_splats(spec)
    return [o.forward(gt, c, sh_degree=sh, antialias=antialias).copy() for c in cams]


def _pair(cams, targets, init, sh, num_iters, K, **kw):
    r32 = TrainStepRef(Oracle, cams, targets, init, sh, num_iters, np.float32, **kw)
    r64 = TrainStepRef(Oracle, cams, targets, init, sh, num_iters, np.float64, **kw)
    for _ in range(K):
        r32.train_step(); r64.train_step()
    return r32, r64


def _r64(cams, targets, init, sh, num_iters, K, **kw):
    r = TrainStepRef(Oracle, cams, targets, init, sh, num_iters, np.float64, **kw)
    for _ in range(K):
        r.train_step()
    return r


def _pinned(r32, r64, init, share, pos_update=1e-2 / 2):
    """float32 against float64 of the restatement through `_compare` itself (got = the float32 trajectory): asserts the share, and that
    the float32 restatement alone uses at most half of the update bar (pos_update: what it may use of the positions')"""
    rep = {}
    _compare({k: r32.P[k].astype(np.float32) for k in KEYS}, r32, r64, init, RTOL, share, rep)
    for k in KEYS:
        assert rep[k]["rel_l2_of_update"] < (pos_update if k == "pos" else 1e-2 / 2), (k, rep[k])
    return {k: round(rep[k]["comparable"], 4) for k in KEYS}


def _median_difference(on, off, init, k, band=slice(None)):
    """median over the elements of group k that moved in either trajectory of |on - off| / max(|on|, 1e-2) (the tolerance's own scale)"""
    a, b, i0 = on.P[k][:, band] if k == "shN" else on.P[k], off.P[k][:, band] if k == "shN" else off.P[k], init[k]
    i0 = (i0[:, band] if k == "shN" else i0).reshape(a.shape)
    moved = (a != i0) | (b != i0)
    assert moved.mean() > 0.5, (k, moved.mean())
    return float(np.median((np.abs(a - b) / np.maximum(np.abs(a), 1e-2))[moved]))


# ---- the restatement's own pieces -----------------------------------------------------------------------------------------------
def test_pack_formula_on_explicit_values():
    """float32(rint(clip(t * 255, 0, 255))) * float32(1 / 255): the ends, the clamps, ties to even on both parities, one ulp either side"""
    f = np.float32
    inv = f(1.0 / 255.0)
    q = lambda v: pack_unpack_u8(np.array([v], np.float32))[0]
    assert q(0.0) == 0.0 and q(1.0) == f(255) * inv and q(1.7) == f(255) * inv and q(-0.3) == 0.0 and q(-1e-9) == 0.0
    assert pack_unpack_u8(np.zeros(3, np.float64)).dtype == np.float32
    for k in (0, 1, 2, 3, 126, 127, 253, 254):                  # t * 255 = k + 0.5 exactly (k + 0.5 is a float32, the quotient is chosen to hit it)
        t = f(k + 0.5) / f(255)
        cands = [c for c in (np.nextafter(t, f(0)), t, np.nextafter(t, f(2))) if c * f(255) == f(k + 0.5)]
        assert cands, k                                         # (a float32 whose product with 255 rounds to the tie exists for these k)
        even = k if k % 2 == 0 else k + 1
        assert q(cands[0]) == f(even) * inv, (k, q(cands[0]))   # round half to even: down for even k, up for odd k
    for k in (0, 1, 126, 127):                                  # one float32 ulp of the PRODUCT either side of the tie
        lo, hi = np.nextafter(f(k + 0.5), f(0)), np.nextafter(f(k + 0.5), f(300))
        r = lambda x: np.rint(np.clip(x, f(0), f(255)))
        assert r(lo) == k and r(hi) == k + 1
    # and through the whole formula: values whose product lies one ulp below / above the tie
    for k in (1, 2, 127, 128):
        for side, want in ((-1, k), (+1, k + 1)):
            target = np.nextafter(f(k + 0.5), f(0) if side < 0 else f(300))
            t = target / f(255)
            for c in (np.nextafter(t, f(0)), t, np.nextafter(t, f(2))):
                if c * f(255) == target:
                    assert q(c) == f(want) * inv, (k, side)
    x = np.linspace(-0.2, 1.2, 100001).astype(np.float32)
    got = pack_unpack_u8(x)
    assert got.min() == 0.0 and got.max() == f(255) * inv and np.abs(got - np.clip(x, 0, 1)).max() <= 0.5 / 255 + 1e-7
    assert np.array_equal(np.unique(np.rint(got * 255)), np.arange(256, dtype=np.float32))


def test_mask_equals_the_literal_double_loop():
    for W, H in ((72, 52), (7, 13), (16, 16)):
        m = ellipse_mask(W, H)
        assert m.shape == (H, W) and m.dtype == np.float32
        want = np.zeros((H, W), np.float32)
        f = np.float32
        for y in range(H):
            for x in range(W):
                u = (f(x) + f(0.5)) / f(W) * f(2.0) - f(1.0)
                v = (f(y) + f(0.5)) / f(H) * f(2.0) - f(1.0)
                want[y, x] = 1.0 if u * u + v * v <= f(1.0) else 0.0
        assert np.array_equal(m, want)
        assert m[H // 2, W // 2] == 1 and m[0, 0] == 0 and m[H - 1, W - 1] == 0
        if min(W, H) > 10:
            assert abs(m.mean() - np.pi / 4) < 0.03               # an ellipse inscribed in the image, whatever its aspect


def test_degree_schedule_and_active_chunks():
    assert [sh_degree_at(s, 3) for s in (0, 999, 1000, 1999, 2000, 2999, 3000, 3001, 50000)] == [0, 0, 1, 1, 2, 2, 3, 3, 3]
    assert [sh_degree_at(s, 1) for s in (0, 999, 1000, 5000)] == [0, 0, 1, 1]
    assert [sh_degree_at(s, 3, progressive=False) for s in (0, 999, 3000)] == [3, 3, 3]
    # degree d uses the first 3 ((d + 1)^2 - 1) of a splat's 45 floats = 0, 9, 24, 45 -> 0, 3, 6, 12 float4 chunks (of 12, 48 floats with the pad)
    assert [shn_active_chunks(d) for d in range(4)] == [0, 3, 6, 12]
    for d in range(4):
        assert 4 * shn_active_chunks(d) >= 3 * ((d + 1) ** 2 - 1) > 4 * (shn_active_chunks(d) - 1)


def test_restated_shn_gate_follows_the_degree():
    """the restated Adam step leaves the bands above the step's degree alone — values and moments — and takes no shN step at degree 0"""
    c, spec, cams = _case("progressive")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"], 0.05)
    r = TrainStepRef(Oracle, cams, tg, init, 3, 2003, np.float64, start_step=1998, progressive=True)
    for want_deg in (1, 1, 2, 2, 2):
        assert r.degree() == want_deg
        r.train_step()
    i0 = init["shN"].astype(np.float64)
    assert np.array_equal(r.P["shN"][:, 8:], i0[:, 8:]) and not r.M["shN"][:, 8:].any() and not r.V["shN"][:, 8:].any()
    assert (r.P["shN"][:, :8] != i0[:, :8]).mean() > 0.9
    r0 = TrainStepRef(Oracle, cams, tg, init, 3, 10, np.float64, progressive=True)
    r0.train_step()
    assert np.array_equal(r0.P["shN"], i0) and not r0.M["shN"].any()


# ---- discrimination and pinned fraction, per GPU case -------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [1000, 2000, 3000])
def test_progressive_case_is_pinned_and_discriminates(boundary):
    """measured (oracle targets; share of each group the float32 restatement pins, pos sh0 shN opacity scale rot):
    1000: 1 1 1 .973 1 1   2000: 1 1 1 .951 .999 1   3000: 1 .996 1 1 .999 1 (the default reset at 3000 clamps every opacity);
    relative L2 of the float32 restatement's own update: positions 5.1e-2 / 4.5e-2 / 5.0e-2 (POS_UPDATE_BAR_AT_FINAL_RATE), others <= 1.2e-5.
    median difference on the moved shN elements, progressive on vs off: 3.7e-2 / 3.1e-2 / 1.1e-2; on the moved sh0 elements, start_step
    on vs off: 2.9e-2 / 3.4e-2 / 3.5e-2"""
    c, spec, cams = _case("progressive")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"], 0.05)
    b = boundary
    kw = dict(start_step=b - 2, progressive=True, reset_alpha_every=3000)
    r32, r64 = _pair(cams, tg, init, 3, b + 3, 5, **kw)
    shares = _pinned(r32, r64, init, SHARE_L1, pos_update=0.055)
    off = _r64(cams, tg, init, 3, b + 3, 5, start_step=b - 2, reset_alpha_every=3000)
    d_prog = _median_difference(r64, off, init, "shN")
    zero = _r64(cams, tg, init, 3, b + 3, 5, progressive=True, reset_alpha_every=3000)
    d_start = _median_difference(r64, zero, init, "sh0")
    print(b, shares, d_prog, d_start)
    assert d_prog > 10 * RTOL and d_start > 10 * RTOL, (d_prog, d_start)


@pytest.mark.parametrize("w", [0.2, 0.0])
def test_loss_path_case_is_pinned_and_discriminates(w):
    """measured (oracle targets): pinned share, worst group (opacity) .9935 with SSIM 0.2, .9945 with L1 only. These options act on
    every group through the photometric gradient; the group asserted is the opacities, whose Adam step is the largest in the
    tolerance's own scale: median difference, 8-bit targets on vs off 2.4e-3 (SSIM) / 3.2e-3 (L1), mask on vs off 6.9e-3 / 1.0e-2
    (the other groups, informative: sh0 1.8e-4 .. 8.3e-4, shN 5e-4 .. 2.2e-3, scale and rot 1e-4 .. 5.5e-4)"""
    c, spec, cams = _case("loss_path")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"])
    K = c["K"]
    r32, r64 = _pair(cams, tg, init, c["sh"], K, K, ssim_weight=w, pack_u8=True, mask=True)
    shares = _pinned(r32, r64, init, SHARE_SSIM if w > 0 else SHARE_L1)
    no_pack = _r64(cams, tg, init, c["sh"], K, K, ssim_weight=w, mask=True)
    no_mask = _r64(cams, tg, init, c["sh"], K, K, ssim_weight=w, pack_u8=True)
    d_pack, d_mask = _median_difference(r64, no_pack, init, "opacity"), _median_difference(r64, no_mask, init, "opacity")
    print(w, shares, d_pack, d_mask)
    assert d_pack > 10 * RTOL and d_mask > 10 * RTOL, (d_pack, d_mask)
    assert r64.losses[0] == pytest.approx(no_mask.losses[0], rel=1e-12)          # the reported loss stays unmasked


def test_antialias_case_is_pinned_and_discriminates():
    """measured (oracle targets): pinned share, worst group (opacity) .9975; median difference antialias on vs off: opacity 1.9e-2
    (sh0 1.6e-3, shN 4.4e-3, scale 1.2e-3)"""
    c, spec, cams = _case("antialias")
    tg = _oracle_targets(spec, cams, c["sh"], antialias=True)
    init = _start_model(spec, c["seed"])
    K = c["K"]
    r32, r64 = _pair(cams, tg, init, c["sh"], K, K, antialias=True)
    shares = _pinned(r32, r64, init, SHARE_L1)
    d = _median_difference(r64, _r64(cams, tg, init, c["sh"], K, K), init, "opacity")
    print(shares, d)
    assert d > 10 * RTOL, d


def _reset_step_size():
    """|step| of the Adam update at it = 7 from zeroed moments: lr (0.1 / (1 - 0.9^7)) / sqrt(0.001 / (1 - 0.999^7)), whatever |g|"""
    return LR["opacitylr"] * (0.1 / (1 - 0.9 ** 7)) / np.sqrt(0.001 / (1 - 0.999 ** 7))


@pytest.mark.parametrize("K", [6, 7])
def test_reset_case_is_pinned_and_discriminates(K):
    """measured (oracle targets): every group pinned to >= .9999 at K = 6 and K = 7; median difference of the opacities, reset on vs
    off: 0.81 at both. At K = 7 the float64 restatement obeys the closed form of the step after a reset (to Adam's eps); a step counter that was
    reset too would have moved each opacity by lr = 0.05 instead of 0.0253: 5e-3 of |logit(0.01)| = 4.6, 50x the element tolerance."""
    c, spec, cams = _case("reset")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"])
    r32 = TrainStepRef(Oracle, cams, tg, init, c["sh"], K, np.float32, reset_alpha_every=c["every"])
    r64 = TrainStepRef(Oracle, cams, tg, init, c["sh"], K, np.float64, reset_alpha_every=c["every"])
    for _ in range(6):
        r32.train_step(); r64.train_step()
    cap = np.log(0.01 / 0.99)
    assert (r64.P["opacity"] <= cap).all() and (r64.P["opacity"] == cap).mean() > 0.9 and not r64.M["opacity"].any() and not r64.V["opacity"].any()
    assert r64.M["sh0"].any() and r64.step == 6
    if K == 7:
        o6 = r64.P["opacity"].copy()
        r32.train_step(); G = r64.train_step()
        g = G["opacity"].reshape(-1)
        assert (g != 0).mean() > 0.5
        want = o6 - np.sign(g) * _reset_step_size()
        # (exact but for Adam's eps = 1e-15 beside sqrt(v) = sqrt(0.001 / (1 - 0.999^7)) |g|, which shortens the step of a tiny gradient)
        bound = _reset_step_size() * 1e-15 / (np.sqrt(0.001 / (1 - 0.999 ** 7)) * np.maximum(np.abs(g), 1e-300)) + 1e-11
        assert (np.abs(r64.P["opacity"] - want)[g != 0] <= bound[g != 0]).all() and np.array_equal(r64.P["opacity"][g == 0], o6[g == 0])
        assert np.abs(r64.P["opacity"] - want).max() < 1e-6
        assert abs(LR["opacitylr"] - _reset_step_size()) / abs(cap) > 10 * RTOL
    shares = _pinned(r32, r64, init, SHARE_L1)
    d = _median_difference(r64, _r64(cams, tg, init, c["sh"], K, K), init, "opacity")
    print(K, shares, d)
    assert d > 10 * RTOL, d


def test_prune_case_is_pinned_and_discriminates():
    """measured (oracle targets): the rule prunes 201 of 1500, every decision with a 5 % margin; pinned share (pos sh0 shN opacity scale
    rot) at the prune step 1 .9996 .9998 .9927 1 .9993, two steps on 1 .9992 .9996 .9885 1 .999. Discrimination of what run B is for (the
    moments travel with their rows), two steps after the prune, median difference on the moved elements: moments zeroed instead of
    carried sh0 3.1e-3, opacity 4.0e-2; moments carried one row off sh0 1.3e-3, opacity 1.1e-2."""
    c, spec, cams = _case("prune")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _prune_start_model(spec, cams, c["seed"])
    K, more = c["K"], c["more"]
    r32, r64 = _pair(cams, tg, init, c["sh"], K + more, K)
    prune, margin = r64.prune_decisions()
    firm = margin > 0.05
    p32, _ = r32.prune_decisions()
    assert firm.mean() > 0.9 and np.array_equal(prune[firm], p32[firm])
    assert 0.12 * c["n"] < prune.sum() < 0.2 * c["n"], prune.sum()
    op = 1 / (1 + np.exp(-r64.P["opacity"]))
    smax = np.exp(r64.P["scale"].max(1))
    assert ((op < 0.005) & firm).sum() > 0.08 * c["n"] and ((smax > 0.1 * r64.extent) & firm).sum() > 0.02 * c["n"]
    assert ((op >= 0.005) & (op < 0.01) & firm).sum() >= 5          # survivors just above the opacity threshold: it is 0.005 that is pinned
    keep = ~prune
    shares_a = _pinned(r32, r64, init, SHARE_L1)
    at_prune = {k: r64.P[k][keep].copy() for k in KEYS}
    variants = {}
    for name in ("carried", "zeroed", "shifted"):
        r = _r64(cams, tg, init, c["sh"], K + more, K)
        r.apply_prune(keep)
        assert r.P["pos"].shape[0] == keep.sum() and r.M["shN"].shape == (keep.sum(), 15, 3)
        for k in KEYS:
            if name == "zeroed":
                r.M[k][:] = 0; r.V[k][:] = 0
            if name == "shifted":
                r.M[k], r.V[k] = np.roll(r.M[k], 1, axis=0), np.roll(r.V[k], 1, axis=0)
        for _ in range(more):
            r.train_step()
        variants[name] = r
    r32.apply_prune(keep); r64.apply_prune(keep)
    for _ in range(more):
        r32.train_step(); r64.train_step()
    for k in KEYS:
        assert np.array_equal(r64.P[k], variants["carried"].P[k])
    shares_b = _pinned(r32, r64, {k: init[k][keep] for k in KEYS}, SHARE_L1)
    print(int(prune.sum()), shares_a, shares_b)
    for name in ("zeroed", "shifted"):
        for k in ("sh0", "opacity"):
            d = _median_difference(r64, variants[name], at_prune, k)
            print(name, k, d)
            assert d > 10 * RTOL, (name, k, d)


def _mean2d_statistics(cams, tg, init, sh, K, W):
    """ten steps of the float64 restatement; besides its own statistics, the one the product used to accumulate with --absgrad 0:
    |g| W/2 (the norm taken BEFORE the (W/2, H/2) scaling) — equal to hypot(gx W/2, gy H/2) only on square images"""
    r = TrainStepRef(Oracle, cams, tg, init, sh, K, np.float64)
    norm_first = np.zeros(init["pos"].shape[0])
    for _ in range(K):
        r.train_step()
        gm, vis = r.orc.get("dL_dmean2d"), r.orc.get("radii") > 0
        norm_first += np.where(vis, np.hypot(gm[:, 0], gm[:, 1]) * 0.5 * W, 0)
    return r, norm_first


def test_adc_mean2d_case_discriminates():
    """measured (oracle targets, 96x48): at the median of the restated statistic half the splats split (1495 keep / 1498 split / 7
    prune), 97.7 % of the decisions have a 5 % margin; on those, the abs-grad statistic decides differently for 17.7 % of the splats, and
    the norm-before-scaling statistic (|g| W/2) for 4.0 % — the GPU test sees either being used instead."""
    c, spec, cams = _case("adc")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"])
    r, norm_first = _mean2d_statistics(cams, tg, init, c["sh"], c["K"], c["W"])
    avg = r.grad_accum_mean2d / np.maximum(r.denom, 1)
    grow = float(np.median(avg[r.denom > 0]))
    act, margin = r.adc_actions(grow, stat="mean2d")
    firm = margin > 0.05
    assert firm.mean() > 0.9 and min(np.bincount(act, minlength=4)[[0, 2]]) > 0.2 * c["n"]
    act_abs, _ = r.adc_actions(grow, stat="absgrad")
    r.grad_accum_mean2d = norm_first
    act_nf, margin_nf = r.adc_actions(grow, stat="mean2d")
    d_abs, d_nf = (act_abs != act)[firm].mean(), (act_nf != act)[firm & (margin_nf > 0.05)].mean()
    print(grow, np.bincount(act, minlength=4), firm.mean(), d_abs, d_nf)
    assert d_abs > 0.01 and d_nf > 0.01, (d_abs, d_nf)
    assert (norm_first >= avg * r.denom * (1 - 1e-12)).all()          # W > H: scaling both components by W/2 can only be larger


def _adc_limits(r, W):
    """the flags of the post-reset refinement case, from the restated state after its ten steps: growGrad2d at the median of the
    abs-grad statistic, pruneScale3d at the 0.9 quantile of max exp(scale) / extent, pruneScale2d so that the radius limit is the 0.97
    quantile of max_radii (in the middle between two pixels) -> (grow, pruneScale3d, pruneScale2d, max_world_scale, max_screen_radius),
    the last two as trainer_refine.cpp densify() computes them in float32 from the flags"""
    f = np.float32
    avg = r.grad_accum / np.maximum(r.denom, 1)
    grow = float(f(np.median(avg[r.denom > 0])))
    ps3 = f(np.quantile(np.exp(r.P["scale"].max(1)), 0.9) / r.extent)
    ps2 = f((int(np.quantile(r.max_radii, 0.97)) + 0.5) / W)
    return grow, float(ps3), float(ps2), float(ps3 * f(r.extent)), max(1, int(ps2 * f(W)))


def test_adc_after_reset_case_discriminates():
    """measured (oracle targets, 96x48, opacity resets at 4 and 8, the refinement at 10): the limits are 0.677 x extent = 0.372 and 14
    pixels; with them 336 splats are pruned instead of 6, 90.7 % of the decisions have a 5 % margin under both rules, and on those 239
    splats change action against the limits-off rule: 126 that would have split and 113 that would have been kept; 183 by the world
    limit alone, 17 by the screen limit alone, 39 by both — the GPU test sees either limit being ignored, or checked after the growth."""
    c, spec, cams = _case("adc_limits")
    tg = _oracle_targets(spec, cams, c["sh"])
    init = _start_model(spec, c["seed"])
    r = _r64(cams, tg, init, c["sh"], c["K"], c["K"], reset_alpha_every=c["every"])
    grow, ps3, ps2, mws, lim = _adc_limits(r, c["W"])
    off, m_off = r.adc_actions(grow)
    on, m_on = r.adc_actions(grow, max_world_scale=mws, max_screen_radius=lim)
    legacy, m_legacy = r.adc_actions(grow, 0.005, "absgrad")
    assert np.array_equal(off, legacy) and np.array_equal(m_off, m_legacy)           # the defaults are the rule before any reset
    firm = (m_on > 0.05) & (m_off > 0.05)
    changed = (on != off) & firm
    world, screen = np.exp(r.P["scale"].max(1)) > mws, r.max_radii > lim
    counts = dict(firm=float(firm.mean()), changed=int(changed.sum()), were_split=int((changed & (off == 2)).sum()),
                  were_kept=int((changed & (off == 0)).sum()), world_only=int((changed & world & ~screen).sum()),
                  screen_only=int((changed & screen & ~world).sum()))
    print(grow, ps3, ps2, mws, lim, np.bincount(off, minlength=4), np.bincount(on, minlength=4), counts)
    assert (on[changed] == 3).all() and (m_on > 0.05).mean() > 0.85
    assert min(counts["were_split"], counts["were_kept"], counts["world_only"], counts["screen_only"]) >= 5, counts
    assert lim >= 10 and (r.max_radii[r.denom == 0] == 0).all()


# ---- the product ------------------------------------------------------------------------------------------------------------------------
def _src(c):
    return f"synthetic:N={c['n']},W={c['W']},H={c['H']},cams={c['cams']},sh={c['sh']},seed={c['seed']}"


def _product(tmp_path, tag, c, init, flags, start, stop):
    """writes `init` as the model of iteration `start`, resumes the product from it (--load_itr, gs_train.cpp:113) up to `stop`"""
    out = str(tmp_path / tag / "it")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    _write_ply(f"{out}_{start}.ply", init)
    p = _run(["--inputPath", _src(c), "--maxIteration", str(stop), "--outputPath", out, "--load_itr", str(start)] + flags, timeout=600)
    assert "(resumed)" in p.stderr and "densify @" not in p.stderr, p.stderr[-1500:]
    return p, _read_ply(f"{out}_{stop}.ply")


# The one wider bar. The progressive cases resume at the END of the position-rate schedule (num_iters = b + 3: lr = extent x poslrFinal
# = 8.8e-7), so five steps move a coordinate of magnitude 1 .. 10 by <= 1e-5, some twenty float32 ulps: storing the parameter in float32
# alone costs the float32 restatement 4.5e-2 .. 5.1e-2 of the update against float64 (measured: test_progressive_case_is_pinned_and_
# discriminates, which bounds it by 5.5e-2), with every ELEMENT within 2e-7 of the trajectory. Two float32 runs that round differently
# add their errors: the bar is 2 x the measured 5.1e-2. Every other group, and the positions of every other case, keep 1e-2.
POS_UPDATE_BAR_AT_FINAL_RATE = 0.1


def _bars(got, r32, r64, init, report, ssim, pos_update_bar=1e-2):
    """the bars of the two trajectory tests of tests/test_train_step.py"""
    if ssim:
        _compare(got, r32, r64, init, RTOL, SHARE_SSIM, report, worst_rtol=1e-3, quantile=0.995)
    else:
        _compare(got, r32, r64, init, RTOL, SHARE_L1, report)
    for k in KEYS:
        assert report[k]["rel_l2_of_update"] < (pos_update_bar if k == "pos" else 1e-2), (k, report[k])


def _dump(case, report):
    out_dir = os.path.dirname(_PARITY_REPORT)                 # the run-report directory of the parity suites, beside their reports
    os.makedirs(out_dir, exist_ok=True)
    json.dump(report, open(os.path.join(out_dir, f"train_step_options_{case}.json"), "w"), indent=1)


def _loss_line(p, step):
    m = re.search(r"Iteraions %d, loss : ([0-9.eE+-]+)" % step, p.stderr)
    assert m, p.stderr[-1500:]
    return float(m.group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", [1000, 2000, 3000])
def test_plugin_progressive_sh_across_a_boundary(tmp_path, boundary):
    """--progressTrain 1 (the CLI default), SH degree 3, resumed two steps below a degree boundary and run three steps past it, from a
    model with non-zero shN in every band: the five steps follow TrainStepRef(start_step = b - 2, progressive) — the Adam bias
    correction, the position-rate schedule and the SH degree of the step NUMBER — under the bars of the L1-only trajectory test; the
    bands above the final degree are bit-identical to the loaded model, the band unlocked at the boundary has moved and carries the
    trajectory's three (not five) Adam steps. At 3000 the default --resetAlphaEvery 3000 fires inside the window and is restated too.
    Pinned share measured on the CPU (oracle targets; pos sh0 shN opacity scale rot): 1000: 1 1 1 .973 1 1; 2000: 1 1 1 .951 .999 1;
    3000: 1 .996 1 1 .999 1. On the GPU the same shares were measured; worst pinned element 2.6e-5."""
    c, spec, cams = _case("progressive")
    b = boundary
    init = _start_model(spec, c["seed"], 0.05)
    p, got = _product(tmp_path, "m", c, init, _flags(progressTrain=1), b - 2, b + 3)
    assert got["pos"].shape[0] == c["n"]
    tg = _hip_targets(spec, cams, c["sh"])
    r32, r64 = _pair(cams, tg, init, c["sh"], b + 3, 5, start_step=b - 2, progressive=True, reset_alpha_every=3000)
    deg = b // 1000
    lo, hi = deg * deg - 1, (deg + 1) ** 2 - 1                                   # the coefficients of the band unlocked at step b
    report = {}
    new_moved = (got["shN"][:, lo:hi] != init["shN"][:, lo:hi]).mean()
    report["unlocked_band_moved"] = float(new_moved)
    report["loss_line"] = [_loss_line(p, b), r64.losses[2]]
    try:
        assert np.array_equal(got["shN"][:, hi:].view(np.uint32), init["shN"][:, hi:].view(np.uint32)), "a band above the step's degree was touched"
        assert new_moved > 0.9 and (r64.P["shN"][:, lo:hi] != init["shN"][:, lo:hi]).mean() > 0.9
        # three steps of the unlocked band, not five: each Adam step moves an element by at most lr bc1 / sqrt(bc2) x |m| / sqrt(v)
        # <= lr / 20 x 3.2 here; what matters is that the band follows the trajectory, which gave it three
        _bars(got, r32, r64, init, report, ssim=False, pos_update_bar=POS_UPDATE_BAR_AT_FINAL_RATE)
        assert abs(report["loss_line"][0] - r64.losses[2]) < 2e-4 * max(r64.losses[2], 1e-3)
    finally:
        _dump(f"progressive_{b}", report)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [0.2, 0.0])
def test_plugin_reference_cli_loss_path(tmp_path, w):
    """--packLevel 1 --useMask 1 (8-bit training views expanded into the shared staging image, the inscribed-ellipse mask on the planar
    gradient) with --ssim 0.2 (the CLI's loss) and with --ssim 0, 12 steps at 72x52 against TrainStepRef(pack_u8, mask) under the bars of
    the matching trajectory test; the `Iteraions 0` line is the UNMASKED restated loss. Pinned share measured on the CPU (oracle
    targets), worst group (opacity): .9935 with SSIM, .9945 with L1 only; every other group >= .9998."""
    c, spec, cams = _case("loss_path")
    K = c["K"]
    init = _start_model(spec, c["seed"])
    p, got = _product(tmp_path, "m", c, init, _flags(ssim=w, packLevel=1, useMask=1), 0, K)
    assert "PackF32ToU8: 8-bit training views" in p.stderr and "useMask 1" in p.stderr
    tg = _hip_targets(spec, cams, c["sh"])
    r32, r64 = _pair(cams, tg, init, c["sh"], K, K, ssim_weight=w, pack_u8=True, mask=True)
    report = {"loss_line": [_loss_line(p, 0), r64.losses[0]]}
    try:
        _bars(got, r32, r64, init, report, ssim=w > 0)
        assert abs(report["loss_line"][0] - r64.losses[0]) < 2e-4 * max(r64.losses[0], 1e-3)
    finally:
        _dump("loss_path_ssim" if w > 0 else "loss_path_l1", report)


@pytest.mark.gpu
def test_plugin_mip_antialiased(tmp_path):
    """--mipAntiliased 1, L1 only, 8 steps against TrainStepRef(antialias) on anti-aliased targets (the product renders its training
    views with the option too). Pinned share measured on the CPU (oracle targets): opacity .9975, every other group 1."""
    c, spec, cams = _case("antialias")
    K = c["K"]
    init = _start_model(spec, c["seed"])
    p, got = _product(tmp_path, "m", c, init, _flags(mipAntiliased=1), 0, K)
    assert "mipAntiliased 1" in p.stderr
    tg = _hip_targets(spec, cams, c["sh"], antialias=True)
    r32, r64 = _pair(cams, tg, init, c["sh"], K, K, antialias=True)
    report = {"loss_line": [_loss_line(p, 0), r64.losses[0]]}
    try:
        _bars(got, r32, r64, init, report, ssim=False)
        assert abs(report["loss_line"][0] - r64.losses[0]) < 2e-4 * max(r64.losses[0], 1e-3)
    finally:
        _dump("antialias", report)


def _logit_001_f32():
    """logf(0.01f / (1.f - 0.01f)) as dvs_reset_opacity evaluates it on the host"""
    libm = C.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    return np.float32(libm.logf(np.float32(0.01) / (np.float32(1.0) - np.float32(0.01))))


@pytest.mark.gpu
def test_plugin_opacity_reset_inside_the_step(tmp_path):
    """--resetAlphaEvery 6 with ADC selected but never refining (--warmupLength 100000). Run to 6: the reset is the last thing that
    happens — every opacity <= float32 logit(0.01), the opacities equal min(trajectory, logit(0.01)) and the other groups the trajectory
    under the bars. Run to 7: with the opacity moments zeroed and the step counter NOT reset (it = 7), every opacity with a non-zero
    gradient moves by exactly lr (0.1 / (1 - 0.9^7)) / sqrt(0.001 / (1 - 0.999^7)) = 0.02532 against the sign of the oracle gradient —
    moments left in place or a counter reset to 1 (a step of 0.05) give something else. Pinned share measured on the CPU (oracle
    targets): >= .9999 in every group at 6 and at 7."""
    c, spec, cams = _case("reset")
    init = _start_model(spec, c["seed"])
    flags = _flags(resetAlphaEvery=c["every"])
    tg = _hip_targets(spec, cams, c["sh"])
    report = {}
    try:
        _, got6 = _product(tmp_path, "k6", c, init, flags, 0, 6)
        r32, r64 = _pair(cams, tg, init, c["sh"], 6, 6, reset_alpha_every=c["every"])
        cap = _logit_001_f32()
        report["max_opacity_at_6"], report["cap"] = float(got6["opacity"].max()), float(cap)
        assert (got6["opacity"] <= cap).all(), (got6["opacity"].max(), cap)
        assert (r64.P["opacity"] == np.log(0.01 / 0.99)).mean() > 0.9             # (the clamp binds: min(trajectory, logit) is the logit nearly everywhere)
        report["k6"] = {}
        _bars(got6, r32, r64, init, report["k6"], ssim=False)
        _, got7 = _product(tmp_path, "k7", c, init, flags, 0, 7)
        r32, r64 = _pair(cams, tg, init, c["sh"], 7, 6, reset_alpha_every=c["every"])
        o6 = r64.P["opacity"].copy()
        r32.train_step(); G = r64.train_step()
        g = G["opacity"].reshape(-1)
        want = o6 - np.sign(g) * _reset_step_size()
        den = np.maximum(np.abs(want), 1e-2)
        sure = (np.abs(r32.P["opacity"].astype(np.float64) - r64.P["opacity"]) <= 0.25 * RTOL * np.maximum(np.abs(r64.P["opacity"]), 1e-2)) & (g != 0)
        err = np.abs(got7["opacity"].astype(np.float64) - want) / den
        report["k7_closed_form"] = dict(share=float(sure.mean()), worst=float(err[sure].max()), step=float(_reset_step_size()))
        assert sure.mean() >= SHARE_L1 and err[sure].max() <= RTOL, report["k7_closed_form"]
        report["k7"] = {}
        _bars(got7, r32, r64, init, report["k7"], ssim=False)
    finally:
        _dump("reset", report)


@pytest.mark.gpu
def test_plugin_light_prune_keeps_rows_and_moments_together(tmp_path):
    """--pruneStrategy 1 --pruneEvery 10 with refinement over (--refineStopIter 1), 1500 splats (the last 64-splat shN tile is partial),
    from a model with a tenth of the splats at logit -8, 3 % around the 0.005 threshold and 4 % oversized. Run A ends at the prune
    step: the logged counts match the file, the pruned set is prune_decisions() wherever the decision has a 5 % margin, the survivors
    carry — in order, all six groups — the trajectory under the bars. Run B goes two steps further and is compared with the
    restatement after apply_prune: the two Adam steps use the moments that travelled with their rows (zeroed or misplaced moments move
    the median sh0 / opacity element by > 10x the tolerance: test_prune_case_is_pinned_and_discriminates). Pinned share measured on the
    CPU (oracle targets), worst group (opacity): .9927 at the prune step, .9885 two steps on; every other group >= .999."""
    c, spec, cams = _case("prune")
    K, more, n = c["K"], c["more"], c["n"]
    init = _prune_start_model(spec, cams, c["seed"])
    flags = _flags(refineStopIter=1, pruneStrategy=1, pruneEvery=10)
    tg = _hip_targets(spec, cams, c["sh"])
    report = {}
    try:
        pa, gotA = _product(tmp_path, "a", c, init, flags, 0, K)
        m = re.findall(r"light prune @(\d+): (\d+) -> (\d+) splats", pa.stderr)
        assert m == [(str(K), str(n), str(gotA["pos"].shape[0]))], (m, gotA["pos"].shape)
        r32, r64 = _pair(cams, tg, init, c["sh"], K, K)
        want, margin = r64.prune_decisions()
        firm = margin > 0.05
        act = _decode_actions({k: r64.P[k].astype(np.float32) for k in KEYS}, gotA)
        assert set(act.tolist()) <= {0, 3}
        pruned = act == 3
        report["pruned"], report["firm"] = int(pruned.sum()), float(firm.mean())
        assert firm.mean() > 0.9 and 0.12 * n < want.sum() < 0.2 * n
        assert np.array_equal(pruned[firm], want[firm]), np.flatnonzero(pruned[firm] != want[firm])[:10]
        keep = ~pruned
        init_kept = {k: init[k][keep] for k in KEYS}
        r32.apply_prune(keep); r64.apply_prune(keep)
        report["a"] = {}
        _bars(gotA, r32, r64, init_kept, report["a"], ssim=False)
        pb, gotB = _product(tmp_path, "b", c, init, flags, 0, K + more)
        assert re.findall(r"light prune @(\d+): (\d+) -> (\d+) splats", pb.stderr) == [(str(K), str(n), str(int(keep.sum())))]
        assert gotB["pos"].shape[0] == keep.sum()
        r32, r64 = _pair(cams, tg, init, c["sh"], K + more, K)
        r32.apply_prune(keep); r64.apply_prune(keep)
        for _ in range(more):
            r32.train_step(); r64.train_step()
        report["b"] = {}
        _bars(gotB, r32, r64, init_kept, report["b"], ssim=False)
    finally:
        _dump("prune", report)


@pytest.mark.gpu
def test_plugin_adc_without_absgrad_uses_the_scaled_norm(tmp_path):
    """--absgrad 0, one view per step, 96x48: ten steps ending in ONE refinement with growGrad2d at the median of the restated statistic
    hypot(gx W/2, gy H/2) of the signed dL/dmean2D (the rule include/dvs_train.h documents for dvs_densify_accumulate). The actions decoded
    from the saved model equal adc_actions(stat="mean2d") wherever the decision has a 5 % margin. The norm taken before the scaling
    (|g| W/2, what the product accumulated until this test existed) decides 4 % of those splats differently on this image, the abs-grad
    statistic 18 % (test_adc_mean2d_case_discriminates)."""
    c, spec, cams = _case("adc")
    K, n = c["K"], c["n"]
    init = _start_model(spec, c["seed"])
    tg = _hip_targets(spec, cams, c["sh"])
    r64, _ = _mean2d_statistics(cams, tg, init, c["sh"], K, c["W"])
    avg = r64.grad_accum_mean2d / np.maximum(r64.denom, 1)
    grow = float(np.float32(np.median(avg[r64.denom > 0])))
    flags = _flags(absgrad=0, warmupLength=5, refineEvery=10, refineStopIter=1000, growGrad2d="%.9g" % grow)
    out = str(tmp_path / "m" / "it")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    _write_ply(out + "_0.ply", init)
    p = _run(["--inputPath", _src(c), "--maxIteration", str(K), "--outputPath", out, "--load_itr", "0"] + flags, timeout=600)
    assert "useAbsGrad 0" in p.stderr and "(resumed)" in p.stderr
    m = re.search(r"densify @10: (\d+) -> (\d+) splats", p.stderr)
    assert m and int(m.group(1)) == n, p.stderr[-1500:]
    got = _read_ply(out + f"_{K}.ply")
    assert got["pos"].shape[0] == int(m.group(2))
    want, margin = r64.adc_actions(grow, stat="mean2d")
    firm = margin > 0.05
    act = _decode_actions({k: r64.P[k].astype(np.float32) for k in KEYS}, got)
    report = dict(grow=grow, firm=float(firm.mean()), want=np.bincount(want, minlength=4).tolist(), got=np.bincount(act, minlength=4).tolist(),
                  differ_on_firm=int((act != want)[firm].sum()))
    _dump("adc_mean2d", report)
    assert firm.mean() > 0.9 and min(np.bincount(want, minlength=4)[[0, 2]]) > 0.2 * n, report
    assert np.array_equal(act[firm], want[firm]), (np.flatnonzero(act[firm] != want[firm])[:10], report)


@pytest.mark.gpu
def test_plugin_adc_after_an_opacity_reset_prunes_by_both_limits(tmp_path):
    """--resetAlphaEvery 4, 96x48: ten steps with opacity resets at 4 and 8 ending in ONE refinement at 10 > resetAlphaEvery, the first
    kind of refinement that also prunes by world size (--pruneScale3d x extent) and screen radius (--pruneScale2d x the longer image
    side), both set from the restated state so that they bite (test_adc_after_reset_case_discriminates: some 240 splats change action).
    The actions decoded from the saved model equal adc_actions(max_world_scale, max_screen_radius) wherever the decision has a 5 %
    margin, and the logged count is the file's."""
    c, spec, cams = _case("adc_limits")
    K, n = c["K"], c["n"]
    init = _start_model(spec, c["seed"])
    tg = _hip_targets(spec, cams, c["sh"])
    r64 = _r64(cams, tg, init, c["sh"], K, K, reset_alpha_every=c["every"])
    grow, ps3, ps2, mws, lim = _adc_limits(r64, c["W"])
    flags = _flags(warmupLength=5, refineEvery=10, refineStopIter=1000, resetAlphaEvery=c["every"], growGrad2d="%.9g" % grow,
                   pruneScale3d="%.9g" % ps3, pruneScale2d="%.9g" % ps2)
    out = str(tmp_path / "m" / "it")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    _write_ply(out + "_0.ply", init)
    p = _run(["--inputPath", _src(c), "--maxIteration", str(K), "--outputPath", out, "--load_itr", "0"] + flags, timeout=600)
    assert "(resumed)" in p.stderr
    m = re.findall(r"densify @(\d+): (\d+) -> (\d+) splats", p.stderr)
    got = _read_ply(out + f"_{K}.ply")
    assert m == [("10", str(n), str(got["pos"].shape[0]))], (m, got["pos"].shape, p.stderr[-1500:])
    want, margin = r64.adc_actions(grow, max_world_scale=mws, max_screen_radius=lim)
    off, m_off = r64.adc_actions(grow)
    firm = margin > 0.05
    act = _decode_actions({k: r64.P[k].astype(np.float32) for k in KEYS}, got)
    changed = (want != off) & firm & (m_off > 0.05)
    report = dict(grow=grow, pruneScale3d=ps3, pruneScale2d=ps2, max_world_scale=mws, max_screen_radius=lim, firm=float(firm.mean()),
                  want=np.bincount(want, minlength=4).tolist(), got=np.bincount(act, minlength=4).tolist(),
                  limits_off=np.bincount(off, minlength=4).tolist(), changed_by_the_limits=int(changed.sum()),
                  differ_on_firm=int((act != want)[firm].sum()))
    _dump("adc_after_reset", report)
    assert firm.mean() > 0.85 and changed.sum() >= 5 and min(np.bincount(want, minlength=4)[[0, 2, 3]]) > 0.05 * n, report
    assert np.array_equal(act[firm], want[firm]), (np.flatnonzero(act[firm] != want[firm])[:10], report)
