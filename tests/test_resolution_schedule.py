"""Coarse-to-fine training of the plugin (config resolutionSchedule / numDownscales; CLI --resolutionSchedule, --numDownscales) at step
level, through `gaussian_train` like tests/test_train_step.py: the steps of every level follow tests/train_step_ref.py when its
cameras and targets are swapped for the level's before each step (cameras: dvs_camera_downscale; targets and masks: the numpy
restatement of the box filter, tests/resolution_ref.py), under the bars of the trajectory tests this build already has; off means
nothing of it runs; a resume lands on the level of its step number; held-out quality still improves with the schedule on.

CPU part (not marked gpu): the pinned share of both parity legs, float32 against float64 of the restatement alone with
oracle-rendered targets — the 0.90 / 0.85 the GPU legs assert are caps on what a float32 implementation can pin, not measurements."""
import json
import os
import re
import shutil
import numpy as np
import pytest
import divshot_amd as dv
from oracle.oracle import Oracle
from train_step_ref import TrainStepRef, KEYS, ellipse_mask
from resolution_ref import level_of_step, downsample_np
from test_gpu_parity import REPORT as _PARITY_REPORT
from test_train_step import _run, _read_ply, _scene, _hip_targets, _compare, COMMON
from test_train_step_options import _bars, _pinned, _oracle_targets, _loss_line, SHARE_L1, SHARE_SSIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The scene of both parity legs. The seed is chosen on the CPU alone, by the rule the cases of tests/test_train_step_options.py are
# chosen by (the float32 restatement by itself pins the asserted share AND uses at most half of the 1e-2 update bar: `_pinned`), seeds
# tried from 11 upwards: 11 fails it on the second leg (a few splats on the fractional edge of the level mask receive a noise-level
# gradient, which Adam's eps = 1e-15 turns into full-size steps of either sign: float32 alone is 0.6 % of the update off in four
# groups), 12 passes with 2.5e-3 in sh0 / shN, 13 is the first at which every group but the positions is below 2e-4 (the positions'
# 2.4e-3 is float32 storage of the coordinate and the same at every seed).
N, W, H, CAMS, SH, SEED = 2000, 142, 110, 4, 1, 13
SRC = f"synthetic:N={N},W={W},H={H},cams={CAMS},sh={SH},seed={SEED}"
LEG1 = dict(K=12, every=4, levels=2, flags=COMMON + ["--warmupLength", "100000"], ref={})
LEG2 = dict(K=8, every=4, levels=1, ref=dict(ssim_weight=0.2),
            flags=["--ssim", "0.2", "--packLevel", "1", "--useMask", "1", "--densifyStrategy", "0", "--progressTrain", "0", "--absgrad", "1",
                   "--warmupLength", "100000"])
START_LINE = re.compile(r"resolution @(\d+): (\d+x\d+) \(1/(\d+)\)")
END_LINE = re.compile(r"resolution: (\d+) steps at (\d+x\d+): ([0-9.eE+-]+) ms/step")


def _schedule(leg):
    return ["--resolutionSchedule", str(leg["every"]), "--numDownscales", str(leg["levels"])]


def _level_inputs(cams, targets, levels, u8, mask):
    """per level k: the cameras, the fp32 targets the product trains on and the masks. 8-bit views (u8) are box-filtered from their
    bytes, as the product does; level 0 is the existing path (the bytes expanded, the 0/1 mask)."""
    f32 = np.float32
    bytes_ = [np.rint(np.clip(np.asarray(t, f32) * f32(255.0), f32(0.0), f32(255.0))).astype(np.uint8) for t in targets]
    full_mask = ellipse_mask(W, H)
    out = []
    for k in range(levels + 1):
        d = 1 << k
        lc = [dv.camera_downscale(c, d) for c in cams]
        lt = [downsample_np(b if u8 else np.asarray(t, f32), d) for b, t in zip(bytes_, targets)]
        lm = downsample_np(full_mask[None], d)[0] if mask else None
        out.append((lc, lt, lm))
    return out


def _restated(cams, targets, init, leg, dtype, u8=False, mask=False):
    """TrainStepRef over the leg's K steps, its cameras / targets / masks swapped to the level's before each step"""
    lv = _level_inputs(cams, targets, leg["levels"], u8, mask)
    r = TrainStepRef(Oracle, cams, targets, init, SH, leg["K"], dtype, mask=mask, **leg["ref"])
    levels = []
    for step in range(leg["K"]):
        k = level_of_step(step, leg["every"], leg["levels"])
        lc, lt, lm = lv[k]
        r.cams, r.targets = lc, [np.asarray(t, r.dt) for t in lt]
        if mask:
            r.mask = [np.asarray(lm, r.dt)] * len(cams)
        r.train_step()
        levels.append(k)
    return r, levels


def _perturbed_start(spec):
    """a start like load_synthetic's (the CPU legs have no product run to take it from)"""
    from test_train_step_options import _start_model
    return _start_model(spec, SEED)


@pytest.mark.parametrize("leg,u8,mask,share", [(LEG1, False, False, SHARE_L1), (LEG2, True, True, SHARE_SSIM)], ids=["l1_three_levels", "u8_mask_ssim"])
def test_schedule_case_is_pinned_on_the_cpu(leg, u8, mask, share):
    """float32 against float64 of the restatement alone, oracle-rendered targets, 142x110: the share of each group that the float32
    restatement pins is at least what the GPU leg asserts and it uses at most half of the update bar (measured; pos sh0 shN opacity
    scale rot — three levels, L1: 1 1 1 .998 1 1; 8-bit views + mask + SSIM, two levels: 1 1 1 .996 .9998 1), and the levels are the
    rule's."""
    spec, cams = _scene(N, W, H, CAMS, SH, SEED)
    targets = _oracle_targets(spec, cams, SH)
    init = _perturbed_start(spec)
    r32, lv = _restated(cams, targets, init, leg, np.float32, u8, mask)
    r64, _ = _restated(cams, targets, init, leg, np.float64, u8, mask)
    assert lv == [max(leg["levels"] - s // leg["every"], 0) for s in range(leg["K"])] and lv[0] == leg["levels"] and lv[-1] == 0
    print("pinned share:", _pinned(r32, r64, init, share))                   # (asserts the share and half of the update bar)
    np.testing.assert_allclose(r32.losses, r64.losses, rtol=2e-4)
    # the level is in the numbers: the same steps at full resolution throughout end somewhere else
    flat = TrainStepRef(Oracle, cams, [np.asarray(t) for t in _level_inputs(cams, targets, 0, u8, mask)[0][1]], init, SH, leg["K"], np.float64,
                        mask=mask, **leg["ref"])
    for _ in range(leg["K"]):
        flat.train_step()
    moved = np.abs(flat.P["sh0"] - init["sh0"]) > 0
    diff = np.abs(flat.P["sh0"] - r64.P["sh0"]) / np.maximum(np.abs(r64.P["sh0"]), 1e-2)
    assert np.median(diff[moved]) > 10 * 1e-4, np.median(diff[moved])


def _product(tmp, leg, extra):
    out = str(tmp / "m" / "it")
    _run(["--inputPath", SRC, "--maxIteration", "0", "--outputPath", out] + leg["flags"])
    init = _read_ply(out + "_0.ply")
    p = _run(["--inputPath", SRC, "--maxIteration", str(leg["K"]), "--outputPath", out] + leg["flags"] + extra)
    return out, init, p, _read_ply(out + f"_{leg['K']}.ply")


@pytest.fixture(scope="module")
def scene_and_targets():
    spec, cams = _scene(N, W, H, CAMS, SH, SEED)
    return cams, _hip_targets(spec, cams, SH)


@pytest.fixture(scope="module")
def leg1_run(tmp_path_factory):
    return _product(tmp_path_factory.mktemp("res1"), LEG1, _schedule(LEG1))


def _dump(name, report):
    out_dir = os.path.dirname(_PARITY_REPORT)                 # the run-report directory of the parity suites, beside their reports
    os.makedirs(out_dir, exist_ok=True)
    json.dump(report, open(os.path.join(out_dir, name), "w"), indent=1)


@pytest.mark.gpu
def test_plugin_three_levels_match_the_restatement(leg1_run, scene_and_targets):
    """12 iterations with --resolutionSchedule 4 --numDownscales 2 (L1 only, no refinement): steps 0-3 at 35x27, 4-7 at 71x55, 8-11 at
    142x110 — the full size is cropped at 1/4 in both directions and exact at 1/2. Bars of
    test_plugin_trajectory_matches_oracle_plus_numpy_adam: every element the float32 restatement pins within 1e-4 (floor 1e-2) of the
    float64 trajectory, >= 0.90 of each group pinned, the update within 1e-2 in relative L2; the logged loss of iteration 0 within 2e-4."""
    out, init, p, got = leg1_run
    cams, targets = scene_and_targets
    starts = [(int(m.group(1)), m.group(2), int(m.group(3))) for m in START_LINE.finditer(p.stderr)]
    assert starts == [(1, "35x27", 4), (5, "71x55", 2), (9, "142x110", 1)], p.stderr[-3000:]
    ends = [(int(m.group(1)), m.group(2)) for m in END_LINE.finditer(p.stderr)]
    assert ends == [(4, "35x27"), (4, "71x55"), (4, "142x110")], p.stderr[-3000:]
    assert "IGNORED by this build: resolutionSchedule" not in p.stderr and "config: resolutionSchedule 4, numDownscales 2" in p.stderr
    assert got["pos"].shape[0] == N and "densify @" not in p.stderr
    r32, lv = _restated(cams, targets, init, LEG1, np.float32)
    r64, _ = _restated(cams, targets, init, LEG1, np.float64)
    assert lv == [2] * 4 + [1] * 4 + [0] * 4
    report = {"loss_line": [_loss_line(p, 0), r64.losses[0]]}
    try:
        _compare(got, r32, r64, init, 1e-4, 0.90, report)
        for k in KEYS:
            assert report[k]["rel_l2_of_update"] < 1e-2, (k, report[k])
        assert abs(report["loss_line"][0] - r64.losses[0]) < 2e-4 * max(r64.losses[0], 1e-3), report["loss_line"]
    finally:
        _dump("resolution_schedule_parity_l1.json", report)


@pytest.mark.gpu
def test_plugin_two_levels_with_u8_views_mask_and_ssim(tmp_path, scene_and_targets):
    """--packLevel 1 --useMask 1 --ssim 0.2, 8 iterations with --resolutionSchedule 4 --numDownscales 1: four steps at 71x55 on targets
    box-filtered from the BYTES, gradients weighted by the box-filtered mask, SSIM over the level's size; four at full size on the
    existing path. Bars of test_plugin_reference_cli_loss_path with SSIM: 99.5 % of the pinned elements within 1e-4, every one within
    1e-3, >= 0.85 of each group pinned, the update within 1e-2; the `Iteraions 0` line is the unmasked restated loss within 2e-4."""
    cams, targets = scene_and_targets
    out, init, p, got = _product(tmp_path, LEG2, _schedule(LEG2))
    assert "PackF32ToU8: 8-bit training views" in p.stderr and "useMask 1" in p.stderr
    starts = [(int(m.group(1)), m.group(2), int(m.group(3))) for m in START_LINE.finditer(p.stderr)]
    assert starts == [(1, "71x55", 2), (5, "142x110", 1)], p.stderr[-3000:]
    r32, _ = _restated(cams, targets, init, LEG2, np.float32, u8=True, mask=True)
    r64, _ = _restated(cams, targets, init, LEG2, np.float64, u8=True, mask=True)
    report = {"loss_line": [_loss_line(p, 0), r64.losses[0]]}
    try:
        _bars(got, r32, r64, init, report, ssim=True)
        assert abs(report["loss_line"][0] - r64.losses[0]) < 2e-4 * max(r64.losses[0], 1e-3), report["loss_line"]
    finally:
        _dump("resolution_schedule_parity_u8_mask_ssim.json", report)


@pytest.mark.gpu
def test_off_means_off(tmp_path, leg1_run):
    """--resolutionSchedule 0 is the run without the flag, byte for byte, and logs nothing of the schedule. Two runs of this build can
    only be compared byte for byte where the build itself is reproducible: the composite backward adds a splat's gradient once per
    tile with fp32 atomics, in an order that differs from run to run — except in an image of ONE 16x16 tile, where
    every row receives a single add onto zero. So the byte comparison runs at 16x16 (12 steps, 2000 splats), and the model that the
    schedule does change is the three-level run's against a plain run of its own scene."""
    one_tile = ["--inputPath", f"synthetic:N={N},W=16,H=16,cams={CAMS},sh={SH},seed={SEED}", "--maxIteration", str(LEG1["K"])] + LEG1["flags"]
    a, b, c = (str(tmp_path / t / "it") for t in "abc")
    pa = _run(one_tile + ["--outputPath", a])
    pb = _run(one_tile + ["--outputPath", b, "--resolutionSchedule", "0"])
    pc = _run(["--inputPath", SRC, "--maxIteration", str(LEG1["K"]), "--outputPath", c] + LEG1["flags"])
    for p in (pa, pb, pc):
        assert "resolution" not in p.stderr, p.stderr[-3000:]
    blob = open(a + "_12.ply", "rb").read()
    assert blob == open(b + "_12.ply", "rb").read()
    assert _read_ply(a + "_12.ply")["pos"].shape[0] == N
    on, off = leg1_run[3], _read_ply(c + "_12.ply")
    assert not np.array_equal(on["sh0"], off["sh0"])                          # and the schedule does change what is trained


@pytest.mark.gpu
def test_resume_lands_on_the_level_of_its_step(tmp_path, leg1_run):
    out = str(tmp_path / "m" / "it")
    os.makedirs(os.path.dirname(out))
    shutil.copy(leg1_run[0] + "_12.ply", out + "_6.ply")
    p = _run(["--inputPath", SRC, "--maxIteration", "9", "--outputPath", out, "--load_itr", "6"] + LEG1["flags"] + _schedule(LEG1))
    assert "(resumed)" in p.stderr, p.stderr[-3000:]
    starts = [(int(m.group(1)), m.group(2), int(m.group(3))) for m in START_LINE.finditer(p.stderr)]
    assert starts == [(7, "71x55", 2), (9, "142x110", 1)], p.stderr[-3000:]
    assert "resolution @7: 71x55 (1/2)" in p.stderr
    assert [(int(m.group(1)), m.group(2)) for m in END_LINE.finditer(p.stderr)] == [(2, "71x55"), (1, "142x110")]


EVAL_LINE = re.compile(r"eval @(\d+): (\d+) views, PSNR (\S+) dB, SSIM (\S+), L1 (\S+)")


@pytest.mark.gpu
def test_held_out_quality_still_improves_with_the_schedule(tmp_path):
    """20000 splats @ 256x256, 4 cameras (camera 0 held out), 400 iterations, --resolutionSchedule 100: 100 steps at 64x64, 100 at
    128x128, 200 at full size; the evaluation is at full size throughout. Only the sign is asserted — nobody has measured by how much
    the curves with and without the schedule differ; both go to resolution_schedule_quality.json in the run-report directory."""
    curves = {}
    for tag, extra in (("schedule_100", ["--resolutionSchedule", "100"]), ("off", [])):
        out = str(tmp_path / tag / "iteration")
        p = _run(["--inputPath", "synthetic:N=20000,W=256,H=256,cams=4,sh=1,seed=3", "--maxIteration", "400", "--outputPath", out,
                  "--evalHoldout", "4", "--evalEvery", "100"] + extra)
        lines = [(int(m.group(1)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in EVAL_LINE.finditer(p.stderr)]
        assert [l[0] for l in lines] == [100, 200, 300, 400], p.stderr[-3000:]
        curves[tag] = dict(iteration=[l[0] for l in lines], psnr=[l[1] for l in lines], ssim=[l[2] for l in lines], l1=[l[3] for l in lines],
                           ms_per_step={m.group(2): float(m.group(3)) for m in END_LINE.finditer(p.stderr)})
        if extra:
            starts = [(int(m.group(1)), m.group(2), int(m.group(3))) for m in START_LINE.finditer(p.stderr)]
            assert starts == [(1, "64x64", 4), (101, "128x128", 2), (201, "256x256", 1)], p.stderr[-3000:]
    _dump("resolution_schedule_quality.json", curves)
    print("held-out PSNR by evaluation:", {k: v["psnr"] for k, v in curves.items()})
    psnr = curves["schedule_100"]["psnr"]
    assert np.isfinite(psnr).all() and psnr[-1] > psnr[0], curves
