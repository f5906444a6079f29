"""`--mipFilter3d 1` in the product: gaussian_train against a restated step, its saves, its recompute rule, its off path, two ranks.

The restated step is TrainStepRef (tests/train_step_ref.py) with the filter around the oracle: the reference filter of the positions the
run was loaded with (tests/filter3d_ref.py; the plugin computes it at load and keeps it for 100 steps) -> apply -> the oracle's forward
and backward on the effective scale and opacity -> chain -> the restatement's own Adam on the trained values. The trajectory is held to
the bars tests/test_train_step_options.py uses for its 8-step L1-only runs (`_bars`: rtol 1e-4 with floor 1e-2, relative L2 of the update
< 1e-2, pinned share >= 0.90). The CPU test measures that share for this scene, and that a run WITHOUT the filter is told apart.

Scene: 600 splats, 4 cameras, 64x48 (4 x 3 tiles), SH degree 1, 8 steps, L1 only, ADC with its warm-up beyond the run."""
import os
import re
import numpy as np
import pytest
from oracle.oracle import Oracle
import filter3d_ref as F
from train_step_ref import TrainStepRef, KEYS
from test_train_step import _run, _read_ply, _hip_targets
from test_train_step_options import _flags, _start_model, _oracle_targets, _bars, _pinned, _median_difference, _product, _src, _scene, RTOL, SHARE_L1

CASE = dict(n=600, W=64, H=48, cams=4, sh=1, seed=41, K=8)


class FilteredStepRef(TrainStepRef):
    """TrainStepRef with the 3D smoothing filter of `filter_pos` under the cameras `filter_cams` (default: the start model's, all cameras)"""
    def __init__(self, *a, filter_pos=None, filter_cams=None, **kw):
        super().__init__(*a, **kw)
        pos = self.P["pos"] if filter_pos is None else filter_pos
        self.filt = F.compute(pos, F.pack_cameras(self.cams if filter_cams is None else filter_cams), np.float64)[0].astype(self.dt)

    def gradients(self):
        f = self.dt.type
        trained = self.P
        se, oe = F.apply(trained["scale"], trained["opacity"], self.filt, f)
        self.P = dict(trained, scale=se.astype(self.dt), opacity=oe.astype(self.dt))       # what the rasterizer reads
        try:
            G = super().gradients()
        finally:
            self.P = trained
        gs, go = F.chain(trained["scale"], trained["opacity"], self.filt, G["scale"], G["opacity"], f)
        G["scale"], G["opacity"] = gs.astype(self.dt), go.astype(self.dt)
        return G


def _case():
    spec, cams = _scene(CASE["n"], CASE["W"], CASE["H"], CASE["cams"], CASE["sh"], CASE["seed"])
    return spec, cams, _start_model(spec, CASE["seed"])


def _pair(cls, cams, tg, init, K):
    r32, r64 = (cls(Oracle, cams, tg, init, CASE["sh"], K, dt) for dt in (np.float32, np.float64))
    for _ in range(K):
        r32.train_step(); r64.train_step()
    return r32, r64


def test_filtered_case_is_pinned_and_discriminates():
    """float32 against float64 of the restatement pins the share the GPU test asserts, and the filter moves the trajectory: with it on and
    off the median moved opacity differs by more than 10x the element tolerance; the scales, whose rate is a tenth of the opacity's, by
    more than 2x (a median above 1x already puts half the moved elements outside the bar). Measured (pos sh0 shN opacity scale rot): share
    1 1 1 .995 1 1; median difference opacity 4.9e-3, scale 2.9e-4."""
    spec, cams, init = _case()
    tg = _oracle_targets(spec, cams, CASE["sh"])
    r32, r64 = _pair(FilteredStepRef, cams, tg, init, CASE["K"])
    assert 0 < r64.filt.min() and np.median(r64.filt / np.exp(init["scale"].max(1))) > 0.1, "the filter is negligible beside the splats"
    share = _pinned(r32, r64, init, SHARE_L1)
    off = TrainStepRef(Oracle, cams, tg, init, CASE["sh"], CASE["K"], np.float64)
    for _ in range(CASE["K"]):
        off.train_step()
    diff = {k: _median_difference(r64, off, init, k) for k in ("opacity", "scale")}
    print("pinned share", share, "median difference", diff)
    assert diff["opacity"] > 10 * RTOL and diff["scale"] > 2 * RTOL, diff


@pytest.fixture(scope="module")
def filtered_run(tmp_path_factory):
    """ONE run of the product shared by the tests below: 8 steps from the start model, through --load_itr 0"""
    spec, cams, init = _case()
    p, got = _product(tmp_path_factory.mktemp("f3d"), "m", CASE, init, _flags(mipFilter3d=1), 0, CASE["K"])
    out = re.search(r"saved \d+ splats to (\S+)_%d\.ply" % CASE["K"], p.stderr).group(1)
    return dict(spec=spec, cams=cams, init=init, p=p, got=got, out=out)


@pytest.mark.gpu
def test_plugin_steps_follow_the_restated_filtered_step(filtered_run, gpu_device):
    """8 steps of --mipFilter3d 1 against FilteredStepRef under the bars of the 8-step L1-only trajectory tests; the filter is computed
    once at load (a resume logs it) and again for the save, nowhere between."""
    r = filtered_run
    tg = _hip_targets(r["spec"], r["cams"], CASE["sh"])
    r32, r64 = _pair(FilteredStepRef, r["cams"], tg, r["init"], CASE["K"])
    report = {}
    _bars(r["got"], r32, r64, r["init"], report, ssim=False)
    print({k: (round(v["comparable"], 4), v["worst"], v["rel_l2_of_update"]) for k, v in report.items()})
    err = r["p"].stderr
    assert "config: mipFilter3d 1" in err and "(resumed)" in err
    lines = re.findall(r"filter3d @(\d+): (\d+) splats, (\d+) seen, filter min/median/max ([0-9.eE+-]+)/([0-9.eE+-]+)/([0-9.eE+-]+), ([0-9.]+) ms", err)
    assert [(int(a), int(b)) for a, b, *_ in lines] == [(0, CASE["n"]), (CASE["K"], CASE["n"])], err[-2000:]
    filt, seen = F.compute(r["init"]["pos"], F.pack_cameras(r["cams"]))
    assert int(lines[0][2]) == seen.sum() and np.allclose([float(v) for v in lines[0][3:6]], [filt.min(), np.sort(filt)[CASE["n"] // 2], filt.max()], rtol=1e-4)


@pytest.mark.gpu
def test_saves_keep_the_trained_model_and_export_the_fused_one(filtered_run, gpu_device):
    """<out>_8.ply holds the trained values (it is what the trajectory test compares); <out>_8.fused.ply, implied by the option, is the
    reference apply of that file under the reference filter of ITS positions — every other group bit for bit the resume PLY's."""
    r = filtered_run
    got = r["got"]
    fused = _read_ply(f"{r['out']}_{CASE['K']}.fused.ply")
    assert "exportFormats 32" in r["p"].stderr and "(implied by mipFilter3d)" in r["p"].stderr and "fused.ply %d splats" % CASE["n"] in r["p"].stderr
    for k in ("pos", "sh0", "shN", "rot"):
        assert np.array_equal(fused[k].view(np.uint32), got[k].view(np.uint32)), k
    filt = F.compute(got["pos"], F.pack_cameras(r["cams"]))[0]
    rs, ro = F.apply(got["scale"], got["opacity"], filt)
    f32 = filt.astype(np.float32)
    rs32, ro32 = F.apply(got["scale"], got["opacity"], f32, np.float32)
    scaled = lambda x, ref: float((np.abs(x.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max())
    for name, x, ref, r32 in (("scale", fused["scale"], rs, rs32), ("opacity", fused["opacity"], ro, ro32)):
        e_dev, e_32 = scaled(x, ref), scaled(r32, ref)
        print(f"fused {name}: device {e_dev:.3g}, float32 restatement {e_32:.3g}, bar {4 * e_32:.3g}")
        assert e_dev <= 4 * e_32, name
    assert np.all(fused["opacity"] < got["opacity"]) and np.all(fused["scale"] > got["scale"])


@pytest.mark.gpu
def test_a_refinement_and_a_resume_recompute_the_filter(tmp_path, gpu_device):
    """A run that crosses one refinement (at 5 of 8 steps) logs the filter of the new splat set right after it, with the new count, and the
    fused file has that count; resuming from its model logs the filter at load."""
    out = str(tmp_path / "it")
    flags = _flags(mipFilter3d=1, warmupLength=2, refineEvery=5, growGrad2d=0.00002)
    p = _run(["--inputPath", _src(CASE), "--maxIteration", "8", "--outputPath", out] + flags)
    err = p.stderr
    m = re.search(r"densify @5: (\d+) -> (\d+) splats", err)
    assert m and int(m.group(2)) != int(m.group(1)), err[-2000:]
    n_new = int(m.group(2))
    after = err[m.end():]
    lines = [(int(a), int(b)) for a, b in re.findall(r"filter3d @(\d+): (\d+) splats", err)]
    assert lines == [(0, CASE["n"]), (5, n_new), (8, n_new)] and "filter3d @5" in after, lines
    assert _read_ply(f"{out}_8.fused.ply")["pos"].shape[0] == n_new == _read_ply(f"{out}_8.ply")["pos"].shape[0]
    q = _run(["--inputPath", _src(CASE), "--maxIteration", "9", "--outputPath", out, "--load_itr", "8"] + flags)
    lines = [(int(a), int(b)) for a, b in re.findall(r"filter3d @(\d+): (\d+) splats", q.stderr)]
    assert "(resumed)" in q.stderr and lines == [(8, n_new), (9, n_new)], q.stderr[-2000:]


@pytest.mark.gpu
def test_off_is_untouched(tmp_path, gpu_device):
    """--mipFilter3d 0 and no flag at all: byte-identical models, the same log, no filter3d line, no fused file. Two trainings are compared,
    so the views are ONE tile (16x12): the size at which the trainer repeats from run to run (above it the composite backward's fp32
    atomics land in another order each run, with or without this option)."""
    runs = []
    src = f"synthetic:N={CASE['n']},W=16,H=12,cams={CASE['cams']},sh={CASE['sh']},seed={CASE['seed']}"
    for tag, extra in (("zero", ["--mipFilter3d", "0"]), ("none", [])):
        out = str(tmp_path / tag / "it")
        os.makedirs(os.path.dirname(out))
        p = _run(["--inputPath", src, "--maxIteration", "6", "--outputPath", out] + _flags() + extra)
        assert "filter3d" not in p.stderr and "mipFilter3d" not in p.stderr and sorted(os.listdir(os.path.dirname(out))) == ["it_6.ply"], p.stderr[-1500:]
        runs.append((open(out + "_6.ply", "rb").read(), re.sub(r"\S*/it_6\.ply", "", p.stderr)))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > CASE["n"] * 236
    strip = lambda log: [l for l in log.splitlines() if " ms" not in l and "it/s" not in l]
    assert strip(runs[0][1]) == strip(runs[1][1])


@pytest.mark.gpu
def test_two_ranks_stay_bit_identical_with_the_filter(tmp_path, gpu_device):
    """two ranks over the TCP test backend, the filter on, one refinement inside the run: the replicas' models are the same bytes"""
    from test_gpu_multirank import _plugin_run
    args = ["--inputPath", _src(CASE), "--maxIteration", "8"] + _flags(mipFilter3d=1, warmupLength=2, refineEvery=5, growGrad2d=0.00002)
    out, res = _plugin_run(tmp_path, "w2", args, 2)
    assert "TEST backend" in res[0][2] and "filter3d @5" in res[0][2] and "densify @5" in res[0][2]
    a, b = open(out + "_8.ply", "rb").read(), open(out + "_8.ply.rank1", "rb").read()
    assert len(a) > CASE["n"] * 236 and a == b, "the two replicas differ"
    assert os.path.exists(out + "_8.fused.ply")


@pytest.mark.gpu
def test_two_ranks_pipelined_exchange_with_the_filter_equals_unpipelined(tmp_path, gpu_device):
    """DVS_EXCHANGE_PIPELINE=1 (DVS_A9_CHUNKS=2) with the filter on: apply runs per chunk in front of the next iteration's early projection,
    and that projection is not made when the filter is due at the next step. 135 steps over one refinement (at 30: the filter of the new
    set) and one periodic recompute (at 130), two ranks, views of ONE tile (16x12: the trainer repeats bit for bit there): the replicas
    are the same bytes and so are the pipelined and the unpipelined run, model and fused export alike."""
    from test_gpu_multirank import _plugin_run
    src = f"synthetic:N={CASE['n']},W=16,H=12,cams={CASE['cams']},sh={CASE['sh']},seed={CASE['seed']}"
    args = ["--inputPath", src, "--maxIteration", "135"] + _flags(mipFilter3d=1, warmupLength=2, refineEvery=30, refineStopIter=40, growGrad2d=0.00002)
    base = {"DVS_EXCHANGE": "factorised", "DVS_A9_CHUNKS": "2"}
    outp, resp = _plugin_run(tmp_path, "p", args, 2, dict(base, DVS_EXCHANGE_PIPELINE="1"))
    outu, resu = _plugin_run(tmp_path, "u", args, 2, base)
    assert "PIPELINED across the iteration boundary" in resp[0][2] and "PIPELINED" not in resu[0][2]
    for res in (resp, resu):
        lines = [int(a) for a in re.findall(r"filter3d @(\d+):", res[0][2])]
        assert lines == [0, 30, 130, 135] and "densify @30" in res[0][2], lines
    m = re.search(r"densify @30: (\d+) -> (\d+) splats", resp[0][2])
    assert int(m.group(2)) >= 512, "too few splats left for two A9 chunks: the pipelined path would not run after the refinement"
    p0, p1, u0 = (open(f, "rb").read() for f in (outp + "_135.ply", outp + "_135.ply.rank1", outu + "_135.ply"))
    assert len(p0) > 512 * 236 and p0 == p1, "pipelined: the two replicas differ"
    assert p0 == u0, "the pipelined run differs from the unpipelined one"
    assert open(outp + "_135.fused.ply", "rb").read() == open(outu + "_135.fused.ply", "rb").read()
