"""LOD export through the plugin, end to end: gaussian_train on a small synthetic scene with --eval --exportLod 2 --lodResolution 32, the
same run with --exportOrient +y, and a run without the flag. Every <outputPath>_<it>.lod<k>.ply loads with the project's PLY reader,
equals the restatement (tests/lod_ref.py) applied to the saved full PLY within the bounds of tests/test_gpu_lod.py — and the library's own
merge of that PLY bit for bit —, the log and the eval JSON carry the per-level scores, the oriented run's levels are the transform of
the merged model, and without the flag nothing is written or logged."""
import json
import math
import os
import re
import subprocess
import numpy as np
import pytest
import lod_ref as L
import transform_ref as T
import test_gpu_lod as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
SCENE = ["--inputPath", "synthetic:N=2000,W=64,H=64,cams=8,sh=1,seed=1", "--maxIteration", "5", "--eval"]
LOD = ["--exportLod", "2", "--lodResolution", "32"]
IT, DEGREE = 5, 1


def _run(args):
    e = dict(os.environ)
    for k in ("DVS_EXPORT_FORMATS", "DVS_EXPORT_TRANSFORM", "DVS_EXPORT_ORIENT", "DVS_EXPORT_LOD", "DVS_LOD_RESOLUTION"):
        e.pop(k, None)
    p = subprocess.run([DRIVER] + SCENE + args, capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("levels")
    on, orient, off = (str(base / t / "iteration") for t in ("on", "orient", "off"))
    return on, _run(["--outputPath", on] + LOD), orient, _run(["--outputPath", orient, "--exportOrient", "+y"] + LOD), off, _run(["--outputPath", off])


def _level_lattice(model, k):
    ok = np.isfinite(model["pos"]).all(1)
    bounds = np.concatenate([model["pos"][ok].min(0), model["pos"][ok].max(0)])
    return L.lattice_for(bounds, 32 >> (k - 1))


def _device_merge(dev, model, k):
    import torch
    from divshot_amd import lod as LOD_
    o, c, d = _level_lattice(model, k)
    t = {key: torch.from_numpy(np.ascontiguousarray(model[key])).to(dev) for key in L.KEYS}
    out, counts = LOD_.merge_splats(t, lattice=LOD_.make_lattice(o, c, d), sh_degree=DEGREE, shn_layout=0)
    return {key: v.cpu().numpy() for key, v in out.items()}, counts


def test_levels_load_and_equal_the_restatement_of_the_full_ply(gpu_device, runs):
    from divshot_amd._lib import read_ply
    on, p_on = runs[0], runs[1]
    model = read_ply(on + f"_{IT}.ply")
    n = len(model["opacity"])
    sizes = []
    for k in (1, 2):
        level = read_ply(on + f"_{IT}.lod{k}.ply")
        m = len(level["opacity"])
        sizes.append(m)
        o, c, d = _level_lattice(model, k)
        ref, info = L.merge(model, o, c, d, DEGREE, np.float64)
        assert m == info["m"] and info["n_dropped"] == 0
        single = info["single"]
        for key in L.KEYS:
            assert np.array_equal(level[key][single].view(np.uint32), ref[key][single].astype(np.float32).view(np.uint32)), (k, key)
        assert np.array_equal(L.cell_keys(level["pos"], o, c, d), info["keys"])
        assert (level["shN"][~single][:, L.LIMIT[DEGREE]:] == 0).all()
        e = G.errors(level, ref, info, G.extent(model["pos"]))
        print(f"level {k}: {n} -> {m} splats ({int((~single).sum())} merged clusters), mu {e[0]:.3e} sh {e[1]:.3e} alpha {e[2]:.3e} cov {e[3]:.3e}")
        assert e[0] <= G.BOUND_MU and e[1] <= G.BOUND_SH and e[2] <= G.BOUND_ALPHA and e[3] <= G.BOUND_COV, e
        mine, counts = _device_merge(gpu_device, model, k)                   # the trainer calls the library on the tiled arrays: the same bytes
        assert counts["m"] == m
        for key in L.KEYS:
            assert np.array_equal(level[key].view(np.uint32), mine[key].reshape(level[key].shape).view(np.uint32)), (k, key)
    assert 0 < sizes[1] <= sizes[0] <= n and sizes[1] < n


def test_log_and_eval_json_carry_the_scores(gpu_device, runs):
    on, p_on = runs[0], runs[1]
    err = p_on.stderr
    assert len(re.findall(r"config: lodExport 2 levels, resolution 32", err)) == 1, err[-3000:]
    full = re.search(rf"eval @{IT}: 1 views, PSNR (\S+) dB", err)
    assert full, err[-3000:]
    doc = json.load(open(on + f"_{IT}_eval.json"))
    assert sorted(doc["lod"]) == ["1", "2"]
    for k, res in ((1, 32), (2, 16)):
        line = re.search(rf"lod @{IT}: level {k}, lattice \d+x\d+x\d+ \(resolution {res}, cell \S+\): 2000 -> (\d+) splats, 0 dropped; count [\d.]+ ms, "
                         rf"merge [\d.]+ ms, file [\d.]+ ms; PSNR (\S+) dB \(full model (\S+) dB\), SSIM (\S+), L1 (\S+), score [\d.]+ ms", err)
        assert line, err[-3000:]
        rec = doc["lod"][str(k)]
        assert rec["n_splats"] == int(line.group(1)) and line.group(3) == full.group(1)
        assert rec["psnr"] == float(line.group(2)) and rec["ssim"] == float(line.group(4)) and rec["l1"] == float(line.group(5).rstrip(","))
        assert all(math.isfinite(rec[key]) for key in ("psnr", "ssim", "l1", "mse")) and 0 < rec["psnr"] < 100 and rec["ssim"] <= 1.0
        print(f"level {k}: {rec['n_splats']} splats, PSNR {rec['psnr']:.3f} dB (full model {float(full.group(1)):.3f} dB)")
    assert doc["mean"]["psnr"] == float(full.group(1))


def test_oriented_run_writes_the_transform_of_the_levels(gpu_device, runs):
    """The levels are merged in the training frame and then taken into the export frame like every other export: each file equals the
    restatement of dvs_transform_splats (tests/transform_ref.py) applied, bit for bit, to the library's merge of the run's own resume
    PLY (which stays in the training frame) — the levels of the first run, as far as the trainer repeats run to run."""
    from divshot_amd import transform as X
    from divshot_amd._lib import read_ply
    orient, p = runs[2], runs[3]
    line = re.search(r"config: exportTransform p' = s R p \+ t with R = \[(.*?)\], t = \((.*?)\), s = (\S+),", p.stderr)
    assert line, p.stderr[-3000:]
    R = np.array([float(v) for v in line.group(1).replace(";", " ").split()], np.float32)
    t = np.array([float(v) for v in line.group(2).split(",")], np.float32)
    s = np.float32(line.group(3))
    assert s == 1.0 and not np.allclose(R.reshape(3, 3), np.eye(3))
    D = X.sh_rotation(R)
    model = read_ply(orient + f"_{IT}.ply")
    for k in (1, 2):
        level = read_ply(orient + f"_{IT}.lod{k}.ply")
        merged, counts = _device_merge(gpu_device, model, k)
        assert counts["m"] == len(level["opacity"]) > 0
        want = T.transform_splats(R, t, s, D, merged["pos"], merged["shN"], merged["scale"], merged["rot"], DEGREE)
        for key in ("pos", "shN", "scale", "rot"):
            assert np.array_equal(level[key].view(np.uint32), want[key].reshape(level[key].shape).view(np.uint32)), (k, key)
        for key in ("sh0", "opacity"):
            assert np.array_equal(level[key].view(np.uint32), merged[key].reshape(level[key].shape).view(np.uint32)), (k, key)
    # the scores are taken before the transform, in the cameras' frame: finite and a model's, not a misplaced one's
    doc = json.load(open(orient + f"_{IT}_eval.json"))
    base = json.load(open(runs[0] + f"_{IT}_eval.json"))
    for k in ("1", "2"):
        assert abs(doc["lod"][k]["psnr"] - base["lod"][k]["psnr"]) <= 1.0, (doc["lod"][k], base["lod"][k])


def test_without_the_flag_nothing_is_written_or_logged(gpu_device, runs):
    off, p_off = runs[4], runs[5]
    assert sorted(os.listdir(os.path.dirname(off))) == [f"iteration_{IT}.ply", f"iteration_{IT}_eval.json"]
    assert "lod" not in json.load(open(off + f"_{IT}_eval.json"))
    assert "lod @" not in p_off.stderr and "lodExport" not in p_off.stderr and ".lod" not in p_off.stderr
