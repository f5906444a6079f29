"""Held-out evaluation of the plugin (config evalHoldout / evalEvery; CLI --eval, --evalHoldout, --evalEvery): the numbers it reports
for cameras it did not train on are the image metrics of what the saved PLY renders, at the bars the metric kernel itself is held to
(tests/test_gpu_image_metrics.py); held-out views get better while the others are trained; off means nothing of it happens; a split
that leaves nothing to train or test on turns evaluation off and trains on."""
import json
import os
import re
import subprocess
import numpy as np
import pytest
from metrics_ref import image_metrics_np, assert_metrics_close
from train_step_ref import pack_unpack_u8
from test_train_step import DRIVER, _read_ply, _scene, _hip_targets

pytestmark = pytest.mark.gpu

EVAL_LINE = re.compile(r"eval @(\d+): (\d+) views, PSNR (\S+) dB, SSIM (\S+), L1 (\S+)")
SHORT = ["--inputPath", "synthetic:N=3000,W=96,H=80,cams=9,sh=2,seed=4", "--maxIteration", "60"]


def _cli(args):
    p = subprocess.run([DRIVER] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def short_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eval") / "m" / "iteration")
    return out, _cli(SHORT + ["--eval", "--evalEvery", "30", "--outputPath", out])


def test_reported_numbers_are_the_metrics_of_the_saved_model(short_run):
    import torch
    from divshot_amd.raster import Rasterizer, params_to_device
    out, p = short_run
    assert re.search(r"evaluation: 2 of 9 cameras held out of training \(evalHoldout 8: cameras 0 8\)", p.stderr), p.stderr[-3000:]
    lines = [(int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in EVAL_LINE.finditer(p.stderr)]
    assert [(l[0], l[1]) for l in lines] == [(30, 2), (60, 2)], p.stderr[-3000:]
    assert not os.path.exists(out + "_30_eval.json")                          # the file belongs to a save
    J = json.load(open(out + "_60_eval.json"))
    assert (J["iteration"], J["n_splats"], J["sh_degree"], J["holdout"]) == (60, 3000, 2, 8)
    assert [v["camera"] for v in J["views"]] == [0, 8] and set(J["mean"]) == {"psnr", "ssim", "l1", "mse"}
    for k in J["mean"]:
        assert abs(J["mean"][k] - np.mean([v[k] for v in J["views"]])) <= 1e-14 * abs(J["mean"][k])
    assert lines[-1][2:] == (J["mean"]["psnr"], J["mean"]["ssim"], J["mean"]["l1"])       # 17 digits: the same doubles
    # the same two views from the saved PLY through the C-ABI, against the plugin's targets: HIP render of the generating scene, then 8 bits
    spec, cams = _scene(3000, 96, 80, 9, 2, 4)
    targets = _hip_targets(spec, cams, 2)
    A = _read_ply(out + "_60.ply")
    r = Rasterizer(0, max_splats=spec.n, max_w=spec.width, max_h=spec.height)
    P = params_to_device(A, torch.device("cuda", 0))
    for v in J["views"]:
        img = r.forward(P, cams[v["camera"]], sh_degree=2).detach().cpu().numpy()
        ref = image_metrics_np(img, pack_unpack_u8(targets[v["camera"]]))
        assert_metrics_close((v["mse"], v["l1"], v["ssim"], v["psnr"]), ref, f"camera {v['camera']}")
    r.close()


def test_held_out_view_improves_while_the_others_train(tmp_path):
    out = str(tmp_path / "model" / "iteration")
    p = _cli(["--inputPath", "synthetic:N=20000,W=256,H=256,cams=4,sh=1,seed=3", "--maxIteration", "400", "--outputPath", out,
              "--evalHoldout", "4", "--evalEvery", "100"])
    assert re.search(r"evaluation: 1 of 4 cameras held out of training \(evalHoldout 4: cameras 0\)", p.stderr), p.stderr[-3000:]
    lines = [(int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))) for m in EVAL_LINE.finditer(p.stderr)]
    assert [(l[0], l[1]) for l in lines] == [(100, 1), (200, 1), (300, 1), (400, 1)], p.stderr[-3000:]
    assert np.isfinite(np.array([l[2:] for l in lines])).all()
    print("held-out PSNR by evaluation:", [l[2] for l in lines])
    assert lines[-1][2] > lines[0][2], lines                                  # only the sign: nobody has measured by how much
    J = json.load(open(out + "_400_eval.json"))
    assert [v["camera"] for v in J["views"]] == [0] and J["mean"]["psnr"] == lines[-1][2]
    assert all(np.isfinite(list(v.values())).all() for v in J["views"])


def test_off_means_off(tmp_path, short_run):
    out = str(tmp_path / "m" / "iteration")
    p = _cli(SHORT + ["--outputPath", out])
    assert os.path.exists(out + "_60.ply")
    assert not [f for f in os.listdir(os.path.dirname(out)) if f.endswith("_eval.json")]
    assert "eval @" not in p.stderr and "held out" not in p.stderr and "evaluation" not in p.stderr, p.stderr[-3000:]
    # and the split does change what is trained on: with cameras 0 and 8 held out the model is another one
    on, off = _read_ply(short_run[0] + "_60.ply"), _read_ply(out + "_60.ply")
    assert not np.array_equal(on["sh0"], off["sh0"])


def test_degenerate_split_trains_with_evaluation_off(tmp_path):
    out = str(tmp_path / "m" / "iteration")
    p = _cli(["--inputPath", "synthetic:N=2000,W=64,H=64,cams=1,sh=1,seed=2", "--maxIteration", "20", "--eval", "--evalEvery", "10", "--outputPath", out])
    assert p.stderr.count("evaluation is OFF") == 1, p.stderr[-3000:]
    assert "eval @" not in p.stderr and os.path.exists(out + "_20.ply") and not os.path.exists(out + "_20_eval.json")
