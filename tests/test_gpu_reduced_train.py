"""The .reduced.ply export end to end: gaussian_train on a small synthetic scene with --eval --exportFormat reduced --cullSH 1. The file
exists and reads back, its block counts sum to the model's splats and match the log line, the decoded model's score is logged and in the
eval JSON with finite numbers, the full PLY and the full model's evaluation are what a run without the flag gives on the same parameters,
--cullSH 0 puts every splat in the block of the model's degree, a modelPath ending in .reduced.ply turns the export on, and without any of
it nothing new is written or logged. The PSNR drop is printed, not bounded: it cannot be derived in advance."""
import json
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import reduced_ply_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
SCENE = ["--inputPath", "synthetic:N=2000,W=64,H=64,cams=8,sh=2", "--maxIteration", "30", "--eval"]
LINE = r"export @30: reduced (\d+) splats \((\d+)/(\d+)/(\d+)/(\d+) by degree\), (\d+) bytes, degree select [\d.]+ ms, codebooks [\d.]+ ms " \
       r"\((\d+) iterations at most\), pack [\d.]+ ms"


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("DVS_EXPORT_FORMATS", "DVS_SH_CULL_THRESHOLD", "DVS_REDUCED_HALF"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([DRIVER] + SCENE + args, capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """30 iterations with the export and cullSH, the same without either, and a run without the flag that resumes from the first one's
    model at iteration 30 and saves at once (two trainings of this build are not comparable bit for bit — the composite backward's fp32
    atomics — so the run whose evaluation must EQUAL the first one's scores the very same parameters)."""
    base = tmp_path_factory.mktemp("e2e")
    on, off, same = (str(base / t / "iteration") for t in ("on", "off", "same"))
    p_on = _run(["--outputPath", on, "--exportFormat", "reduced", "--cullSH", "1"])
    p_off = _run(["--outputPath", off])
    os.makedirs(os.path.dirname(same))
    shutil.copy(on + "_30.ply", same + "_30.ply")
    p_same = _run(["--outputPath", same, "--load_itr", "30"])
    assert "(resumed)" in p_same.stderr, p_same.stderr[-3000:]
    return on, p_on, off, p_off, same


def test_file_counts_and_log_line(gpu_device, runs):
    on, p = runs[0], runs[1]
    path = on + "_30.reduced.ply"
    assert os.path.exists(path)
    counts, half, payload = R.parse(open(path, "rb").read())                 # (asserts the header's shape and the exact size)
    model = R.read(path)
    m = re.search(LINE, p.stderr)
    assert m, p.stderr[-3000:]
    assert int(m.group(1)) == 2000 == sum(counts) == len(model["opacity"])
    assert [int(m.group(k)) for k in range(2, 6)] == list(counts) and counts[3] == 0      # a model of degree 2
    assert int(m.group(6)) == os.path.getsize(path) and not half and 1 <= int(m.group(7)) <= 100
    assert all(np.isfinite(model[k]).all() for k in R.FIELDS)
    print(f"degree histogram {list(counts)}, {os.path.getsize(path)} bytes = {os.path.getsize(path) / 2000:.2f} B per splat "
          f"(full PLY {os.path.getsize(on + '_30.ply') / 2000:.0f})")
    assert "config: exportFormats 8" in p.stderr and "config: reduced export" in p.stderr and "without measurement" in p.stderr
    assert not [l for l in p.stderr.splitlines() if "IGNORED" in l and "cullSH" in l]


def test_decoded_model_score_is_reported(gpu_device, runs):
    on, p = runs[0], runs[1]
    J = json.load(open(on + "_30_eval.json"))
    assert set(J["exports"]) == {"reduced"} and set(J["exports"]["reduced"]) == {"psnr", "ssim", "l1", "mse"}
    assert all(np.isfinite(v) for v in J["exports"]["reduced"].values())
    m = re.search(r"export @30: reduced decoded model: PSNR (\S+) dB \(full model (\S+) dB\), SSIM (\S+), L1 (\S+)", p.stderr)
    assert m and all(np.isfinite(float(g)) for g in m.groups()), p.stderr[-3000:]
    assert float(m.group(1)) == J["exports"]["reduced"]["psnr"] and float(m.group(2)) == J["mean"]["psnr"]
    print(f"held-out PSNR: full model {J['mean']['psnr']:.6f} dB, decoded .reduced.ply model {J['exports']['reduced']['psnr']:.6f} dB; "
          f"SSIM {J['mean']['ssim']:.6f} -> {J['exports']['reduced']['ssim']:.6f}")


def test_full_model_outputs_are_what_they_were(gpu_device, runs):
    on, p, off, q, same = runs
    J, K, K2 = (json.load(open(x + "_30_eval.json")) for x in (on, off, same))
    assert "exports" not in K and set(J) - {"exports"} == set(K)
    assert open(same + "_30.ply", "rb").read() == open(on + "_30.ply", "rb").read()
    assert {k: v for k, v in J.items() if k != "exports"} == K2              # digit for digit: the same parameters without the flag
    assert sorted(os.listdir(os.path.dirname(off))) == ["iteration_30.ply", "iteration_30_eval.json"]
    assert "export" not in q.stderr and "export" not in q.stdout and "reduced" not in q.stderr and "cullSH" not in q.stderr      # (no path says so)


def test_without_cullsh_every_splat_keeps_the_model_degree(gpu_device, tmp_path):
    out = str(tmp_path / "iteration")
    p = _run(["--outputPath", out, "--exportFormat", "reduced", "--cullSH", "0", "--reducedHalf", "1"])
    counts, half, _ = R.parse(open(out + "_30.reduced.ply", "rb").read())
    assert list(counts) == [0, 0, 2000, 0] and half
    assert os.path.getsize(out + "_30.reduced.ply") == len(R.header(counts, True)) + 2000 * R.stride(2, True) + 20480
    assert re.search(LINE, p.stderr) and "half-float positions" in p.stderr


def test_model_path_suffix_turns_the_export_on(gpu_device, tmp_path):
    out = str(tmp_path / "scene.reduced.ply")
    p = _run(["--outputPath", out])
    assert os.path.exists(out + "_30.ply") and os.path.exists(out + "_30.reduced.ply")
    assert "turned on by the suffix of modelPath" in p.stderr and "config: exportFormats 8" in p.stderr
    counts, _, _ = R.parse(open(out + "_30.reduced.ply", "rb").read())
    assert sum(counts) == 2000
