"""Mesh clean-up end to end through gaussian_train, in the manner of tests/test_gpu_mesh_pipeline.py: the same small synthetic scene
at --meshResolution 32, once plain and once with --meshMinComponent 5 --meshNormals 1; the second file's positions, colours and faces
must equal tests/mesh_clean_ref.py applied to the FIRST file, exactly, and a run with both settings explicitly 0 must write the plain
run's bytes. Both compare two trainings, so the scene is one the trainer repeats on from run to run: views of 32x16 = 2 x 1 tiles, where
a gradient row receives at most two fp32 atomic addends and their order cannot matter (tests/test_gpu_dataset_jpeg.py explains and
measures this); 20 steps, before any refinement. The mesh of such views is coarse, which does not matter here."""
import os
import re
import subprocess
import numpy as np
import pytest
import mesh_ref as MR
import mesh_clean_ref as CR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
BOUNDS = {"DVS_MESH_BOUNDS": "-3,-2.5,2,3,2.5,8"}          # around the synthetic scene's splats (test_gpu_mesh_pipeline.py)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, gpu_device):
    def go(extra, env_extra):
        out = str(tmp_path_factory.mktemp("out") / "iteration")
        env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_MESH_")}
        env.update(BOUNDS)
        env.update(env_extra)
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=20000,W=32,H=16,cams=8,sh=1,seed=9", "--maxIteration", "20", "--outputPath", out,
                            "--meshResolution", "32"] + extra, capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        path = out + "_20_mesh.ply"
        assert os.path.exists(path), p.stderr[-3000:]
        return path, p.stderr
    return {"plain": go([], {}), "clean": go(["--meshMinComponent", "5", "--meshNormals", "1"], {}),
            "zeros": go([], {"DVS_MESH_MIN_COMPONENT": "0", "DVS_MESH_NORMALS": "0"})}


def test_cleaned_file_is_the_reference_applied_to_the_plain_file(runs):
    (plain, plain_log), (clean, log) = runs["plain"], runs["clean"]
    xyz0, rgb0, tri0 = MR.parse_mesh_ply(plain)              # (the old parser: no normals in the plain file)
    assert len(xyz0) > 0 and len(tri0) > 0
    xyz, rgb, tri, nrm = CR.parse_mesh_ply(clean)
    assert nrm is not None and nrm.shape == xyz.shape
    rxyz, rrgb, rtri, _, info = CR.clean(xyz0, rgb0, tri0, 500)
    print(f"plain {len(xyz0)} vertices / {len(tri0)} triangles; {info}")
    assert xyz.tobytes() == rxyz.tobytes() and rgb.tobytes() == rrgb.tobytes() and tri.tobytes() == rtri.tobytes()
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert ((np.abs(length - 1) <= 1e-5) | (length == 0)).all()
    m = re.search(r"mesh @20: (\d+) vertices, (\d+) triangles, .*extraction [0-9.]+ ms, cleanup: (\d+) of (\d+) components kept \(largest (\d+) triangles, "
                  r"min 5 %\), [0-9.]+ ms, normals [0-9.]+ ms -> ", log)
    assert m, log[-3000:]
    assert [int(v) for v in m.groups()] == [info["kept_vertices"], info["kept_triangles"], info["kept_components"], info["n_components"], info["largest"]]
    assert re.search(r"config: mesh clean-up: components with fewer than 5 % .*vertex normals", log), log[-3000:]
    assert "cleanup:" not in plain_log and ", normals" not in plain_log and "config: mesh clean-up" not in plain_log


def test_both_settings_zero_is_the_plain_file(runs):
    assert open(runs["plain"][0], "rb").read() == open(runs["zeros"][0], "rb").read()
    assert "cleanup:" not in runs["zeros"][1] and "config: mesh clean-up" not in runs["zeros"][1]
