"""Mesh decimation end to end through gaussian_train, in the manner of tests/test_gpu_mesh_clean_pipeline.py: the same small synthetic
scene at --meshResolution 32 (a scene the trainer repeats from run to run, see there), once plain, once with --meshDecimate 2
--meshNormals 1 and once with DVS_MESH_DECIMATE=0. The second file's positions, colours and faces must equal
tests/mesh_decimate_ref.py applied to the FIRST file on the lattice the log line's own %.9g fields give (origin = lower bound - voxel / 2,
cell = 2 voxels), exactly; positions, colours and faces do not depend on the normals, which the plain file does not hold, so the second
file's normals are checked for what they must be: unit length or zero."""
import os
import re
import subprocess
import numpy as np
import pytest
import mesh_ref as MR
import mesh_clean_ref as CR
import mesh_decimate_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
BOUNDS = {"DVS_MESH_BOUNDS": "-3,-2.5,2,3,2.5,8"}          # around the synthetic scene's splats (test_gpu_mesh_pipeline.py)
FACTOR = 2


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
    return {"plain": go([], {}), "decimated": go(["--meshDecimate", str(FACTOR), "--meshNormals", "1"], {}),
            "zero": go([], {"DVS_MESH_DECIMATE": "0"})}


def test_decimated_file_is_the_reference_applied_to_the_plain_file(runs):
    (plain, plain_log), (dec, log) = runs["plain"], runs["decimated"]
    xyz0, rgb0, tri0 = MR.parse_mesh_ply(plain)              # (the old parser: no normals in the plain file)
    assert len(xyz0) > 0 and len(tri0) > 0
    xyz, rgb, tri, nrm = CR.parse_mesh_ply(dec)
    assert nrm is not None and nrm.shape == xyz.shape
    m = re.search(r"mesh @20: (\d+) vertices, (\d+) triangles, grid (\d+)x(\d+)x(\d+), voxel ([^,]+), bounds ([^,]+),([^,]+),([^,]+),.*extraction [0-9.]+ ms, "
                  r"normals [0-9.]+ ms, decimate: (\d+) voxels per cell, (\d+) -> (\d+) vertices, (\d+) -> (\d+) triangles \((\d+) degenerate, "
                  r"(\d+) duplicate\), [0-9.]+ ms -> ", log)
    assert m, log[-3000:]
    dims = [int(m.group(k)) for k in (3, 4, 5)]
    voxel = np.float32(m.group(6))                           # %.9g: the float32 itself
    lo = [np.float32(m.group(k)) for k in (7, 8, 9)]
    origin, cell, ncell = DR.lattice(lo, voxel, dims, FACTOR)
    rxyz, rrgb, rtri, _, info = DR.decimate(xyz0, rgb0, tri0, origin, cell, ncell)
    print(f"plain {len(xyz0)} vertices / {len(tri0)} triangles; lattice {ncell} cells of {cell} from {origin}; {info}")
    assert 0 < info["out_triangles"] < len(tri0) and info["n_bad"] == 0
    assert xyz.tobytes() == rxyz.tobytes() and rgb.tobytes() == rrgb.tobytes() and tri.tobytes() == rtri.tobytes()
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert ((np.abs(length - 1) <= 1e-5) | (length == 0)).all()
    assert [int(m.group(k)) for k in (1, 2, 10, 11, 12, 13, 14, 15, 16)] == [
        info["out_vertices"], info["out_triangles"], FACTOR, len(xyz0), info["out_vertices"], len(tri0), info["out_triangles"], info["n_degenerate"],
        info["n_duplicate"]]
    assert re.search(r"config: mesh decimation: vertex clustering on cells of 2 voxels", log), log[-3000:]
    assert "decimate" not in plain_log and "config: mesh decimation" not in plain_log


def test_the_variable_at_zero_is_the_plain_file(runs):
    assert open(runs["plain"][0], "rb").read() == open(runs["zero"][0], "rb").read()
    assert "decimate" not in runs["zero"][1] and "config: mesh decimation" not in runs["zero"][1]
