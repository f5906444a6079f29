"""The export frame's two remaining doors: the class methods a linked host calls (setExportTransform, setExportOrientation,
clearExportTransform; tests/hosts/export_frame_host.cpp) and the mesh, which dvs_transform_points moves into the same frame."""
import os
import re
import subprocess
import numpy as np
import pytest
import transform_ref as T
from mesh_clean_ref import parse_mesh_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
TRS = "0.5,-1,2,0.3,-0.7,1.1,2.5"


def _sim():
    from divshot_amd import transform as X
    v = [float(x) for x in TRS.split(",")]
    return X.similarity_from_trs(v[0:3], v[3:6], v[6])


def test_class_methods_set_replace_and_clear_the_frame(gpu_device, tmp_path):
    from divshot_amd import transform as X
    import divshot_amd as dv
    from divshot_amd._lib import read_ply
    exe = str(tmp_path / "export_frame_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hosts", "export_frame_host.cpp"),
                           "-o", exe, "-L", LIB, "-lgstrain", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    d = tmp_path / "m"
    d.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("DVS_EXPORT_FORMATS", "DVS_EXPORT_TRANSFORM", "DVS_EXPORT_ORIENT")}
    p = subprocess.run([exe, "synthetic:N=2000,W=20,H=12,cams=8,sh=2", str(d), "10"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "early 0 set 1 orient 1 bad_scale 0 bad_axis 0 iterations 10 cameras 8" in p.stdout, p.stdout
    assert sorted(os.listdir(d)) == ["a_10.ply", "a_10.transformed.ply", "b_10.ply", "b_10.transformed.ply", "c_10.ply"]
    raw = [open(d / f"{k}_10.ply", "rb").read() for k in "abc"]
    assert raw[0] == raw[1] == raw[2]                                           # the training frame never moves
    model, a, b = read_ply(str(d / "a_10.ply")), read_ply(str(d / "a_10.transformed.ply")), read_ply(str(d / "b_10.transformed.ply"))
    assert np.abs(model["shN"][:, :24]).max() > 0                               # (progressiveTrain off: the bands carry values)
    sim = _sim()
    want = T.transform_splats(sim.R, sim.t, sim.s, X.sh_rotation(sim.R), model["pos"], model["shN"], model["scale"], model["rot"], 2)
    for k in ("pos", "shN", "scale", "rot"):
        assert np.array_equal(a[k].view(np.uint32), want[k].reshape(a[k].shape).view(np.uint32)), k
    assert not np.array_equal(a["shN"], model["shN"])
    # b: the +y frame (the refused calls after it changed nothing): the scene's mean camera-up goes onto +y
    spec = dv.make_spec(2000, 20, 12, sh_degree=2, n_cams=8)
    cams = [dv.synth_camera(spec, i) for i in range(8)]
    up = -np.array([[c.view[1], c.view[5], c.view[9]] for c in cams], np.float64).mean(axis=0)
    up /= np.linalg.norm(up)
    A = np.concatenate([model["pos"].astype(np.float64), np.ones((2000, 1))], axis=1)
    M = np.linalg.lstsq(A, b["pos"].astype(np.float64), rcond=None)[0]
    R = M[:3].T
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and np.abs(R @ up - np.array([0.0, 1.0, 0.0])).max() <= 1e-5
    assert np.array_equal(b["scale"], model["scale"])                           # s = 1
    for word in ("setExportOrientation before loadTrainData", "from setExportTransform(", "from setExportOrientation +y", "setExportTransform: position"):
        assert word in p.stderr, word


@pytest.fixture(scope="module")
def mesh_runs(tmp_path_factory):
    """one training run, then two runs that resume from its PLY and extract the mesh at once (export_mesh), with and without the
    transform: the same parameters, so the two meshes differ by the frame alone"""
    base = tmp_path_factory.mktemp("meshframe")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DVS_MESH_", "DVS_EXPORT_"))}
    env["DVS_MESH_BOUNDS"] = "-3,-2.5,2,3,2.5,8"                                 # around the synthetic splats: the default box is empty there
    scene = ["--inputPath", "synthetic:N=20000,W=256,H=192,cams=8,sh=1,seed=9", "--maxIteration", "60"]

    def go(args):
        p = subprocess.run([DRIVER] + scene + args, capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        return p.stderr

    out = str(base / "iteration")
    go(["--outputPath", out])
    mesh = ["--outputPath", out, "--load_itr", "60", "--meshResolution", "32", "--meshNormals", "1", "--exportMesh", "1"]
    go(mesh)
    plain = parse_mesh_ply(out + "_60_mesh.ply")
    log = go(mesh + ["--exportTransform", TRS])
    return plain, parse_mesh_ply(out + "_60_mesh.ply"), log


def test_mesh_shares_the_frame(gpu_device, mesh_runs):
    (xyz, rgb, tri, nrm), (xyz2, rgb2, tri2, nrm2), log = mesh_runs
    assert len(xyz) > 0 and len(tri) > 0 and nrm is not None and nrm2 is not None
    assert np.array_equal(tri, tri2) and np.array_equal(rgb, rgb2)
    sim = _sim()
    want_x, want_n = T.transform_points(sim.R, sim.t, sim.s, xyz, nrm)
    assert np.array_equal(xyz2.view(np.uint32), want_x.view(np.uint32))
    assert np.array_equal(nrm2.view(np.uint32), want_n.view(np.uint32))
    assert re.search(r"mesh @60: .*in the training frame: the vertices and normals are written in the export frame", log)
