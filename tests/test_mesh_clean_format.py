"""The mesh clean-up's entry points without a GPU: the CLI lists --meshMinComponent / --meshNormals and refuses bad values, the mesh
writer's optional normals round-trip and leave the plain file's bytes alone, GaussianTrainConfig keeps its size and offsets (the
settings travel as environment variables and through setMeshCleanup, not in the struct), the libraries export the new symbols."""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np
import divshot_amd as dv
from divshot_amd import _lib
import mesh_ref as MR
import mesh_clean_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.25, -2]], np.float32)
NRM = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0, 0], [-1, 0, 0]], np.float32)
RGB = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [7, 8, 9]], np.uint8)
TRI = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)


def test_cli_lists_the_flags_and_refuses_bad_values(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--meshMinComponent [0]" in out and "--meshNormals [0]" in out, out
    for value in ("101", "-1", "abc", "1.234", ""):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), "--meshMinComponent", value],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "Command Line Error: --meshMinComponent takes" in p.stdout, (value, p.stdout)
    for value in ("2", "yes", ""):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), "--meshNormals", value],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "Command Line Error: --meshNormals takes" in p.stdout, (value, p.stdout)


def test_normals_round_trip(tmp_path):
    path = str(tmp_path / "n.ply")
    _lib.write_mesh_ply(path, XYZ, RGB, TRI, normals=NRM)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    props = [h.split()[-1] for h in head if h.startswith("property")]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "vertex_indices"]
    xyz, rgb, tri, nrm = CR.parse_mesh_ply(path)
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, RGB) and np.array_equal(tri, TRI) and nrm.tobytes() == NRM.tobytes()
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 4 * 27 + 2 * 13
    empty = str(tmp_path / "e.ply")
    z = np.zeros((0, 3))
    _lib.write_mesh_ply(empty, z, z, z, normals=z)
    xyz, rgb, tri, nrm = CR.parse_mesh_ply(empty)
    assert xyz.shape == tri.shape == nrm.shape == (0, 3)


def test_without_normals_the_bytes_are_what_they_were(tmp_path):
    path = str(tmp_path / "p.ply")
    _lib.write_mesh_ply(path, XYZ, RGB, TRI)
    assert open(path, "rb").read() == MR.build_mesh_ply(XYZ, RGB, TRI)
    again = str(tmp_path / "q.ply")
    _lib.write_mesh_ply(again, XYZ, RGB, TRI, normals=None)
    assert open(again, "rb").read() == MR.build_mesh_ply(XYZ, RGB, TRI)
    xyz, rgb, tri, nrm = CR.parse_mesh_ply(path)
    assert nrm is None and np.array_equal(xyz, XYZ) and np.array_equal(tri, TRI)


def test_config_struct_is_unchanged():
    """what tests/test_importance_abi.py prints, with the values of the commit before the clean-up: no field was added; the class still
    holds one pointer behind its public fields (setMeshCleanup's state lives in the implementation)"""
    prog = r'''
#include <cstdio>
#include <cstddef>
#include "gaussian_trainer_scene.hpp"
int main() {
  GaussianTrainConfig c;
  std::printf("%zu %zu %zu %zu %zu %d %zu\n", sizeof(GaussianTrainConfig), alignof(GaussianTrainConfig), offsetof(GaussianTrainConfig, exportFormats),
              offsetof(GaussianTrainConfig, renderSampling), offsetof(GaussianTrainConfig, importancePrune), (int)c.importancePrune,
              sizeof(GaussianTrainerScene));
  void (GaussianTrainerScene::*f)(float, bool) = &GaussianTrainerScene::setMeshCleanup;
  return f ? 0 : 1; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        lib = os.path.join(ROOT, "divshot_amd", "lib")
        subprocess.check_call(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", lib, "-lgstrain",
                               "-Wl,-rpath," + lib, "-Wl,-rpath-link," + lib])
        values = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert values == [312, 8, 304, 310, 311, 0, 80], values


def test_symbols_are_exported_and_bound():
    for name in ("dvs_mesh_components", "dvs_mesh_clean_scratch_bytes", "dvs_mesh_clean_count", "dvs_mesh_clean_write", "dvs_mesh_extract_normals"):
        assert hasattr(dv.lib, name) and name in _lib._MESH_PROTOS, name
    h = _lib.host_lib()
    assert hasattr(h, "gstrain_write_mesh_ply") and hasattr(h, "gstrain_write_mesh_ply_normals")
    assert _lib._MESH_HOST_PROTOS["gstrain_write_mesh_ply"][1] == [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64]
    assert C.sizeof(_lib.MeshCleanInfo) == 24
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "divshot_amd", "lib", "libgstrain.so")]).decode()
    assert "GaussianTrainerScene::setMeshCleanup(float, bool)" in out


def test_bad_arguments_are_refused_before_a_device_is_touched():
    info = _lib.MeshCleanInfo()
    assert dv.lib.dvs_mesh_clean_count(None, 4, 256, 2, 10001, 512, C.byref(info)) == 1          # min_bp above 10000
    assert dv.lib.dvs_mesh_clean_count(None, 4, 256, 2, 100, None, C.byref(info)) == 1            # no scratch
    assert dv.lib.dvs_mesh_clean_count(None, 4, 256, 2, 100, 520, C.byref(info)) == 1             # misaligned scratch
    assert dv.lib.dvs_mesh_clean_count(None, 4, 256, 2, 100, 512, None) == 1                      # no info
    assert dv.lib.dvs_mesh_components(None, 4, None, 2, 256, None) == 1 and dv.lib.dvs_mesh_components(None, 4, 256, 2, None, None) == 1
    assert dv.lib.dvs_mesh_clean_write(None, 4, 256, 256, 256, 256, 2, 512, 256, 256, None, 256) == 1      # normals without out_normals
    assert dv.lib.dvs_mesh_extract_normals(None, None, 512, 256) == 1
    sizes = [dv.lib.dvs_mesh_clean_scratch_bytes(v, t) for v, t in ((0, 0), (1, 1), (1000, 2000), (5_000_000, 10_000_000))]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 256 == 0 for s in sizes)
    assert sizes[3] >= 12 * 5_000_000 + 4 * 10_000_000
