"""Mesh decimation without a GPU: the CLI lists --meshDecimate and refuses bad values, the library exports and binds the three entry
points, GaussianTrainConfig and GaussianTrainerScene keep their sizes (the setting travels as DVS_MESH_DECIMATE and through
setMeshDecimate, not in the struct), invalid arguments are refused before a device is touched — and the reference itself
(tests/mesh_decimate_ref.py) on an analytic sphere: what vertex clustering must and must not do to a closed surface."""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import _lib
import mesh_ref as MR
import mesh_decimate_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
NAMES = ("dvs_mesh_decimate_scratch_bytes", "dvs_mesh_decimate_count", "dvs_mesh_decimate_write")


def test_cli_lists_the_flag_and_refuses_bad_values(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--meshDecimate [0]" in out, out
    for value in ("1", "17", "-2", "abc", "2.5", ""):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), "--meshDecimate", value],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (value, p.stdout)
        assert f"Command Line Error: --meshDecimate takes 0 (off) or an integer 2..16, not '{value}'" in p.stdout, (value, p.stdout)


def test_symbols_are_exported_and_bound():
    for name in NAMES:
        assert hasattr(dv.lib, name) and name in _lib._MESH_PROTOS, name
    assert C.sizeof(_lib.MeshDecimateInfo) == 24
    assert [n for n, _ in _lib.MeshDecimateInfo._fields_] == ["out_vertices", "out_triangles", "n_clusters", "n_degenerate", "n_duplicate", "n_bad"]
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "divshot_amd", "lib", "libgstrain.so")]).decode()
    assert "GaussianTrainerScene::setMeshDecimate(int)" in out


def test_config_struct_is_unchanged():
    """the program of tests/test_mesh_clean_format.py with its values: no field was added, the class still holds one pointer behind
    its public fields (setMeshDecimate's state lives in the implementation)"""
    prog = r'''
#include <cstdio>
#include <cstddef>
#include "gaussian_trainer_scene.hpp"
int main() {
  GaussianTrainConfig c;
  std::printf("%zu %zu %zu %zu %zu %d %zu\n", sizeof(GaussianTrainConfig), alignof(GaussianTrainConfig), offsetof(GaussianTrainConfig, exportFormats),
              offsetof(GaussianTrainConfig, renderSampling), offsetof(GaussianTrainConfig, importancePrune), (int)c.importancePrune,
              sizeof(GaussianTrainerScene));
  void (GaussianTrainerScene::*f)(int) = &GaussianTrainerScene::setMeshDecimate;
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


def test_bad_arguments_are_refused_before_a_device_is_touched():
    info = _lib.MeshDecimateInfo()
    origin = (C.c_float * 3)(0, 0, 0)
    good = (C.c_int32 * 3)(4, 4, 4)
    count = dv.lib.dvs_mesh_decimate_count

    def call(scratch=512, origin_=origin, cell=0.5, ncell=good, info_=C.byref(info)):
        return count(None, 4, 256, 256, 2, origin_, cell, ncell, scratch, info_)
    assert call(scratch=None) == 1                                  # no scratch
    assert call(scratch=520) == 1                                   # misaligned scratch
    assert call(info_=None) == 1 and call(origin_=None) == 1 and call(ncell=None) == 1
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert call(cell=cell) == 1, cell
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert call(ncell=(C.c_int32 * 3)(*bad)) == 1, bad
    write = dv.lib.dvs_mesh_decimate_write
    assert write(None, 4, 256, 256, 256, 256, 2, 512, 256, 256, None, 256) == 1      # normals without out_normals
    assert write(None, 4, 256, 256, None, 256, 2, 512, 256, 256, 256, 256) == 1      # out_normals without normals
    assert write(None, 4, 256, 256, None, 256, 2, None, 256, 256, None, 256) == 1    # no scratch
    assert write(None, 4, 256, 256, None, 256, 2, 520, 256, 256, None, 256) == 1     # misaligned scratch
    sizes = [dv.lib.dvs_mesh_decimate_scratch_bytes(v, t) for v, t in ((0, 0), (1, 1), (1000, 2000), (5_000_000, 10_000_000))]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 256 == 0 for s in sizes)
    assert dv.lib.dvs_mesh_decimate_scratch_bytes(1000, 3000) >= sizes[2] and dv.lib.dvs_mesh_decimate_scratch_bytes(2000, 2000) >= sizes[2]


# ---- the reference on an analytic sphere ----------------------------------------------------------------------------------------------
# A 40^3 grid holding the exact signed distance (in voxels) of a sphere of radius 15 voxels about a generic centre, extracted by
# tests/mesh_ref.py's marching tetrahedra: 12690 vertices, 25376 triangles. The lattice is the plugin's (half a voxel before the grid).
N, RADIUS, CENTRE = 40, 15.0, np.array([19.3, 20.2, 19.1])
ORIGIN, VOXEL = (-2.5, -2.5, -2.5), 0.125


@pytest.fixture(scope="module")
def sphere():
    k, j, i = np.mgrid[0:N, 0:N, 0:N]
    tsdf = (np.sqrt((i - CENTRE[0]) ** 2 + (j - CENTRE[1]) ** 2 + (k - CENTRE[2]) ** 2) - RADIUS).astype(np.float32)
    rgb = np.stack([i / N, j / N, k / N], -1).astype(np.float32)
    xyz, col, tri = MR.marching_tets(tsdf, np.ones_like(tsdf), rgb, ORIGIN, VOXEL)
    return xyz.astype(np.float32), col, tri


@pytest.mark.parametrize("factor", [2, 3])
def test_reference_on_the_sphere(sphere, factor):
    xyz0, rgb0, tri0 = sphere
    origin, cell, ncell = DR.lattice(ORIGIN, VOXEL, (N, N, N), factor)
    xyz, rgb, tri, nrm, info = DR.decimate(xyz0, rgb0, tri0, origin, cell, ncell)
    assert nrm is None and info["n_bad"] == 0
    assert len(xyz) == info["out_vertices"] == len(rgb) and len(tri) == info["out_triangles"]
    # every output vertex lies inside its cell (it is a mean of points of that cell), up to 1e-5 of the cell size. Its cell: output o
    # stands for the o-th, in key order, of the cells that a triangle with three different cells touches
    members = DR.cell_keys(xyz0, origin, cell, ncell)
    own = np.unique(members)                                         # (ascending)
    assert len(own) == info["n_clusters"]
    corner = np.searchsorted(own, members)[tri0]
    alive = (corner[:, 0] != corner[:, 1]) & (corner[:, 1] != corner[:, 2]) & (corner[:, 0] != corner[:, 2])
    stand_for = own[np.unique(corner[alive])]
    assert len(stand_for) == len(xyz)
    cell_ijk = np.stack([stand_for % ncell[0], (stand_for // ncell[0]) % ncell[1], stand_for // (ncell[0] * ncell[1])], -1)
    q = (xyz.astype(np.float64) - origin.astype(np.float64)) / float(cell)
    assert (q >= cell_ijk - 1e-5).all() and (q <= cell_ijk + 1 + 1e-5).all()
    # no output triangle is degenerate or repeated (as a rotation class), and the count falls
    t = tri.astype(np.int64)
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
    canon = {DR.rotate_min_first(*row) for row in t.tolist()}
    assert len(canon) == len(t)
    assert 0 < len(t) < len(tri0) and len(xyz) < len(xyz0)
    assert len(tri0) == len(t) + info["n_degenerate"] + info["n_duplicate"]
    # orientation: the share of output triangles whose normal points towards the sphere's centre
    p = xyz.astype(np.float64) - (np.array(ORIGIN) + CENTRE * VOXEL)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    inward = ((np.cross(b - a, c - a) * (a + b + c)).sum(1) < 0).mean()
    print(f"F={factor}: {len(xyz0)} -> {len(xyz)} vertices, {len(tri0)} -> {len(t)} triangles, {info}, inward share {inward:.5f}")
    assert inward <= 0.01
