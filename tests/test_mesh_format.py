"""The mesh file writer (gsply::write_mesh_ply through the host-only library): binary little-endian PLY, x y z float + red green blue
uchar per vertex, `list uchar uint vertex_indices` per face. No GPU."""
import numpy as np
import pytest
from divshot_amd import _lib
import mesh_ref as MR

XYZ = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -2.25], [1, 1, 3e-3], [0.5, 0.5, 1e6]], np.float32)
RGB = np.array([[0, 1, 2], [255, 254, 253], [10, 128, 200], [7, 7, 7], [90, 0, 180]], np.uint8)
TRI = np.array([[0, 1, 2], [1, 3, 2], [0, 4, 1], [4, 3, 1]], np.uint32)


def test_round_trip_byte_for_byte(tmp_path):
    path = str(tmp_path / "m.ply")
    _lib.write_mesh_ply(path, XYZ, RGB, TRI)
    assert open(path, "rb").read() == MR.build_mesh_ply(XYZ, RGB, TRI)
    xyz, rgb, tri = MR.parse_mesh_ply(path)
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, RGB) and np.array_equal(tri, TRI)


def test_empty_mesh_is_a_valid_file(tmp_path):
    path = str(tmp_path / "e.ply")
    _lib.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint32))
    xyz, rgb, tri = MR.parse_mesh_ply(path)
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and tri.shape == (0, 3)
    assert open(path, "rb").read() == MR.build_mesh_ply(xyz, rgb, tri)


def test_index_out_of_range_is_refused_with_a_message(tmp_path):
    path = str(tmp_path / "bad.ply")
    bad = TRI.copy()
    bad[2, 1] = 5
    with pytest.raises(_lib.DvsError, match=r"triangle 2 has index 5 but there are 5 vertices"):
        _lib.write_mesh_ply(path, XYZ, RGB, bad)
    import os
    assert not os.path.exists(path)
