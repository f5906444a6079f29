"""Level-of-detail export without a GPU: the library exports and binds the entry points, dvs_lod_lattice_for gives a hand-computed
lattice and refuses what is not one, invalid arguments are refused before a device is touched, the setting travels beside the config
struct (setLodExport, DVS_EXPORT_LOD / DVS_LOD_RESOLUTION), and the CLI lists and checks its two flags."""
import ctypes as C
import os
import subprocess
import numpy as np
import divshot_amd as dv
from divshot_amd import _lib
from divshot_amd import lod as LOD
import lod_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
NAMES = ("dvs_lod_lattice_for", "dvs_lod_scratch_bytes", "dvs_lod_merge_count", "dvs_lod_merge_write")


def test_symbols_are_exported_and_bound():
    for name in NAMES:
        assert hasattr(dv.lib, name) and name in _lib._EXPORT_PROTOS, name
    assert C.sizeof(_lib.LodLattice) == 28 and [n for n, _ in _lib.LodLattice._fields_] == ["origin", "cell", "dims"]
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "divshot_amd", "lib", "libgstrain.so")]).decode()
    assert "GaussianTrainerScene::setLodExport(int, int)" in out


def test_lattice_for_a_hand_computed_box():
    """the box (1, -2, 0.5) .. (9, 2, 0.5) at resolution 8: the longest side is 8, so cell = fp32(8 (1 + 1e-5) / 8) = fp32(1.00001); the
    sides 8, 4, 0 take ceil(8 / 1.00001) = 8, ceil(4 / 1.00001) = 4 and max(1, 0) = 1 cells; the origin is the box's minimum"""
    g = LOD.lattice_for([1, -2, 0.5, 9, 2, 0.5], 8)
    assert list(g.origin) == [1.0, -2.0, 0.5] and list(g.dims) == [8, 4, 1]
    assert np.float32(g.cell) == np.float32(1.00001) and g.cell > 1.0
    # the box's maximum lands inside the last cell of every axis, its minimum in the first
    keys = L.cell_keys(np.array([[9, 2, 0.5], [1, -2, 0.5]], np.float32), list(g.origin), g.cell, list(g.dims))
    assert keys.tolist() == [(0 * 4 + 3) * 8 + 7, 0]
    o, c, d = L.lattice_for([1, -2, 0.5, 9, 2, 0.5], 8)                       # the restatement agrees
    assert o.tolist() == list(g.origin) and c == np.float32(g.cell) and d == list(g.dims)
    big = LOD.lattice_for([0, 0, 0, 1, 1, 1], 1024)
    assert list(big.dims) == [1024, 1024, 1024]


def test_lattice_for_refuses():
    good = np.array([0, 0, 0, 8, 4, 2], np.float32)
    g = _lib.LodLattice()
    f = dv.lib.dvs_lod_lattice_for
    assert f(good.ctypes.data, 8, C.byref(g)) == 0
    for res in (3, 1025, 0, -1):
        assert f(good.ctypes.data, res, C.byref(g)) == 1, res
    for bad in ([2, 2, 2, 2, 2, 2], [0, 0, 0, -1, 4, 2], [0, 0, 0, float("nan"), 4, 2], [0, float("-inf"), 0, 8, 4, 2], [0, 0, 0, 8, float("inf"), 2]):
        b = np.array(bad, np.float32)
        assert f(b.ctypes.data, 8, C.byref(g)) == 1, bad
    assert f(None, 8, C.byref(g)) == 1 and f(good.ctypes.data, 8, None) == 1


def test_bad_arguments_are_refused_before_a_device_is_touched():
    g = LOD.make_lattice([0, 0, 0], 1.0, [4, 4, 4])
    counts = (C.c_uint32 * 2)(7, 7)
    count, write = dv.lib.dvs_lod_merge_count, dv.lib.dvs_lod_merge_write

    def c(n=4, pos=256, opa=256, scale=256, rot=256, lat=g, scratch=512, cnt=counts):
        return count(None, n, pos, opa, scale, rot, C.byref(lat) if lat is not None else None, scratch, cnt)
    assert c(pos=None) == 1 and c(opa=None) == 1 and c(scale=None) == 1 and c(rot=None) == 1        # null
    assert c(pos=260) == 1 and c(rot=264) == 1                                                      # off a 16-byte boundary
    assert c(scratch=None) == 1 and c(scratch=528) == 1 and c(lat=None) == 1 and c(cnt=None) == 1 and c(n=-1) == 1
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert c(lat=LOD.make_lattice([0, 0, 0], cell, [4, 4, 4])) == 1, cell
    for dims in ([0, 4, 4], [4, 1025, 4], [4, 4, -1]):
        assert c(lat=LOD.make_lattice([0, 0, 0], 1.0, dims)) == 1, dims
    assert c(lat=LOD.make_lattice([0, float("nan"), 0], 1.0, [4, 4, 4])) == 1
    assert c(n=0, pos=None, opa=None, scale=None, rot=None) == 0 and list(counts) == [0, 0]        # n = 0: {0, 0}, nothing launched

    def w(n=4, D=3, ins=(256,) * 6, lin=0, scratch=512, outs=(256,) * 6, lout=0):
        return write(None, n, D, *ins, lin, scratch, *outs, lout)
    for k in range(6):
        assert w(ins=tuple(None if j == k else 256 for j in range(6))) == 1, k
        assert w(outs=tuple(None if j == k else 256 for j in range(6))) == 1, k
        assert w(ins=tuple(264 if j == k else 256 for j in range(6))) == 1, k
    assert w(D=-1) == 1 and w(D=4) == 1 and w(lin=2) == 1 and w(lout=-1) == 1 and w(scratch=None) == 1 and w(scratch=520) == 1 and w(n=-1) == 1
    assert w(n=0, ins=(None,) * 6, outs=(None,) * 6) == 0
    sizes = [dv.lib.dvs_lod_scratch_bytes(n) for n in (0, 1, 1000, 1_000_000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 256 == 0 for s in sizes)


def test_cli_lists_the_flags_and_refuses_bad_values(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--exportLod [0]" in out and "--lodResolution [256]" in out, out
    for flag, value, words in (("--exportLod", "5", "takes a number of levels 0 (off) .. 4, not '5'"), ("--exportLod", "-1", "takes a number of levels 0 (off) .. 4, not '-1'"),
                               ("--exportLod", "two", "takes a number of levels 0 (off) .. 4, not 'two'"), ("--lodResolution", "8", "takes a resolution 32..1024, not '8'"),
                               ("--lodResolution", "1025", "takes a resolution 32..1024, not '1025'"), ("--lodResolution", "", "takes a resolution 32..1024, not ''")):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), flag, value], capture_output=True, text=True,
                           timeout=60)
        assert p.returncode == 1, (flag, value, p.stdout)
        assert f"Command Line Error: {flag} {words}" in p.stdout, (flag, value, p.stdout)
    assert not list(tmp_path.iterdir())
