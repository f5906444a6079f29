"""The focus region without a GPU: dvs_region_from_trs against tests/region_ref.py, every refusal of the three entry points (they come
before anything touches a device), the exported symbols of both libraries, the CLI's flags, and the size of GaussianTrainConfig, which
the feature must not change. The reference itself is pinned too: the seeds the GPU tests use leave at most 1 % of their random centres
within the comparison band of a face."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import _lib, region
import region_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
PLUGIN, DRIVER = os.path.join(LIB, "libgstrain.so"), os.path.join(LIB, "gaussian_train")
INVALID = 1
# host-side double -> float conversions: the 1e-6 tests/test_sky_ref.py holds the host's fp64 -> fp32 ray matrix to (the rounding itself is 6e-8)
TOL = 1e-6

CASES = {
    "identity": ((0, 0, 0), (0, 0, 0), (1, 1, 1)),
    "translation": ((0.5, -2.0, 3.25), (0, 0, 0), (1, 1, 1)),
    "rot_x": ((0, 0, 0), (0.7, 0, 0), (1, 1, 1)),
    "rot_y": ((0, 0, 0), (0, -1.1, 0), (1, 1, 1)),
    "rot_z": ((0, 0, 0), (0, 0, 2.3), (1, 1, 1)),
    "scale": ((0, 0, 0), (0, 0, 0), (2.0, 0.5, -3.0)),
    "all": ((0.3, -0.2, 1.5), (0.4, -0.9, 1.7), (1.5, 0.75, 2.0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_from_trs_equals_the_reference(name):
    pos, rot, scale = CASES[name]
    lo, hi = (-1.0, -2.0, -0.5), (1.0, 0.25, 4.0)
    reg, b2w = region.region_from_trs(pos, rot, scale, lo, hi)
    w2b_ref, F_ref = RR.from_trs(pos, rot, scale)
    w2b = np.array(list(reg.w2b), np.float64).reshape(3, 4)
    assert np.abs(w2b - w2b_ref).max() <= TOL * max(1.0, np.abs(w2b_ref).max()), (w2b, w2b_ref)
    assert np.abs(b2w.astype(np.float64) - F_ref).max() <= TOL * max(1.0, np.abs(F_ref).max())
    assert list(reg.lo) == list(lo) and list(reg.hi) == list(hi)
    if name == "identity":
        assert np.array_equal(w2b, np.eye(4)[:3]) and np.array_equal(b2w, np.eye(4, dtype=np.float32))
    if name == "rot_z":                                  # the sense of the rotation: F turns +x towards +y for a positive angle about z
        assert b2w[1, 0] > 0 and abs(b2w[1, 0] - np.sin(2.3)) < 1e-6
    if name == "rot_x":
        assert b2w[2, 1] > 0
    if name == "rot_y":
        assert b2w[0, 2] < 0                             # angle -1.1: +z goes towards -x


def test_from_trs_refuses():
    f = dv.lib.dvs_region_from_trs
    ok = dict(pos=(0, 0, 0), rot=(0, 0, 0), scale=(1, 1, 1), lo=(0, 0, 0), hi=(1, 1, 1))

    def call(out=True, b2w=True, null=None, **kw):
        a = {k: np.array(v, np.float32) for k, v in dict(ok, **kw).items()}
        reg, m = _lib.Region(), np.zeros(16, np.float32)
        ptr = {k: (None if k == null else v.ctypes.data) for k, v in a.items()}
        return f(ptr["pos"], ptr["rot"], ptr["scale"], ptr["lo"], ptr["hi"], C.byref(reg) if out else None, m.ctypes.data if b2w else None)
    assert call() == 0
    for k in range(3):
        for bad in (0.0, -0.0, np.nan, np.inf):
            s = [1.0, 1.0, 1.0]; s[k] = bad
            assert call(scale=s) == INVALID, (k, bad)
        lo = [0.0, 0.0, 0.0]; lo[k] = 1.5
        assert call(lo=lo) == INVALID                    # lo > hi
        for name in ("pos", "rot", "lo", "hi"):
            v = list(ok[name]); v[k] = np.nan
            assert call(**{name: v}) == INVALID, (name, k)
    for name in ok:
        assert call(null=name) == INVALID, name
    assert call(out=False) == INVALID and call(b2w=False) == INVALID
    assert call(lo=(1, 1, 1)) == 0                       # lo == hi: a degenerate box is a box


def test_plan_and_mask_refuse_bad_arguments():
    reg, _ = region.region_from_trs((0, 0, 0), (0, 0, 0), (1, 1, 1), (0, 0, 0), (1, 1, 1))
    f = dv.lib.dvs_region_plan
    ok = dict(n=8, pos=256, region=C.byref(reg), action=512, offsets=768, scratch=1024, new_count=2048)

    def plan(**kw):
        a = dict(ok, **kw)
        return f(None, a["n"], a["pos"], a["region"], a["action"], a["offsets"], a["scratch"], a["new_count"])
    assert plan(n=0) == INVALID and plan(n=-5) == INVALID
    for name in ("pos", "region", "action", "offsets", "scratch", "new_count"):
        assert plan(**{name: None}) == INVALID, name
    assert plan(new_count=2052) == INVALID               # misaligned
    g = dv.lib.dvs_region_mask_views
    views = (_lib.RegionMaskView * 17)()
    spec = dv.make_spec(10, 16, 16, sh_degree=0, n_cams=1)
    for v in views:
        v.cam = dv.synth_camera(spec, 0); v.out = 4096
    assert g(None, None, 1, 16, 16, C.byref(reg)) == INVALID
    assert g(None, views, 1, 16, 16, None) == INVALID
    assert g(None, views, 0, 16, 16, C.byref(reg)) == INVALID and g(None, views, 17, 16, 16, C.byref(reg)) == INVALID
    assert g(None, views, 1, 0, 16, C.byref(reg)) == INVALID and g(None, views, 1, 16, -1, C.byref(reg)) == INVALID
    assert g(None, views, 1, 32, 16, C.byref(reg)) == INVALID            # not the cameras' size
    views[0].out = None
    assert g(None, views, 1, 16, 16, C.byref(reg)) == INVALID


def test_symbols_are_exported_and_bound():
    for name in ("dvs_region_from_trs", "dvs_region_plan", "dvs_region_mask_views"):
        assert hasattr(dv.lib, name) and name in _lib._REGION_PROTOS, name
    out = subprocess.check_output(["nm", "-DC", "--defined-only", PLUGIN]).decode()
    for member in ("GaussianTrainerScene::getFocusRegion() const", "GaussianTrainerScene::getFocusRegionTransform() const"):
        assert any(line.split(None, 2)[1] in "TW" and line.split(None, 2)[2] == member for line in out.splitlines() if len(line.split(None, 2)) == 3), member


def test_ctypes_mirrors_have_the_c_layout(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dvs_region.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dvs_region), offsetof(dvs_region, lo), offsetof(dvs_region, hi), sizeof(dvs_region_mask_view),
         offsetof(dvs_region_mask_view, in_mask), offsetof(dvs_region_mask_view, out));
  return 0; }'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got == [C.sizeof(_lib.Region), _lib.Region.lo.offset, _lib.Region.hi.offset, C.sizeof(_lib.RegionMaskView),
                   _lib.RegionMaskView.in_mask.offset, _lib.RegionMaskView.out.offset]


def test_config_struct_keeps_its_size_and_the_header_declares_the_getters(tmp_path):
    """sizeof(GaussianTrainConfig) is what the tail-padding rule of tests/test_importance_abi.py says, enableFocusRegion still sits between
    enableBg and cullSH, and a host can call both getters with the editor's structured binding"""
    prog = r'''
#include <cstdio>
#include <cstddef>
#include "gaussian_trainer_scene.hpp"
int use(const GaussianTrainerScene& s) { auto [a, b] = s.getFocusRegion(); auto m = s.getFocusRegionTransform(); return (int)(a.x + b.x) + (int)sizeof m; }
int main() {
  std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(GaussianTrainConfig), alignof(GaussianTrainConfig), offsetof(GaussianTrainConfig, exportFormats),
              offsetof(GaussianTrainConfig, enableBg), offsetof(GaussianTrainConfig, enableFocusRegion), offsetof(GaussianTrainConfig, cullSH));
  return 0; }'''
    src, exe = str(tmp_path / "t.cpp"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", LIB, "-lgstrain",
                           "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    size, align, off_formats, off_bg, off_focus, off_cull = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert size == (off_formats + 4 + align - 1) // align * align
    assert off_focus == off_bg + 1 and off_cull == off_focus + 1


def test_cli_lists_the_flags_and_refuses_bad_values(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    for flag in ("--enableFocusRegion [0]", "--focusRegion []", "--focusRotation []"):
        assert flag in out, (flag, out)
    base = [DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x")]
    for flag, values in (("--enableFocusRegion", ("2", "yes", "")), ("--focusRegion", ("1,2,3", "0,0,0,1,1", "0,0,0,1,1,0", "0,0,0,1,1,1,2", "a,b,c,d,e,f")),
                         ("--focusRotation", ("1,2", "1,2,3,4", "x,y,z"))):
        for value in values:
            p = subprocess.run(base + [flag, value], capture_output=True, text=True, timeout=60)
            assert p.returncode == 1 and flag + " takes" in p.stdout, (flag, value, p.stdout)


# ---- what the GPU tests rely on, shown on the reference alone -------------------------------------------------------------------------
ROTATED = dict(pos=(0.25, -0.5, 0.125), rot=(0.4, -0.9, 1.7), scale=(1.5, 0.75, 2.0), lo=(-1.0, -1.5, -0.6), hi=(1.0, 2.0, 0.7), seed=7, n=70001, band=1e-5)


def rotated_points():
    return np.random.default_rng(ROTATED["seed"]).uniform(-2.0, 2.0, (ROTATED["n"], 3)).astype(np.float32)


def test_the_rotated_case_leaves_few_centres_near_a_face():
    reg, _ = region.region_from_trs(ROTATED["pos"], ROTATED["rot"], ROTATED["scale"], ROTATED["lo"], ROTATED["hi"])
    action, _, count, near = RR.plan(rotated_points(), list(reg.w2b), ROTATED["lo"], ROTATED["hi"], ROTATED["band"])
    assert near.mean() <= 0.01, near.mean()
    assert 0.05 * ROTATED["n"] < count < 0.95 * ROTATED["n"], count     # the box cuts through the cloud
