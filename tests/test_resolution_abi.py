"""The coarse-to-fine entry points without a GPU: dvs_downsample_view has the C layout (checked against gcc, as tests/test_metrics_abi.py
does), the CLI lists --resolutionSchedule / --numDownscales, dvs_camera_downscale equals its numpy restatement field by field, and the
geometric claim behind the level camera holds on the CPU oracle: a splat drawn at pixel x of the full image is drawn at
(x + 0.5) / d - 0.5 of the level image, at the same depth."""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np
import pytest
import divshot_amd as dv
from divshot_amd import _lib
from oracle.oracle import Oracle
from resolution_ref import level_of_step, clamp_levels, downsample_np, camera_downscale_np, camera_fields, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
INVALID = 1                                                  # DVS_ERR_INVALID


def test_downsample_view_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dvs_train.h"
int main(void) {
  printf("%zu %zu %zu %d\n", sizeof(dvs_downsample_view), offsetof(dvs_downsample_view, src), offsetof(dvs_downsample_view, dst),
         DVS_DOWNSAMPLE_MAX_VIEWS);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    D = _lib.DownsampleView
    assert out == [C.sizeof(D), D.src.offset, D.dst.offset, 16]


def test_cli_help_lists_the_schedule_flags():
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--resolutionSchedule [0]" in out and "--numDownscales [2]" in out, out


def test_level_of_step_and_clamp():
    assert [level_of_step(s, 4, 2) for s in range(0, 13)] == [2] * 4 + [1] * 4 + [0] * 5
    assert level_of_step(6, 4, 2) == 1 and level_of_step(10 ** 6, 3000, 2) == 0 and level_of_step(0, 0, 2) == 0
    assert clamp_levels(2, 142, 110) == 2 and clamp_levels(3, 142, 110) == 2          # 110 >> 3 = 13 < 16
    assert clamp_levels(9, 1920, 1080) == 3 and clamp_levels(2, 40, 31) == 0 and clamp_levels(-1, 640, 480) == 0


def test_downsample_restatement_on_explicit_values():
    a = np.arange(2 * 5 * 7, dtype=np.uint8).reshape(2, 5, 7) * 3
    o = downsample_np(a, 2)
    assert o.shape == (2, 2, 3) and o.dtype == np.float32
    blk = a[1, 2:4, 4:6].astype(np.int64).sum()
    assert o[1, 1, 2] == np.float32(blk) * (np.float32(1) / np.float32(255)) * np.float32(0.25)
    f = np.float32
    b = np.array([[[1e8, 1.0, 3.0], [-1e8, 1.0, 5.0]]], f)                            # the order of the fp32 additions is visible
    assert downsample_np(b, 2)[0, 0, 0] == ((f(1e8) + f(1.0)) + f(-1e8) + f(1.0)) * f(0.25) == f(0.25)
    assert same_bits(downsample_np(b, 1), b) and downsample_np(np.array([[[-0.0]]], f), 1).view(np.uint32)[0, 0, 0] == 0x80000000


@pytest.mark.parametrize("W,H", [(142, 110), (128, 96)])
def test_camera_downscale_matches_the_restatement(W, H):
    spec = dv.make_spec(10, W, H, sh_degree=1, n_cams=4, seed=5)
    for ci in range(4):
        cam = dv.synth_camera(spec, ci)
        cam.bg[0], cam.bg[1], cam.bg[2] = 0.25, 0.5, 0.75
        full = camera_fields(cam)
        for d in (1, 2, 4, 8):
            got = camera_fields(dv.camera_downscale(cam, d))
            want = camera_downscale_np(cam, d)
            for k in want:
                assert same_bits(got[k], want[k]), (W, H, ci, d, k, got[k], want[k])
            assert (got["width"], got["height"]) == (W // d, H // d)
            for k in ("view", "campos", "bg"):
                assert same_bits(got[k], full[k])
            assert got["focal_x"] * d == full["focal_x"] and got["focal_y"] * d == full["focal_y"]
            if W % d == 0:
                assert same_bits(got["proj"][0::4], full["proj"][0::4]) and same_bits(got["tan_fovx"], full["tan_fovx"])
            else:
                assert not same_bits(got["proj"][0::4], full["proj"][0::4]) and got["tan_fovx"] < full["tan_fovx"]
            if H % d == 0:
                assert same_bits(got["proj"][1::4], full["proj"][1::4]) and same_bits(got["tan_fovy"], full["tan_fovy"])
            else:
                assert not same_bits(got["proj"][1::4], full["proj"][1::4]) and got["tan_fovy"] < full["tan_fovy"]
            assert same_bits(got["proj"][2::4], full["proj"][2::4]) and same_bits(got["proj"][3::4], full["proj"][3::4])
    # what the two sizes are here for: 142x110 is cropped at 4 in both directions and exact at 2; 128x96 is exact at every factor
    assert 142 % 4 and 110 % 4 and not 142 % 2 and not 110 % 2 and not 128 % 8 and not 96 % 8


def test_camera_downscale_argument_checks():
    f = _lib.lib.dvs_camera_downscale
    cam = dv.synth_camera(dv.make_spec(10, 40, 24, sh_degree=1), 0)
    out = _lib.Camera()
    assert f(C.byref(cam), 2, C.byref(out)) == 0 and (out.width, out.height) == (20, 12)
    for bad in (0, 3, 5, 6, 16, -2):
        assert f(C.byref(cam), bad, C.byref(out)) == INVALID, bad
    assert f(None, 2, C.byref(out)) == INVALID and f(C.byref(cam), 2, None) == INVALID
    assert f(C.byref(cam), 2, C.byref(cam)) == INVALID and f(C.byref(cam), 1, C.byref(cam)) == INVALID       # in == out
    small = dv.synth_camera(dv.make_spec(10, 40, 7, sh_degree=1), 0)
    assert f(C.byref(small), 4, C.byref(out)) == 0 and f(C.byref(small), 8, C.byref(out)) == INVALID       # 7 / 8 == 0
    one = _lib.Camera()
    assert f(C.byref(cam), 1, C.byref(one)) == 0 and bytes(one) == bytes(cam)                              # factor 1 is a copy


@pytest.mark.parametrize("d", [2, 4])
def test_level_camera_draws_every_splat_at_the_box_filters_position(d):
    """fp64 oracle, the 600 splats of make_spec(600, 142, 110): for every splat visible under both cameras the depth is identical and
    |mean2d_level - ((mean2d_full + 0.5) / d - 0.5)| <= 1e-3 px. The only error is the fp32 rounding of proj' (about 6e-8 relative, times
    W: 1e-5 px), so the bar leaves two orders of margin."""
    spec = dv.make_spec(600, 142, 110, sh_degree=1, n_cams=4, seed=9)
    P = dv.synth_splats(spec)
    o = Oracle(np.float64)
    seen, worst = 0, 0.0
    for ci in range(4):
        cam = dv.synth_camera(spec, ci)
        o.forward(P, cam, sh_degree=1)
        m_full, z_full, r_full = o.get("mean2d").copy(), o.get("depth").copy(), o.get("radii").copy()
        o.forward(P, dv.camera_downscale(cam, d), sh_degree=1)
        m_lvl, z_lvl, r_lvl = o.get("mean2d").copy(), o.get("depth").copy(), o.get("radii").copy()
        both = (r_full > 0) & (r_lvl > 0)
        seen += int(both.sum())
        assert np.array_equal(z_full[both], z_lvl[both])
        err = np.abs(m_lvl[both] - ((m_full[both] + 0.5) / d - 0.5)).max()
        worst = max(worst, float(err))
        assert err <= 1e-3, (ci, d, err)
    print(f"factor {d}: {seen} splat views, worst position error {worst:.3e} px")
    assert seen > 600                                                       # (most of the 600 are visible from each of the 4 cameras)
