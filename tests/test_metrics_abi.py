"""The image-metric entry points without a GPU: dvs_metrics_view has the C layout (checked against gcc, in the manner of
tests/test_abi.py::test_struct_layout_matches_c), the scratch size is positive and monotone, and the CLI lists the evaluation flags."""
import ctypes as C
import os
import subprocess
import tempfile
from divshot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")


def test_metrics_view_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dvs_train.h"
int main(void) {
  printf("%zu %zu %zu %zu %d\n", sizeof(dvs_metrics_view), offsetof(dvs_metrics_view, img), offsetof(dvs_metrics_view, target),
         offsetof(dvs_metrics_view, mask), DVS_METRICS_MAX_VIEWS);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    M = _lib.MetricsView
    assert out == [C.sizeof(M), M.img.offset, M.target.offset, M.mask.offset, 16]


def test_scratch_bytes_is_positive_and_monotone():
    f = _lib.lib.dvs_image_metrics_scratch_bytes
    assert f(1, 1, 1) > 0
    sizes = [1, 7, 16, 17, 53, 256, 1920]
    for w0, w1 in zip(sizes, sizes[1:]):
        for h in (1, 37, 1080):
            for v in (1, 3, 16):
                assert 0 < f(w0, h, v) <= f(w1, h, v) and 0 < f(h, w0, v) <= f(h, w1, v), (w0, w1, h, v)
    for v in range(1, 16):
        assert f(53, 37, v) < f(53, 37, v + 1)
    assert f(16, 16, 1) < f(17, 16, 1) and f(16, 16, 1) < f(16, 17, 1)      # a tile more in either direction
    # room for every workgroup's slot: at least three fp32 sums per 16x16 tile and view
    assert f(1920, 1080, 8) >= 120 * 68 * 8 * 3 * 4


def test_cli_help_lists_the_evaluation_flags():
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    for flag in ("--eval ", "--evalHoldout", "--evalEvery"):
        assert flag in out, out
