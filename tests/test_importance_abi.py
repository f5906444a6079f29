"""The importance-prune entry points without a GPU: the three symbols are exported, refuse bad arguments before they touch a device,
the CLI lists --importancePrune and refuses a bad value, and GaussianTrainConfig::importancePrune sits in the struct's tail padding
directly behind renderSampling (checked with a compiled probe, in the manner of tests/test_export_format.py)."""
import ctypes as C
import os
import subprocess
import tempfile
import divshot_amd as dv
from divshot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
INVALID = 1


def test_symbols_are_exported_and_bound():
    for name in ("dvs_raster_importance_views", "dvs_importance_scratch_bytes", "dvs_importance_plan"):
        assert hasattr(dv.lib, name) and name in _lib._PROTOS, name


def test_importance_views_refuses_bad_arguments():
    f = dv.lib.dvs_raster_importance_views
    opts = dv.Opts()
    assert f(None, None, C.byref(opts), None, 16, None, None) == INVALID            # NULL ctx
    assert f(None, None, None, None, 16, None, None) == INVALID                     # ... and NULL opts
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))                      # never dereferenced: the argument checks come first
    assert f(fake, None, None, None, 16, None, None) == INVALID                     # NULL opts
    assert f(fake, None, C.byref(opts), None, None, None, None) == INVALID          # NULL score_sum
    assert f(fake, None, C.byref(opts), None, 24, None, None) == INVALID            # misaligned score_sum
    assert f(fake, None, C.byref(opts), None, 16, 36, None) == INVALID              # misaligned score_max
    assert f(fake, None, C.byref(opts), None, 16, 32, 40) == INVALID                # misaligned hits
    assert b"dvs_raster_importance_views" in dv.lib.dvs_last_error()


def test_importance_plan_refuses_bad_arguments():
    f = dv.lib.dvs_importance_plan
    ok = dict(n=8, score=256, keep=4, action=512, offsets=768, scratch=1024, new_count=2048)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["n"], a["score"], a["keep"], a["action"], a["offsets"], a["scratch"], a["new_count"])
    assert call(n=0) == INVALID and call(n=-3) == INVALID
    assert call(keep=0) == INVALID
    for name in ("score", "action", "offsets", "scratch", "new_count"):
        assert call(**{name: None}) == INVALID, name
    assert call(score=260) == INVALID and call(scratch=1028) == INVALID             # misaligned


def test_scratch_bytes_covers_the_state_the_histograms_and_two_words_per_block():
    f = dv.lib.dvs_importance_scratch_bytes
    assert f(0) == 0 and f(-1) == 0
    for n in (1, 255, 256, 257, 70001, 3_000_000):
        assert f(n) >= 32 + 8 * 256 * 4 + 2 * ((n + 255) // 256) * 4 and f(n) % 16 == 0, n
    assert f(1) <= f(257) <= f(70001) <= f(3_000_000)


def test_cli_lists_the_flag_and_refuses_a_bad_value(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--importancePrune [0]" in out, out
    for value in ("91", "-1", "abc", "12.5", ""):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), "--importancePrune", value],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--importancePrune takes" in p.stdout, (value, p.stdout)


def test_config_field_sits_in_the_tail_padding():
    """importancePrune is the byte behind renderSampling, 0 by default, and the struct still ends at exportFormats plus its padding"""
    prog = r'''
#include <cstdio>
#include <cstddef>
#include "gaussian_trainer_scene.hpp"
int main() {
  GaussianTrainConfig c;
  std::printf("%zu %zu %zu %zu %zu %d\n", sizeof(GaussianTrainConfig), alignof(GaussianTrainConfig), offsetof(GaussianTrainConfig, exportFormats),
              offsetof(GaussianTrainConfig, renderSampling), offsetof(GaussianTrainConfig, importancePrune), (int)c.importancePrune);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size, align, off_formats, off_sampling, off_new, default = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert off_new == off_sampling + 1 and default == 0
    assert size == (off_formats + 4 + align - 1) // align * align
