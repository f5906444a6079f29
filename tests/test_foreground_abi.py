"""The mask carve's entry points without a GPU: the three symbols are exported and bound, every DVS_ERR_INVALID refusal comes before
anything touches a device and names its function in dvs_last_error(), the CLI lists --maskCarve and refuses a bad value, the config
struct keeps its size and offsets (the switch is a setter and an environment variable, not a field), and a host can call setMaskCarve."""
import ctypes as C
import os
import subprocess
import divshot_amd as dv
from divshot_amd import _lib, prune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
INVALID = 1


def test_symbols_are_exported_and_bound():
    for name in ("dvs_raster_foreground_views", "dvs_foreground_plan"):
        assert hasattr(dv.lib, name) and name in _lib._PROTOS, name
    assert callable(prune.foreground_votes) and callable(prune.foreground_plan)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, "libgstrain.so")]).decode()
    assert "setMaskCarve" in out


def test_foreground_views_refuses_bad_arguments():
    f = dv.lib.dvs_raster_foreground_views
    opts = dv.Opts()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))                      # never dereferenced: the argument checks come first
    assert f(None, None, C.byref(opts), None, None, 16, 32) == INVALID              # NULL ctx
    assert f(fake, None, None, None, None, 16, 32) == INVALID                       # NULL opts
    assert f(fake, None, C.byref(opts), None, None, None, 32) == INVALID            # NULL fg_sum
    assert f(fake, None, C.byref(opts), None, None, 16, None) == INVALID            # NULL bg_sum
    assert b"dvs_raster_foreground_views: null argument" in dv.lib.dvs_last_error()
    assert f(fake, None, C.byref(opts), None, None, 24, 32) == INVALID              # misaligned fg_sum
    assert f(fake, None, C.byref(opts), None, None, 16, 40) == INVALID              # misaligned bg_sum
    assert b"dvs_raster_foreground_views" in dv.lib.dvs_last_error() and b"aligned" in dv.lib.dvs_last_error()


def test_foreground_plan_refuses_bad_arguments():
    f = dv.lib.dvs_foreground_plan
    ok = dict(n=8, fg=256, bg=512, percent=50, action=768, offsets=1024, scratch=1280, new_count=2048)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["n"], a["fg"], a["bg"], a["percent"], a["action"], a["offsets"], a["scratch"], a["new_count"])
    for bad in (dict(n=0), dict(n=-3), dict(percent=0), dict(percent=101), dict(percent=-1), dict(new_count=2052)):
        assert call(**bad) == INVALID, bad
        assert b"dvs_foreground_plan" in dv.lib.dvs_last_error(), bad
    for name in ("fg", "bg", "action", "offsets", "scratch", "new_count"):
        assert call(**{name: None}) == INVALID, name
        assert b"dvs_foreground_plan: null argument" in dv.lib.dvs_last_error(), name


def test_cli_lists_the_flag_and_refuses_a_bad_value(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--maskCarve [0]" in out, out
    for value in ("101", "-1", "x", "12.5", "", "1000"):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), "--maskCarve", value],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "Command Line Error: --maskCarve takes" in p.stdout, (value, p.stdout)


def test_config_struct_is_unchanged_and_a_host_can_call_the_setter(tmp_path):
    """sizeof(GaussianTrainConfig) is what the tail-padding rule of tests/test_importance_abi.py says and importancePrune is still its last
    byte in use; setMaskCarve links against the plugin"""
    prog = r'''
#include <cstdio>
#include <cstddef>
#include "gaussian_trainer_scene.hpp"
void use(GaussianTrainerScene& s) { s.setMaskCarve(50); }
int main() {
  std::printf("%zu %zu %zu %zu %zu\n", sizeof(GaussianTrainConfig), alignof(GaussianTrainConfig), offsetof(GaussianTrainConfig, exportFormats),
              offsetof(GaussianTrainConfig, renderSampling), offsetof(GaussianTrainConfig, importancePrune));
  return 0; }'''
    src, exe = str(tmp_path / "t.cpp"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", LIB, "-lgstrain",
                           "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    size, align, off_formats, off_sampling, off_prune = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert size == (off_formats + 4 + align - 1) // align * align
    assert off_sampling == off_formats + 6 and off_prune == off_sampling + 1 and off_prune == size - 1
