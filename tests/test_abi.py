"""The C-ABI library loads without a GPU, exports every symbol include/*.h declares, and the ctypes mirrors
have the C layout (sizeof / offsetof checked against gcc)."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import divshot_amd as dv
from divshot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    names = []
    for h in ("dvs_raster.h", "dvs_scene.h", "dvs_train.h", "dvs_comm.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names += re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_every_declared_symbol_is_exported_and_bound():
    names = declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(dv.lib, n), f"{n} is declared in include/ but not exported by libdvsraster.so"
        assert n in _lib._PROTOS, f"{n} has no ctypes prototype"
    assert set(_lib._PROTOS) <= set(names), set(_lib._PROTOS) - set(names)
    assert b"gfx950" in dv.lib.dvs_version()


def test_struct_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dvs_raster.h"
#include "dvs_scene.h"
#include "dvs_train.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dvs_splats), sizeof(dvs_camera), sizeof(dvs_opts), sizeof(dvs_fwd_state),
         sizeof(dvs_splat_grads), sizeof(dvs_scene_spec));
  printf("%zu %zu %zu %zu\n", offsetof(dvs_camera, campos), offsetof(dvs_camera, bg), offsetof(dvs_fwd_state, num_rendered),
         offsetof(dvs_scene_spec, seed));
  printf("%zu %zu %zu %zu %zu\n", sizeof(dvs_adam_group), sizeof(dvs_densify_params), sizeof(dvs_mcmc_sets),
         offsetof(dvs_adam_group, lr), offsetof(dvs_densify_params, revised_opacity));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    sizes = [int(v) for v in out[:6]]
    assert sizes == [C.sizeof(_lib.Splats), C.sizeof(_lib.Camera), C.sizeof(_lib.Opts), C.sizeof(_lib.FwdState),
                     C.sizeof(_lib.SplatGrads), C.sizeof(_lib.SceneSpec)]
    offs = [int(v) for v in out[6:10]]
    assert offs == [_lib.Camera.campos.offset, _lib.Camera.bg.offset, _lib.FwdState.num_rendered.offset, _lib.SceneSpec.seed.offset]
    train = [int(v) for v in out[10:]]           # the structs of include/dvs_train.h
    assert train == [C.sizeof(_lib.AdamGroup), C.sizeof(_lib.DensifyParams), C.sizeof(_lib.McmcSets), _lib.AdamGroup.lr.offset,
                     _lib.DensifyParams.revised_opacity.offset]


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        return
    assert not dv.lib.dvs_create(0, 1024, 64, 64)
    assert b"no such HIP device" in dv.lib.dvs_last_error() or b"hip" in dv.lib.dvs_last_error().lower()


def test_scene_generator_is_deterministic():
    import numpy as np
    spec = dv.make_spec(1000, 320, 200, sh_degree=2, n_cams=8)
    a, b = dv.synth_splats(spec), dv.synth_splats(spec)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert not a["shN"][:, 8:].any() and a["shN"][:, :8].any()       # bands above degree 2 are zero
    cams = [dv.synth_camera(spec, i) for i in range(8)]
    assert list(cams[0].campos) == [0.0, 0.0, 0.0]
    for c in cams[1:]:
        assert abs(np.hypot(c.campos[0], c.campos[1]) - 0.5) < 1e-6   # 0.5-radius ring
        # look-at point (0,0,7) projects to the image centre
        p = np.array([0, 0, 7, 1.0])
        hom = p @ np.array(list(c.proj)).reshape(4, 4)
        assert abs(hom[0] / hom[3]) < 1e-5 and abs(hom[1] / hom[3]) < 1e-5


def test_release_build_has_no_ablation_knobs():
    """The timing-only ablation knobs of earlier rounds (they could skip the flush / the publish / the atomics of the composite backward,
    i.e. silently zero gradients) were removed from the source together with the build that compiled them in: the shipped libraries do
    not even contain the names, so no environment variable can reach such code."""
    knobs = (b"DVS_TR_DEBUG", b"DVS_MM_DEBUG", b"DVS_FWD_DEBUG", b"DVS_A9V_NOHOIST", b"DVS_BWD_EXTRA_LDS")
    libs = [_lib.LIB_PATH, os.path.join(ROOT, "divshot_amd", "lib", "libgstrain.so")]
    for path in libs:
        if not os.path.exists(path):
            continue
        blob = open(path, "rb").read()
        for k in knobs:
            assert k not in blob, f"{os.path.basename(path)} still carries the experiment knob {k.decode()}"
    assert os.environ.get("DVS_RASTER_LIB") or os.path.basename(_lib.LIB_PATH) == "libdvsraster.so"


def test_release_build_ships_one_forward_and_one_backward_kernel():
    """libdvsraster.so contains the composite forward (k_render_fwd), the composite backward (k_render_bwd_tr) and the
    round-2 backward kept as the parity tests' cross-check (k_render_bwd_blocks) — none of the retired kernels ("reduce" = k_render_bwd,
    "mm", the per-block forward), neither as host stubs nor as device code."""
    if os.environ.get("DVS_RASTER_LIB"):
        return                                              # a library substituted for an A/B run: not the one this test is about
    blob = open(_lib.LIB_PATH, "rb").read()
    for retired in (b"k_render_bwd_mm", b"k_render_fwd_blocks", b"12k_render_bwdILb"):       # (Itanium mangling: <length><name>I...)
        assert retired not in blob, f"libdvsraster.so still contains the retired kernel {retired.decode()}"
    for shipped in (b"12k_render_fwdILb", b"15k_render_bwd_trILb", b"19k_render_bwd_blocksILb"):
        assert shipped in blob, shipped


def test_retired_variants_are_refused():
    """dvs_set_backward_variant / dvs_set_forward_variant answer DVS_ERR_UNSUPPORTED for kernels the library does not contain (needs a device
    for the context; on CPU the symbols and the error code are checked)."""
    import torch
    assert hasattr(dv.lib, "dvs_set_backward_variant") and hasattr(dv.lib, "dvs_set_forward_variant")
    if not torch.cuda.is_available() or os.environ.get("DVS_RASTER_LIB"):
        return
    ctx = dv.lib.dvs_create(0, 1024, 64, 64)
    assert ctx
    try:
        assert dv.lib.dvs_set_backward_variant(ctx, 1) == 5 and dv.lib.dvs_set_backward_variant(ctx, 2) == 5      # reduce, mm: DVS_ERR_UNSUPPORTED
        assert b"retired" in dv.lib.dvs_last_error()
        assert dv.lib.dvs_set_forward_variant(ctx, 0) == 5
        assert dv.lib.dvs_set_backward_variant(ctx, 0) == 0 and dv.lib.dvs_set_backward_variant(ctx, 3) == 0 and dv.lib.dvs_set_forward_variant(ctx, 1) == 0
    finally:
        dv.lib.dvs_destroy(ctx)
