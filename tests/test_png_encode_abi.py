"""The C-ABI and the command line of PNG output, without a GPU: both dvs_png_encode_* symbols are exported by libdvsraster.so and
bound; dvs_png_encode_bytes is height * (1 + rowbytes), 0 for what the call refuses; every DVS_ERR_INVALID case of
dvs_png_encode_views returns that status before anything touches a device (a call that went on would report a HIP error here, or
fault on the made-up pointers); `gaussian_train --help` lists the three flags, bad values exit 1 with `<flag> takes`, and depth or
alpha with the JPEG format is refused. The class member renderCameraToPng is declared in the header, so tests/test_plugin.py pins its
export; no new C symbol enters libgstrain.so."""
import ctypes as C
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
INVALID = 1
RGB8, GRAY8, GRAY16 = 0, 1, 2


def test_both_symbols_are_exported_and_bound():
    from divshot_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, "libdvsraster.so")]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"dvs_png_encode_bytes", "dvs_png_encode_views"} <= exported
    assert {"dvs_png_encode_bytes", "dvs_png_encode_views"} <= set(_lib._IMAGE_PROTOS) and not {"dvs_png_encode_bytes", "dvs_png_encode_views"} & set(_lib._PROTOS)
    assert "gstrain_png_write" in _lib._PNG_HOST_PROTOS and "gstrain_png_write" not in _lib._PROTOS
    assert _lib.lib.dvs_png_encode_views.restype is C.c_int and _lib.lib.dvs_png_encode_bytes.restype is C.c_size_t
    hdr = open(os.path.join(ROOT, "include", "dvs_image.h")).read()
    assert "#define DVS_PNG_ENCODE_MAX_VIEWS 16" in hdr and hdr.index("dvs_png_reconstruct(void*") < hdr.index("dvs_png_encode_views(void*")
    plug = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(LIB, "libgstrain.so")]).decode()
    assert "GaussianTrainerScene::renderCameraToPng(" in plug and "png_write" not in plug and "dvs_png_encode" not in plug


def test_encode_bytes():
    from divshot_amd import _lib
    f = _lib.lib.dvs_png_encode_bytes
    assert f(RGB8, 1, 1) == 4 and f(GRAY8, 1, 1) == 2 and f(GRAY16, 1, 1) == 3
    assert f(RGB8, 17, 5) == 5 * 52 and f(GRAY8, 17, 5) == 5 * 18 and f(GRAY16, 17, 5) == 5 * 35
    assert f(RGB8, 1920, 1080) == 1080 * 5761
    assert f(RGB8, 65500, 65500) == 65500 * (1 + 3 * 65500) and f(GRAY16, 65500, 65500) == 65500 * (1 + 2 * 65500)     # past 2^32
    for kind, w, h in ((3, 8, 8), (-1, 8, 8), (RGB8, 0, 8), (RGB8, 8, 0), (GRAY8, 65501, 8), (GRAY16, 8, 65501), (GRAY8, -4, 8)):
        assert f(kind, w, h) == 0, (kind, w, h)


def test_every_invalid_case_returns_before_a_device_is_touched():
    from divshot_amd import _lib
    f = _lib.lib.dvs_png_encode_views
    fake = 0x10000                                               # never dereferenced: a refusal comes first
    one = lambda p: (C.c_void_p * 1)(p)
    good = dict(stream=None, kind=RGB8, w=8, h=8, scale=255.0, images=one(fake), filtered=one(fake + 1), sat=None, n=1)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["stream"], a["kind"], a["w"], a["h"], a["scale"], a["images"], a["filtered"], a["sat"], a["n"])

    assert call(images=None) == INVALID and call(filtered=None) == INVALID
    assert call(images=one(None)) == INVALID and call(filtered=one(None)) == INVALID
    assert call(n=0) == INVALID and call(n=-1) == INVALID
    many = (C.c_void_p * 17)(*[fake] * 17)
    assert call(images=many, filtered=many, n=17) == INVALID
    two = (C.c_void_p * 2)(fake, None)
    assert call(images=two, filtered=(C.c_void_p * 2)(fake, fake), n=2) == INVALID and call(images=(C.c_void_p * 2)(fake, fake), filtered=two, n=2) == INVALID
    assert call(kind=3) == INVALID and call(kind=-1) == INVALID
    for w, h in ((0, 8), (8, 0), (65501, 8), (8, 65501), (-1, 8)):
        assert call(w=w, h=h) == INVALID, (w, h)
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), -0.0):
        assert call(scale=scale) == INVALID, scale
    assert call(images=one(fake + 2)) == INVALID                 # off a float's boundary


def run_cli(*args):
    return subprocess.run([DRIVER] + list(args), capture_output=True, text=True, timeout=60)


def test_help_lists_the_flags_and_bad_values_are_command_line_errors(tmp_path):
    p = run_cli("--help")
    assert p.returncode == 0
    for flag in ("--renderFormat [jpg]", "--renderLayers [color]", "--renderDepthScale [1000]"):
        assert flag in p.stdout, p.stdout
    base = ["--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x")]
    bad = [("--renderFormat", "bmp"), ("--renderFormat", ""), ("--renderLayers", "depth"), ("--renderLayers", "color,"), ("--renderLayers", "color,color"),
           ("--renderLayers", "color,alpha,depth"), ("--renderLayers", "colour"), ("--renderLayers", ""), ("--renderDepthScale", "0"), ("--renderDepthScale", "-5"),
           ("--renderDepthScale", "nan"), ("--renderDepthScale", "inf"), ("--renderDepthScale", "1e60"), ("--renderDepthScale", "12x"), ("--renderDepthScale", "")]
    for flag, value in bad:
        p = run_cli(*base, "--renderFormat", "png", f"{flag}={value}") if flag != "--renderFormat" else run_cli(*base, f"{flag}={value}")
        assert p.returncode == 1 and "Command Line Error" in p.stdout and f"{flag} takes" in p.stdout, (flag, value, p.stdout, p.stderr)


def test_depth_or_alpha_with_jpg_is_refused(tmp_path):
    base = ["--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x")]
    for layers in ("color,depth", "color,alpha", "color,depth,alpha"):
        for fmt in ([], ["--renderFormat", "jpg"]):
            p = run_cli(*base, *fmt, "--renderLayers", layers)
            assert p.returncode == 1 and "--renderLayers takes" in p.stdout and "png" in p.stdout, (layers, fmt, p.stdout)
    assert not os.path.exists(str(tmp_path / "x"))
