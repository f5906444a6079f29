"""The sky texture file (divshot_amd/gstrain/sky_io.cpp) without a GPU, through libgsplyio.so's gstrain_sky_* entry points: 16-byte header
(magic DVSSKY1\\0, uint32 width, uint32 height) + height * width * 3 little-endian fp32. Round trip bit for bit; truncated and over-long
files, a wrong magic and width != 2 * height are refused with a message. And the CLI lists --enableBg / --skyResolution and refuses bad
values."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))       # host only: no HIP runtime behind it
    lib.gstrain_sky_write.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_char_p, C.c_int]
    lib.gstrain_sky_read.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int]
    return lib


def read(lib, path):
    dims = (C.c_uint32 * 2)()
    err = C.create_string_buffer(256)
    if lib.gstrain_sky_read(path.encode(), dims, None, 0, err, 256) != 0:
        return None, err.value.decode()
    out = np.empty((dims[1], dims[0], 3), np.float32)
    assert lib.gstrain_sky_read(path.encode(), dims, out.ctypes.data, out.size, err, 256) == 0
    return out, ""


@pytest.mark.parametrize("h", [2, 16, 128])
def test_round_trip_and_layout(lib, tmp_path, h):
    tex = np.random.default_rng(h).normal(0, 1, (h, 2 * h, 3)).astype(np.float32)
    path = str(tmp_path / "a.sky")
    err = C.create_string_buffer(256)
    assert lib.gstrain_sky_write(path.encode(), 2 * h, h, tex.ctypes.data, err, 256) == 0, err.value
    raw = open(path, "rb").read()
    assert raw[:16] == b"DVSSKY1\0" + struct.pack("<II", 2 * h, h) and raw[16:] == tex.astype("<f4").tobytes()
    back, _ = read(lib, path)
    assert np.array_equal(back.view(np.uint32), tex.view(np.uint32))


def test_refusals(lib, tmp_path):
    h = 4
    tex = np.arange(h * 2 * h * 3, dtype=np.float32)
    good = b"DVSSKY1\0" + struct.pack("<II", 2 * h, h) + tex.tobytes()
    cases = {"truncated": good[:-3], "header only": good[:16], "short header": good[:9], "over-long": good + b"\0",
             "magic": b"DVSSKY2\0" + good[8:], "shape": good[:8] + struct.pack("<II", 2 * h - 1, h) + good[16:],
             "flat": good[:8] + struct.pack("<II", 2, 1) + good[16:]}
    for name, data in cases.items():
        path = str(tmp_path / (name.replace(" ", "_") + ".sky"))
        open(path, "wb").write(data)
        out, msg = read(lib, path)
        assert out is None and msg, name
    assert "magic" in read(lib, str(tmp_path / "magic.sky"))[1] and "2 * height" in read(lib, str(tmp_path / "shape.sky"))[1]
    assert read(lib, str(tmp_path / "missing.sky"))[0] is None
    err = C.create_string_buffer(256)
    assert lib.gstrain_sky_write(str(tmp_path / "x.sky").encode(), 9, 4, tex.ctypes.data, err, 256) != 0 and err.value
    assert lib.gstrain_sky_write(str(tmp_path / "x.sky").encode(), 8, 4, None, err, 256) != 0


def test_cli_lists_the_flags_and_refuses_bad_values(tmp_path):
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--enableBg [0]" in out and "--skyResolution [128]" in out, out
    for flag, value in (("--enableBg", "2"), ("--enableBg", "yes"), ("--skyResolution", "abc"), ("--skyResolution", "-4"), ("--skyResolution", "")):
        p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=10", "--outputPath", str(tmp_path / "x"), flag, value], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and f"{flag} takes" in p.stdout, (flag, value, p.stdout)
