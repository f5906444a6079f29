"""The .spz export without a GPU: the numpy restatement tests/spz_ref.py against a fixture recorded from the reference's own
packGaussians / unpackGaussians / saveSpz (tests/golden/spz_pack_v3.npz: recorded data only), the file gstrain_write_spz writes, the
inputs of the GPU tests against the alpha allowance's cap, the CLI switch, and the rules on explicit values."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import numpy as np
import pytest
import spz_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
DRIVER = os.path.join(LIB, "gaussian_train")
GPU_SIZES = (1, 63, 64, 65, 1000, 2049)                    # the sizes tests/test_gpu_spz.py packs on the device
f32 = np.float32


class Layout(C.Structure):                                 # dvs_spz_layout
    _fields_ = [("off", C.c_uint64 * 6), ("bytes", C.c_uint64 * 6), ("total", C.c_uint64)]


@pytest.fixture(scope="module")
def plyio():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))       # host only: no HIP runtime behind it
    lib.gstrain_write_spz.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.POINTER(Layout), C.c_char_p, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "spz_pack_v3.npz"))
    model = {k: g["in_" + k] for k in S.FIELDS}
    return g, model


def _ulp_close(got, want, ulps):
    fin = np.isfinite(want)
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]) and \
        (np.abs(got[fin].astype(np.float64) - want[fin]) <= ulps * np.spacing(np.abs(want[fin]))).all()


def test_restatement_reproduces_the_reference_pack(golden):
    """600 splats at degree 3, packed by the reference's packGaussians: positions to +-2047.9 and on half steps of the fixed point, SH
    values with x * 128 half-integer of both signs and on the buckets' half steps, quaternions with tied and with negative largest
    components, scales and colours past both ends of their bytes. Every section bit for bit; the alpha byte may differ by one only
    where alpha_slack allows (the reference takes a float32 sigmoid, the restatement a float64 one)."""
    g, model = golden
    got = S.pack(model, 3)
    for name in S.SECTIONS:
        want = g["packed_" + name]
        assert got[name].shape == want.shape, name
        if name != "alphas":
            assert np.array_equal(got[name], want), (name, int((got[name] != want).sum()))
    d = got["alphas"].astype(np.int64) - g["packed_alphas"].astype(np.int64)
    slack = S.alpha_slack(model["opacity"])
    print(f"alpha bytes off by one {int((d != 0).sum())}, eligible {int(slack.sum())}")
    assert slack.any() and slack.mean() <= 0.01
    assert (np.abs(d) <= 1).all() and not (d != 0)[~slack].any()


def test_restatement_reproduces_the_reference_unpack(golden):
    """unpackGaussians of the reference's own sections: bit for bit, but the opacity logit (logf of another C library) and the
    reconstructed quaternion component (its sqrt), both within 2 ulp. The reference's rotations are (x, y, z, w)."""
    g, _ = golden
    n = len(g["packed_alphas"])
    dec = S.unpack({name: g["packed_" + name] for name in S.SECTIONS}, 3)
    for key, ref in (("pos", "positions"), ("scale", "scales"), ("sh0", "colors"), ("shN", "sh")):
        assert np.array_equal(dec[key].reshape(-1).view(np.uint32), g["unpacked_" + ref].view(np.uint32)), key
    assert _ulp_close(dec["opacity"], g["unpacked_alphas"], 2)
    assert not np.isfinite(g["unpacked_alphas"]).all() or g["packed_alphas"].min() > 0       # (bytes 0 / 255 decode to -inf / +inf)
    want = g["unpacked_rotations"].reshape(n, 4)[:, [3, 0, 1, 2]]                             # -> (w, x, y, z)
    rebuilt = np.zeros((n, 4), bool)
    rebuilt[np.arange(n), (dec["largest"] + 1) % 4] = True                                    # the format's index k is column (k + 1) % 4
    assert np.array_equal(dec["rot"][~rebuilt].view(np.uint32), want[~rebuilt].view(np.uint32))
    assert _ulp_close(dec["rot"][rebuilt], want[rebuilt], 2)


def test_reader_reads_the_reference_written_file(golden):
    g, model = golden
    n, degree, aa, sec = S.parse_spz(gzip.decompress(g["spz_file"].tobytes()))
    assert (n, degree, aa) == (600, 3, True)
    for name in S.SECTIONS:
        assert np.array_equal(sec[name], g["packed_" + name]), name


def test_inputs_of_the_gpu_tests_stay_under_the_allowance_cap():
    for n in GPU_SIZES:
        assert S.alpha_slack(S.random_model(n, seed=n)["opacity"]).mean() <= 0.01, n
    for name in S.EDGE_CASES:
        with np.errstate(over="ignore", invalid="ignore"):
            assert S.alpha_slack(S.edge_model(name)["opacity"]).mean() <= 0.01, name


def _in_device_layout(sec, n, degree):
    off, size, total = S.layout(n, degree)
    buf = np.full(total, 0xEE, np.uint8)                                     # the gaps between the sections must not reach the file
    for name, o, b in zip(S.SECTIONS, off, size):
        buf[o:o + b] = sec[name]
    lay = Layout()
    for k in range(6):
        lay.off[k], lay.bytes[k] = off[k], size[k]
    lay.total = total
    return buf, lay


@pytest.mark.parametrize("n,degree,aa", [(600, 3, 1), (1, 3, 0), (65, 2, 0), (1000, 1, 1), (257, 0, 0)])
def test_spz_file_is_the_header_then_the_sections(plyio, tmp_path, n, degree, aa):
    sec = S.pack(S.random_model(n, seed=n), degree)
    buf, lay = _in_device_layout(sec, n, degree)
    path = str(tmp_path / "m.spz")
    err = C.create_string_buffer(256)
    assert plyio.gstrain_write_spz(path.encode(), n, degree, aa, buf.ctypes.data, C.byref(lay), err, 256) == 0, err.value
    raw = gzip.open(path, "rb").read()
    assert len(raw) == 16 + (20 + 3 * S.DIM[degree]) * n
    if degree == 3:
        assert len(raw) == 16 + 65 * n
    assert struct.unpack("<IIIBBBB", raw[:16]) == (0x5053474E, 3, n, degree, 12, aa, 0)
    assert raw[:16] == S.header(n, degree, bool(aa))
    assert raw[16:] == b"".join(sec[name].tobytes() for name in S.SECTIONS)      # file order: positions, alphas, colors, scales, rotations, sh
    got_n, got_degree, got_aa, got = S.read_spz(path)
    assert (got_n, got_degree, got_aa) == (n, degree, bool(aa)) and all(np.array_equal(got[k], sec[k]) for k in S.SECTIONS)


def test_unwritable_path_fails_with_a_message(plyio, tmp_path):
    sec = S.pack(S.random_model(10, seed=1), 3)
    buf, lay = _in_device_layout(sec, 10, 3)
    err = C.create_string_buffer(256)
    bad = str(tmp_path / "no" / "dir.spz")
    assert plyio.gstrain_write_spz(bad.encode(), 10, 3, 0, buf.ctypes.data, C.byref(lay), err, 256) == 1
    assert bad.encode() in err.value and not os.path.exists(bad)


def test_cli_lists_the_switch():
    out = subprocess.check_output([DRIVER, "--help"]).decode()
    assert "--exportSpz [0]" in out


def test_layout_sections_start_on_16_bytes():
    for n in GPU_SIZES:
        for degree in range(4):
            off, size, total = S.layout(n, degree)
            assert all(o % 16 == 0 for o in off) and total % 16 == 0 and off[0] == 0
            assert all(off[k + 1] >= off[k] + size[k] for k in range(5)) and total >= off[5] + size[5]
            assert sum(size) == (20 + 3 * S.DIM[degree]) * n


def test_restatement_on_explicit_values():
    nan = np.nan
    shN = np.zeros((5, 45), f32)
    shN[0, :4] = (0.5 / 128, -0.5 / 128, nan, 1.0)                            # x * 128 = +-0.5 rounds away from zero: q = 129 / 127
    shN[0, 9:12] = (0.5 / 128, -0.5 / 128, 8.0 / 128)                        # bucket 16: q = 129, 127 -> 128; q = 136 -> (136 + 8) / 16 * 16 = 144
    shN[1, 0] = (4.0 - 128) / 128                                            # q = 4: a bucket's half step rounds up, (4 + 4) / 8 * 8 = 8
    shN[1, 1] = -5.0                                                         # r clamps to -512, q = -384 -> byte 0
    model = {"pos": np.array([[3000, -3000, 1.0], [0.5 / 4096, -0.5 / 4096, nan], [np.inf, -1.5 / 4096, 2047.5], [0, 0, 0], [0, 0, 0]], f32),
             "sh0": np.array([[0, 10, -10], [nan, 1 / 0.15 / 255 * 0.5, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], f32), "shN": shN,
             "opacity": np.array([0, 30, -30, nan, 2.0], f32),
             "scale": np.array([[-10, 0, 6], [-11, -10 + 0.5 / 16, nan], [0, 0, 0], [0, 0, 0], [0, 0, 0]], f32),
             "rot": np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0.5, 0.5, 0.5, 0.5], [-2, 0, 0, 0], [0, 1, -1, 0]], f32)}
    p = S.pack(model, 3)
    fixed = lambda b: int.from_bytes(bytes(b), "little", signed=False)
    pos = [fixed(p["positions"][3 * k:3 * k + 3]) for k in range(9)]
    assert pos[0] == 0x7FFFFF and pos[1] == 0x800000 and pos[2] == 4096      # 3000 saturates at 2^23 - 1, -3000 at -2^23
    assert pos[3] == 1 and pos[4] == 0xFFFFFF and pos[5] == 0                # +-0.5 steps round away from zero; NaN -> 0
    assert pos[6] == 0 and pos[7] == 0xFFFFFE and pos[8] == 2047 * 4096 + 2048       # inf -> 0; -1.5 -> -2
    assert list(p["alphas"]) == [128, 255, 0, 0, 225]                        # 127.5 -> 128; a NaN logit -> 0; sigmoid(2) * 255 = 224.6
    assert list(p["colors"][:6]) == [128, 255, 0, 0, 128, 128]               # 127.5 rounds up; NaN -> 0; 127.5 + 0.5 = 128
    assert list(p["scales"][:6]) == [0, 160, 255, 0, 1, 0]                   # (s + 10) * 16: -16 and NaN -> 0, 0.5 -> 1
    comp = [fixed(p["rotations"][4 * k:4 * k + 4]) for k in range(5)]
    assert comp[0] == 3 << 30 and comp[1] == 3 << 30                         # identity and the zero quaternion: (0, 0, 0, 1), largest = w
    m = int(np.float32(511.0) * (np.float32(0.5) / np.float32(0.70710678)) + np.float32(0.5))
    assert comp[2] == (0 << 30) | (m << 20) | (m << 10) | m and m == 361     # all equal: the first index (x) is the largest
    assert comp[3] == (3 << 30) | (512 << 20) | (512 << 10) | 512            # -w alone: negated, so the zeros carry the sign bit (-0)
    assert comp[4] == (0 << 30) | ((512 | 511) << 20)                        # (x, y, z, w) = (1, -1, 0, 0) / sqrt 2: x largest, y negative at full scale
    sh = p["sh"].reshape(5, 45)
    assert list(sh[0, :4]) == [128, 128, 128, 255]                           # q = 129 -> 133 / 8 * 8 = 128; q = 127 -> 131 / 8 * 8 = 128; NaN -> 128; 1.0 -> 256 -> 255
    assert list(sh[0, 9:12]) == [128, 128, 144] and list(sh[1, :2]) == [8, 0] and sh[2, 0] == 128
    d = S.unpack(p, 3)
    assert d["pos"][0, 0] == f32(2047.999755859375) and d["pos"][0, 1] == -2048 and d["pos"][0, 2] == 1
    assert d["opacity"][1] == np.inf and d["opacity"][2] == -np.inf
    assert abs(float(d["opacity"][0]) - np.log(128 / 127)) < 5e-7             # a / (1 - a) near 1: three float32 roundings of 6e-8 each, log' = 1
    assert np.array_equal(d["rot"][0], [1, 0, 0, 0]) and np.array_equal(d["rot"][1], [1, 0, 0, 0])
    assert d["shN"][0, 3] == f32(127 / 128) and d["shN"][2, 0] == 0 and d["scale"][0, 2] == f32(255 / 16 - 10)
    assert not d["shN"][:, 3 * 15:].any() and not S.unpack(S.pack(model, 1), 1)["shN"][:, 9:].any()
