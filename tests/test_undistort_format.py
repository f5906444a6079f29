"""The definition of dvs_undistort_view without a GPU (tests/undistort_ref.py) and the reader of distorted cameras.
  * zero coefficients reproduce the source byte for byte, every pixel valid;
  * the float32 / 1/32-pixel restatement against an independent float64 implementation of COLMAP's forward models with float64
    bilinear resampling, on a smooth image (adjacent pixels differ by at most 16 levels): at most 1 level apart wherever both call the
    pixel valid — the coordinate is quantised by at most 1/64 pixel per axis, worth at most 0.25 level per axis at that slope, and
    each side rounds to a whole level on its own (0.5 each): 1.5 in all, so two integers differ by at most 1. Validity may differ only
    where the float64 coordinate lies within 1/32 pixel of the source's border;
  * the fp32 (u + du, v + dv) pushed back through a float64 Newton inverse returns (u, v) to 1e-5, for all three models;
  * tests/golden/undistort_37x29.npz pins the restatement itself;
  * the descriptor the library fills (dvs_undistort_desc_from_colmap, host code) equals the restatement's, and what it refuses;
  * the reader: gstrain_dataset_open_ex with flag bit 0 returns fx, fy, cx, cy and k1, k2, p1, p2 of SIMPLE_RADIAL, RADIAL and OPENCV
    cameras from .bin and from .txt; gstrain_dataset_open still refuses them; OPENCV_FISHEYE is refused under both; truncated parameter
    blocks are refused with a message; and the same inputs go through dataset_check --distorted built with
    -fsanitize=address,undefined as a stand-alone host program (nothing is loaded into Python)."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
SRC = os.path.join(ROOT, "divshot_amd", "gstrain")
W, H = 12, 8

# (model id, COLMAP parameters) at 37x29: barrel, pincushion, RADIAL with k1 and k2 of opposite sign, OPENCV with tangential terms
CASES = [(2, [30.0, 18.5, 14.5, -0.2]), (2, [30.0, 18.5, 14.5, 0.3]), (3, [31.0, 17.0, 15.25, 0.25, -0.1]),
         (4, [31.5, 29.25, 20.75, 12.5, 0.21, -0.06, 0.013, -0.009])]


@pytest.mark.parametrize("shape", [(37, 29), (1, 1)])
def test_zero_coefficients_are_the_identity(shape):
    w, h = shape
    src = np.random.default_rng(5).integers(0, 256, (3, h, w), dtype=np.uint8)
    for model, params in ((2, [30.0, w / 2, h / 2, 0.0]), (3, [27.3, 0.31 * w, 0.77 * h, 0.0, 0.0]), (4, [31.7, 28.9, 0.4 * w, 0.6 * h, 0.0, 0.0, 0.0, 0.0])):
        dst, mask, invalid = U.undistort(src, U.descriptor(model, params, w, h))
        assert np.array_equal(dst, src) and (mask == 1.0).all() and invalid == 0, (model, shape)
    src_mask = np.random.default_rng(6).integers(0, 2, (h, w), dtype=np.uint8)
    _, mask, _ = U.undistort(src, U.descriptor(2, [30.0, w / 2, h / 2, 0.0], w, h), src_mask)
    assert np.array_equal(mask, src_mask.astype(np.float32))


@pytest.mark.parametrize("model,params", CASES)
def test_against_float64_colmap_models(model, params):
    w, h = 37, 29
    src = U.smooth_image(w, h, 3, seed=model)
    dst, mask, invalid = U.undistort(src, U.descriptor(model, params, w, h))
    xs, ys = U.source_coordinates64(model, params, w, h)
    valid = mask == 1.0
    assert invalid == int((~valid).sum())
    both = 0
    for p in range(3):
        ref, valid64 = U.resample64(src[p], xs, ys)
        ok = valid & valid64
        both = int(ok.sum())
        err = np.abs(dst[p].astype(int) - ref.astype(int))[ok]
        print(f"model {model} plane {p}: {both} pixels valid in both, max |difference| {err.max()} levels, {int((valid != valid64).sum())} validity differences")
        assert err.max() <= 1
        near = (np.abs(xs) <= 1 / 32) | (np.abs(xs - (w - 1)) <= 1 / 32) | (np.abs(ys) <= 1 / 32) | (np.abs(ys - (h - 1)) <= 1 / 32)
        assert near[valid != valid64].all()
        assert (dst[p][~valid] == 0).all()
    assert both > w * h // 2


@pytest.mark.parametrize("model,params", CASES)
def test_round_trip_through_a_float64_newton_inverse(model, params):
    w, h = 37, 29
    desc = U.descriptor(model, params, w, h)
    _, _, ud, vd = U.source_coordinates(desc)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    fx, fy, cx, cy = U.split_params(model, params)[:4]
    u, v = (x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy
    assert np.hypot(u, v).max() < 0.9                                        # every case's model is monotonic along a ray out to there: Newton converges
    bu, bv = U.undistort_point64(model, params, ud.astype(np.float64), vd.astype(np.float64))
    err = max(np.abs(bu - u).max(), np.abs(bv - v).max())
    print(f"model {model}: round-trip error {err:.3e} over all {w * h} pixels")
    assert err <= 1e-5


def test_golden_pins_the_restatement():
    g = np.load(U.GOLDEN)
    want = U.golden_case()
    assert sorted(g.files) == sorted(want)
    for k in want:
        assert np.array_equal(g[k], want[k]), k
    desc = U.descriptor(U.GOLDEN_MODEL, list(g["params"]), 37, 29)
    assert g["desc"].dtype == np.float32 and np.array_equal(g["desc"], np.array([desc[n] for n in U.FIELDS], np.float32))
    assert desc["fx"] != desc["fy"] and all(desc[n] != 0 for n in ("k1", "k2", "p1", "p2"))
    assert 0 < int(g["invalid"]) < 37 * 29 // 2 and int(g["invalid"]) == int((g["mask"] == 0).sum())
    assert (g["mask_with_source_mask"] <= g["mask"]).all() and g["mask_with_source_mask"].sum() < g["mask"].sum()


def test_the_library_fills_the_same_descriptor():
    from divshot_amd import _lib
    for model, params in CASES + [(2, [1 / 3, 2 / 3, 0.1, 1e-3]), (4, [1234.567, 1230.1, 959.5, 540.25, -0.11, 0.017, 1e-4, -3e-4])]:
        d = _lib.undistort_desc(model, params, 1920, 1080)
        want = U.descriptor(model, params, 1920, 1080)
        assert (d.width, d.height) == (1920, 1080)
        for n in U.FIELDS:
            assert np.float32(getattr(d, n)).tobytes() == want[n].tobytes(), (model, n)
    out = _lib.UndistortDesc()
    call = _lib.lib.dvs_undistort_desc_from_colmap
    good = (C.c_double * 8)(30.0, 30.0, 6.0, 4.0, 0.1, 0.0, 0.0, 0.0)
    assert call(4, good, 12, 8, C.byref(out)) == 0
    for model in (0, 1, 5, 6, -1):
        assert call(model, good, 12, 8, C.byref(out)) == 1
    for w, h in ((0, 8), (12, 0), (65537, 8), (12, 65537)):
        assert call(4, good, w, h, C.byref(out)) == 1
    assert call(4, good, 65536, 65536, C.byref(out)) == 0
    assert call(4, None, 12, 8, C.byref(out)) == 1 and call(4, good, 12, 8, None) == 1
    for k, v in ((0, 0.0), (0, -30.0), (1, 0.0), (0, np.nan), (2, np.inf), (4, np.nan), (7, -np.inf), (0, 1e-60), (5, 1e60)):
        bad = (C.c_double * 8)(*good)
        bad[k] = v
        assert call(4, bad, 12, 8, C.byref(out)) == 1, (k, v)


# ---- the reader ----
@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))
    lib.gstrain_dataset_open.restype = C.c_void_p
    lib.gstrain_dataset_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_open_ex.restype = C.c_void_p
    lib.gstrain_dataset_open_ex.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_int]
    lib.gstrain_dataset_close.argtypes = [C.c_void_p]
    lib.gstrain_dataset_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.gstrain_dataset_camera.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.gstrain_dataset_camera_distortion.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


CAMERAS = [dict(id=3, model="SIMPLE_RADIAL", width=W, height=H, params=[10.25, 6.125, 3.875, -0.0625]),
           dict(id=1, model="RADIAL", width=W, height=H, params=[11.5, 5.5, 4.25, 0.1, -1 / 3]),
           dict(id=8, model="OPENCV", width=W, height=H, params=[1 / 3, 2 / 3, 6.0, 4.0, 0.3, -0.07, 1e-3, -2e-3]),
           dict(id=5, model="PINHOLE", width=W, height=H, params=[10.0, 9.0, 6.0, 4.0])]
EXPECTED = [([10.25, 10.25, 6.125, 3.875], [-0.0625, 0.0, 0.0, 0.0]), ([11.5, 11.5, 5.5, 4.25], [0.1, -1 / 3, 0.0, 0.0]),
            ([1 / 3, 2 / 3, 6.0, 4.0], [0.3, -0.07, 1e-3, -2e-3]), ([10.0, 9.0, 6.0, 4.0], [0.0, 0.0, 0.0, 0.0])]


def capture(root, cameras=CAMERAS, binary=True):
    r = np.random.default_rng(1)
    images = [dict(id=k + 1, q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.1 * k, 0.0, 0.0]), camera_id=c["id"], name=f"v{k}.ppm") for k, c in enumerate(cameras)]
    points = [dict(id=k + 1, xyz=r.normal(size=3), rgb=r.integers(0, 256, 3)) for k in range(9)]
    pixels = {im["name"]: r.integers(0, 256, (H, W, 3), dtype=np.uint8) for im in images}
    CR.write_dataset(str(root), cameras, images, points, pixels, binary=binary)
    return str(root)


def open_message(lib, root, flags=None):
    err = C.create_string_buffer(1024)
    h = lib.gstrain_dataset_open(root.encode(), err, 1024) if flags is None else lib.gstrain_dataset_open_ex(root.encode(), flags, err, 1024)
    if h:
        lib.gstrain_dataset_close(h)
        return None
    assert err.value, "rejected without a message"
    return err.value.decode()


@pytest.mark.parametrize("binary", [True, False])
def test_distorted_cameras_are_read_with_the_flag(lib, tmp_path, binary):
    root = capture(tmp_path, binary=binary)
    err = C.create_string_buffer(1024)
    h = lib.gstrain_dataset_open_ex(root.encode(), 1, err, 1024)
    assert h, err.value.decode()
    try:
        counts = (C.c_uint64 * 5)()
        assert lib.gstrain_dataset_counts(h, counts) == 0 and list(counts)[:2] == [4, 4]
        for i, (cam, (want_prm, want_k)) in enumerate(zip(CAMERAS, EXPECTED)):
            ints, prm, k = (C.c_uint64 * 4)(), (C.c_double * 4)(), (C.c_double * 4)(9, 9, 9, 9)
            assert lib.gstrain_dataset_camera(h, i, ints, prm) == 0 and lib.gstrain_dataset_camera_distortion(h, i, k) == 0
            assert list(ints) == [cam["id"], {"PINHOLE": 1, **U.MODEL_IDS}[cam["model"]], W, H]
            assert list(prm) == want_prm and list(k) == want_k           # doubles, bit for bit (.txt: repr round-trips)
        assert lib.gstrain_dataset_camera_distortion(h, 4, k) == 1 and lib.gstrain_dataset_camera_distortion(h, 0, None) == 1
    finally:
        lib.gstrain_dataset_close(h)


@pytest.mark.parametrize("binary", [True, False])
def test_without_the_flag_they_are_refused_as_before(lib, tmp_path, binary):
    for k in range(3):
        root = capture(tmp_path / f"c{k}", [CAMERAS[k], CAMERAS[3]], binary)
        for flags in (None, 0, 2):
            msg = open_message(lib, root, flags)
            assert msg and f"camera model {CAMERAS[k]['model']} is not supported: only SIMPLE_PINHOLE and PINHOLE are; undistort the capture first " \
                           "(colmap image_undistorter), as the lineage requires" in msg, msg
        assert open_message(lib, root, 1) is None
    assert open_message(lib, capture(tmp_path / "pinhole", [CAMERAS[3]], binary)) is None


def fisheye_capture(root, binary):
    capture(root, [CAMERAS[3]], binary)
    if binary:
        rec = struct.pack("<IiQQ", 5, 5, W, H) + struct.pack("<8d", 10.0, 10.0, 6.0, 4.0, 0.01, 0.0, 0.0, 0.0)
        open(os.path.join(root, "sparse/0/cameras.bin"), "wb").write(struct.pack("<Q", 1) + rec)
    else:
        open(os.path.join(root, "sparse/0/cameras.txt"), "w").write(f"5 OPENCV_FISHEYE {W} {H} 10.0 10.0 6.0 4.0 0.01 0.0 0.0 0.0\n")
    return str(root)


@pytest.mark.parametrize("binary", [True, False])
def test_fisheye_is_refused_under_both(lib, tmp_path, binary):
    root = fisheye_capture(tmp_path, binary)
    msg = open_message(lib, root)
    assert msg and "OPENCV_FISHEYE" in msg and "only SIMPLE_PINHOLE and PINHOLE are" in msg
    msg = open_message(lib, root, 1)
    assert msg and "OPENCV_FISHEYE" in msg and "undistort" in msg
    for accepted in ("SIMPLE_RADIAL", "RADIAL", "OPENCV"):
        assert accepted in msg.replace("OPENCV_FISHEYE", "")


def truncated_cases(base):
    """-> [(directory, words of the message)]: distorted captures whose parameter block is cut short or not finite"""
    cases = []
    for k in range(3):
        good = CR.sparse_bin([CAMERAS[k]], [], [])["cameras.bin"]
        for cut in (1, 8, 9, 17):                                            # inside the last coefficient .. inside the one before
            root = capture(os.path.join(base, f"cut_{k}_{cut}"), [CAMERAS[k]])
            open(os.path.join(root, "sparse/0/cameras.bin"), "wb").write(good[:-cut])
            cases.append((root, ["cameras.bin", "truncated"]))
        root = capture(os.path.join(base, f"txt_short_{k}"), [CAMERAS[k]], binary=False)
        line = CR.sparse_txt([CAMERAS[k]], [], [])["cameras.txt"].decode().splitlines()[-1]
        open(os.path.join(root, "sparse/0/cameras.txt"), "w").write(" ".join(line.split()[:-1]) + "\n")
        cases.append((root, ["cameras.txt", CAMERAS[k]["model"], "parameters"]))
        root = capture(os.path.join(base, f"nan_{k}"), [dict(CAMERAS[k], params=CAMERAS[k]["params"][:-1] + [float("nan")])])
        cases.append((root, ["distortion coefficient", "finite"]))
    return cases


@pytest.fixture(scope="module")
def truncated(tmp_path_factory):
    return truncated_cases(str(tmp_path_factory.mktemp("truncated")))


def test_truncated_parameter_blocks_are_refused_with_a_message(lib, truncated):
    assert len(truncated) == 18
    for root, words in truncated:
        msg = open_message(lib, root, 1)
        assert msg, root
        for w in words:
            assert w in msg, (root, w, msg)


def test_the_reader_under_the_sanitizers_as_a_host_program(truncated, tmp_path):
    """dataset_check.cpp + dataset_io.cpp built with -fsanitize=address,undefined; run with --distorted on a good distorted capture (.bin
    and .txt), on a fisheye one and on the truncated ones, and without the argument on the good one: exit status 0, one line per
    directory, no sanitizer report"""
    exe = str(tmp_path / "dataset_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(SRC, "dataset_check.cpp"), os.path.join(SRC, "dataset_io.cpp")])
    good, good_txt, fish = capture(tmp_path / "good"), capture(tmp_path / "good_txt", binary=False), fisheye_capture(tmp_path / "fish", True)
    p = subprocess.run([exe, "--distorted", good, good_txt, fish] + [d for d, _ in truncated], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[:2] == ["ok 4 4 9 0", "ok 4 4 9 0"] and len(lines) == 3 + len(truncated), lines
    assert all(l.startswith("rejected: ") and len(l) > 20 for l in lines[2:]), lines
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    p = subprocess.run([exe, good], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("rejected: ") and "SIMPLE_RADIAL" in p.stdout and "only SIMPLE_PINHOLE and PINHOLE are" in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
