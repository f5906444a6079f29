"""The dataset reader (divshot_amd/gstrain/dataset_io.cpp) without a GPU, through libgsplyio.so's gstrain_dataset_* entry points: a
3-camera, 50-point COLMAP model written by tests/colmap_ref.py comes back field for field from .bin and from .txt; one camera record
is spelled out byte by byte; every malformed input is rejected with a message; and the same rejection inputs go through a stand-alone
host program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest
import colmap_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
SRC = os.path.join(ROOT, "divshot_amd", "gstrain")
W, H = 12, 8


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))       # host only: no HIP runtime behind it
    lib.gstrain_dataset_open.restype = C.c_void_p
    lib.gstrain_dataset_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_close.argtypes = [C.c_void_p]
    lib.gstrain_dataset_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.gstrain_dataset_camera.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.gstrain_dataset_image.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gstrain_dataset_read_image.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def model(seed=3):
    """3 cameras (one SIMPLE_PINHOLE, two PINHOLE, ids out of order), 3 images whose names sort differently from their ids, 50 points
    of which 2 have a non-finite coordinate"""
    r = np.random.default_rng(seed)
    cameras = [dict(id=7, model="PINHOLE", width=W, height=H, params=[10.25, 9.75, 6.125, 3.875]),
               dict(id=2, model="SIMPLE_PINHOLE", width=W, height=H, params=[11.5, 5.5, 4.25]),
               dict(id=9, model="PINHOLE", width=W, height=H, params=[1 / 3, 2 / 3, 6.0, 4.0])]
    images = []
    for k, (name, cam) in enumerate([("c_last.ppm", 7), ("a_first.ppm", 9), ("b_mid.jpg", 2)]):
        q = r.normal(size=4)
        q /= np.linalg.norm(q)
        images.append(dict(id=10 + k, q=q, t=r.normal(size=3) * 3, camera_id=cam, name=name,
                           points2d=[(float(r.uniform(0, W)), float(r.uniform(0, H)), int(r.integers(1, 50)) if j % 2 else -1) for j in range(k * 3)]))
    points = []
    for k in range(50):
        xyz = r.normal(size=3) * 5
        if k == 11:
            xyz[1] = np.nan
        if k == 30:
            xyz[2] = np.inf
        points.append(dict(id=100 + k, xyz=xyz, rgb=r.integers(0, 256, 3), error=float(r.uniform()),
                           track=[(10 + int(r.integers(0, 3)), int(r.integers(0, 9))) for _ in range(k % 4)]))
    pixels = {im["name"]: r.integers(0, 256, (H, W, 3), dtype=np.uint8) for im in images}
    masks = {"a_first.ppm": r.integers(0, 256, (H, W), dtype=np.uint8)}
    return cameras, images, points, pixels, masks


def read_all(lib, root):
    err = C.create_string_buffer(1024)
    h = lib.gstrain_dataset_open(root.encode(), err, 1024)
    assert h, err.value.decode()
    try:
        counts = (C.c_uint64 * 5)()
        assert lib.gstrain_dataset_counts(h, counts) == 0
        out = dict(counts=list(counts), cameras=[], images=[])
        for i in range(counts[0]):
            ints, prm = (C.c_uint64 * 4)(), (C.c_double * 4)()
            assert lib.gstrain_dataset_camera(h, i, ints, prm) == 0
            out["cameras"].append((list(ints), list(prm)))
        for i in range(counts[1]):
            ints, pose, rot, name = (C.c_uint64 * 3)(), (C.c_double * 7)(), (C.c_float * 9)(), C.create_string_buffer(256)
            assert lib.gstrain_dataset_image(h, i, ints, pose, rot, name, 256) == 0
            rgb, mask = np.zeros((H, W, 3), np.uint8), np.full((H, W), 77, np.uint8)
            assert lib.gstrain_dataset_read_image(h, i, rgb.ctypes.data, mask.ctypes.data, err, 1024) == 0, err.value.decode()
            out["images"].append(dict(ints=list(ints), pose=np.array(pose), rot=np.array(rot, np.float32).reshape(3, 3), name=name.value.decode(),
                                      rgb=rgb, mask=mask))
        xyz, rgb = np.zeros((counts[2], 3), np.float32), np.zeros((counts[2], 3), np.uint8)
        assert lib.gstrain_dataset_points(h, xyz.ctypes.data, rgb.ctypes.data) == 0
        out["xyz"], out["rgb"] = xyz, rgb
        return out
    finally:
        lib.gstrain_dataset_close(h)


def rejected(lib, root):
    """-> the message of a load that must fail: at open, or at the first image"""
    err = C.create_string_buffer(1024)
    h = lib.gstrain_dataset_open(str(root).encode(), err, 1024)
    if not h:
        assert err.value, "rejected without a message"
        return err.value.decode()
    try:
        counts = (C.c_uint64 * 5)()
        lib.gstrain_dataset_counts(h, counts)
        for i in range(counts[1]):
            rgb = np.zeros((64, 64, 3), np.uint8)
            if lib.gstrain_dataset_read_image(h, i, rgb.ctypes.data, None, err, 1024) != 0:
                assert err.value, "rejected without a message"
                return err.value.decode()
    finally:
        lib.gstrain_dataset_close(h)
    pytest.fail(f"{root} was accepted")


@pytest.mark.parametrize("binary,sub", [(True, "sparse/0"), (False, "sparse/0"), (True, "sparse"), (False, "sparse")])
def test_round_trip(lib, tmp_path, binary, sub):
    cameras, images, points, pixels, masks = model()
    CR.write_dataset(str(tmp_path), cameras, images, points, pixels, binary=binary, sparse_sub=sub, masks=masks)
    got = read_all(lib, str(tmp_path))
    assert got["counts"] == [3, 3, 48, 2, int(binary)]
    for (ints, prm), c in zip(got["cameras"], cameras):                      # file order
        p = c["params"]
        want = [p[0], p[0], p[1], p[2]] if c["model"] == "SIMPLE_PINHOLE" else list(p)
        assert ints == [c["id"], CR.MODEL_IDS[c["model"]], W, H]
        assert prm == [float(v) for v in want]                               # doubles, bit for bit (.txt: repr round-trips)
    by_name = sorted(images, key=lambda im: im["name"])
    assert [g["name"] for g in got["images"]] == ["a_first.ppm", "b_mid.jpg", "c_last.ppm"]
    for g, im in zip(got["images"], by_name):
        assert g["ints"][:2] == [im["id"], im["camera_id"]] and cameras[g["ints"][2]]["id"] == im["camera_id"]
        assert np.array_equal(g["pose"], np.concatenate([im["q"], im["t"]]).astype(np.float64))
        assert np.abs(g["rot"].astype(np.float64) - CR.qvec_to_rotmat(im["q"])).max() <= 2 ** -24
        assert np.array_equal(g["rgb"], pixels[im["name"]])                  # b_mid.jpg is found as images/b_mid.ppm
        want_mask = (masks[im["name"]] > 127).astype(np.uint8) if im["name"] in masks else np.ones((H, W), np.uint8)
        assert np.array_equal(g["mask"], want_mask)
    keep = [p for p in points if np.isfinite(p["xyz"]).all()]
    assert np.array_equal(got["xyz"], np.array([p["xyz"] for p in keep]).astype(np.float32))
    assert np.array_equal(got["rgb"], np.array([p["rgb"] for p in keep]).astype(np.uint8))


def test_sparse_0_wins_over_sparse_and_bin_over_txt(lib, tmp_path):
    cameras, images, points, pixels, _ = model()
    CR.write_dataset(str(tmp_path), cameras, images, points[:5], pixels, binary=True, sparse_sub="sparse")
    CR.write_dataset(str(tmp_path), cameras, images, points[:7], pixels, binary=False, sparse_sub="sparse/0")
    assert read_all(lib, str(tmp_path))["counts"][2:] == [7, 0, 0]
    CR.write_dataset(str(tmp_path), cameras, images, points[:9], pixels, binary=True, sparse_sub="sparse/0")
    assert read_all(lib, str(tmp_path))["counts"][2:] == [9, 0, 1]


def test_one_camera_record_spelled_out():
    """camera 5, PINHOLE (model id 1), 640x480, fx 500, fy 501.5, cx 320, cy 240.25: 4 + 4 + 8 + 8 + 4 * 8 bytes, little-endian"""
    want = bytes.fromhex("05000000" "01000000" "8002000000000000" "e001000000000000"
                         "0000000000407f40" "0000000000587f40" "0000000000007440" "0000000000086e40")
    assert CR.camera_record(dict(id=5, model="PINHOLE", width=640, height=480, params=[500.0, 501.5, 320.0, 240.25])) == want


def test_the_spelled_out_record_is_read(lib, tmp_path):
    cameras, images, points, _, _ = model()
    rec = bytes.fromhex("05000000" "01000000" "0c00000000000000" "0800000000000000"
                        "0000000000407f40" "0000000000587f40" "0000000000007440" "0000000000086e40")
    for im in images:
        im["camera_id"] = 5
    CR.write_dataset(str(tmp_path), cameras, images, points, {})
    with open(tmp_path / "sparse/0/cameras.bin", "wb") as f:
        f.write(struct.pack("<Q", 1) + rec)
    err = C.create_string_buffer(512)
    h = lib.gstrain_dataset_open(str(tmp_path).encode(), err, 512)
    assert h, err.value
    ints, prm = (C.c_uint64 * 4)(), (C.c_double * 4)()
    assert lib.gstrain_dataset_camera(h, 0, ints, prm) == 0
    lib.gstrain_dataset_close(h)
    assert list(ints) == [5, 1, 12, 8] and list(prm) == [500.0, 501.5, 320.0, 240.25]


def rejection_cases(base):
    """-> [(name, directory, words the message must contain)]: each a copy of a good capture with one defect"""
    cameras, images, points, pixels, masks = model()
    cases = []

    def fresh(name, binary=True):
        d = os.path.join(base, name)
        CR.write_dataset(d, cameras, images, points, pixels, binary=binary, masks=masks)
        return d

    for binary in (True, False):
        d = fresh(f"radial_{int(binary)}", binary)
        bad = [dict(cameras[0]), dict(id=2, model="SIMPLE_RADIAL", width=W, height=H, params=[10.0, 6.0, 4.0, 0.01]), cameras[2]]
        files = (CR.sparse_bin if binary else CR.sparse_txt)(bad, images, points)
        name = "cameras.bin" if binary else "cameras.txt"
        open(os.path.join(d, "sparse/0", name), "wb").write(files[name])
        cases.append((f"radial_{int(binary)}", d, ["SIMPLE_RADIAL", "undistort"]))
    good = CR.sparse_bin(cameras, images, points)
    for fname, data in good.items():
        for cut in sorted({0, 5, 8, 9, 30, len(data) // 3, len(data) // 2, len(data) - 9, len(data) - 1}):
            d = fresh(f"cut_{fname}_{cut}")
            open(os.path.join(d, "sparse/0", fname), "wb").write(data[:cut])
            cases.append((f"cut_{fname}_{cut}", d, [fname]))
    for fname in good:
        d = fresh(f"huge_{fname}")
        open(os.path.join(d, "sparse/0", fname), "wb").write(struct.pack("<Q", 2 ** 60) + good[fname][8:])
        cases.append((f"huge_{fname}", d, [fname, "count", "overruns"]))
    d = fresh("huge_track")                                                  # a 2^60 track length inside the first point record
    data = bytearray(good["points3D.bin"])
    data[8 + 43:8 + 51] = struct.pack("<Q", 2 ** 60)
    open(os.path.join(d, "sparse/0/points3D.bin"), "wb").write(bytes(data))
    cases.append(("huge_track", d, ["track", "overruns"]))
    d = fresh("unknown_camera")
    bad_images = [dict(im) for im in images]
    bad_images[1]["camera_id"] = 4
    open(os.path.join(d, "sparse/0/images.bin"), "wb").write(CR.sparse_bin(cameras, bad_images, points)["images.bin"])
    cases.append(("unknown_camera", d, ["unknown camera id 4"]))
    d = fresh("size_mismatch")
    CR.write_ppm(os.path.join(d, "images/a_first.ppm"), np.zeros((H, W + 1, 3), np.uint8))
    cases.append(("size_mismatch", d, [f"{W + 1}x{H}", f"{W}x{H}"]))
    d = fresh("short_ppm")
    raw = open(os.path.join(d, "images/a_first.ppm"), "rb").read()
    open(os.path.join(d, "images/a_first.ppm"), "wb").write(raw[:-7])
    cases.append(("short_ppm", d, ["truncated"]))
    d = fresh("jpeg_bytes")
    open(os.path.join(d, "images/a_first.ppm"), "wb").write(b"\xff\xd8\xff\xe0" + bytes(64))
    cases.append(("jpeg_bytes", d, ["PPM"]))
    d = fresh("missing_image")
    os.remove(os.path.join(d, "images/b_mid.ppm"))
    cases.append(("missing_image", d, ["b_mid", "PPM"]))
    d = fresh("no_images_dir")
    shutil.rmtree(os.path.join(d, "images"))
    cases.append(("no_images_dir", d, ["images/"]))
    d = fresh("no_sparse")
    shutil.rmtree(os.path.join(d, "sparse"))
    cases.append(("no_sparse", d, ["sparse"]))
    cases.append(("no_directory", os.path.join(base, "does_not_exist"), ["not a directory"]))
    return cases


@pytest.fixture(scope="module")
def rejections(tmp_path_factory):
    return rejection_cases(str(tmp_path_factory.mktemp("rejections")))


def test_malformed_inputs_are_rejected_with_a_message(lib, rejections):
    assert len(rejections) > 30
    for name, d, words in rejections:
        msg = rejected(lib, d)
        for w in words:
            assert w in msg, (name, w, msg)


def test_rejections_under_the_sanitizers_as_a_host_program(rejections, tmp_path):
    """dataset_check.cpp + dataset_io.cpp built with -fsanitize=address,undefined and run directly on every rejection directory and on one
    good capture: exit status 0, one line per directory, no sanitizer report. Nothing is loaded into Python."""
    exe = str(tmp_path / "dataset_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(SRC, "dataset_check.cpp"), os.path.join(SRC, "dataset_io.cpp")])
    good = str(tmp_path / "good")
    cameras, images, points, pixels, masks = model()
    CR.write_dataset(good, cameras, images, points, pixels, masks=masks)
    p = subprocess.run([exe, good] + [d for _, d, _ in rejections], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[0] == "ok 3 3 48 2" and len(lines) == 1 + len(rejections)
    assert all(l.startswith("rejected: ") and len(l) > 20 for l in lines[1:]), lines
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
