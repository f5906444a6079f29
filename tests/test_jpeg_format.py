"""Baseline JPEG without a GPU. The host decoder (divshot_amd/gstrain/jpeg_io.cpp, through libgsplyio.so's gstrain_jpeg_* entry points)
returns tests/jpeg_ref.py's coefficients, quantiser tables and geometry exactly on every fixture of tests/golden/jpeg/ (written once by
tests/golden/make_jpeg_fixtures.py with PIL; no test imports PIL). The integer pipeline that dvs_jpeg_reconstruct implements is held
against the fp64 inverse DCT of T.81 A.3.3 and against the recorded PIL pixels. Every malformed input is rejected with its words, and
the same inputs plus 300 single-byte mutations go through a stand-alone host program built with -fsanitize=address,undefined. The
loader's image path resolver is checked for its precedence rules.

Bounds. IDCT: the integer transform keeps 4 fractional bits after the column pass and a 13-bit table; the issue's bound is 1 level
against the fp64 transform, on every fixture sample and on 10 000 random blocks with coefficients in [-256, 255]. PIL: per fixture the
integer pipeline may differ from PIL by at most what the fp64-IDCT variant differs from PIL (both recorded in jpeg_expected.npz at
fixture time) plus 1 level."""
import ctypes as C
import glob
import os
import struct
import subprocess
import numpy as np
import pytest
import colmap_ref as CR
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
SRC = os.path.join(ROOT, "divshot_amd", "gstrain")
FIX = os.path.join(ROOT, "tests", "golden", "jpeg")
REJECTED = {"progressive": ["progressive", "SOF2", "baseline"], "adobe_rgb": ["RGB", "Adobe"]}
ACCEPTED = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FIX, "*.jpg")) if os.path.basename(f)[:-4] not in REJECTED)


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_expected.npz"))


@pytest.fixture(scope="module")
def frames():
    """jpeg_ref's coefficients of every accepted fixture, decoded once"""
    return {n: J.decode_coefficients(open(os.path.join(FIX, n + ".jpg"), "rb").read()) for n in ACCEPTED}


def _message(path):
    from divshot_amd import _lib
    with pytest.raises(_lib.DvsError) as e:
        _lib.jpeg_decode_coefficients(str(path))
    assert str(e.value), "rejected without a message"
    return str(e.value)


def test_fixture_set():
    want = {"c444_37x29", "c422_37x29", "c420_37x29", "c444_40x24", "c422_40x24", "c420_40x24", "c420_40x24_opt", "c420_40x24_rst3", "gray_37x29",
            "q100_37x29", "q5_37x29", "s_8x8", "s_1x1", "s_17x1", "dqt16_40x24"}
    assert set(ACCEPTED) == want
    for f in glob.glob(os.path.join(FIX, "*.jpg")):
        assert os.path.getsize(f) < 8192
    raw = open(os.path.join(FIX, "c420_40x24_rst3.jpg"), "rb").read()
    assert b"\xff\xdd\x00\x04\x00\x03" in raw and b"\xff\xd0" in raw                  # DRI 3 and a restart marker
    assert b"\xff\xdb\x00\x83\x10" in open(os.path.join(FIX, "dqt16_40x24.jpg"), "rb").read()   # a DQT segment with Pq = 1


@pytest.mark.parametrize("name", ACCEPTED)
def test_coefficients_tables_and_geometry_equal_the_restatement(frames, name):
    from divshot_amd import _lib
    desc, coef = _lib.jpeg_decode_coefficients(os.path.join(FIX, name + ".jpg"))
    f = frames[name]
    assert (desc.width, desc.height, desc.components, desc.hs, desc.vs) == (f.width, f.height, f.ncomp, f.hs[0], f.vs[0])
    for c in range(f.ncomp):
        assert (desc.blocks_w[c], desc.blocks_h[c], desc.offset[c]) == (f.bw[c], f.bh[c], f.offset[c]) and desc.offset[c] % 8 == 0
        assert np.array_equal(np.array(desc.quant[c][:], np.uint16), f.quant[c])
    assert coef.dtype == np.int16 and np.array_equal(coef, f.coef)
    assert np.abs(coef).max() > 0
    w, h = (int(v) for v in name.split("_")[1].split("x"))
    assert (f.width, f.height) == (w, h)
    assert f.bw[0] == -(-w // (8 * f.hs[0])) * f.hs[0] and f.bh[0] == -(-h // (8 * f.vs[0])) * f.vs[0]


def test_table_is_the_formula():
    import math
    assert J.IDCT_T.shape == (8, 8) and J.IDCT_T[0, 0] == 2896 and J.IDCT_T[1, 0] == 4017 and J.IDCT_T[7, 3] == -4017
    for u in range(8):
        for x in range(8):
            assert J.IDCT_T[u, x] == round(8192 * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16))


def test_integer_idct_within_one_level_of_fp64(frames):
    worst = 0
    for name, f in frames.items():
        assert J.clamped_count(f) == 0, name                                     # the clamp never bites on an encoder's stream
        for c in range(f.ncomp):
            F = J.dequantise(f, c)
            d = int(np.abs(J.idct_int(F) - J.idct_fp64(F)).max())
            worst = max(worst, d)
            assert d <= 1, (name, c, d)
    F = np.random.default_rng(1180).integers(-256, 256, (10000, 8, 8))
    d = np.abs(J.idct_int(F) - J.idct_fp64(F))
    print(f"integer vs fp64 IDCT: fixtures worst {worst}; 10 000 random blocks worst {d.max()}, {(d > 0).mean() * 100:.2f} % of samples differ")
    assert d.max() <= 1


def test_definition_is_overflow_free_at_the_extremes():
    """every int16 coefficient with every quantiser up to 65535: jpeg_ref asserts the int32 range at each intermediate"""
    r = np.random.default_rng(5)
    for q in (1, 255, 65535):
        for coef in (32767, -32768):
            f = J.synthetic_frame(16, 16, 2, 2, coef=coef, quant=q)
            J.reconstruct(f)
        signs = np.where(r.random(6 * 64) < 0.5, -32768, 32767)
        f = J.synthetic_frame(16, 16, 2, 2, coef=signs, quant=q)
        J.reconstruct(f)
    # the worst case of each pass: the signs of one table column / row
    for y in range(8):
        F = np.where(J.IDCT_T[:, y][:, None] * np.ones((1, 8)) < 0, J.F_MIN, J.F_MAX).astype(np.int64)
        J.idct_int(F)
        J.idct_int(np.where(np.outer(J.IDCT_T[:, y], J.IDCT_T[:, y]) < 0, J.F_MIN, J.F_MAX).astype(np.int64))


@pytest.mark.parametrize("name", ACCEPTED)
def test_pixels_reproduce_the_recorded_pil_differences(frames, expected, name):
    f = frames[name]
    got, got64 = J.reconstruct(f), J.reconstruct(f, "fp64")
    assert np.array_equal(got, expected[name + "/int"]) and np.array_equal(got64, expected[name + "/fp64"])
    pil = expected[name + "/pil"].astype(int)
    d_int, d_fp = int(np.abs(got.astype(int) - pil).max()), int(np.abs(got64.astype(int) - pil).max())
    print(f"{name}: |int - PIL| <= {d_int}, |fp64 - PIL| <= {d_fp}")
    assert d_int == int(expected[name + "/d_int"]) and d_fp == int(expected[name + "/d_fp64"])
    assert d_int <= d_fp + 1
    if f.ncomp == 1:
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_16_bit_dqt_decodes_like_its_8_bit_original(frames):
    a, b = frames["c420_40x24"], frames["dqt16_40x24"]
    assert np.array_equal(a.coef, b.coef) and all(np.array_equal(x, y) for x, y in zip(a.quant, b.quant))


def _segments(data):
    out, pos = [], 2
    while True:
        L = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((data[pos + 1], pos, pos + 2 + L))
        if data[pos + 1] == 0xDA:
            return out
        pos += 2 + L


def truncations(data):
    """about 40 cut points: inside every marker segment (its marker, its length, its body), and through the scan to the last byte"""
    cuts = {0, 1, 2, 3, len(data) - 1, len(data) - 2, len(data) - 3}
    for _, a, b in _segments(data):
        cuts |= {a + 1, a + 3, (a + b) // 2}
    scan = _segments(data)[-1][2]
    cuts |= {scan + k * (len(data) - scan) // 8 for k in range(8)}
    return sorted(c for c in cuts if 0 <= c < len(data))


@pytest.fixture(scope="module")
def hostile(tmp_path_factory):
    """-> [(name, file, words)]"""
    base = tmp_path_factory.mktemp("hostile")
    good = open(os.path.join(FIX, "c420_40x24_rst3.jpg"), "rb").read()
    cases = []

    def add(name, data, words):
        p = str(base / (name + ".jpg"))
        open(p, "wb").write(data)
        cases.append((name, p, words))

    cuts = truncations(good)
    assert 35 <= len(cuts) <= 50, len(cuts)
    for c in cuts:                                                           # (a cut right where a restart marker belongs reads as a missing marker)
        add(f"cut_{c}", good[:c], ["not a JPEG"] if c < 4 else [("truncated", "restart marker")])
    segs = _segments(good)
    m, a, b = next(s for s in segs if s[0] == 0xDB)
    add("length_ffff", good[:a + 2] + b"\xff\xff" + good[a + 4:], ["segment length 65535", "overruns"])
    m, a, b = next(s for s in segs if s[0] == 0xC4)
    bad = bytearray(good)
    bad[a + 5:a + 21] = bytes([255] * 16)                                    # 16 counts of 255: 4080 symbols in a segment of a few dozen bytes
    add("dht_counts", bytes(bad), ["Huffman", "counts overrun"])
    bad = bytearray(good)
    delta = 3 - bad[a + 5]                                                   # three codes of length 1, the total count unchanged
    bad[a + 5] = 3
    j = next(j for j in range(1, 16) if bad[a + 5 + j] >= delta)
    bad[a + 5 + j] -= delta
    add("dht_oversubscribed", bytes(bad), ["Huffman", "over-subscribed"])
    m, a, b = next(s for s in segs if s[0] == 0xC0)
    for name, at, val, words in (("precision_12", a + 4, 12, ["12-bit"]), ("four_components", a + 9, 4, ["4 components"]),
                                 ("height_0", None, None, ["size"]), ("sampling_4x1", a + 11, 0x41, ["sampling factors"])):
        bad = bytearray(good)
        if at is None:
            bad[a + 5:a + 7] = b"\x00\x00"
        else:
            bad[at] = val
        if name == "four_components":
            bad[a + 2:a + 4] = struct.pack(">H", 8 + 12)
            bad[b:b] = bytes([4, 0x11, 1])
        add(name, bytes(bad), words)
    bad = bytearray(good)
    bad[a + 5:a + 7] = struct.pack(">H", 65501)
    add("height_65501", bytes(bad), ["65501", "65500"])
    for name, marker, words in (("sof_arithmetic", 0xC9, ["arithmetic"]), ("sof_lossless", 0xC3, ["lossless"])):
        bad = bytearray(good)
        bad[a + 1] = marker
        add(name, bytes(bad), words)
    add("no_tables", good[:segs[0][1]] + b"".join(good[x:y] for mk, x, y in segs if mk not in (0xDB,)) + good[segs[-1][2]:], ["missing quantiser table"])
    add("no_huffman", good[:segs[0][1]] + b"".join(good[x:y] for mk, x, y in segs if mk not in (0xC4,)) + good[segs[-1][2]:], ["missing Huffman table"])
    scan = segs[-1][2]
    rst = good.index(b"\xff\xd0", scan)
    add("wrong_restart", good[:rst + 1] + b"\xd3" + good[rst + 2:], ["restart marker"])
    add("missing_restart", good[:rst] + good[rst + 2:], ["restart marker"])
    sa, sb = segs[-1][1], segs[-1][2]
    one = good[:sa] + b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0]) + good[sb:]
    add("multi_scan", one, ["multi-scan"])
    add("not_jpeg", b"P6\n4 4\n255\n" + bytes(48), ["not a JPEG"])
    add("empty", b"", ["not a JPEG"])
    return cases


def test_rejections_come_with_their_words(hostile):
    for name, words in REJECTED.items():
        msg = _message(os.path.join(FIX, name + ".jpg"))
        for w in words:
            assert w in msg, (name, w, msg)
    assert len(hostile) > 50
    for name, path, words in hostile:
        msg = _message(path)
        assert os.path.basename(path) in msg, (name, msg)
        for w in words:                                                     # a tuple: any one of its words
            assert any(v in msg for v in (w if isinstance(w, tuple) else (w,))), (name, w, msg)
        with pytest.raises(ValueError):                                     # the restatement rejects it too
            J.decode_coefficients(open(path, "rb").read())
    assert "does_not_exist" in _message(os.path.join(FIX, "does_not_exist.jpg"))


def test_a_huge_image_in_a_small_file_is_refused_before_anything_is_sized(tmp_path):
    good = bytearray(open(os.path.join(FIX, "c444_40x24.jpg"), "rb").read())
    m, a, b = next(s for s in _segments(bytes(good)) if s[0] == 0xC0)
    good[a + 5:a + 9] = struct.pack(">HH", 65500, 65500)
    p = tmp_path / "huge.jpg"
    p.write_bytes(bytes(good))
    assert "coefficients" in _message(p) and "cap" in _message(p)
    good[a + 5:a + 9] = struct.pack(">HH", 4000, 4000)
    p.write_bytes(bytes(good))
    assert "cannot hold" in _message(p)


def test_hostile_inputs_under_the_sanitizers_as_a_host_program(hostile, tmp_path):
    """jpeg_check.cpp + jpeg_io.cpp built with -fsanitize=address,undefined (the Makefile's jpeg_check_asan target) and run directly on all
    fixtures, all hostile files and 300 seeded single-byte mutations: exit status 0, one `ok ` / `rejected: ` line per file, no
    sanitizer report. Nothing is loaded into Python."""
    lib = str(tmp_path / "lib")
    subprocess.check_call(["make", "-C", SRC, "jpeg_check_asan", "LIBDIR=" + lib], stdout=subprocess.DEVNULL)
    exe = os.path.join(lib, "jpeg_check_asan")
    files = sorted(glob.glob(os.path.join(FIX, "*.jpg"))) + [p for _, p, _ in hostile]
    r = np.random.default_rng(300)
    sources = [open(os.path.join(FIX, n + ".jpg"), "rb").read() for n in ("c420_40x24_rst3", "c422_37x29", "gray_37x29", "dqt16_40x24")]
    for k in range(300):
        data = bytearray(sources[k % len(sources)])
        data[int(r.integers(2, len(data)))] = int(r.integers(0, 256))
        p = str(tmp_path / f"mut_{k:03d}.jpg")
        open(p, "wb").write(bytes(data))
        files.append(p)
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(files)
    assert all(l.startswith("ok ") or (l.startswith("rejected: ") and len(l) > 20) for l in lines), [l for l in lines if not l.startswith(("ok ", "rejected: "))]
    n_fix = len(glob.glob(os.path.join(FIX, "*.jpg")))
    assert sum(l.startswith("ok ") for l in lines[:n_fix]) == len(ACCEPTED)
    assert all(l.startswith("rejected: ") for l in lines[n_fix:n_fix + len(hostile)])
    mutated = lines[n_fix + len(hostile):]
    print(f"mutations: {sum(l.startswith('ok ') for l in mutated)} accepted, {sum(l.startswith('rejected') for l in mutated)} rejected")
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


# ---- the loader's path resolver ----
@pytest.fixture(scope="module")
def dlib():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))
    lib.gstrain_dataset_open.restype = C.c_void_p
    lib.gstrain_dataset_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_close.argtypes = [C.c_void_p]
    lib.gstrain_dataset_resolve_image.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_read_image.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def _capture(root, names):
    cameras = [dict(id=1, model="PINHOLE", width=40, height=24, params=[30.0, 30.0, 20.0, 12.0])]
    images = [dict(id=k + 1, q=np.array([1.0, 0, 0, 0]), t=np.zeros(3), camera_id=1, name=n) for k, n in enumerate(names)]
    points = [dict(id=1, xyz=np.array([0.0, 0.0, 2.0]), rgb=np.array([1, 2, 3]))]
    CR.write_dataset(str(root), cameras, images, points, {})


def _resolve(dlib, root, index=0):
    err = C.create_string_buffer(1024)
    h = dlib.gstrain_dataset_open(str(root).encode(), err, 1024)
    assert h, err.value
    try:
        path, jpeg = C.create_string_buffer(1024), C.c_int(-1)
        rc = dlib.gstrain_dataset_resolve_image(h, index, path, 1024, C.byref(jpeg), err, 1024)
        return (os.path.basename(path.value.decode()), jpeg.value) if rc == 0 else err.value.decode()
    finally:
        dlib.gstrain_dataset_close(h)


def test_resolver_precedence(dlib, tmp_path):
    jpg = open(os.path.join(FIX, "c420_40x24.jpg"), "rb").read()
    ppm = lambda p: CR.write_ppm(str(p), np.zeros((24, 40, 3), np.uint8))
    img = tmp_path / "images"
    _capture(tmp_path, ["a.jpg"])
    msg = _resolve(dlib, tmp_path)                                           # nothing exists: the present words and the names tried
    assert "a.jpg does not exist (nor a.ppm); JPEG and PNG are not decoded here, convert the images to PPM" in msg, msg
    assert all(n in msg for n in ("a.jpg, ", "a.jpeg", "a.JPG", "a.JPEG")), msg
    (img / "a.JPEG").write_bytes(jpg)
    assert _resolve(dlib, tmp_path) == ("a.JPEG", 1)
    (img / "a.JPG").write_bytes(jpg)
    assert _resolve(dlib, tmp_path) == ("a.JPG", 1)
    (img / "a.jpeg").write_bytes(jpg)
    assert _resolve(dlib, tmp_path) == ("a.jpeg", 1)
    ppm(img / "a.ppm")
    assert _resolve(dlib, tmp_path) == ("a.ppm", 0)                          # .ppm is retried before the JPEG names, as before
    (img / "a.jpg").write_bytes(jpg)
    assert _resolve(dlib, tmp_path) == ("a.jpg", 1)                          # the named file exists: it wins, a JPEG by its extension
    for k, (name, want) in enumerate([("b.JpEg", 1), ("c.ppm", 0), ("d.png", 0), ("e", 0)]):
        root = tmp_path / f"named_{k}"
        _capture(root, [name])
        (root / "images" / name).write_bytes(jpg)                           # any other existing file is read as PPM, whatever it holds
        assert _resolve(dlib, root) == (name, want)
    root = tmp_path / "ppm_named_jpeg_present"
    _capture(root, ["f.ppm"])
    (root / "images" / "f.jpg").write_bytes(jpg)
    assert _resolve(dlib, root) == ("f.jpg", 1)                              # an absent .ppm name finds the capture's .jpg


def test_read_image_still_reads_ppm_only(dlib, tmp_path):
    """the host-side read_image is as it was: a JPEG is the loader's to decode (resolve_image says which file is one)"""
    _capture(tmp_path, ["a.jpg"])
    (tmp_path / "images" / "a.jpg").write_bytes(open(os.path.join(FIX, "c420_40x24.jpg"), "rb").read())
    err = C.create_string_buffer(1024)
    h = dlib.gstrain_dataset_open(str(tmp_path).encode(), err, 1024)
    rgb = np.zeros((24, 40, 3), np.uint8)
    assert dlib.gstrain_dataset_read_image(h, 0, rgb.ctypes.data, None, err, 1024) != 0
    dlib.gstrain_dataset_close(h)
    assert b"a.jpg: not a binary PPM (P6) file; JPEG and PNG are not decoded here, convert the images to PPM" in err.value
