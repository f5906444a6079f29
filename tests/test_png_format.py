"""PNG without a GPU. The host half (divshot_amd/gstrain/png_io.cpp, through libgsplyio.so's gstrain_png_* entry points) returns
tests/png_ref.py's descriptor and filtered scanlines exactly for every legal colour type / bit depth pair, however the IDAT stream is
cut into chunks; every refusal of png_io.hpp's list is made, each recognised by a distinctive word of its message; the loader's image
resolver tells PNG apart and keeps its precedence, the old entry point answers as before, and the mask lookup order holds. Nothing
here has a tolerance: PNG is lossless and every comparison is `==`."""
import ctypes as C
import os
import struct
import zlib
import numpy as np
import pytest
import colmap_ref as CR
import png_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
W, H = 37, 29


def _decode(data):
    from divshot_amd import _lib
    return _lib.png_decode_filtered(data)


def _message(data):
    from divshot_amd import _lib
    with pytest.raises(_lib.DvsError) as e:
        _lib.png_decode_filtered(bytes(data))
    assert str(e.value), "refused without a message"
    return str(e.value)


def _case(ctype, depth, seed=0):
    """(stream, palette, tRNS) of a 37x29 picture of that pair: random filtered bytes, the filters cycling 0..4"""
    rng = np.random.default_rng(100 * ctype + depth + seed)
    stream = P.random_stream(rng, W, H, depth, ctype, filters=[(y + seed) % 5 for y in range(H)])
    palette = rng.integers(0, 256, (min(1 << depth, 200), 3), dtype=np.uint8) if ctype == 3 else None
    trns = {3: bytes(rng.integers(0, 256, 2, dtype=np.uint8)), 0: struct.pack(">H", 1), 2: struct.pack(">HHH", 1, 2, 3)}.get(ctype)
    return stream, palette, trns


@pytest.mark.parametrize("split", [None, 1], ids=["one_idat", "1_byte_idats"])
@pytest.mark.parametrize("ctype,depth", P.PAIRS)
def test_descriptor_and_filtered_bytes_equal_the_reference(ctype, depth, split):
    stream, palette, trns = _case(ctype, depth)
    data = P.write_png(W, H, depth, ctype, stream, palette=palette, trns=trns, split=split,
                       extra_before_idat=P.chunk(b"gAMA", struct.pack(">I", 45455)) + P.chunk(b"acTL", struct.pack(">II", 1, 0)))
    if split == 1:
        assert data.count(b"IDAT") >= len(zlib.compress(stream.tobytes(), 6))        # cut inside the zlib header too
    ref = P.decode_filtered(data)
    desc, filtered = _decode(data)
    assert (desc.width, desc.height, desc.bit_depth, desc.color_type) == (W, H, depth, ctype) == (ref.width, ref.height, ref.depth, ref.ctype)
    assert np.array_equal(filtered, ref.filtered) and np.array_equal(filtered, stream)
    assert filtered.size == H * (1 + P.row_bytes(W, depth, ctype))
    assert np.array_equal(np.ctypeslib.as_array(desc.palette).reshape(256, 4), ref.palette)
    assert desc.has_key == (1 if ctype in (0, 2) else 0)
    if desc.has_key:
        assert list(desc.key)[:len(ref.key)] == ref.key


def test_a_file_on_disk_and_trailing_ancillary_chunks(tmp_path):
    stream, _, _ = _case(2, 8)
    data = P.write_png(W, H, 8, 2, stream)
    data = data[:-12] + P.chunk(b"tEXt", b"k\0v") + P.chunk(b"IEND")
    (tmp_path / "a.png").write_bytes(data)
    desc, filtered = _decode(str(tmp_path / "a.png"))
    assert desc.has_key == 0 and np.array_equal(filtered, stream)
    assert np.array_equal(np.ctypeslib.as_array(desc.palette).reshape(256, 4), np.repeat([[0, 0, 0, 255]], 256, 0))
    assert "cannot open" in _message_path(str(tmp_path / "absent.png"))


def _message_path(path):
    from divshot_amd import _lib
    with pytest.raises(_lib.DvsError) as e:
        _lib.png_decode_filtered(path)
    return str(e.value)


def _parts(ctype=2, depth=8, w=5, h=3):
    rng = np.random.default_rng(3)
    stream = P.random_stream(rng, w, h, depth, ctype)
    return stream, zlib.compress(stream.tobytes())


def _file(head, *chunks):
    return P.SIG + head + b"".join(chunks)


IEND = P.chunk(b"IEND")
PLTE3 = P.chunk(b"PLTE", bytes(range(9)))


def _refusals():
    stream, z = _parts()
    idat = P.chunk(b"IDAT", z)
    good = P.ihdr(5, 3, 8, 2)
    pal_stream, pal_z = _parts(3, 8)
    pal_idat = P.chunk(b"IDAT", pal_z)
    cases = {
        "signature": (b"\x88" + (P.SIG + good + idat + IEND)[1:], "signature"),
        "crc": (_file(good, P.chunk(b"IDAT", z, crc=(zlib.crc32(b"IDAT" + z) ^ 1) & 0xFFFFFFFF), IEND), "CRC"),
        "first_chunk": (P.SIG + P.chunk(b"gAMA", struct.pack(">I", 1)) + good + idat + IEND, "not IHDR"),
        "pair_rgb4": (_file(P.ihdr(5, 3, 4, 2), idat, IEND), "illegal"),
        "pair_palette16": (_file(P.ihdr(5, 3, 16, 3), idat, IEND), "illegal"),
        "pair_type5": (_file(P.ihdr(5, 3, 8, 5), idat, IEND), "illegal"),
        "pair_depth3": (_file(P.ihdr(5, 3, 3, 0), idat, IEND), "illegal"),
        "side_zero": (_file(P.ihdr(5, 0, 8, 2), idat, IEND), "image size"),
        "side_65501": (_file(P.ihdr(65501, 3, 8, 2), idat, IEND), "image size"),
        "adam7": (_file(P.ihdr(5, 3, 8, 2, interlace=1), idat, IEND), "Adam7"),
        "compression": (_file(P.ihdr(5, 3, 8, 2, compression=1), idat, IEND), "compression method"),
        "filter_method": (_file(P.ihdr(5, 3, 8, 2, filter_method=1), idat, IEND), "filter method"),
        "critical_chunk": (_file(good, P.chunk(b"ABCD", b"x"), idat, IEND), "critical"),
        "no_plte": (_file(P.ihdr(5, 3, 8, 3), pal_idat, IEND), "without a PLTE"),
        "plte_not_3n": (_file(P.ihdr(5, 3, 8, 3), P.chunk(b"PLTE", bytes(10)), pal_idat, IEND), "multiple of 3"),
        "plte_257": (_file(P.ihdr(5, 3, 8, 3), P.chunk(b"PLTE", bytes(771)), pal_idat, IEND), "more than 256"),
        "trns_longer_than_plte": (_file(P.ihdr(5, 3, 8, 3), PLTE3, P.chunk(b"tRNS", bytes(4)), pal_idat, IEND), "longer than the palette"),
        "trns_length_type2": (_file(good, P.chunk(b"tRNS", bytes(2)), idat, IEND), "wrong length"),
        "trns_length_type0": (_file(P.ihdr(5, 3, 8, 0), P.chunk(b"tRNS", bytes(6)), idat, IEND), "wrong length"),
        "trns_on_type4": (_file(P.ihdr(5, 3, 8, 4), P.chunk(b"tRNS", bytes(2)), idat, IEND), "alpha channel"),
        "trns_on_type6": (_file(P.ihdr(5, 3, 8, 6), P.chunk(b"tRNS", bytes(2)), idat, IEND), "alpha channel"),
        "idat_not_consecutive": (_file(good, P.chunk(b"IDAT", z[:5]), P.chunk(b"tEXt", b"k\0v"), P.chunk(b"IDAT", z[5:]), IEND), "not consecutive"),
        "no_idat": (_file(good, IEND), "no IDAT"),
        "no_iend": (_file(good, idat), "IEND"),
        "truncated_in_idat": ((P.SIG + good + idat + IEND)[:60], "truncated"),
        "inflate_error": (_file(good, P.chunk(b"IDAT", z[:2] + b"\x07" + z[3:]), IEND), "inflate error"),
        "inflate_incomplete": (_file(good, P.chunk(b"IDAT", z[:-6]), IEND), "inflate error"),
        "stream_shorter": (_file(good, P.chunk(b"IDAT", zlib.compress(stream.tobytes()[:-1])), IEND), "shorter"),
        "stream_longer": (_file(good, P.chunk(b"IDAT", zlib.compress(stream.tobytes() + b"\0")), IEND), "longer"),
        "stream_far_shorter": (_file(P.ihdr(60000, 60000, 16, 6), idat, IEND), "shorter"),
    }
    five = stream.copy()
    five[16] = 5                                                             # the filter byte of row 1: offset y * (1 + rowbytes)
    cases["filter_byte_5"] = (_file(good, P.chunk(b"IDAT", zlib.compress(five.tobytes())), IEND), "filter type 5")
    return cases


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_by_name(name):
    data, word = REFUSALS[name]
    msg = _message(data)
    assert word in msg, msg


def test_the_good_file_of_the_refusal_cases_is_accepted():
    stream, z = _parts()
    desc, filtered = _decode(_file(P.ihdr(5, 3, 8, 2), P.chunk(b"IDAT", z), IEND))
    assert np.array_equal(filtered, stream)


def test_every_truncation_is_a_refusal():
    stream, z = _parts()
    data = _file(P.ihdr(5, 3, 8, 2), P.chunk(b"IDAT", z), IEND)
    for n in range(len(data)):
        assert _message(data[:n])


# ---- the resolver ----
@pytest.fixture(scope="module")
def dlib():
    lib = C.CDLL(os.path.join(LIB, "libgsplyio.so"))
    lib.gstrain_dataset_open.restype = C.c_void_p
    lib.gstrain_dataset_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.gstrain_dataset_close.argtypes = [C.c_void_p]
    for name in ("gstrain_dataset_resolve_image", "gstrain_dataset_resolve_image_kind", "gstrain_dataset_resolve_mask"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def _capture(root, names):
    cameras = [dict(id=1, model="PINHOLE", width=40, height=24, params=[30.0, 30.0, 20.0, 12.0])]
    images = [dict(id=k + 1, q=np.array([1.0, 0, 0, 0]), t=np.zeros(3), camera_id=1, name=n) for k, n in enumerate(names)]
    points = [dict(id=1, xyz=np.array([0.0, 0.0, 2.0]), rgb=np.array([1, 2, 3]))]
    CR.write_dataset(str(root), cameras, images, points, {})


def _resolve(dlib, root, call="gstrain_dataset_resolve_image_kind", index=0):
    err = C.create_string_buffer(1024)
    h = dlib.gstrain_dataset_open(str(root).encode(), err, 1024)
    assert h, err.value
    try:
        path, kind = C.create_string_buffer(1024), C.c_int(-1)
        rc = getattr(dlib, call)(h, index, path, 1024, C.byref(kind), err, 1024)
        return (os.path.relpath(path.value.decode(), str(root)) if path.value else "", kind.value) if rc == 0 else err.value.decode()
    finally:
        dlib.gstrain_dataset_close(h)


PPM, JPEG, PNG = 0, 1, 2


def test_resolver_kinds_and_precedence(dlib, tmp_path):
    img = tmp_path / "images"
    _capture(tmp_path, ["a.jpg"])
    msg = _resolve(dlib, tmp_path)
    assert "a.jpg does not exist (nor a.ppm); JPEG and PNG are not decoded here, convert the images to PPM" in msg and "a.png or a.PNG" in msg, msg
    (img / "a.PNG").write_bytes(b"x")
    assert _resolve(dlib, tmp_path) == ("images/a.PNG", PNG)
    (img / "a.png").write_bytes(b"x")
    assert _resolve(dlib, tmp_path) == ("images/a.png", PNG)                 # .png is tried before .PNG
    (img / "a.JPEG").write_bytes(b"x")
    assert _resolve(dlib, tmp_path) == ("images/a.JPEG", JPEG)               # every JPEG name is tried before the PNG names
    (img / "a.ppm").write_bytes(b"x")
    assert _resolve(dlib, tmp_path) == ("images/a.ppm", PPM)                 # and .ppm before those, as ever
    for k, (name, want) in enumerate([("b.PnG", PNG), ("c.png", PNG), ("d.PNG", PNG), ("e.JpG", JPEG), ("f.ppm", PPM), ("g", PPM), ("h.png.bak", PPM)]):
        root = tmp_path / f"named_{k}"
        _capture(root, [name])
        (root / "images" / name).write_bytes(b"x")                          # an existing named file wins; its kind is its extension's
        if not name.endswith(".ppm"):
            (root / "images" / (os.path.splitext(name)[0] + ".ppm")).write_bytes(b"x")
        assert _resolve(dlib, root) == ("images/" + name, want)


def test_the_old_entry_point_answers_as_before_for_a_png_name(dlib, tmp_path):
    _capture(tmp_path, ["d.png", "e.PnG", "f.jpg"])
    for n in ("d.png", "e.PnG", "f.jpg"):
        (tmp_path / "images" / n).write_bytes(b"x")
    assert _resolve(dlib, tmp_path, "gstrain_dataset_resolve_image", 0) == ("images/d.png", 0)      # is_jpeg stays 0
    assert _resolve(dlib, tmp_path, "gstrain_dataset_resolve_image", 1) == ("images/e.PnG", 0)
    assert _resolve(dlib, tmp_path, "gstrain_dataset_resolve_image", 2) == ("images/f.jpg", 1)
    root = tmp_path / "absent"
    _capture(root, ["a.jpg"])
    (root / "images" / "a.png").write_bytes(b"x")
    assert _resolve(dlib, root, "gstrain_dataset_resolve_image") == ("images/a.png", 0)             # found by the new retry, still "not a JPEG"


def test_mask_lookup_order(dlib, tmp_path):
    NONE, PGM, MPNG = 0, 1, 2
    _capture(tmp_path, ["view.jpg"])
    call = "gstrain_dataset_resolve_mask"
    assert _resolve(dlib, tmp_path, call) == ("", NONE)                      # no masks/ at all: all ones
    os.makedirs(tmp_path / "masks")
    (tmp_path / "masks" / "view.PNG").write_bytes(b"x")                      # not a name that is looked for
    assert _resolve(dlib, tmp_path, call) == ("", NONE)
    (tmp_path / "masks" / "view.jpg.png").write_bytes(b"x")
    assert _resolve(dlib, tmp_path, call) == ("masks/view.jpg.png", MPNG)    # COLMAP's <image name>.png
    (tmp_path / "masks" / "view.png").write_bytes(b"x")
    assert _resolve(dlib, tmp_path, call) == ("masks/view.png", MPNG)        # <stem>.png comes before it
    (tmp_path / "masks" / "view.pgm").write_bytes(b"x")
    assert _resolve(dlib, tmp_path, call) == ("masks/view.pgm", PGM)         # and <stem>.pgm first, as ever
