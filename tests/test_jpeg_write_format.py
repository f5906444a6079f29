"""Baseline JPEG writing without a GPU. The host entropy coder (divshot_amd/gstrain/jpeg_write.cpp, through libgsplyio.so's
gstrain_jpeg_encode) against the project's two decoders (the C one, gstrain_jpeg_open*, and tests/jpeg_ref.py): a frame goes in, the
same frame comes out. The encoder's quantiser tables against tables recorded from PIL. The integer definition of the device's half
(tests/jpeg_enc_ref.py, what dvs_jpeg_encode_views computes) against the fp64 forward DCT of T.81 A.3.3 and against PIL's own
encode -> decode, recorded in tests/golden/jpeg_enc_expected.npz by tests/golden/make_jpeg_enc_fixtures.py (no test imports PIL).

Bars of the fidelity check (figures: DESIGN.md §8 row 9). The definition carries six fractional bits of a coefficient into the
quantiser; an earlier form that rounded the coefficient to an integer first lost up to 0.10 dB on the smooth image below by rounding
twice. Two sets of images:
  - a 128x96 smooth synthetic picture that was never a JPEG, without and with sigma = 6 noise (12 288 pixels: one coefficient moves
    its PSNR by about 1e-3 dB, so the set can resolve the 0.1 dB mark): PSNR(decode(encode(img)), img) of the integer variant lies at
    most 0.1 dB below the fp64 variant's in every case — the mark itself, not a measured figure; measured: 0.0519 dB and 0.0113 dB.
  - the 16 small images the check was specified on (the decoded fixtures, 1 to 1073 pixels, plus 40x24 noise), Q 50 / 90 / 100, both
    samplings, 96 cases: each case within twice the largest gap measured, against fp64 and against PIL, and the MEAN gap against fp64
    within 0.1 dB (measured 0.0555 dB). The largest gap is 4.1497 dB, against both, on ONE image: s_1x1 at Q 50 (either sampling), a single
    pixel. Its DC is 8 (Y - 128), the quantiser 16, so the exact coefficient sits on a rounding tie; fp64 rounds it away from zero, the
    13-bit table's DC gain of 0.99979 puts the integer variant just below the tie, and the one pixel moves by a level. Without that
    image the largest gaps are 0.2636 dB against fp64 and 0.3816 dB against PIL: single coefficients on ties of requantised 17- to
    1073-pixel images, of either sign (the integer variant is ahead by up to 1.64 dB). Such a bar
    says little; the first set is the one that judges the arithmetic.
Int and fp64 differ on 0.38 % of the quantised coefficients of the second set (at most 1.6 % in one case), always by exactly one step."""
import ctypes as C
import glob
import os
import subprocess
import numpy as np
import pytest
import jpeg_ref as J
import jpeg_enc_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "divshot_amd", "gstrain")
FIX = os.path.join(ROOT, "tests", "golden", "jpeg")
SIZES = [(1, 1), (8, 8), (17, 1), (37, 29), (40, 24)]
CONTENTS = ["zero", "last", "extreme", "dc_alternating", "random"]
GAP_FP64, GAP_PIL = 4.1497, 4.1497                           # the largest gaps measured on the small images (dB; both s_1x1, Q 50, 4:2:0); bars twice these
GAP_MARK = 0.1                                               # dB: per case on the 128x96 images, and for the mean over the small ones
IMAGES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FIX, "*.jpg")) if os.path.basename(f)[:-4] not in ("progressive", "adobe_rgb"))
ROUND_TRIP_ERROR_Q100_444 = 4                                # e of tests/test_gpu_render_views.py: largest |decode(encode(img)) - img| at Q 100 / 4:4:4


def desc_of(f):
    from divshot_amd._lib import JpegDesc
    d = JpegDesc()
    d.width, d.height, d.components, d.hs, d.vs = f.width, f.height, f.ncomp, f.hs[0], f.vs[0]
    for c in range(f.ncomp):
        d.blocks_w[c], d.blocks_h[c], d.offset[c] = f.bw[c], f.bh[c], f.offset[c]
        for k in range(64):
            d.quant[c][k] = int(f.quant[c][k])
    return d


def frame(W, H, s, content):
    f = J.synthetic_frame(W, H, s, s, seed=0)
    n = len(f.coef)
    if content == "zero":
        f.coef[:] = 0
    elif content == "last":                                  # a run of 62 zeros after coefficient 0: three ZRL, then the value
        f.coef[:] = 0
        f.coef[63::64] = -3
        f.coef[0::64] = 0
    elif content == "extreme":
        f.coef[:] = np.where(np.random.default_rng(1).random(n) < 0.5, -1023, 1023)
    elif content == "dc_alternating":
        f.coef[:] = 0
        f.coef[0::64] = np.where(np.arange(n // 64) % 2 == 0, 1023, -1023)
    return f


def same_frame(desc, coef, f):
    assert (desc.width, desc.height, desc.components, desc.hs, desc.vs) == (f.width, f.height, f.ncomp, f.hs[0], f.vs[0])
    for c in range(f.ncomp):
        assert (desc.blocks_w[c], desc.blocks_h[c], desc.offset[c]) == (f.bw[c], f.bh[c], f.offset[c])
        assert np.array_equal(np.array(desc.quant[c][:], np.uint16), f.quant[c])
    assert coef.dtype == np.int16 and np.array_equal(coef, f.coef)


def scan_of(data):
    at = data.index(b"\xff\xda")
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):-2]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("s", [1, 2], ids=["444", "420"])
@pytest.mark.parametrize("size", SIZES, ids=lambda v: "%dx%d" % v)
def test_round_trip_returns_the_frame(tmp_path, size, s, content):
    from divshot_amd import _lib
    f = frame(size[0], size[1], s, content)
    data = _lib.jpeg_encode_coefficients(desc_of(f), f.coef)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    g = J.decode_coefficients(data)                          # the restatement
    assert (g.width, g.height, g.ncomp, g.hs, g.vs, g.bw, g.bh, g.offset) == (f.width, f.height, f.ncomp, f.hs, f.vs, f.bw, f.bh, f.offset)
    assert all(np.array_equal(a, b) for a, b in zip(g.quant, f.quant)) and np.array_equal(g.coef, f.coef)
    same_frame(*_lib.jpeg_decode_coefficients(data), f)      # the C decoder, from memory ...
    p = tmp_path / "f.jpg"
    p.write_bytes(data)
    same_frame(*_lib.jpeg_decode_coefficients(str(p)), f)    # ... and through gstrain_jpeg_open
    scan = scan_of(data)
    assert all(scan[i + 1] == 0 for i in range(len(scan) - 1) if scan[i] == 0xFF) and scan[-1:] != b"\xff"    # every FF is stuffed
    if content == "random":
        assert b"\xff\x00" in scan                           # seed 0: the 16-bit codes of the rare run/size symbols begin with FF
    if content == "last":
        assert np.count_nonzero(f.coef) == len(f.coef) // 64


def test_stream_layout():
    """SOI, APP0, two DQT for a frame whose chroma tables agree (three when they differ), SOF0, four DHT, SOS, one scan, EOI"""
    from divshot_amd import _lib
    f = E.frame_for(40, 24, E.SAMPLING_420, 75)
    data = _lib.jpeg_encode_coefficients(desc_of(f), f.coef)
    markers, pos = [], 2
    while data[pos + 1] != 0xDA:
        markers.append(data[pos + 1])
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4]
    assert data[2:11] == b"\xff\xe0\x00\x10JFIF\x00"
    assert b"\xff\xdd" not in data[:pos]                     # no restart interval
    g = J.synthetic_frame(40, 24, 2, 2, seed=3)              # three different tables
    assert _lib.jpeg_encode_coefficients(desc_of(g), g.coef).count(b"\xff\xdb\x00\x43") == 3


def test_rejections_come_with_a_message():
    from divshot_amd import _lib
    f = frame(40, 24, 2, "zero")
    for at in (5, 64):                                       # an AC and a DC coefficient
        for v in (1024, -1024):
            bad = f.coef.copy()
            bad[at] = v
            with pytest.raises(_lib.DvsError, match=str(v)):
                _lib.jpeg_encode_coefficients(desc_of(f), bad)
    d = desc_of(f)
    d.blocks_w[1] += 1
    with pytest.raises(_lib.DvsError, match="blocks"):
        _lib.jpeg_encode_coefficients(d, f.coef)
    with pytest.raises(_lib.DvsError, match="coefficients"):
        _lib.jpeg_encode_coefficients(desc_of(f), f.coef[:-64])
    for field, value, word in (("width", 0, "size"), ("components", 2, "components"), ("hs", 3, "sampling")):
        d = desc_of(f)
        setattr(d, field, value)
        with pytest.raises(_lib.DvsError, match=word):
            _lib.jpeg_encode_coefficients(d, f.coef)
    for q in (0, 256):
        d = desc_of(f)
        d.quant[1][7] = q
        with pytest.raises(_lib.DvsError, match="quantiser %d" % q):
            _lib.jpeg_encode_coefficients(d, f.coef)
    h = _lib.host_lib()
    err = C.create_string_buffer(256)
    ints, offs = (C.c_int32 * 15)(), (C.c_uint64 * 4)()
    for args in ((None, C.addressof(d.quant), offs, f.coef.ctypes.data), (ints, None, offs, f.coef.ctypes.data), (ints, C.addressof(d.quant), None, f.coef.ctypes.data),
                 (ints, C.addressof(d.quant), offs, None)):
        assert not h.gstrain_jpeg_encode(*args, err, 256) and b"NULL" in err.value
    assert not h.gstrain_jpeg_encode(None, None, None, None, None, 0)
    assert h.gstrain_jpeg_encoded_size(None) == 0 and h.gstrain_jpeg_encoded_bytes(None, None) != 0
    assert not h.gstrain_jpeg_open_memory(None, 0, err, 256)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_enc_expected.npz"))


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quantisers_equal_the_recorded_pil_tables(recorded, quality):
    from divshot_amd import _lib
    for sampling in (E.SAMPLING_420, E.SAMPLING_444):
        d = _lib.jpeg_encode_desc(37, 29, sampling, quality)
        luma, chroma = (np.array(d.quant[c][:], np.uint16) for c in (0, 1))
        assert np.array_equal(luma, recorded[f"quant/{quality}/luma"]) and np.array_equal(chroma, recorded[f"quant/{quality}/chroma"])
        assert np.array_equal(np.array(d.quant[2][:], np.uint16), chroma)
        want = E.quant_tables(quality)
        assert np.array_equal(luma, want[0]) and np.array_equal(chroma, want[1])
        assert luma.min() >= 1 and max(luma.max(), chroma.max()) <= 255


def test_descriptor_is_the_restatements_frame():
    from divshot_amd import _lib
    for (W, H) in SIZES + [(64, 48), (65500, 3)]:
        for sampling in (E.SAMPLING_420, E.SAMPLING_444):
            d, f = _lib.jpeg_encode_desc(W, H, sampling, 90), E.frame_for(W, H, sampling, 90)
            assert (d.width, d.height, d.components, d.hs, d.vs) == (W, H, 3, f.hs[0], f.vs[0])
            assert [(d.blocks_w[c], d.blocks_h[c], d.offset[c]) for c in range(3)] == [(f.bw[c], f.bh[c], f.offset[c]) for c in range(3)]
            assert _lib.lib.dvs_jpeg_encode_coef_count(C.byref(d)) == len(f.coef) and len(f.coef) % 64 == 0
    bad = _lib.JpegDesc()
    for args in ((0, 8, 0, 90), (8, 65501, 0, 90), (8, 8, 2, 90), (8, 8, -1, 90), (8, 8, 0, 0), (8, 8, 0, 101)):
        assert _lib.lib.dvs_jpeg_encode_desc(*args, C.byref(bad)) == 1
    assert _lib.lib.dvs_jpeg_encode_desc(8, 8, 0, 90, None) == 1
    assert _lib.lib.dvs_jpeg_encode_coef_count(None) == 0
    d = _lib.jpeg_encode_desc(8, 8, 0, 90)
    d.quant[0][0] = 256
    assert _lib.lib.dvs_jpeg_encode_coef_count(C.byref(d)) == 0
    # the quantisers the library hands out are 1..255 at every quality, which is what the kernel's division rests on: n / q =
    # (n * (2^20 / q + 1)) >> 20 in 32 bits for every n = (|F| + 32 q) >> 6 < 2^12. (This restates the kernel's formula; the check of the
    # kernel itself is the == parity of tests/test_gpu_jpeg_encode.py.)
    qs = np.unique(np.concatenate([np.array(_lib.jpeg_encode_desc(8, 8, 0, Q).quant[c][:], np.uint64) for Q in range(1, 101) for c in (0, 1)]))
    assert qs.min() == 1 and qs.max() == 255
    n, q = np.arange(4096, dtype=np.uint64)[:, None], np.arange(1, 256, dtype=np.uint64)[None, :]
    prod = n * ((1 << 20) // q + 1)
    assert prod.max() < 1 << 32 and np.array_equal(prod >> 20, n // q)


def test_definition_is_overflow_free_and_bounded():
    """jpeg_enc_ref asserts the int32 range at each intermediate: the extreme images (through the library's descriptor and entropy coder,
    whose limits the bounds are for), and per table row the signs that maximise it"""
    from divshot_amd import _lib
    worst = 0
    for rgb in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255)):
        img = np.broadcast_to(np.array(rgb, np.uint8)[:, None, None], (3, 16, 16))
        for s in (E.SAMPLING_420, E.SAMPLING_444):
            f = E.encode_bytes(img, s, 100)
            assert np.abs(f.coef).max() <= 1023
            d = _lib.jpeg_encode_desc(16, 16, s, 100)
            assert np.array_equal(J.decode_coefficients(_lib.jpeg_encode_coefficients(d, f.coef)).coef, f.coef)     # the clamp keeps it codable
    for u in range(8):
        for v in range(8):
            s = np.where(np.outer(J.IDCT_T[v], J.IDCT_T[u]) < 0, -128, 127).astype(np.int64)
            for sign in (1, -1):
                F = E.fdct_int(np.clip(sign * s, -128, 127))
                worst = max(worst, int(np.abs(F).max()))
    assert worst < (1 << 16) + (1 << 6)                      # F in 1/64 units; (worst + 32 * 255) >> 6 < 2^12, the division's range
    assert (worst + 32 * 255) >> 6 < 1 << 12
    assert np.array_equal(E.to_bytes(np.array([np.nan, np.inf, -np.inf, -1, 2, 0.5 / 255, 1.5 / 255, 2.5 / 255], np.float32)), [0, 255, 0, 0, 255, 0, 2, 2])


@pytest.fixture(scope="module")
def images(recorded):
    out = {n: J.decode(open(os.path.join(FIX, n + ".jpg"), "rb").read()) for n in IMAGES}
    out["noise_40x24"] = recorded["noise_40x24"]
    return out


def test_fidelity_of_the_integer_definition(recorded, images):
    assert len(images) == 16
    gap64 = gap_pil = -1.0
    share, e, gaps = [], 0, []
    for name, img in images.items():
        for Q in (50, 90, 100):
            for s, tag in ((E.SAMPLING_420, "420"), (E.SAMPLING_444, "444")):
                fi, ff = E.encode_bytes(img, s, Q, "int"), E.encode_bytes(img, s, Q, "fp64")
                back = J.reconstruct(fi)
                p_int, p_64, p_pil = E.psnr(back, img), E.psnr(J.reconstruct(ff), img), float(recorded[f"pil_psnr/{name}/{Q}/{tag}"])
                d = fi.coef.astype(int) - ff.coef.astype(int)
                assert np.abs(d).max() <= 1, (name, Q, tag)                          # never more than one quantisation step
                share.append(float((d != 0).mean()))
                a, b = (0.0 if p_int == p_64 else p_64 - p_int), (0.0 if p_int == p_pil else p_pil - p_int)
                gap64, gap_pil = max(gap64, a), max(gap_pil, b)
                gaps.append(a)
                assert a <= 2 * GAP_FP64 and b <= 2 * GAP_PIL, (name, Q, tag, p_int, p_64, p_pil)
                if Q == 100 and s == E.SAMPLING_444:
                    e = max(e, int(np.abs(back.astype(int) - img.astype(int)).max()))
    print(f"integer definition: largest gap below fp64 {gap64:.4f} dB (mean {np.mean(gaps):.4f} dB), below PIL {gap_pil:.4f} dB; int and fp64 differ on {np.mean(share) * 100:.2f} % of the "
          f"coefficients (at most {max(share) * 100:.2f} % in a case); largest round-trip error at Q 100 / 4:4:4: {e} levels")
    assert e <= ROUND_TRIP_ERROR_Q100_444
    assert gap64 <= GAP_FP64 + 1e-3 and gap_pil <= GAP_PIL + 1e-3                   # the recorded gaps are the measured ones
    assert np.mean(gaps) <= GAP_MARK


def smooth_image(noise):
    """uint8 [3][96][128]: a smooth synthetic picture that no JPEG codec has touched"""
    H, W = 96, 128
    y, x = np.mgrid[0:H, 0:W]
    px = np.stack([127 + 100 * np.sin(x / 9.0 + y / 23.0), 127 + 100 * np.cos(y / 7.0 - x / 31.0), 40 + 1.2 * x + 0.6 * y])
    if noise:
        px = px + np.random.default_rng(5).normal(0, noise, px.shape)
    return np.clip(np.rint(px), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("noise", [0, 6])
def test_fidelity_on_an_image_that_resolves_the_mark(noise):
    """12 288 pixels, never requantised: every case within 0.1 dB of the fp64 variant; and the library codes what the definition gives"""
    from divshot_amd import _lib
    img = smooth_image(noise)
    worst, share = -1.0, []
    for Q in (50, 90, 100):
        for s in (E.SAMPLING_420, E.SAMPLING_444):
            fi, ff = E.encode_bytes(img, s, Q, "int"), E.encode_bytes(img, s, Q, "fp64")
            p_int, p_64 = E.psnr(J.reconstruct(fi), img), E.psnr(J.reconstruct(ff), img)
            d = fi.coef.astype(int) - ff.coef.astype(int)
            assert np.abs(d).max() <= 1
            share.append(float((d != 0).mean()))
            worst = max(worst, p_64 - p_int)
            assert p_64 - p_int <= GAP_MARK, (noise, Q, s, p_int, p_64)
    print(f"128x96, noise {noise}: largest gap below fp64 {worst:.4f} dB; int and fp64 differ on at most {max(share) * 100:.2f} % of the coefficients")
    f = E.encode_bytes(img, E.SAMPLING_420, 90)
    same_frame(*_lib.jpeg_decode_coefficients(_lib.jpeg_encode_coefficients(_lib.jpeg_encode_desc(128, 96, E.SAMPLING_420, 90), f.coef)), f)


def test_entropy_coder_under_the_sanitizers_as_a_host_program(tmp_path):
    """jpeg_write_check.cpp + jpeg_write.cpp + jpeg_io.cpp built with -fsanitize=address,undefined (the Makefile's jpeg_write_check_asan
    target) and run directly: the synthetic frames round-trip, the malformed ones are refused, no sanitizer report. Nothing is loaded
    into Python."""
    lib = str(tmp_path / "lib")
    subprocess.check_call(["make", "-C", SRC, "jpeg_write_check_asan", "LIBDIR=" + lib], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(lib, "jpeg_write_check_asan")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "0 failures" and len(lines) == 50 + 10 + 1 + 1 and all(l.startswith("ok ") for l in lines[:-1])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
