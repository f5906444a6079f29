"""dvs_jpeg_reconstruct (csrc/jpeg.hip) on the GPU against tests/jpeg_ref.py, byte for byte: the result is defined in integer arithmetic,
so every comparison is ==. Cases: every fixture of tests/golden/jpeg/ (coefficients from the C++ host decoder: partial MCUs in both
directions, 4:4:4 / 4:2:2 / 4:2:0 / grayscale, 1x1, 17x1, 8x8); a misaligned output pointer and an odd width (byte path); 64x48 at
4:2:0 on an aligned pointer (16-byte path) and the same image through the byte path; images of random coefficients that span several
workgroups in both directions at each sampling (a workgroup owns 8 x 2 MCUs, so the chroma halo crosses workgroup borders); the
hostile set — every coefficient +-32767 with quantisers 255 and 65535 — where the clamps decide; two calls, identical bytes; invalid
arguments. Every output sits between guard bytes."""
import ctypes as C
import glob
import os
import numpy as np
import pytest
import jpeg_ref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "jpeg")
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FIX, "*.jpg")) if os.path.basename(f)[:-4] not in ("progressive", "adobe_rgb"))
INVALID = 1
GUARD = 64                                                   # bytes kept around the output
FILL = 0xA5
# (W, H, hs, vs, components): more than one workgroup (64 hs x 16 vs pixels) in x and in y, partial MCUs at both edges
SPANNING = [(200, 70, 2, 2, 3), (300, 40, 2, 1, 3), (150, 40, 1, 1, 3), (150, 40, 1, 1, 1), (256, 64, 2, 2, 3), (130, 33, 2, 2, 3)]


def _desc(f):
    from divshot_amd._lib import JpegDesc
    d = JpegDesc()
    d.width, d.height, d.components, d.hs, d.vs = f.width, f.height, f.ncomp, f.hs[0], f.vs[0]
    for c in range(f.ncomp):
        d.blocks_w[c], d.blocks_h[c], d.offset[c] = f.bw[c], f.bh[c], f.offset[c]
        for k in range(64):
            d.quant[c][k] = int(f.quant[c][k])
    return d


def _run(dev, desc, coef, shift=0):
    """-> uint8 [3][H][W]; the output starts `shift` bytes past a 16-byte boundary"""
    import torch
    from divshot_amd._lib import lib
    n = 3 * desc.width * desc.height
    d_coef = torch.from_numpy(np.ascontiguousarray(coef, np.int16)).to(dev)
    out = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0 and d_coef.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_jpeg_reconstruct(stream, C.byref(desc), d_coef.data_ptr(), out.data_ptr() + GUARD + shift) == 0
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:GUARD + shift] == FILL).all() and (h[GUARD + shift + n:] == FILL).all(), "a write outside the output"
    return h[GUARD + shift:GUARD + shift + n].reshape(3, desc.height, desc.width).copy()


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_expected.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_bytes_equal_the_restatement(gpu_device, expected, name):
    from divshot_amd import _lib
    desc, coef = _lib.jpeg_decode_coefficients(os.path.join(FIX, name + ".jpg"))
    want = J.decode(open(os.path.join(FIX, name + ".jpg"), "rb").read())
    assert np.array_equal(want, expected[name + "/int"])
    _same(_run(gpu_device, desc, coef), want, name)
    if desc.components == 1:
        assert np.array_equal(want[0], want[1]) and np.array_equal(want[0], want[2])


@pytest.mark.parametrize("shift", [1, 5, 8])
def test_misaligned_pointer_and_odd_width_take_the_byte_path(gpu_device, expected, shift):
    from divshot_amd import _lib
    for name in ("c420_37x29", "c422_37x29", "c420_40x24"):
        desc, coef = _lib.jpeg_decode_coefficients(os.path.join(FIX, name + ".jpg"))
        _same(_run(gpu_device, desc, coef, shift), expected[name + "/int"], (name, shift))


def test_64x48_takes_the_16_byte_path_and_both_paths_agree(gpu_device):
    f = J.synthetic_frame(64, 48, 2, 2, seed=11)
    want = J.reconstruct(f)
    assert len(np.unique(want)) > 100
    vec = _run(gpu_device, _desc(f), f.coef)
    _same(vec, want, "16-byte path")
    _same(_run(gpu_device, _desc(f), f.coef, 4), want, "byte path")


@pytest.mark.parametrize("shape", SPANNING, ids=lambda s: "%dx%d_%dx%d_%d" % s)
def test_images_that_span_workgroups(gpu_device, shape):
    W, H, hs, vs, n = shape
    f = J.synthetic_frame(W, H, hs, vs, ncomp=n, seed=W + H)
    want = J.reconstruct(f)
    _same(_run(gpu_device, _desc(f), f.coef), want, shape)
    if W % 16 == 0:
        _same(_run(gpu_device, _desc(f), f.coef, 3), want, (shape, "byte path"))


@pytest.mark.parametrize("quant", [255, 65535])
def test_hostile_coefficients_are_defined(gpu_device, quant):
    r = np.random.default_rng(quant)
    base = J.synthetic_frame(48, 32, 2, 2)
    signs = np.where(r.random(len(base.coef)) < 0.5, -32767, 32767)
    for coef in (32767, -32767, signs):
        f = J.synthetic_frame(48, 32, 2, 2, coef=coef, quant=quant)
        _same(_run(gpu_device, _desc(f), f.coef), J.reconstruct(f), (quant, "all" if np.ndim(coef) == 0 else "mixed"))


def test_two_calls_identical_bytes(gpu_device):
    f = J.synthetic_frame(200, 70, 2, 2, seed=3)
    assert _run(gpu_device, _desc(f), f.coef).tobytes() == _run(gpu_device, _desc(f), f.coef).tobytes()


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    f = J.synthetic_frame(40, 24, 2, 2, seed=1)
    coef = torch.from_numpy(f.coef).to(gpu_device)
    out = torch.zeros(3 * 40 * 24 + 64, dtype=torch.uint8, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_jpeg_reconstruct(st, C.byref(_desc(f)), coef.data_ptr(), out.data_ptr()) == 0
    assert lib.dvs_jpeg_reconstruct(st, None, coef.data_ptr(), out.data_ptr()) == INVALID
    assert lib.dvs_jpeg_reconstruct(st, C.byref(_desc(f)), None, out.data_ptr()) == INVALID
    assert lib.dvs_jpeg_reconstruct(st, C.byref(_desc(f)), coef.data_ptr(), None) == INVALID
    assert lib.dvs_jpeg_reconstruct(st, C.byref(_desc(f)), coef.data_ptr() + 2, out.data_ptr()) == INVALID
    for field, value in (("width", 0), ("height", 65501), ("components", 2), ("components", 4), ("hs", 3), ("vs", 4), ("hs", 1)):
        d = _desc(f)
        setattr(d, field, value)
        assert lib.dvs_jpeg_reconstruct(st, C.byref(d), coef.data_ptr(), out.data_ptr()) == INVALID, (field, value)
    d = _desc(f)
    d.blocks_w[1] += 1
    assert lib.dvs_jpeg_reconstruct(st, C.byref(d), coef.data_ptr(), out.data_ptr()) == INVALID
    d = _desc(f)
    d.offset[2] += 4
    assert lib.dvs_jpeg_reconstruct(st, C.byref(d), coef.data_ptr(), out.data_ptr()) == INVALID
    torch.cuda.synchronize()
