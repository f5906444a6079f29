"""dvs_jpeg_encode_views (csrc/jpeg_enc.hip) on the GPU against tests/jpeg_enc_ref.py, coefficient for coefficient: the result is defined
bit for bit, so every comparison is == and covers the padding blocks. Shapes 1x1, 8x8, 17x1, 37x29 (partial MCU on both axes, odd
chroma edge), 40x24 (2.5 MCU columns at 4:2:0), 64x48, and 200x70 / 130x33, which span several workgroups (a workgroup owns 8 x 2
MCUs) on both axes; both samplings; quality 1, 50, 90, 100; 64x48 once from a 16-byte aligned pointer (16-byte loads) and once from a
pointer 4 bytes further (element loads); a batch of three views against the single-view results; NaN, +-inf, values below 0 and above
1 and values on the k + 0.5 rounding ties; two calls; invalid arguments; and through both halves on the device: dvs_jpeg_reconstruct of
the encoder's output equals jpeg_ref.reconstruct of the restated coefficients. Every coefficient array sits between guard values."""
import ctypes as C
import numpy as np
import pytest
import jpeg_ref as J
import jpeg_enc_ref as E

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 64                                                   # int16 values kept around each view's coefficients
FILL = 0x5A5A
SHAPES = [(1, 1), (8, 8), (17, 1), (37, 29), (40, 24), (64, 48), (200, 70), (130, 33)]
SAMPLINGS = [E.SAMPLING_420, E.SAMPLING_444]


def image(W, H, seed):
    """fp32 [3][H][W] in about [-0.1, 1.1]: smooth ramps plus noise, so that blocks have DC and AC content and the clamp is met"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x + 2 * y) % 37 / 36.0, ((3 * x + y) % 53) / 52.0, ((x * y) % 29) / 28.0])
    return (base * 1.1 - 0.05 + r.normal(0, 0.08, (3, H, W))).astype(np.float32)


def run(dev, imgs, sampling, quality, shift=0):
    """imgs: list of fp32 [3][H][W] -> list of int16 coefficient arrays; every image starts `shift` bytes past a 16-byte boundary"""
    import torch
    from divshot_amd import _lib
    _, H, W = imgs[0].shape
    desc = _lib.jpeg_encode_desc(W, H, sampling, quality)
    count = _lib.lib.dvs_jpeg_encode_coef_count(C.byref(desc))
    n = len(imgs)
    stride = count + 2 * GUARD                               # (a multiple of 8: every view's coefficients start on a 16-byte boundary)
    d_coef = torch.full((n * stride,), FILL, dtype=torch.int16, device=dev)
    d_imgs, ptrs = [], (C.c_void_p * n)()
    for k, im in enumerate(imgs):
        buf = torch.zeros(3 * H * W + 8, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0 and shift % 4 == 0
        buf[shift // 4:shift // 4 + 3 * H * W] = torch.from_numpy(np.ascontiguousarray(im).reshape(-1)).to(dev)
        d_imgs.append(buf)
        ptrs[k] = buf.data_ptr() + shift
    outs = (C.c_void_p * n)(*[d_coef.data_ptr() + 2 * (k * stride + GUARD) for k in range(n)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.dvs_jpeg_encode_views(stream, C.byref(desc), ptrs, outs, n) == 0
    torch.cuda.synchronize()
    h = d_coef.cpu().numpy().reshape(n, stride)
    assert (h[:, :GUARD] == FILL).all() and (h[:, GUARD + count:] == FILL).all(), "a write outside the coefficients"
    return [h[k, GUARD:GUARD + count].copy() for k in range(n)]


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


@pytest.fixture(scope="module")
def wanted():
    """the restatement's coefficients, computed once per (shape, sampling, quality)"""
    cache = {}

    def get(shape, sampling, quality, seed=None):
        key = (shape, sampling, quality, seed)
        if key not in cache:
            cache[key] = E.encode(image(shape[0], shape[1], shape[0] + shape[1] if seed is None else seed), sampling, quality).coef
        return cache[key]
    return get


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["420", "444"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_coefficients_equal_the_restatement(gpu_device, wanted, shape, sampling):
    img = image(shape[0], shape[1], shape[0] + shape[1])
    for quality in (1, 50, 90, 100):
        want = wanted(shape, sampling, quality)
        same(run(gpu_device, [img], sampling, quality)[0], want, (shape, sampling, quality))
    assert np.count_nonzero(wanted(shape, sampling, 100)) > 0


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["420", "444"])
def test_64x48_vector_and_element_loads_agree(gpu_device, wanted, sampling):
    img = image(64, 48, 112)
    want = wanted((64, 48), sampling, 90)
    same(run(gpu_device, [img], sampling, 90)[0], want, "16-byte loads")
    same(run(gpu_device, [img], sampling, 90, shift=4)[0], want, "element loads")


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["420", "444"])
def test_a_batch_of_three_equals_the_single_views(gpu_device, wanted, sampling):
    imgs = [image(37, 29, seed) for seed in (1, 2, 3)]
    batch = run(gpu_device, imgs, sampling, 90)
    for k, im in enumerate(imgs):
        single = run(gpu_device, [im], sampling, 90)[0]
        same(batch[k], single, ("batch against single", k))
        same(single, wanted((37, 29), sampling, 90, seed=k + 1), ("single against the restatement", k))
    assert not np.array_equal(batch[0], batch[1])


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["420", "444"])
def test_special_values_and_rounding_ties(gpu_device, sampling):
    W, H = 40, 24
    r = np.random.default_rng(9)
    k = r.integers(0, 255, (3, H, W)).astype(np.float64)
    img = ((k + 0.5) / 255.0).astype(np.float32)             # products that land on or beside k + 0.5
    prod = img * np.float32(255.0)
    assert np.count_nonzero(prod - np.floor(prod) == 0.5) > 100      # real ties, both to even and to odd neighbours
    img[0, 0, :8] = [np.nan, np.inf, -np.inf, -0.0, -3.5, 7.25, 1.0, 0.0]
    img[1, 5, 3:7] = [np.nan, 1e30, -1e30, 1e-30]
    img[2, H - 1, W - 1] = np.nan                            # the pixel the padding repeats
    for quality in (50, 100):
        same(run(gpu_device, [img], sampling, quality)[0], E.encode(img, sampling, quality).coef, (sampling, quality))


def test_two_calls_identical_bytes(gpu_device):
    img = image(200, 70, 5)
    assert run(gpu_device, [img], E.SAMPLING_420, 75)[0].tobytes() == run(gpu_device, [img], E.SAMPLING_420, 75)[0].tobytes()


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd import _lib
    lib = _lib.lib
    W, H = 40, 24
    desc = _lib.jpeg_encode_desc(W, H, E.SAMPLING_420, 90)
    count = lib.dvs_jpeg_encode_coef_count(C.byref(desc))
    img = torch.zeros(3 * H * W, dtype=torch.float32, device=gpu_device)
    coef = torch.zeros(17 * count + 8, dtype=torch.int16, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = lambda p: (C.c_void_p * 1)(p)
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(img.data_ptr()), one(coef.data_ptr()), 1) == 0
    assert lib.dvs_jpeg_encode_views(st, None, one(img.data_ptr()), one(coef.data_ptr()), 1) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), None, one(coef.data_ptr()), 1) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(img.data_ptr()), None, 1) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(None), one(coef.data_ptr()), 1) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(img.data_ptr()), one(None), 1) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(img.data_ptr()), one(coef.data_ptr() + 2), 1) == INVALID      # off a 16-byte boundary
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), one(img.data_ptr()), one(coef.data_ptr()), 0) == INVALID
    imgs17 = (C.c_void_p * 17)(*[img.data_ptr()] * 17)
    outs17 = (C.c_void_p * 17)(*[coef.data_ptr() + 2 * k * count for k in range(17)])
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), imgs17, outs17, 17) == INVALID
    assert lib.dvs_jpeg_encode_views(st, C.byref(desc), imgs17, outs17, 16) == 0
    for field, value in (("width", 0), ("height", 65501), ("components", 1), ("hs", 1), ("vs", 1), ("hs", 3)):
        d = _lib.jpeg_encode_desc(W, H, E.SAMPLING_420, 90)
        setattr(d, field, value)
        assert lib.dvs_jpeg_encode_views(st, C.byref(d), one(img.data_ptr()), one(coef.data_ptr()), 1) == INVALID, (field, value)
    for edit in ("blocks", "offset", "overlap", "quant0", "quant256"):
        d = _lib.jpeg_encode_desc(W, H, E.SAMPLING_420, 90)
        if edit == "blocks":
            d.blocks_w[1] += 1
        elif edit == "offset":
            d.offset[2] += 4
        elif edit == "overlap":
            d.offset[1] = 0
        elif edit == "quant0":
            d.quant[0][5] = 0
        else:
            d.quant[2][63] = 256
        assert lib.dvs_jpeg_encode_views(st, C.byref(d), one(img.data_ptr()), one(coef.data_ptr()), 1) == INVALID, edit
    torch.cuda.synchronize()


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["420", "444"])
def test_through_both_halves_on_the_device(gpu_device, wanted, sampling):
    """dvs_jpeg_reconstruct(dvs_jpeg_encode_views(x)) == jpeg_ref.reconstruct(jpeg_enc_ref.encode(x))"""
    import torch
    from divshot_amd import _lib
    shape = (37, 29)
    img = image(shape[0], shape[1], shape[0] + shape[1])
    f = E.encode(img, sampling, 90)
    same(f.coef, wanted(shape, sampling, 90), "the restatement twice")
    desc = _lib.jpeg_encode_desc(shape[0], shape[1], sampling, 90)
    count = _lib.lib.dvs_jpeg_encode_coef_count(C.byref(desc))
    d_img = torch.from_numpy(img).to(gpu_device).contiguous()
    d_coef = torch.zeros(count, dtype=torch.int16, device=gpu_device)
    d_rgb = torch.zeros(3 * shape[0] * shape[1], dtype=torch.uint8, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.dvs_jpeg_encode_views(st, C.byref(desc), (C.c_void_p * 1)(d_img.data_ptr()), (C.c_void_p * 1)(d_coef.data_ptr()), 1) == 0
    assert _lib.lib.dvs_jpeg_reconstruct(st, C.byref(desc), d_coef.data_ptr(), d_rgb.data_ptr()) == 0
    torch.cuda.synchronize()
    got = d_rgb.cpu().numpy().reshape(3, shape[1], shape[0])
    want = J.reconstruct(f)
    assert np.array_equal(got, want)
    assert want.std() > 20                                    # a picture, not a flat field
