"""dvs_png_encode_views (csrc/png_enc.hip) on the GPU against tests/png_enc_ref.py, byte for byte: the result is defined bit for bit, so
every comparison is ==. Shapes 1x1 (a row shorter than a lane's 4 bytes), 3x2, 17x5 (rows that are no multiple of 4, H across the
4-row workgroup), 64x48, 257x9 (several workgroups), 1030x3 (several iterations per lane: 3090 bytes over 64 lanes x 4) and 40x1;
all three kinds; the image generator of test_gpu_jpeg_encode.py plus a constant picture, a ramp and noise; scales 255, 1000 and 65535;
inputs and outputs at offsets 0 and 4 / 0, 1, 2, 3 from a 16-byte boundary (every store path: the bytes are the same); guard bytes around
every output; a batch of three against the single views; two calls; the saturation counts, added to a start value that is not zero;
and through both halves on the device: dvs_png_reconstruct of the encoder's stream is the quantised samples (GRAY16 through the
decoder's 16 -> 8 rule)."""
import ctypes as C
import numpy as np
import pytest
import png_enc_ref as PE
import png_ref

pytestmark = pytest.mark.gpu

GUARD = 32
FILL = 0xA5
SHAPES = [(1, 1), (3, 2), (17, 5), (64, 48), (257, 9), (1030, 3), (40, 1)]
SCALES = [255.0, 1000.0, 65535.0]
KIND_IDS = ["rgb8", "gray8", "gray16"]


def run(dev, imgs, kind, scale, in_shift=0, out_shift=0, sat_start=None):
    """imgs: list of fp32 arrays of one shape ([3][H][W] or [H][W]) -> (list of uint8 streams, uint32 counts or None). Every image
    starts in_shift bytes and every output out_shift bytes past a 16-byte boundary; the outputs lie between guard bytes."""
    import torch
    from divshot_amd import _lib
    H, W = imgs[0].shape[-2:]
    n = len(imgs)
    nbytes = _lib.lib.dvs_png_encode_bytes(kind, W, H)
    assert nbytes == H * (1 + W * PE.BPP[kind]) and in_shift % 4 == 0
    stride = (nbytes + 2 * GUARD + 16 + 15) // 16 * 16
    d_out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 16 == 0
    keep, ins = [], (C.c_void_p * n)()
    for k, im in enumerate(imgs):
        flat = np.ascontiguousarray(im, np.float32).reshape(-1)
        buf = torch.zeros(flat.size + 8, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[in_shift // 4:in_shift // 4 + flat.size] = torch.from_numpy(flat).to(dev)
        keep.append(buf)
        ins[k] = buf.data_ptr() + in_shift
    outs = (C.c_void_p * n)(*[d_out.data_ptr() + k * stride + GUARD + out_shift for k in range(n)])
    d_sat = None if sat_start is None else torch.tensor(list(sat_start), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.dvs_png_encode_views(stream, kind, W, H, scale, ins, outs, None if d_sat is None else d_sat.data_ptr(), n)
    assert rc == 0, _lib.lib.dvs_last_error()
    torch.cuda.synchronize()
    h = d_out.cpu().numpy().reshape(n, stride)
    lo = GUARD + out_shift
    assert (h[:, :lo] == FILL).all() and (h[:, lo + nbytes:] == FILL).all(), "a write outside the stream"
    return [h[k, lo:lo + nbytes].copy() for k in range(n)], None if d_sat is None else d_sat.cpu().numpy().astype(np.int64)


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


@pytest.fixture(scope="module")
def wanted():
    """the restatement's (stream, filters, saturated), computed once per (shape, picture, kind, scale)"""
    cache = {}

    def get(shape, which, kind, scale):
        key = (shape, which, kind, scale)
        if key not in cache:
            cache[key] = PE.encode(PE.plane_of(pictures(shape)[which], kind), scale, kind)
        return cache[key]
    return get


_PICTURES = {}


def pictures(shape):
    if shape not in _PICTURES:
        W, H = shape
        _PICTURES[shape] = [PE.image(W, H, W + H)] + PE.specials(W, H) + [PE.smooth(W, H)]
    return _PICTURES[shape]


@pytest.mark.parametrize("kind", PE.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_streams_and_counts_equal_the_restatement(gpu_device, wanted, shape, kind):
    seen = set()
    for which, img in enumerate(pictures(shape)):
        for scale in SCALES:
            want, filters, nsat = wanted(shape, which, kind, scale)
            got, sat = run(gpu_device, [PE.plane_of(img, kind)], kind, scale, sat_start=[7])
            same(got[0], want, (shape, which, kind, scale))
            assert sat.tolist() == [7 + nsat], (shape, which, kind, scale, sat.tolist(), nsat)
            seen |= set(filters.tolist())
    if shape == (64, 48):
        assert seen == {0, 1, 2, 3, 4}, seen                      # every filter's path ran


@pytest.mark.parametrize("kind", PE.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", [(17, 5), (257, 9), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_every_alignment_gives_the_same_bytes(gpu_device, wanted, shape, kind):
    img = PE.plane_of(pictures(shape)[0], kind)
    want = wanted(shape, 0, kind, 255.0)[0]
    for in_shift in (0, 4):
        for out_shift in (0, 4, 1, 2, 3):
            same(run(gpu_device, [img], kind, 255.0, in_shift, out_shift)[0][0], want, (shape, kind, in_shift, out_shift))


@pytest.mark.parametrize("kind", PE.KINDS, ids=KIND_IDS)
def test_a_batch_of_three_equals_the_single_views(gpu_device, kind):
    W, H = 37, 11
    scale = 1000.0 if kind == PE.GRAY16 else 255.0
    imgs = [PE.plane_of(PE.image(W, H, seed) * np.float32(1.0 if kind != PE.GRAY16 else 40.0 + 30.0 * seed), kind) for seed in (1, 2, 3)]
    batch, sat = run(gpu_device, imgs, kind, scale, out_shift=3, sat_start=[5, 0, 1 << 20])
    counts = []
    for k, im in enumerate(imgs):
        single, one = run(gpu_device, [im], kind, scale, sat_start=[0])
        want, _, nsat = PE.encode(im, scale, kind)
        same(batch[k], single[0], ("batch against single", k))
        same(single[0], want, ("single against the restatement", k))
        assert one.tolist() == [nsat]
        counts.append(nsat)
    assert sat.tolist() == [5 + counts[0], counts[1], (1 << 20) + counts[2]]
    assert not np.array_equal(batch[0], batch[1]) and min(counts) > 0
    if kind == PE.GRAY16:
        assert counts[0] < counts[2] < W * H                      # some of a view saturates, not all of it


def test_special_values_and_rounding_ties(gpu_device):
    W, H = 40, 6
    r = np.random.default_rng(9)
    for kind, scale in ((PE.RGB8, 255.0), (PE.GRAY8, 255.0), (PE.GRAY16, 1000.0), (PE.GRAY16, 65535.0)):
        M = PE.MAX_SAMPLE[kind]
        k = r.integers(0, min(M, 4000), (3, H, W)).astype(np.float64)
        img = ((k + 0.5) / scale).astype(np.float32)
        prod = img * np.float32(scale)
        assert np.count_nonzero(prod - np.floor(prod) == 0.5) > 50
        img[0, 0, :8] = [np.nan, np.inf, -np.inf, -0.0, -3.5, 70.25, M / scale, 0.0]
        img[0, 3, 3:7] = [np.nan, 1e30, -1e30, 1e-30]
        img[0, H - 1, W - 1] = np.inf
        x = PE.plane_of(img, kind)
        want, _, nsat = PE.encode(x, scale, kind)
        got, sat = run(gpu_device, [x], kind, scale, sat_start=[0])
        same(got[0], want, (kind, scale))
        assert sat.tolist() == [nsat] and nsat >= 3


def test_two_calls_identical_bytes_and_a_null_count(gpu_device):
    img = PE.image(257, 9, 5)
    a, _ = run(gpu_device, [img], PE.RGB8, 255.0)
    b, sat = run(gpu_device, [img], PE.RGB8, 255.0, sat_start=[0])
    assert a[0].tobytes() == b[0].tobytes() and sat[0] > 0


@pytest.mark.parametrize("kind", PE.KINDS, ids=KIND_IDS)
def test_through_both_halves_on_the_device(gpu_device, kind):
    """dvs_png_reconstruct(dvs_png_encode_views(x)) == the quantised samples of x (GRAY16: through the decoder's 16 -> 8 rule)"""
    import torch
    from divshot_amd import _lib
    W, H = 67, 21
    scale = 65535.0 if kind == PE.GRAY16 else 255.0
    img = PE.plane_of(PE.image(W, H, 8), kind)
    stream, _ = run(gpu_device, [img], kind, scale)
    desc = _lib.PngDesc()
    desc.width, desc.height = W, H
    desc.color_type, desc.bit_depth = PE.PNG_TYPE[kind]
    assert _lib.lib.dvs_png_filtered_bytes(C.byref(desc)) == stream[0].size
    d_f = torch.from_numpy(stream[0]).to(gpu_device)
    d_rgb = torch.zeros(3 * W * H, dtype=torch.uint8, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.dvs_png_reconstruct(st, C.byref(desc), d_f.data_ptr(), d_rgb.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = d_rgb.cpu().numpy().reshape(3, H, W)
    s = PE.quantise(img, scale, kind)[0]
    if kind == PE.GRAY16:
        s = (s * 255 + 32895) >> 16
    want = s if kind == PE.RGB8 else np.broadcast_to(s, (3, H, W))
    assert np.array_equal(got, want.astype(np.uint8)) and got.std() > 20
    # and the unfiltered scanlines the decoder left in place are the raw bytes
    rows = d_f.cpu().numpy().reshape(H, -1)[:, 1:]
    assert np.array_equal(rows, PE.raw_rows(img, scale, kind)[0])
