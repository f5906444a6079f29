"""dvs_png_encode_views restated in numpy, from the definition in include/dvs_image.h (not from the kernel): fp32 planes -> samples ->
raw scanlines -> per row the five filters, their costs and the choice -> the filtered stream, and the count of saturated samples.
  sample   M = 255 or 65535; s = (int)min(M, max(0, rint(x * scale))), the product and rint in fp32, ties to even; NaN -> 0, +inf -> M,
           -inf -> 0; saturated iff rint(x * scale) > M before the clamp (+inf counts, NaN does not)
  raw      RGB8: R G B interleaved; GRAY8: one byte; GRAY16: high byte first
  filters  a = the raw byte bpp to the left, b = above, c = above a; 0 outside the picture; modulo 256:
           0 x | 1 x - a | 2 x - b | 3 x - ((a + b) >> 1) | 4 x - paeth(a, b, c) with the decoder's tie order (png_ref._paeth)
  choice   cost(f) = sum over the row's filtered bytes v of (v if v < 128 else 256 - v); the smallest cost, on a tie the smallest f
  output   per row the filter byte, then the row filtered with it"""
import numpy as np
import png_ref

RGB8, GRAY8, GRAY16 = 0, 1, 2
KINDS = (RGB8, GRAY8, GRAY16)
BPP = {RGB8: 3, GRAY8: 1, GRAY16: 2}
PNG_TYPE = {RGB8: (2, 8), GRAY8: (0, 8), GRAY16: (0, 16)}       # (colour type, bit depth)
MAX_SAMPLE = {RGB8: 255, GRAY8: 255, GRAY16: 65535}


def quantise(x, scale, kind):
    """fp32 array -> (int64 samples, bool saturated), elementwise"""
    m = np.float32(MAX_SAMPLE[kind])
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(scale))          # fp32 product, fp32 rint (to nearest even)
        assert r.dtype == np.float32
        sat = r > m                                                         # False for a NaN
        s = np.where(np.isnan(r), np.float32(0), np.minimum(m, np.maximum(np.float32(0), r)))
    return s.astype(np.int64), sat


def raw_rows(img, scale, kind):
    """img: fp32 [3][H][W] (RGB8) or [H][W] -> (uint8 [H][rowbytes], number of saturated samples)"""
    s, sat = quantise(img, scale, kind)
    if kind == RGB8:
        rows = s.transpose(1, 2, 0).reshape(s.shape[1], -1)                 # R G B per pixel
    elif kind == GRAY8:
        rows = s
    else:
        rows = np.stack([s >> 8, s & 255], -1).reshape(s.shape[0], -1)      # high byte first
    return rows.astype(np.uint8), int(np.count_nonzero(sat))


def filtered_rows(raw, bpp):
    """uint8 [H][rb] -> uint8 [H][5][rb]: every row under every filter"""
    h, rb = raw.shape
    x = raw.astype(np.int64)
    a = np.concatenate([np.zeros((h, bpp), np.int64), x], 1)[:, :rb]
    b = np.concatenate([np.zeros((1, rb), np.int64), x[:-1]], 0)
    c = np.concatenate([np.zeros((h, bpp), np.int64), b], 1)[:, :rb]
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, png_ref._paeth(a, b, c)], 1)
    return ((x[:, None, :] - pred) & 255).astype(np.uint8)


def costs(filt):
    """uint8 [H][5][rb] -> int64 [H][5]"""
    v = filt.astype(np.int64)
    return np.where(v < 128, v, 256 - v).sum(-1)


def encode(img, scale, kind):
    """-> (the filtered stream uint8 [H * (1 + rowbytes)], the chosen filters uint8 [H], saturated count)"""
    raw, nsat = raw_rows(img, scale, kind)
    filt = filtered_rows(raw, BPP[kind])
    choice = np.argmin(costs(filt), 1)                                      # (argmin returns the first of equal minima: the smallest f)
    h, rb = raw.shape
    out = np.zeros((h, rb + 1), np.uint8)
    out[:, 0] = choice
    out[:, 1:] = filt[np.arange(h), choice]
    return out.reshape(-1), choice.astype(np.uint8), nsat


# ---- the images the tests share ----
def image(W, H, seed):
    """the generator of tests/test_gpu_jpeg_encode.py: fp32 [3][H][W] in about [-0.1, 1.1], smooth ramps plus noise"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x + 2 * y) % 37 / 36.0, ((3 * x + y) % 53) / 52.0, ((x * y) % 29) / 28.0])
    return (base * 1.1 - 0.05 + r.normal(0, 0.08, (3, H, W))).astype(np.float32)


def specials(W, H):
    """three fp32 [3][H][W] pictures: a constant one (every row after the first is zeros under Up: Up wins, or None on the first row's
    tie), a vertical ramp that is constant along a row and changes from row to row (favours Sub / Up), and noise (favours None)"""
    r = np.random.default_rng(W * 1000 + H)
    const = np.full((3, H, W), 0.4, np.float32)
    ramp = np.broadcast_to((np.arange(H, dtype=np.float32) * np.float32(0.037) % np.float32(1.0))[None, :, None], (3, H, W)).copy()
    ramp += np.broadcast_to((np.arange(W, dtype=np.float32) * np.float32(0.21) % np.float32(0.9))[None, None, :], (3, H, W)) * np.float32(0.5)
    noise = r.uniform(0, 1, (3, H, W)).astype(np.float32)
    return [const, ramp, noise]


def smooth(W, H):
    """a smooth 2-D gradient with a little curvature, fp32 [3][H][W]: neighbours predict well, so Average and Paeth get their rows"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    g = (np.float32(0.1) + x * np.float32(0.011) + y * np.float32(0.013) + x * y * np.float32(0.0004)).astype(np.float32)
    return np.stack([g, g * np.float32(0.9) + np.float32(0.05), np.float32(1.0) - g])


def plane_of(img, kind):
    """the input a kind takes from a [3][H][W] picture: the picture itself, or its first plane"""
    return img if kind == RGB8 else img[0]
