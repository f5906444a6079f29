"""The parallel half of baseline JPEG ENCODING, restated in numpy: the yardstick of divshot_amd/csrc/jpeg_enc.hip (dvs_jpeg_encode_views,
include/dvs_image.h): planar fp32 RGB -> quantised DCT coefficients in the layout of jpeg_ref.Frame. Imports numpy, the standard
library and jpeg_ref only.

encode(img, sampling, quality) -> Frame, defined bit for bit (every integer intermediate fits int32; computed in int64 with the int32
range asserted at each step):
  float to byte  b = (int)min(255, max(0, rint(x * 255))), the product and rint in fp32, rint to nearest even, NaN -> 0: the rule of the
                 trainer's 8-bit training views (PackF32ToU8), so a render and its target are quantised alike. (+inf -> 255, -inf -> 0.)
  padding        columns >= W and rows >= H up to the MCU grid repeat column W - 1 / row H - 1
  colour         Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
                 Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
                 Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16         (16-bit BT.601; each lands in 0..255)
  subsampling    4:2:0: chroma sample (i, j) = (c[2j][2i] + c[2j][2i+1] + c[2j+1][2i] + c[2j+1][2i+1] + 2) >> 2, inside the MCU
  forward DCT    s = sample - 128; T = jpeg_ref.IDCT_T (the decoder's one 13-bit table, T[u][x]); rows first:
                 row[y][u] = (sum_x T[u][x] * s[y][x] + 2^5) >> 6          (FDCT_FRAC = 7 fractional bits kept; |row| <= 46336 < 2^17)
                 F[v][u]   = (sum_y T[v][y] * row[y][u] + 2^13) >> 14      (|sum| <= 23168 * 46336 < 2^31; F is the coefficient in
                                                                            1/64 units: F_FRAC = 6 fractional bits go into the quantiser,
                                                                            |F| < 2^16 + 2^6)
  quantisation   c = sign(F) * (((|F| + 32 q) >> 6) // q), then clamp to [-1023, 1023]     (= (|F| + 64 q / 2) // (64 q): half away from
                                                                            zero of the coefficient with its fraction; q in 1..255)
encode(..., fdct="fp64") swaps the forward DCT and the division for T.81 A.3.3 in float64 with the quotient rounded half away from zero."""
import math
import numpy as np
import jpeg_ref as J

SAMPLING_420, SAMPLING_444 = 0, 1
FDCT_FRAC, F_FRAC = 7, 6
ROW_SHIFT, COL_SHIFT = J.IDCT_BITS - FDCT_FRAC, J.IDCT_BITS + FDCT_FRAC - F_FRAC
COEF_MAX = 1023
# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quant_tables(quality):
    """the two Annex K tables scaled by the IJG quality rule, clamped to 1..255 -> (luma, chroma) uint16[64], natural order"""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(k, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for k in (K1, K2))


def frame_for(W, H, sampling, quality):
    """the Frame dvs_jpeg_encode_desc describes, with zero coefficients"""
    hs = 2 if sampling == SAMPLING_420 else 1
    lq, cq = quant_tables(quality)
    f = J.synthetic_frame(W, H, hs, hs, coef=0, quant=1)
    f.quant = [lq.copy(), cq.copy(), cq.copy()]
    return f


def to_bytes(x):
    """fp32 [3][H][W] -> uint8, the rule of the 8-bit training views"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(x * np.float32(255.0))
        v = np.where(np.isnan(v), np.float32(0), np.minimum(np.float32(255), np.maximum(np.float32(0), v)))
    return v.astype(np.uint8)


def ycbcr(rgb):
    """uint8 [3][h][w] -> int64 [3][h][w] in 0..255"""
    r, g, b = (rgb[k].astype(np.int64) for k in range(3))
    y = J._i32(19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = J._i32(-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = J._i32(32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    out = np.stack([y, cb, cr])
    assert out.min() >= 0 and out.max() <= 255
    return out


def fdct_int(s):
    """s int64 [..., 8 y, 8 x] (level-shifted samples) -> F int64 [..., 8 v, 8 u] in 1/64 units"""
    row = J._i32(J._i32(np.einsum("ux,...yx->...yu", J.IDCT_T, s)) + (1 << (ROW_SHIFT - 1))) >> ROW_SHIFT
    assert np.abs(row).max(initial=0) < 1 << 17
    return J._i32(J._i32(np.einsum("vy,...yu->...vu", J.IDCT_T, row)) + (1 << (COL_SHIFT - 1))) >> COL_SHIFT


def fdct_fp64(s):
    """T.81 A.3.3 in float64, not rounded"""
    B = np.array([[(math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
    return np.einsum("vy,...yx,ux->...vu", B, s.astype(np.float64), B)


def quantise_int(F, q):
    """F int64 [..., 8, 8] in 1/64 units, q [64] -> int64"""
    q = q.astype(np.int64).reshape(8, 8)
    return np.clip(np.sign(F) * (((np.abs(F) + (q << (F_FRAC - 1))) >> F_FRAC) // q), -COEF_MAX, COEF_MAX)


def quantise_fp64(F, q):
    q = q.astype(np.float64).reshape(8, 8)
    return np.clip(np.sign(F) * np.floor(np.abs(F) / q + 0.5), -COEF_MAX, COEF_MAX).astype(np.int64)


def planes(rgb8, hs):
    """uint8 [3][H][W] -> [Y, Cb, Cr] int64 planes padded to whole MCUs, chroma subsampled when hs = 2"""
    _, H, W = rgb8.shape
    m = 8 * hs
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    pad = rgb8[:, np.minimum(np.arange(Hp), H - 1)][:, :, np.minimum(np.arange(Wp), W - 1)]
    y, cb, cr = ycbcr(pad)
    if hs == 2:
        box = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
        cb, cr = box(cb), box(cr)
    return [y, cb, cr]


def encode_bytes(rgb8, sampling, quality, fdct="int"):
    rgb8 = np.asarray(rgb8, np.uint8)
    _, H, W = rgb8.shape
    f = frame_for(W, H, sampling, quality)
    for c, p in enumerate(planes(rgb8, f.hs[0])):
        assert p.shape == (f.bh[c] * 8, f.bw[c] * 8)
        s = (p - 128).reshape(f.bh[c], 8, f.bw[c], 8).transpose(0, 2, 1, 3)
        co = quantise_int(fdct_int(s), f.quant[c]) if fdct == "int" else quantise_fp64(fdct_fp64(s), f.quant[c])
        f.coef[f.offset[c]:f.offset[c] + co.size] = co.reshape(-1).astype(np.int16)
    return f


def encode(img, sampling, quality, fdct="int"):
    """fp32 [3][H][W] -> Frame: what dvs_jpeg_encode_views writes for one view"""
    return encode_bytes(to_bytes(img), sampling, quality, fdct)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)
