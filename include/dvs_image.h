/*
 * dvs_image.h — C-ABI of the parallel half of baseline JPEG decoding: quantised DCT coefficients (gstrain/jpeg_io.hpp decodes them on
 * the host) -> planar 8-bit RGB on the device, in one kernel: dequantisation, 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB.
 *
 * Conventions of dvs_export.h: `stream` is a hipStream_t, the call is asynchronous and returns a DVS_* status (dvs_raster.h). No
 * scratch, no atomics: two calls on the same inputs return identical bytes. The result is defined bit for bit in integer arithmetic
 * (every intermediate fits int32 for every int16 coefficient and every quantiser up to 65535); tests/jpeg_ref.py restates it:
 *   dequantise   F = clamp(coef * q, -2048, 2047)        (an 8-bit image's DCT coefficients lie in [-1024, 1016] and a quantised one comes
 *                                                         back within q / 2 of its value: a real encoder's stream never clamps)
 *   inverse DCT  separable, direct matrix form, ONE table T[u][x] = round(2^13 * C(u) / 2 * cos((2x + 1) u pi / 16)), C(0) = 1 / sqrt(2),
 *                C(u > 0) = 1:   col[y][u] = (sum_v T[v][y] * F[v][u] + 2^8) >> 9      (columns first; 4 fractional bits are kept)
 *                                s[y][x]   = (sum_u col[y][u] * T[u][x] + 2^16) >> 17   (>> is the arithmetic shift)
 *                                sample    = clamp(s + 128, 0, 255)
 *   upsampling   the triangle filter common decoders apply by default, over the chroma plane cropped to cw = ceil(W / 2) columns (and, for
 *                2x2, ch = ceil(H / 2) rows); an index outside [0, cw - 1] or [0, ch - 1] is clamped into it (edge replication):
 *                2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2,  out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
 *                2x2: t[Y][i] = 3 s[Y>>1][i] + s[far][i],  far = (Y>>1) - 1 for even Y, (Y>>1) + 1 for odd Y;
 *                     out[Y][2i] = (3 t[Y][i] + t[Y][i-1] + 8) >> 4,  out[Y][2i+1] = (3 t[Y][i] + t[Y][i+1] + 7) >> 4
 *   colour       R = clamp(Y + ((91881 (Cr-128) + 32768) >> 16)),  B = clamp(Y + ((116130 (Cb-128) + 32768) >> 16)),
 *                G = clamp(Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16));  a grayscale image writes R = G = B = Y
 */
#ifndef DVS_IMAGE_H
#define DVS_IMAGE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dvs_jpeg_desc {
    int32_t width, height;          /* 1 .. 65500 */
    int32_t components;             /* 1 (grayscale) or 3 (Y, Cb, Cr; the chroma components are sampled 1x1) */
    int32_t hs, vs;                 /* luma sampling: 1x1, 2x1 or 2x2 (1x1 when components = 1) */
    int32_t blocks_w[3], blocks_h[3];   /* per component: 8x8 blocks per row / per column, padded to whole MCUs:
                                           blocks_w = ceil(width / (8 hs)) * (hs for luma, 1 for chroma), blocks_h likewise */
    int32_t _pad;
    uint64_t offset[3];             /* per component: index of its first coefficient in `coef`, a multiple of 8 */
    uint16_t quant[3][64];          /* per component: the quantiser table in natural order (index 8 v + u) */
} dvs_jpeg_desc;

/* rgb = the image of `coef` (component-major, block-row-major, 64 natural-order coefficients per block, as gsjpeg::Frame holds them).
 * `desc` is a HOST pointer, read before the call returns; `coef` is a DEVICE pointer on a 16-byte boundary; `rgb` is a DEVICE pointer
 * to planar [3][height][width] bytes with no alignment requirement: rows leave as 16-byte stores when rgb is on a 16-byte boundary
 * and width is a multiple of 16, as single bytes otherwise, the same bytes either way.
 * DVS_ERR_INVALID for a NULL pointer, coef off a 16-byte boundary, or a desc that contradicts itself (sizes, sampling, block counts,
 * offsets that are no multiple of 8). */
int dvs_jpeg_reconstruct(void* stream, const dvs_jpeg_desc* desc, const int16_t* coef, uint8_t* rgb);

#ifdef __cplusplus
}
#endif
#endif
